// The rank of a quantile, shared by the per-region (quantile_kernels.hip) and the per-pixel (pixel_quantile_kernels.hip) units so that both
// compile the same expression.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rir
{
	// The reference's masked rule (Filters.cpp:92), as quantile_select_kernel states it: the product in float32, rounded half away from zero.
	__device__ __forceinline__ uint32_t qt_rank(uint32_t c, float percent) { return (uint32_t)(int)roundf(__fmul_rn((float)c, percent)); }
} // namespace rir
