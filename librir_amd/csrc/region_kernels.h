// Host-side launcher of the per-region statistics (region_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	// Regions up to this many accumulate in LDS; above it the lanes' partial sums go straight to global memory.
	constexpr int REGION_LDS_MAX = 4096;

	// Device scratch of one call: 32 bytes per (frame, region).
	size_t region_stats_workspace(int64_t npx, int nframes, int nregions);

	// Statistics of frames[n][npx] (uint16) over the regions 0 .. nregions - 1 of labels ([npx] shared, or [n][npx] when per_frame); the
	// outputs are [n][nregions].  Arguments are checked by the caller (npx < 2^31, no overlaps, work >= region_stats_workspace, 8-byte aligned).
	hipError_t launch_region_stats(const uint16_t *frames, const int32_t *labels, int64_t npx, int n, int per_frame, int nregions, int32_t *count,
								   int64_t *sum, int64_t *sumsq, int32_t *vmin, int32_t *vmax, int32_t *argmin, int32_t *argmax, void *work,
								   hipStream_t st);
} // namespace rir
