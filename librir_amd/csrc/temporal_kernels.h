// Host-side launcher of the temporal median filter (temporal_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rir
{
	// Outputs k < count at t = first + k * step of the stack src[n][h][w]: the median of frames max(0, t - r) .. min(n - 1, t + r)
	// (r = window / 2; upper median sorted[c / 2] of a truncated window of c frames), taken where it differs from src[t] by more than
	// `threshold`, in rows < `rows`; src[t] elsewhere.  dst[count][h][w].  Arguments are checked by the caller (odd window <= 63,
	// positions inside the stack, no overlap of src and dst).
	hipError_t launch_temporal_median(const uint16_t *src, uint16_t *dst, int w, int h, int n, int first, int count, int step, int window, int threshold,
									  int rows, hipStream_t st);
} // namespace rir
