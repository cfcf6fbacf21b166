// Host-side launcher of the per-pixel statistics over time (pixel_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	// How a stack of n frames of npx pixels is cut along time: `slabs` workgroups per pixel tile, `per_slab` frames each (the last one may
	// be shorter).  One slab: the workgroup writes the outputs itself; more: partials go through the workspace and a second kernel folds them.
	struct PixelStatsPlan
	{
		int slabs, per_slab;
	};
	PixelStatsPlan pixel_stats_plan(int64_t npx, int n);

	// Device scratch of one call: 20 bytes per (slab, pixel) when there is more than one slab, 8 bytes otherwise (never 0).
	size_t pixel_stats_workspace(int64_t npx, int n);

	// Statistics over time of frames[n][npx] (uint16) into the outputs [npx]; the group sum / sumsq and the group vmin / vmax / argmin / argmax
	// are each all given or all null.  Arguments are checked by the caller (npx < 2^31, t0 + n <= 2^31 - 1, at least one group, no overlaps,
	// work >= pixel_stats_workspace and 8-byte aligned).
	hipError_t launch_pixel_stats(const uint16_t *frames, int64_t npx, int n, int t0, int accumulate, int64_t *sum, int64_t *sumsq, int32_t *vmin,
								  int32_t *vmax, int32_t *argmin, int32_t *argmax, void *work, hipStream_t st);
} // namespace rir
