// Host-side launcher of the per-region geometry (geometry_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	// Regions up to this many accumulate in LDS, 72 bytes a region: two workgroups of 72 KiB fit the 160 KiB of a CU.  Above it the lanes'
	// partial sums go straight to global memory.
	constexpr int GEOMETRY_LDS_MAX = 1024;

	// The kernels accumulate in the outputs themselves; the workspace of the C entry is nominal (0 stays the refusal of the query).
	constexpr size_t GEOMETRY_WORK_BYTES = 8;

	// Geometry of the regions 0 .. nregions - 1 of labels ([h][w] shared, or [n][h][w] when per_frame), weighted by frames[n][h][w] (uint16)
	// when frames is not null: count [n][nregions], bbox [n][nregions][4], moments [n][nregions][5] and, with frames, weighted
	// [n][nregions][3].  Arguments are checked by the caller (w, h <= 32768, w * h < 2^31, no overlaps, weighted null iff frames is).
	hipError_t launch_region_geometry(const int32_t *labels, const uint16_t *frames, int w, int h, int n, int per_frame, int nregions, int32_t *count,
									  int32_t *bbox, int64_t *moments, int64_t *weighted, hipStream_t st);
} // namespace rir
