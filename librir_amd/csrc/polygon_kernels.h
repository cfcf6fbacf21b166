// Host-side launcher of the polygon label maps (polygon_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	constexpr int POLYGON_MAX_POLYGONS = 65536;			// polygons of a set
	constexpr int POLYGON_MAX_POINTS = 1024;			// vertices of a polygon: a row's nodes are sorted in LDS
	constexpr int64_t POLYGON_MAX_PIXELS = 0x7FFF0000LL; // pixels of a map

	// 1 <= w, h with w * h <= POLYGON_MAX_PIXELS, nmaps >= 0, 0 <= npoly <= POLYGON_MAX_POLYGONS, 1 <= max_pts <= POLYGON_MAX_POINTS.
	bool polygon_geometry_ok(int w, int h, int nmaps, int npoly, int max_pts);

	// Device scratch of one call (0: geometry refused): per (map, polygon) the clipped box, the vertex count and the rounded vertices.
	size_t polygon_map_workspace(int w, int h, int nmaps, int npoly, int max_pts);

	// dst[nmaps][h][w] = background, then the polygons of each map's set painted in order (the definition is with rir_polygon_map_device,
	// include/rir_amd_device.h).  values and shifts may be null.  Arguments are checked by the caller (geometry, no overlaps, work >=
	// polygon_map_workspace and 8-byte aligned).
	hipError_t launch_polygon_map(const double *xy, const int32_t *npts, const int32_t *values, int npoly, int max_pts, int nmaps, int sets_per_map,
								  const double *shifts, int w, int h, int32_t background, int32_t *dst, void *work, hipStream_t st);
} // namespace rir
