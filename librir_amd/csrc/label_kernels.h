// Host-side launchers of the connected-component kernels (label_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rir
{
	// Working memory of one labelling of `frames` images (device memory, 8-byte aligned), in bytes; 0: geometry refused.
	size_t label_workspace_bytes(int w, int h, int frames);
	// A batch of images [frames][h][w], every one labelled on its own.
	// cell_bytes: 1, 2, 4, 8 (integers: equal when their bits are), -4 float, -8 double (IEEE ==).  `background`: the cell value, host memory.
	// d_dst [frames][h][w] int32 labels; per image `table_entries` entries of d_xy (2 doubles each) and d_area, of which the first
	// min(count, table_entries) are written; d_count [frames] (= components + 1, the reference's return value): any memory the device can
	// write (device or page-locked host).
	hipError_t launch_label_images(int cell_bytes, const void *d_src, const void *background, int w, int h, int frames, int *d_dst, double *d_xy,
								   int *d_area, int64_t table_entries, int *d_count, void *d_work, hipStream_t st);
	// Hot spots of uint16 frames [frames][h][w], labelled without a mask in memory.  A pixel (y, x) belongs to a component when y < rows and
	// its value is above `low` (d_low_map[h][w] when given, shared by the frames), compared as int32; components are the 4-connected sets
	// of such pixels.  A component keeps its number when it holds a pixel above `high` (d_high_map when given; asked for by use_high),
	// min_area <= its area <= max_area, and - with clear_border - none of its pixels lies in row 0, row rows - 1, column 0 or column
	// w - 1; the others are background.  Kept components are numbered 1, 2, ... in the raster order of their first pixel.  d_dst, d_area
	// and d_count as launch_label_images writes them (d_count = kept components + 1); d_first [frames][table_entries]: the raster index
	// y * w + x of each component's first pixel, -1 in entry 0.  Working memory: label_hot_spots_workspace_bytes (0: geometry refused).
	size_t label_hot_spots_workspace_bytes(int w, int h, int frames);
	hipError_t launch_label_hot_spots(const uint16_t *d_frames, int w, int h, int frames, int rows, int low, const int *d_low_map, bool use_high, int high,
									  const int *d_high_map, int min_area, int max_area, bool clear_border, int *d_dst, int *d_first, int *d_area,
									  int64_t table_entries, int *d_count, void *d_work, hipStream_t st);
	// d_dst [frames][h][w]: `foreground` on the largest component of each image (the first in raster order among equals),
	// `background_as_int` elsewhere; all zero when an image holds no component.
	hipError_t launch_keep_largest_areas(int cell_bytes, const void *d_src, const void *background, int w, int h, int frames, int *d_dst, int foreground,
										 int background_as_int, void *d_work, hipStream_t st);
} // namespace rir
