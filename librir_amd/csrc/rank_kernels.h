// Host-side launcher of the spatial rank filters (rank_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rir
{
	// dst[n][y][x] = the element of 0-based rank `rank` among the size_y x size_x values src[n][clamp(y + dy, 0, rows - 1)][clamp(x + dx, 0,
	// w - 1)], |dy| <= size_y / 2, |dx| <= size_x / 2: the window is always full, coordinates are replicated at the border
	// (scipy.ndimage.rank_filter with mode="nearest").  type: 'H' uint16, 'B' uint8, '?' bool (one byte, 0 / 1).  The image is the first
	// `rows` rows; rows >= `rows` are copied.  Ranks 0 and size_x * size_y - 1 are launch_morphology's erode and dilate.  One launch per 65535
	// frames that reads the stack once and writes it once.  Arguments are checked by the caller (odd sizes 1..15, 0 <= rank < size_x *
	// size_y, 0 <= rows <= h, w, h >= 1, no overlap of src and dst); hipErrorInvalidValue on an unknown type.
	hipError_t launch_rank_filter(int type, const void *src, void *dst, int w, int h, int nframes, int rank, int size_x, int size_y, int rows,
								  hipStream_t st);
} // namespace rir
