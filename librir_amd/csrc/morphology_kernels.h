// Host-side launcher of the flat morphology filters (morphology_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rir
{
	enum
	{
		MORPH_ERODE = 0,	// min over the size_y x size_x window clipped to the image
		MORPH_DILATE = 1,	// max over the same window
		MORPH_OPEN = 2,		// dilate(erode(f)), each stage with its own clipped windows
		MORPH_CLOSE = 3,	// erode(dilate(f))
		MORPH_TOPHAT = 4,	// f - open(f)
		MORPH_BLACKHAT = 5, // close(f) - f
		MORPH_GRADIENT = 6, // dilate(f) - erode(f)
		MORPH_OPS = 7
	};

	// dst[n][h][w] = op(src[n][h][w]) frame by frame, in ONE launch (per 65535 frames) that reads the stack once and writes it once.  type: 'H'
	// uint16, 'B' uint8, '?' bool (one byte, 0 / 1).  The image is the first `rows` rows; rows >= `rows` are copied.  Arguments are checked
	// by the caller (odd sizes 1..15, 0 <= rows <= h, w, h >= 1, no overlap of src and dst); hipErrorInvalidValue on an unknown type or op.
	hipError_t launch_morphology(int type, const void *src, void *dst, int w, int h, int nframes, int op, int size_x, int size_y, int rows,
								 hipStream_t st);
} // namespace rir
