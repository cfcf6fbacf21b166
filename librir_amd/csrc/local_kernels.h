// Host-side launchers of the local window statistics (local_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rir
{
	enum LocalPolarity
	{
		LOCAL_ABOVE = 0,
		LOCAL_BELOW = 1,
		LOCAL_BOTH = 2,
		LOCAL_POLARITIES
	};
	constexpr int LOCAL_K_NUM_MAX = 255, LOCAL_K_DEN_MAX = 64, LOCAL_DELTA_MAX = 65535;

	// Over the size_y x size_x window (odd, 1..15; n cells) around every pixel of src[nframes][h][w], coordinates clamped into the image (its
	// first `rows` rows) as launch_rank_filter clamps them: sum = the window's sum (int32), sumsq = its sum of squares (int64), mean =
	// (sum + n / 2) / n in the type of src.  Each output may be null; in rows >= `rows` mean is a copy of src and the sums are 0.  type:
	// 'H' uint16, 'B' uint8, '?' bool (one byte, 0 / 1).  One launch per 65535 frames that reads the stack once and writes each output once;
	// no workspace.  Arguments are checked by the caller (odd sizes 1..15, 0 <= rows <= h, w, h >= 1, an output, no overlap);
	// hipErrorInvalidValue on an unknown type.
	hipError_t launch_local_stats(int type, const void *src, int w, int h, int nframes, int size_x, int size_y, int rows, int32_t *sum, int64_t *sumsq,
								  void *mean, hipStream_t st);

	// mask[n][y][x] (a 0 / 1 byte) = the z-score test of pixel v against its window's sum S and sum of squares Q: with d = n v - S and
	// V = n Q - S^2, "above" is d > delta n and d^2 k_den^2 > k_num^2 V, "below" the same with -d in the first test, "both" either; 0 in rows
	// >= `rows`.  0 <= k_num <= 255, 1 <= k_den <= 64, |delta| <= 65535: what keeps every product inside int64.
	hipError_t launch_local_threshold(int type, const void *src, uint8_t *mask, int w, int h, int nframes, int size_x, int size_y, int rows, int k_num,
									  int k_den, int delta, int polarity, hipStream_t st);
} // namespace rir
