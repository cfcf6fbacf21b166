// Host-side launcher of the per-region quantiles (quantile_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	// A counting pass keeps the first this many of a frame's 256-bin histograms in LDS (1 KiB each) and sends the counts of the others
	// straight to global memory: the high-byte pass has nregions histograms, the low-byte pass nregions * npercents.
	constexpr int QUANTILE_LDS_MAX = 64;
	constexpr int QUANTILE_MAX_REGIONS = 65536;
	constexpr int QUANTILE_MAX_PERCENTS = 8;

	struct QuantilePercents // by value to the select kernel
	{
		float p[QUANTILE_MAX_PERCENTS];
	};

	// Device scratch of ONE frame, B(nregions, npercents) = nregions * (1024 + 16 + 8 * npercents + 1024 * npercents) bytes:
	//   uint32 hist_hi[nregions][256]             counts of v >> 8
	//   uint16 codes[nregions][8]                 per percent: the high byte whose pixels the low-byte pass counts for it, 0xFFFF for none
	//   int32  sel[nregions][npercents][2]        -1, or owner << 8 | bucket; the rank left inside the bucket
	//   uint32 hist_lo[nregions][npercents][256]  counts of v & 255 among the pixels of the owner's bucket
	// A group of G frames holds G of each array, array after array.
	size_t region_quantiles_frame_bytes(int nregions, int npercents);

	// Quantiles of frames[n][npx] (uint16) over the regions 0 .. nregions - 1 of labels ([npx] shared, or [n][npx] when per_frame):
	// count [n][nregions], values [n][nregions][npercents].  The stack is worked through in groups of work_bytes / B frames.  Arguments are
	// checked by the caller (npx < 2^31, percents in [0, 1], no overlaps, work_bytes >= B, work 8-byte aligned).
	hipError_t launch_region_quantiles(const uint16_t *frames, const int32_t *labels, int64_t npx, int n, int per_frame, int nregions,
									   const QuantilePercents &percents, int npercents, int32_t *count, int32_t *values, void *work, size_t work_bytes,
									   hipStream_t st);
} // namespace rir
