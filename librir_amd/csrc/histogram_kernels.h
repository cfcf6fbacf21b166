// Host-side launcher of the per-region histograms (histogram_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	// A frame has nregions * (nbins + 3) counters, region after region: a region's nbins bins, its two outside counters and its count.  The
	// first this many of them are counted in LDS (4 bytes each: 64 KiB, two workgroups to a CU), the others in global memory directly
	// (DESIGN.md §7).
	constexpr int HISTOGRAM_LDS_MAX = 16384;
	// Where all counters of a frame and 2, 4 or 8 copies of them take at most this many LDS words (20 KiB: eight workgroups still fit a
	// CU), that many copies are kept, a lane adding to copy lane % copies; the copies are summed where the counters leave LDS.
	constexpr int HISTOGRAM_COPY_MAX = 5120;
	constexpr int HISTOGRAM_MAX_COPIES = 8;
	constexpr int HISTOGRAM_MAX_REGIONS = 65536;
	constexpr int HISTOGRAM_MAX_BINS = 65536;
	constexpr int HISTOGRAM_MAX_CELLS = 1 << 24; // nregions * nbins at most

	// The kernels accumulate in the outputs themselves; the workspace of the C entry is nominal (0 stays the refusal of the query).
	constexpr size_t HISTOGRAM_WORK_BYTES = 8;

	// floor(d / width) for d < 2^16 and 2 <= width <= 2^16 without a division is floor(d * M / 2^32) with M = floor(2^32 / width) + 1: the
	// error d * (M - 2^32 / width) / 2^32 is below d / 2^32 < 2^-16 <= 1 / width.  Powers of two (width 1 among them) shift and have M = 0.
	constexpr uint32_t histogram_div_magic(int width) { return (width & (width - 1)) ? (uint32_t)(0x100000000ull / (uint32_t)width) + 1u : 0u; }

	// Histograms of the first `npx` pixels of each of frames[n][stride] (uint16) over the regions 0 .. nregions - 1 of labels ([stride]
	// shared, or [n][stride] when per_frame; null: every pixel is of region 0, and nregions is 1): hist [n][nregions][nbins] of
	// (v - lo) / width, outside [n][nregions][2] (below lo; at or above lo + nbins * width) and count [n][nregions]; outside and count may
	// be null.  The outputs are zeroed first.  Arguments are checked by the caller (0 <= npx <= stride < 2^31, the bounds above, lo and
	// width within 16 bits, no overlaps).
	hipError_t launch_region_histogram(const uint16_t *frames, const int32_t *labels, int64_t stride, int64_t npx, int n, int per_frame, int nregions,
									   int lo, int width, int nbins, int32_t *count, int32_t *hist, int32_t *outside, hipStream_t st);
} // namespace rir
