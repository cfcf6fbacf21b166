// Per-region histograms of a uint16 frame stack (the definition is with rir_region_histogram_device, include/rir_amd_device.h).  One kernel,
// region_histogram_count<LABELS>: <true> reads a label map, <false> reads the frames alone and counts every pixel into region 0.
//
// A frame has nregions * S counters, S = nbins + 3: counter lab * S + slot, with slot = the bin (v - lo) / width for a value inside the
// binned range, nbins for a value below lo, nbins + 1 for a value at or above lo + nbins * width, and nbins + 2 for the region's count.
// The kernel is walk_counters (region_walk.h), the walk of the counting passes of the per-region quantiles, under the policy HgCount: a
// workgroup takes a contiguous range of work items; a thread takes 8 adjacent pixels per step (one 16-byte load of values, two of labels),
// turns each into its counter and keeps the run of its current counter in a register, and beside it the run of its current label for the
// count: a counter is touched only where the key changes, so coarse bins and flat scenes cost one add per run, not per pixel.  The
// quotient is a shift for a width that is a power of two, else a multiply-high by histogram_div_magic(width); there is no division per pixel.
//
// The first HISTOGRAM_LDS_MAX counters of a frame are counted in LDS (the low regions: label_images numbers the background 0); where the
// workgroup's range passes into another frame, and at its end, the non-zero ones are added to the outputs in global memory and reset.
// The runs of the counters beyond go to global memory directly.  The case that the run does not help is a noisy scene, where a run ends at
// almost every pixel and the adds of a wave fall on few addresses: same-address LDS adds of one instruction are done one after the other.
// Where the counters are few (at most HISTOGRAM_COPY_MAX words with the copies), LDS holds 2, 4 or 8 copies of them side by side,
// counter * copies + lane % copies, so that at most 64 / copies lanes of a wave meet on one address; the copies are summed where the
// counters leave LDS.
//
// Every combination is a 32-bit integer add (ds_add_u32 / global_atomic_add): the result does not depend on the launch geometry, the
// number of copies or the order the workgroups run in.  No scratch, no compare-and-swap loop.  Occupancy: 256 threads; the labelled
// kernel takes 47 VGPRs, the label-free one 38, and amdgpu_waves_per_eu(8, 8) holds both to the eight waves a SIMD that the walking grid
// counts on (64 VGPRs at most: a version that needs more spills, and tests/test_region_histogram_cpu.py reads the compiler's report).  So
// the LDS decides: up to 20 KiB (every case with copies) 8 workgroups = 32 waves a CU, at the full 64 KiB 2 workgroups = 8 waves.
#include "histogram_kernels.h"
#include "region_walk.h"

namespace rir
{
	constexpr int HG_BLOCK = WALK_BLOCK, HG_PX = WALK_PX; // the workgroup and the step of region_walk.h
	static_assert(HISTOGRAM_LDS_MAX * 4 <= WALK_LDS_BYTES / 2, "two workgroups of the LDS form fit one CU");
	static_assert(HISTOGRAM_COPY_MAX * 4 * WALK_BLOCKS_PER_CU <= WALK_LDS_BYTES, "the copies cost no resident workgroup");
	static_assert(HISTOGRAM_COPY_MAX <= HISTOGRAM_LDS_MAX, "counters with copies are all in LDS");

	struct HgBins // how a value becomes a slot
	{
		int lo, nbins;
		uint32_t magic; // histogram_div_magic(width); 0: shift
		int shift;
		int lab_shift; // the bits of a slot in a pixel's key: nbins + 2 < 1 << lab_shift
	};

	// A pixel's counter travels as one word, its key (lab + 1) << lab_shift | slot, with lab_shift the bits of nbins + 2: nregions * nbins
	// <= 2^24 keeps it within 28 bits.  0 is a pixel of no region.
	struct HgRun // a thread's open runs: pixels of counter `key`, and pixels of its label, since their last flush
	{
		uint32_t key, cnt, ccnt;
	};

	// The 8 values at p of a frame without a map; CHECK: a pixel at or past `end` gets the value 0.
	template <bool CHECK>
	__device__ __forceinline__ void hg_values8(const uint16_t *__restrict__ f, int64_t p, int64_t end, bool vec, unsigned (&v)[HG_PX])
	{
		if (!CHECK && vec)
		{
			const uint4 q = *reinterpret_cast<const uint4 *>(f + p);
			v[0] = q.x & 0xFFFFu, v[1] = q.x >> 16, v[2] = q.y & 0xFFFFu, v[3] = q.y >> 16;
			v[4] = q.z & 0xFFFFu, v[5] = q.z >> 16, v[6] = q.w & 0xFFFFu, v[7] = q.w >> 16;
		}
		else
		{
#pragma unroll
			for (int j = 0; j < HG_PX; ++j)
				v[j] = (!CHECK || p + j < end) ? f[p + j] : 0u;
		}
	}

	// The histogram as a policy of walk_counters (region_walk.h).  frames [n][stride], of which the first pixels of each are walked;
	// labels [stride] or, per_frame, [n][stride] (LABELS only).  hist [n][nregions][nbins], outside [n][nregions][2] or null, count
	// [n][nregions] or null.
	template <bool LABELS>
	struct HgCount
	{
		typedef uint32_t Key;
		typedef HgRun Run;
		static constexpr uint32_t NONE = 0;

		const uint16_t *__restrict__ frames;
		const int32_t *__restrict__ labels;
		int64_t stride;
		int per_frame, nregions, vec;
		HgBins bins;
		uint32_t *lds;
		int lds_n, cshift, copy; // counters below lds_n are in LDS, at (counter << cshift) + copy
		uint32_t *__restrict__ all_hist, *__restrict__ all_outside, *__restrict__ all_count;
		const uint16_t *f; // of the open frame
		const int32_t *l;
		uint32_t *hist, *outside, *count;

		__device__ __forceinline__ void clear()
		{
			for (int i = threadIdx.x; i < lds_n << cshift; i += HG_BLOCK)
				lds[i] = 0;
		}
		__device__ __forceinline__ void frame(int64_t fi)
		{
			f = frames + fi * stride;
			l = LABELS ? labels + (per_frame ? fi * stride : 0) : nullptr;
			hist = all_hist + fi * nregions * bins.nbins;
			outside = all_outside ? all_outside + fi * nregions * 2 : nullptr;
			count = all_count ? all_count + fi * nregions : nullptr;
		}
		template <bool CHECK>
		__device__ __forceinline__ void keys(int64_t p, int64_t end, uint32_t (&key)[HG_PX])
		{
			unsigned v[HG_PX];
			int lab[HG_PX];
			if constexpr (LABELS)
				load8<CHECK, true>(f, l, p, end, vec, -1, v, lab);
			else
				hg_values8<CHECK>(f, p, end, vec, v);
#pragma unroll
			for (int j = 0; j < HG_PX; ++j)
			{
				const bool valid = LABELS ? (unsigned)lab[j] < (unsigned)nregions : (!CHECK || p + j < end);
				const int d = (int)v[j] - bins.lo;
				const uint32_t q = bins.magic ? __umulhi((uint32_t)d, bins.magic) : (uint32_t)d >> bins.shift; // d >= 0: d < 2^16
				const uint32_t slot = d < 0 ? (uint32_t)bins.nbins : (q < (uint32_t)bins.nbins ? q : (uint32_t)bins.nbins + 1u);
				key[j] = valid ? ((uint32_t)(LABELS ? lab[j] + 1 : 1) << bins.lab_shift | slot) : 0u;
			}
		}
		static __device__ __forceinline__ void add(HgRun &r, unsigned n)
		{
			r.cnt += n;
			r.ccnt += n;
		}
		// where counter (lab, slot) of the open frame is in global memory; null: an output that is not wanted
		__device__ __forceinline__ uint32_t *global(int lab, int slot) const
		{
			if (slot < bins.nbins)
				return hist + (int64_t)lab * bins.nbins + slot;
			if (slot < bins.nbins + 2)
				return outside ? outside + 2 * (int64_t)lab + (slot - bins.nbins) : nullptr;
			return count ? count + lab : nullptr;
		}
		// `cnt` more for counter lab * (nbins + 3) + slot
		__device__ __forceinline__ void put(int lab, int slot, uint32_t cnt) const
		{
			const int at = lab * (bins.nbins + 3) + slot;
			if (at < lds_n)
				walk_add<WALK_WG>(lds + (at << cshift) + copy, cnt);
			else if (uint32_t *dst = global(lab, slot))
				walk_add<WALK_AGENT>(dst, cnt);
		}
		// Close the run of the counter, and that of the label where the label changes; open those of `next`.
		__device__ __forceinline__ void flush(HgRun &r, uint32_t next) const
		{
			const int lab = (int)(r.key >> bins.lab_shift) - 1;
			if (lab >= 0 && r.cnt != 0)
				put(lab, (int)(r.key & ((1u << bins.lab_shift) - 1)), r.cnt);
			if ((next ^ r.key) >> bins.lab_shift)
			{
				if (lab >= 0 && r.ccnt != 0)
					put(lab, bins.nbins + 2, r.ccnt);
				r.ccnt = 0;
			}
			r.key = next;
			r.cnt = 0;
		}
		__device__ __forceinline__ void drain()
		{
			const int S = bins.nbins + 3, copies = 1 << cshift;
			for (int i = threadIdx.x; i < lds_n; i += HG_BLOCK)
			{
				uint32_t c = 0;
				for (int j = 0; j < copies; ++j)
					c += lds[(i << cshift) + j];
				if (c == 0)
					continue;
				for (int j = 0; j < copies; ++j)
					lds[(i << cshift) + j] = 0;
				const int lab = i / S; // per non-zero counter and frame, not per pixel
				if (uint32_t *dst = global(lab, i - lab * S))
					walk_add<WALK_AGENT>(dst, c);
			}
		}
	};

	// npx: the pixels of a frame that are walked (at most stride); the outputs are zero on entry.
	template <bool LABELS>
	__attribute__((amdgpu_waves_per_eu(8, 8))) __global__ __launch_bounds__(HG_BLOCK) void region_histogram_count(
		const uint16_t *__restrict__ frames, const int32_t *__restrict__ labels, int64_t stride, int64_t npx, int per_frame, int nregions, HgBins bins,
		int64_t items, int per_item_frame, int vec, int lds_n, int cshift, uint32_t *__restrict__ hist, uint32_t *__restrict__ outside,
		uint32_t *__restrict__ count)
	{
		extern __shared__ uint32_t hg_lds[];
		HgCount<LABELS> pol{frames, labels, stride, per_frame, nregions, vec, bins, hg_lds, lds_n, cshift, (int)(threadIdx.x & ((1u << cshift) - 1)),
							hist,   outside, count};
		walk_counters(pol, npx, items, per_item_frame);
	}

	hipError_t launch_region_histogram(const uint16_t *frames, const int32_t *labels, int64_t stride, int64_t npx, int n, int per_frame, int nregions,
									   int lo, int width, int nbins, int32_t *count, int32_t *hist, int32_t *outside, hipStream_t st)
	{
		if (n < 0 || npx < 0 || npx > stride || nregions <= 0 || nbins <= 0 || width <= 0 || (!labels && (nregions != 1 || per_frame)))
			return hipErrorInvalidValue;
		if (n == 0)
			return hipSuccess;
		const size_t cells = (size_t)n * nregions;
		hipError_t e = hipMemsetAsync(hist, 0, cells * nbins * 4, st);
		if (e == hipSuccess && outside)
			e = hipMemsetAsync(outside, 0, cells * 8, st);
		if (e == hipSuccess && count)
			e = hipMemsetAsync(count, 0, cells * 4, st);
		if (e != hipSuccess || npx == 0)
			return e;
		int cus = 0;
		e = cu_count(&cus);
		if (e != hipSuccess)
			return e;
		HgBins bins{lo, nbins, histogram_div_magic(width), 0, 1};
		while ((1 << bins.shift) < width)
			++bins.shift;
		while ((1 << bins.lab_shift) <= nbins + 2)
			++bins.lab_shift;
		const int64_t total = (int64_t)nregions * (nbins + 3);
		const int lds_n = (int)std::min<int64_t>(total, HISTOGRAM_LDS_MAX);
		int cshift = 0;
		while ((2 << cshift) <= HISTOGRAM_MAX_COPIES && (total << (cshift + 1)) <= HISTOGRAM_COPY_MAX)
			++cshift;
		const size_t lds = ((size_t)lds_n << cshift) * 4;
		const WalkShape s = walk_launch_shape(npx, n, lds, cus);
		const int vec = walk_vec(stride, labels, frames);
		uint32_t *h = reinterpret_cast<uint32_t *>(hist), *o = reinterpret_cast<uint32_t *>(outside), *c = reinterpret_cast<uint32_t *>(count);
		if (labels)
			region_histogram_count<true><<<s.grid, HG_BLOCK, lds, st>>>(frames, labels, stride, npx, per_frame, nregions, bins, s.items, s.per_item_frame, vec,
																		lds_n, cshift, h, o, c);
		else
			region_histogram_count<false><<<s.grid, HG_BLOCK, lds, st>>>(frames, nullptr, stride, npx, 0, 1, bins, s.items, s.per_item_frame, vec, lds_n, cshift,
																		 h, o, c);
		return hipGetLastError();
	}
} // namespace rir
