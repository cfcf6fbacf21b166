// Per-region quantiles of a uint16 frame stack (the definition is with rir_region_quantiles_device, include/rir_amd_device.h): a two-level
// radix select, 8 + 8 bits, over a group of frames at a time.  Four kernels:
//
//   region_quantiles_count<false>  the high-byte pass.  A workgroup takes a contiguous range of work items of QT_ITEM pixels; a thread takes
//                                  8 adjacent pixels per step (one 16-byte load of values, two of labels), turns each into the index of its
//                                  counter, label * 256 + (v >> 8), and keeps the run of its current counter in a register: the counter is
//                                  touched only where the index changes, which is what keeps a scene of a few hundred levels from sending
//                                  every pixel to the same address.  The first QUANTILE_LDS_MAX histograms of a frame are counted in LDS:
//                                  where the workgroup's range passes into another frame, and at its end, the non-zero counters are added
//                                  to the frame's histograms in global memory and reset.  The runs of the histograms beyond go to global
//                                  memory directly (label_images numbers the background 0, so most pixels of a hot-spot map stay in LDS).
//   region_quantiles_select        one wave per (frame, region) scans the 256 high counters: the count, and per percent the rank t, the
//                                  bucket that holds it and the rank left inside the bucket - or the final value where the region is empty,
//                                  t == 0 or t > count.  Percents of one region that fall in the same bucket share the histogram of the first.
//   region_quantiles_count<true>   the low-byte pass: the same walk; a pixel whose high byte is a chosen bucket of its region counts v & 255
//                                  in that bucket's histogram (buckets of one region differ, so a pixel counts at most once).
//   region_quantiles_finish        one wave per (frame, region, percent) scans the 256 low counters for the rank left.
//
// The walk of the two counting passes - items, frames, runs, the drain - is walk_counters of region_walk.h under the policy QtCount.
//
// Every combination is a 32-bit integer add (ds_add_u32 / global_atomic_add), so the result does not depend on the order the workgroups
// run in; the only floating-point operation is the rank, qt_rank().
#include "quantile_kernels.h"
#include "quantile_rank.h"
#include "region_walk.h"

namespace rir
{
	constexpr int QT_BLOCK = WALK_BLOCK, QT_PX = WALK_PX, QT_STEP = WALK_STEP, QT_ITEM = WALK_ITEM; // the items and steps of region_walk.h
	constexpr int QT_SCAN_GRID = 65536;			  // select / finish: workgroups at most (grid-stride)
	constexpr int QT_WAVES = QT_BLOCK / 64;		  // select / finish: waves per workgroup
	constexpr unsigned QT_NO_CODE = 0xFFFFu;	  // codes: no low-byte histogram for this percent
	static_assert(QUANTILE_LDS_MAX * 1024 <= WALK_LDS_BYTES, "the LDS form fits one CU");
	static_assert(QUANTILE_MAX_PERCENTS == 8, "codes are 8 x 16 bits per region");

	// A pixel's counter within its frame, -1 for none.  High pass: label * 256 + (v >> 8).  Low pass: the codes of the thread's current label
	// are kept in registers (8 x 16 bits, read again where the label changes); the slot whose code is the pixel's high byte counts v & 255.
	template <bool LOW>
	struct QtIndex
	{
		int nregions, nq;
		const uint2 *codes; // low pass: [nregions][2] of the frame
		int cur;
		uint32_t w[4];

		__device__ __forceinline__ void frame(const uint2 *c)
		{
			codes = c;
			cur = INT32_MIN;
			w[0] = w[1] = w[2] = w[3] = 0xFFFFFFFFu;
		}
		__device__ __forceinline__ int operator()(uint32_t v, int lab)
		{
			const bool valid = (unsigned)lab < (unsigned)nregions;
			if constexpr (!LOW)
				return valid ? lab * 256 + (int)(v >> 8) : -1;
			else
			{
				if (lab != cur)
				{
					cur = lab;
					uint2 a = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu), b = a;
					if (valid)
					{
						a = codes[2 * (int64_t)lab];
						b = codes[2 * (int64_t)lab + 1];
					}
					w[0] = a.x, w[1] = a.y, w[2] = b.x, w[3] = b.y;
				}
				const uint32_t hi = v >> 8;
				int slot = -1;
#pragma unroll
				for (int j = 0; j < QUANTILE_MAX_PERCENTS; ++j)
					if (((w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) == hi)
						slot = j;
				return slot < 0 ? -1 : (lab * nq + slot) * 256 + (int)(v & 255u);
			}
		}
	};

	struct QtRun // a thread's open run: pixels of counter `key` since the last flush
	{
		int key;
		uint32_t cnt;
	};

	// Close the run and open one of counter `next`: counters below lds_bins are in LDS, the others in the frame's histograms `hist`.
	__device__ __forceinline__ void qt_flush(QtRun &r, uint32_t *lds, int lds_bins, uint32_t *hist, int next)
	{
		if (r.key >= 0 && r.cnt != 0)
		{
			if (r.key < lds_bins)
				walk_add<WALK_WG>(lds + r.key, r.cnt);
			else
				walk_add<WALK_AGENT>(hist + r.key, r.cnt);
		}
		r.key = next;
		r.cnt = 0;
	}

	// A counting pass as a policy of walk_counters (region_walk.h): the keys are QtIndex's, the counters below lds_bins are in LDS.
	template <bool LOW>
	struct QtCount
	{
		typedef int Key;
		typedef QtRun Run;
		static constexpr int NONE = -1;

		const uint16_t *__restrict__ frames;
		const int32_t *__restrict__ labels;
		int64_t npx;
		int per_frame, nregions, vec;
		const uint2 *__restrict__ codes;
		uint32_t *__restrict__ hist; // [n][bins]
		uint32_t *lds;
		int bins, lds_bins;
		QtIndex<LOW> index;
		const uint16_t *f; // of the open frame
		const int32_t *l;
		uint32_t *h;

		__device__ __forceinline__ void clear()
		{
			for (int i = threadIdx.x; i < lds_bins; i += QT_BLOCK)
				lds[i] = 0;
		}
		__device__ __forceinline__ void frame(int64_t fi)
		{
			f = frames + fi * npx;
			l = labels + (per_frame ? fi * npx : 0);
			h = hist + fi * bins;
			index.frame(LOW ? codes + fi * nregions * 2 : nullptr);
		}
		template <bool CHECK>
		__device__ __forceinline__ void keys(int64_t p, int64_t end, int (&key)[QT_PX])
		{
			unsigned v[QT_PX];
			int lab[QT_PX];
			load8<CHECK, true>(f, l, p, end, vec, -1, v, lab); // a pixel past the end gets label -1, no region: it counts nowhere
#pragma unroll
			for (int j = 0; j < QT_PX; ++j)
				key[j] = index(v[j], lab[j]);
		}
		static __device__ __forceinline__ void add(QtRun &r, unsigned n) { r.cnt += n; }
		__device__ __forceinline__ void flush(QtRun &r, int next) { qt_flush(r, lds, lds_bins, h, next); }
		__device__ __forceinline__ void drain()
		{
			for (int i = threadIdx.x; i < lds_bins; i += QT_BLOCK)
			{
				const uint32_t c = lds[i];
				if (c == 0)
					continue;
				walk_add<WALK_AGENT>(h + i, c);
				lds[i] = 0;
			}
		}
	};

	// hist: [n][slots][256], slots = nregions (high pass) or nregions * nq (low pass); codes (low pass): [n][nregions] x 16 bytes.
	template <bool LOW>
	__global__ __launch_bounds__(QT_BLOCK) void region_quantiles_count(const uint16_t *__restrict__ frames, const int32_t *__restrict__ labels,
																		int64_t npx, int per_frame, int nregions, int nq, int64_t items,
																		int per_item_frame, int vec, const uint2 *__restrict__ codes,
																		uint32_t *__restrict__ hist)
	{
		extern __shared__ uint32_t qt_lds[];
		const int slots = LOW ? nregions * nq : nregions;
		QtCount<LOW> pol{frames, labels, npx, per_frame, nregions, vec, codes, hist, qt_lds, slots * 256, min(slots, QUANTILE_LDS_MAX) * 256};
		pol.index.nregions = nregions;
		pol.index.nq = nq;
		pol.index.frame(nullptr);
		walk_counters(pol, npx, items, per_item_frame);
	}

	// Wave-wide: lane l holds the counters c[0..3] = bins 4l .. 4l + 3 of one histogram.  -> the lane's exclusive prefix; *total for all.
	__device__ __forceinline__ uint32_t qt_scan(const uint32_t c[4], uint32_t *total)
	{
		const int lane = (int)__lane_id();
		const uint32_t own = c[0] + c[1] + c[2] + c[3];
		uint32_t inc = own;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1)
		{
			const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
			if (lane >= d)
				inc += o;
		}
		*total = (uint32_t)__shfl((int)inc, 63, 64);
		return inc - own;
	}

	// Wave-wide, 1 <= t <= total: the first bin whose cumulative count reaches t; *left = t less the count of the bins before it.
	__device__ __forceinline__ int qt_find(const uint32_t c[4], uint32_t excl, uint32_t t, uint32_t *left)
	{
		const uint32_t own = c[0] + c[1] + c[2] + c[3];
		const unsigned long long m = __ballot(excl + own >= t);
		const int lead = __ffsll((long long)m) - 1;
		uint32_t before = excl;
		int k = 0;
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
			const bool step = k == i && before + c[i] < t;
			before += step ? c[i] : 0u;
			k += step ? 1 : 0;
		}
		*left = t - (uint32_t)__shfl((int)before, lead, 64);
		return lead * 4 + __shfl(k, lead, 64);
	}

	__device__ __forceinline__ void qt_load(const uint32_t *hist, uint32_t c[4])
	{
		const uint2 *h = reinterpret_cast<const uint2 *>(hist) + 2 * __lane_id(); // the workspace is 8-byte aligned
		const uint2 a = h[0], b = h[1];
		c[0] = a.x, c[1] = a.y, c[2] = b.x, c[3] = b.y;
	}

	__global__ __launch_bounds__(QT_BLOCK) void region_quantiles_select(const uint32_t *__restrict__ hist_hi, int64_t cells, int nq,
																		 QuantilePercents pc, int32_t *__restrict__ count, int32_t *__restrict__ values,
																		 uint2 *__restrict__ codes, int2 *__restrict__ sel)
	{
		const int lane = (int)__lane_id();
		for (int64_t cell = (int64_t)blockIdx.x * QT_WAVES + threadIdx.x / 64; cell < cells; cell += (int64_t)gridDim.x * QT_WAVES)
		{
			uint32_t c[4], total;
			qt_load(hist_hi + cell * 256, c);
			const uint32_t excl = qt_scan(c, &total);
			int bucket[QUANTILE_MAX_PERCENTS];
			uint32_t code[QUANTILE_MAX_PERCENTS];
#pragma unroll
			for (int j = 0; j < QUANTILE_MAX_PERCENTS; ++j)
			{
				bucket[j] = -1;
				code[j] = QT_NO_CODE;
				if (j >= nq)
					continue;
				const uint32_t t = qt_rank(total, pc.p[j]);
				int value = total == 0 ? -1 : 0; // empty; t == 0 or t > count
				int2 s = make_int2(-1, 0);
				if (t >= 1 && t <= total)
				{
					uint32_t left;
					bucket[j] = qt_find(c, excl, t, &left);
					int owner = j;
#pragma unroll
					for (int i = QUANTILE_MAX_PERCENTS - 1; i >= 0; --i)
						if (i < j && bucket[i] == bucket[j])
							owner = i;
					if (owner == j)
						code[j] = (uint32_t)bucket[j];
					s = make_int2(owner << 8 | bucket[j], (int)left);
				}
				if (lane == 0)
				{
					sel[cell * nq + j] = s;
					if (s.x < 0)
						values[cell * nq + j] = value;
				}
			}
			if (lane == 0)
			{
				count[cell] = (int32_t)total;
				codes[2 * cell] = make_uint2(code[0] | code[1] << 16, code[2] | code[3] << 16);
				codes[2 * cell + 1] = make_uint2(code[4] | code[5] << 16, code[6] | code[7] << 16);
			}
		}
	}

	__global__ __launch_bounds__(QT_BLOCK) void region_quantiles_finish(const uint32_t *__restrict__ hist_lo, const int2 *__restrict__ sel, int64_t cells,
																		 int nq, int32_t *__restrict__ values)
	{
		const int64_t n = cells * nq;
		for (int64_t i = (int64_t)blockIdx.x * QT_WAVES + threadIdx.x / 64; i < n; i += (int64_t)gridDim.x * QT_WAVES)
		{
			const int2 s = sel[i];
			if (s.x < 0)
				continue; // select wrote the value
			const int64_t cell = i / nq;
			uint32_t c[4], total, left;
			qt_load(hist_lo + (cell * nq + (s.x >> 8)) * 256, c);
			const uint32_t excl = qt_scan(c, &total);
			const int v = (s.x & 255) << 8 | qt_find(c, excl, (uint32_t)s.y, &left);
			if (__lane_id() == 0)
				values[i] = v == 65535 ? 0 : v; // 65535 is in the population but in no bin
		}
	}

	size_t region_quantiles_frame_bytes(int nregions, int npercents)
	{
		return (size_t)nregions * (1024 + 16 + (size_t)npercents * (8 + 1024));
	}

	namespace
	{
		template <bool LOW>
		void launch_count(const uint16_t *frames, const int32_t *labels, int64_t npx, int n, int per_frame, int nregions, int nq, int cus,
						  const uint2 *codes, uint32_t *hist, hipStream_t st)
		{
			const size_t lds = (size_t)std::min<int64_t>((int64_t)nregions * (LOW ? nq : 1), QUANTILE_LDS_MAX) * 1024;
			const WalkShape s = walk_launch_shape(npx, n, lds, cus);
			region_quantiles_count<LOW><<<s.grid, QT_BLOCK, lds, st>>>(frames, labels, npx, per_frame, nregions, nq, s.items, s.per_item_frame,
																	   walk_vec(npx, labels, frames), codes, hist);
		}
	} // namespace

	hipError_t launch_region_quantiles(const uint16_t *frames, const int32_t *labels, int64_t npx, int n, int per_frame, int nregions,
									   const QuantilePercents &percents, int npercents, int32_t *count, int32_t *values, void *work, size_t work_bytes,
									   hipStream_t st)
	{
		if (n <= 0 || npx <= 0 || nregions <= 0 || npercents <= 0 || npercents > QUANTILE_MAX_PERCENTS)
			return hipErrorInvalidValue;
		const size_t frame_bytes = region_quantiles_frame_bytes(nregions, npercents);
		if (work_bytes < frame_bytes)
			return hipErrorInvalidValue;
		int cus = 0;
		hipError_t e = cu_count(&cus);
		if (e != hipSuccess)
			return e;
		const int group = (int)std::min<size_t>((size_t)n, work_bytes / frame_bytes);
		const size_t K = (size_t)nregions, Q = (size_t)npercents;
		for (int g0 = 0; g0 < n; g0 += group)
		{
			const int g = std::min(group, n - g0);
			const int64_t cells = (int64_t)g * nregions;
			char *base = static_cast<char *>(work);
			uint32_t *hist_hi = reinterpret_cast<uint32_t *>(base);
			uint2 *codes = reinterpret_cast<uint2 *>(base + (size_t)g * K * 1024);
			int2 *sel = reinterpret_cast<int2 *>(base + (size_t)g * K * (1024 + 16));
			uint32_t *hist_lo = reinterpret_cast<uint32_t *>(base + (size_t)g * K * (1024 + 16 + 8 * Q));
			e = hipMemsetAsync(work, 0, (size_t)g * frame_bytes, st);
			if (e != hipSuccess)
				return e;
			const uint16_t *f = frames + (size_t)g0 * npx;
			const int32_t *l = labels + (per_frame ? (size_t)g0 * npx : 0);
			int32_t *cnt = count + (size_t)g0 * K, *val = values + (size_t)g0 * K * Q;
			launch_count<false>(f, l, npx, g, per_frame, nregions, npercents, cus, nullptr, hist_hi, st);
			const unsigned select_grid = (unsigned)std::min<int64_t>(QT_SCAN_GRID, (cells + QT_WAVES - 1) / QT_WAVES);
			region_quantiles_select<<<select_grid, QT_BLOCK, 0, st>>>(hist_hi, cells, npercents, percents, cnt, val, codes, sel);
			launch_count<true>(f, l, npx, g, per_frame, nregions, npercents, cus, codes, hist_lo, st);
			const unsigned finish_grid = (unsigned)std::min<int64_t>(QT_SCAN_GRID, (cells * npercents + QT_WAVES - 1) / QT_WAVES);
			region_quantiles_finish<<<finish_grid, QT_BLOCK, 0, st>>>(hist_lo, sel, cells, npercents, val);
			e = hipGetLastError();
			if (e != hipSuccess)
				return e;
		}
		return hipSuccess;
	}
} // namespace rir
