// Per-region statistics of a uint16 frame stack (the definition is with rir_region_stats_device, include/rir_amd_device.h).  Three kernels:
//
//   region_stats_init        zeroes the counts and the workspace: every accumulator below starts at 0.
//   region_stats_accumulate  <LDS> the walk of region_walk.h.  A run holds count, sum, sum of squares and two 32-bit keys (value << 16 |
//                            offset in the item) for the minimum and the maximum; a flush widens the keys to frame coordinates.  LDS form:
//                            per-region LDS accumulators, 36 bytes a region.  Global form (nregions > REGION_LDS_MAX): the counts and the
//                            workspace directly.  The wave adds its runs first whenever all its flushing lanes agree (RsWalk::WAVE_ADD).
//   region_stats_finish      turns the workspace into the seven outputs.
//
// Every combination is an integer add or a max of 64-bit keys, so the result does not depend on the order the workgroups run in.  Both
// keys are maxima with 0 as identity: value << 32 | ~index for the maximum and (65535 - value) << 32 | ~index for the minimum; the
// complemented index makes ties fall to the lowest index.  The atomics are native ds_/global_atomic add, add_x2 and umax_x2.
#include "region_kernels.h"
#include "region_walk.h"

namespace rir
{
	constexpr int RS_BLOCK = WALK_BLOCK;
	constexpr int RS_FILL_GRID = 65536; // init / finish: workgroups at most (grid-stride)
	static_assert(WALK_ITEM <= 65536, "offsets in an item fit the 16 bits of a run's keys");

	struct RsAcc // one (frame, region) of the workspace
	{
		unsigned long long sum, sumsq, kmin, kmax;
	};
	static_assert(sizeof(RsAcc) == 32, "workspace layout");

	struct RsRun // a thread's open run: pixels of label `cur` since the last flush
	{
		int cur;
		unsigned cnt, sum;
		unsigned long long sq;
		unsigned amin; // min of value << 16 | offset
		unsigned amax; // max of value << 16 | (0xFFFF - offset)
	};

	// A run's keys in frame coordinates: `base` is the item's first pixel.
	__device__ __forceinline__ unsigned long long rs_kmin(unsigned amin, unsigned base)
	{
		return (unsigned long long)(0xFFFFu - (amin >> 16)) << 32 | (unsigned)~(base + (amin & 0xFFFFu));
	}
	__device__ __forceinline__ unsigned long long rs_kmax(unsigned amax, unsigned base)
	{
		return (unsigned long long)(amax >> 16) << 32 | (unsigned)~(base + (0xFFFFu - (amax & 0xFFFFu)));
	}

	__device__ __forceinline__ void rs_pixel(RsRun &r, unsigned v, unsigned off)
	{
		const unsigned a = v << 16 | off;
		r.cnt += 1;
		r.sum += v;
		r.sq += (unsigned long long)(v * v); // 65535^2 < 2^32
		r.amin = min(r.amin, a);
		r.amax = max(r.amax, a ^ 0xFFFFu);
	}

	// The statistics policy of walk_regions.  LDS form: per-region arrays in LDS (SoA); `count` and `acc` are the frame's rows [nregions].
	template <bool LDS>
	struct RsWalk
	{
		using Run = RsRun;
		static constexpr bool VALUES = true;
		static constexpr int WAVE_ADD = 1;
		unsigned long long *sum, *sumsq, *kmin, *kmax; // LDS form
		unsigned *cnt;
		int32_t *count0, *count; // all frames; this frame
		RsAcc *acc0, *acc;

		static __device__ __forceinline__ void reset(RsRun &r, int label) { r = RsRun{label, 0, 0, 0, 0xFFFFFFFFu, 0}; }
		static __device__ __forceinline__ void pixel(RsRun &r, unsigned v, const WalkPos &pos) { rs_pixel(r, v, pos.off); }
		static __device__ __forceinline__ bool chunk8(RsRun &, const unsigned (&)[WALK_PX], const WalkPos &) { return false; }
		static __device__ __forceinline__ void combine(RsRun &t, int d)
		{
			t.cnt += __shfl_xor(t.cnt, d);
			t.sum += __shfl_xor(t.sum, d);
			t.sq += __shfl_xor(t.sq, d);
			t.amin = min(t.amin, (unsigned)__shfl_xor(t.amin, d));
			t.amax = max(t.amax, (unsigned)__shfl_xor(t.amax, d));
		}
		__device__ __forceinline__ void frame(int64_t fi, int nregions)
		{
			count = count0 + fi * nregions;
			acc = acc0 + fi * nregions;
		}
		__device__ __forceinline__ void global_put(int r, unsigned cnt_, unsigned long long sum_, unsigned long long sq_, unsigned long long kmin_,
												   unsigned long long kmax_) const
		{
			walk_add<WALK_AGENT>(count + r, (int32_t)cnt_);
			walk_add<WALK_AGENT>(&acc[r].sum, sum_);
			walk_add<WALK_AGENT>(&acc[r].sumsq, sq_);
			walk_max<WALK_AGENT>(&acc[r].kmin, kmin_);
			walk_max<WALK_AGENT>(&acc[r].kmax, kmax_);
		}
		__device__ __forceinline__ void put(int r, const RsRun &t, unsigned base) const
		{
			const unsigned long long lo = rs_kmin(t.amin, base), hi = rs_kmax(t.amax, base);
			if constexpr (LDS)
			{
				walk_add<WALK_WG>(cnt + r, t.cnt);
				walk_add<WALK_WG>(sum + r, (unsigned long long)t.sum);
				walk_add<WALK_WG>(sumsq + r, t.sq);
				walk_max<WALK_WG>(kmin + r, lo);
				walk_max<WALK_WG>(kmax + r, hi);
			}
			else
				global_put(r, t.cnt, t.sum, t.sq, lo, hi);
		}
		__device__ __forceinline__ void carve(unsigned long long *lds, int nregions)
		{
			sum = lds, sumsq = lds + nregions, kmin = lds + 2 * nregions, kmax = lds + 3 * nregions;
			cnt = reinterpret_cast<unsigned *>(lds + 4 * nregions);
		}
		__device__ __forceinline__ void clear(int r) const
		{
			sum[r] = sumsq[r] = kmin[r] = kmax[r] = 0;
			cnt[r] = 0;
		}
		__device__ __forceinline__ void drain(int r) const
		{
			if (cnt[r] == 0)
				return;
			global_put(r, cnt[r], sum[r], sumsq[r], kmin[r], kmax[r]);
			clear(r);
		}
	};

	template <bool LDS>
	__global__ __launch_bounds__(RS_BLOCK) void region_stats_accumulate(const uint16_t *__restrict__ frames, const int32_t *__restrict__ labels,
																		 int64_t npx, int per_frame, int nregions, int64_t items, int per_item_frame,
																		 int vec, int32_t *__restrict__ count, RsAcc *__restrict__ acc)
	{
		RsWalk<LDS> walk{};
		walk.count0 = count;
		walk.acc0 = acc;
		walk_regions<LDS>(walk, frames, labels, 1u, npx, per_frame, nregions, items, per_item_frame, vec);
	}

	__global__ __launch_bounds__(RS_BLOCK) void region_stats_init(int32_t *__restrict__ count, RsAcc *__restrict__ acc, int64_t cells)
	{
		for (int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * RS_BLOCK)
		{
			count[i] = 0;
			acc[i] = RsAcc{0, 0, 0, 0};
		}
	}

	__global__ __launch_bounds__(RS_BLOCK) void region_stats_finish(const int32_t *__restrict__ count, const RsAcc *__restrict__ acc, int64_t cells,
																	int64_t *__restrict__ sum, int64_t *__restrict__ sumsq, int32_t *__restrict__ vmin,
																	int32_t *__restrict__ vmax, int32_t *__restrict__ argmin, int32_t *__restrict__ argmax)
	{
		for (int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * RS_BLOCK)
		{
			const RsAcc a = acc[i];
			sum[i] = (int64_t)a.sum;
			sumsq[i] = (int64_t)a.sumsq;
			const bool any = count[i] != 0;
			vmin[i] = any ? (int32_t)(0xFFFFu - (unsigned)(a.kmin >> 32)) : -1;
			argmin[i] = any ? (int32_t)~(unsigned)a.kmin : -1;
			vmax[i] = any ? (int32_t)(a.kmax >> 32) : -1;
			argmax[i] = any ? (int32_t)~(unsigned)a.kmax : -1;
		}
	}

	size_t region_stats_workspace(int64_t npx, int nframes, int nregions)
	{
		(void)npx;
		return (size_t)nframes * (size_t)nregions * sizeof(RsAcc);
	}

	hipError_t launch_region_stats(const uint16_t *frames, const int32_t *labels, int64_t npx, int n, int per_frame, int nregions, int32_t *count,
								   int64_t *sum, int64_t *sumsq, int32_t *vmin, int32_t *vmax, int32_t *argmin, int32_t *argmax, void *work,
								   hipStream_t st)
	{
		if (n <= 0 || npx <= 0 || nregions <= 0)
			return hipErrorInvalidValue;
		int cus = 0;
		const hipError_t e = cu_count(&cus);
		if (e != hipSuccess)
			return e;
		RsAcc *acc = static_cast<RsAcc *>(work);
		const int64_t cells = (int64_t)n * nregions;
		const unsigned fill_grid = (unsigned)std::min<int64_t>(RS_FILL_GRID, (cells + RS_BLOCK - 1) / RS_BLOCK);
		region_stats_init<<<fill_grid, RS_BLOCK, 0, st>>>(count, acc, cells);
		const size_t lds = nregions <= REGION_LDS_MAX ? (size_t)nregions * (4 * sizeof(unsigned long long) + sizeof(unsigned)) : 0;
		const WalkShape s = walk_launch_shape(npx, n, lds, cus);
		const int vec = walk_vec(npx, labels, frames);
		if (lds)
			region_stats_accumulate<true><<<s.grid, RS_BLOCK, lds, st>>>(frames, labels, npx, per_frame, nregions, s.items, s.per_item_frame, vec, count, acc);
		else
			region_stats_accumulate<false><<<s.grid, RS_BLOCK, 0, st>>>(frames, labels, npx, per_frame, nregions, s.items, s.per_item_frame, vec, count, acc);
		region_stats_finish<<<fill_grid, RS_BLOCK, 0, st>>>(count, acc, cells, sum, sumsq, vmin, vmax, argmin, argmax);
		return hipGetLastError();
	}
} // namespace rir
