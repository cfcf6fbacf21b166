// Per-region statistics of a uint16 frame stack (the definition is with rir_region_stats_device, include/rir_amd_device.h).  Three kernels:
//
//   region_stats_init        zeroes the counts and the workspace: every accumulator below starts at 0.
//   region_stats_accumulate  <LDS> a grid-stride loop over work items of RS_ITEM pixels of one frame.  A thread takes 8 adjacent pixels per
//                            step (one 16-byte load of values, two of labels) and keeps the run of its current label in registers: count,
//                            sum, sum of squares and two 32-bit keys (value << 16 | offset in the item) for the minimum and the maximum.  A
//                            run is flushed where the thread's label changes and at the end of the item; when every lane of the wave
//                            flushes the same label, the wave adds its runs with shuffles first and one lane flushes.  LDS form: flushes
//                            go to per-region LDS accumulators, and at the end of the item the regions with a non-zero count (the ones
//                            this item touched) go to global memory and are reset.  Global form (nregions > REGION_LDS_MAX): flushes go
//                            to global memory directly.
//   region_stats_finish      turns the workspace into the seven outputs.
//
// Every combination is an integer add or a max of 64-bit keys, so the result does not depend on the order the workgroups run in.  Both
// keys are maxima with 0 as identity: value << 32 | ~index for the maximum and (65535 - value) << 32 | ~index for the minimum; the
// complemented index makes ties fall to the lowest index.  The atomics are native ds_/global_atomic add, add_x2 and umax_x2.
#include <algorithm>

#include "region_kernels.h"

namespace rir
{
	constexpr int RS_BLOCK = 256;
	constexpr int RS_PX = 8;									  // pixels per thread and step
	constexpr int RS_STEP = RS_BLOCK * RS_PX;					  // pixels per workgroup and step
	constexpr int RS_ITEM = 16384;								  // pixels per work item
	constexpr int RS_BLOCKS_PER_CU = 8;							  // accumulate grid: at most this many workgroups per CU
	constexpr int RS_LDS_BYTES = 160 * 1024;					  // LDS per CU
	constexpr int RS_FILL_GRID = 65536;							  // init / finish: workgroups at most (grid-stride)
	static_assert(RS_ITEM % RS_STEP == 0, "an item is whole steps");
	static_assert(RS_ITEM <= 65536, "offsets in an item fit the 16 bits of a run's keys");
	static_assert((long long)64 * (RS_ITEM / RS_BLOCK) * 65535 < (1ll << 32), "a wave's runs in one item sum to less than 2^32");

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

	__device__ __forceinline__ void rs_reset(RsRun &r, int label)
	{
		r.cur = label;
		r.cnt = 0;
		r.sum = 0;
		r.sq = 0;
		r.amin = 0xFFFFFFFFu;
		r.amax = 0;
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

	template <class T>
	__device__ __forceinline__ void rs_add(T *p, T v, int scope)
	{
		if (scope == __HIP_MEMORY_SCOPE_WORKGROUP)
			__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		else
			__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__device__ __forceinline__ void rs_max(unsigned long long *p, unsigned long long v, int scope)
	{
		if (scope == __HIP_MEMORY_SCOPE_WORKGROUP)
			__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		else
			__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}

	// Where flushes go.  LDS form: per-region arrays in LDS (SoA, 36 bytes a region); global form: the frame's row of counts and workspace.
	template <bool LDS>
	struct RsSink
	{
		unsigned long long *sum, *sumsq, *kmin, *kmax; // LDS form
		unsigned *cnt;
		RsAcc *acc; // global form: [nregions] of this frame
		int32_t *count;

		__device__ __forceinline__ void put(int r, unsigned cnt_, unsigned long long sum_, unsigned long long sq_, unsigned long long kmin_,
											unsigned long long kmax_) const
		{
			if constexpr (LDS)
			{
				rs_add(cnt + r, cnt_, __HIP_MEMORY_SCOPE_WORKGROUP);
				rs_add(sum + r, sum_, __HIP_MEMORY_SCOPE_WORKGROUP);
				rs_add(sumsq + r, sq_, __HIP_MEMORY_SCOPE_WORKGROUP);
				rs_max(kmin + r, kmin_, __HIP_MEMORY_SCOPE_WORKGROUP);
				rs_max(kmax + r, kmax_, __HIP_MEMORY_SCOPE_WORKGROUP);
			}
			else
			{
				rs_add(count + r, (int32_t)cnt_, __HIP_MEMORY_SCOPE_AGENT);
				rs_add(&acc[r].sum, sum_, __HIP_MEMORY_SCOPE_AGENT);
				rs_add(&acc[r].sumsq, sq_, __HIP_MEMORY_SCOPE_AGENT);
				rs_max(&acc[r].kmin, kmin_, __HIP_MEMORY_SCOPE_AGENT);
				rs_max(&acc[r].kmax, kmax_, __HIP_MEMORY_SCOPE_AGENT);
			}
		}
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

	// Flush the runs of the lanes with `go` (their label is about to change, or the item ends), called by the whole wave at one point.  When
	// the wave is complete and every flushing lane holds the same label, the runs are added across the wave and one lane flushes.
	template <bool LDS>
	__device__ __forceinline__ void rs_flush(bool go, const RsRun &r, int nregions, unsigned base, const RsSink<LDS> &sink)
	{
		const unsigned long long m = __ballot(go);
		if (m == 0)
			return;
		const int lead = __ffsll((long long)m) - 1;
		const int label = __shfl(r.cur, lead);
		if (__ballot(1) == ~0ull && __ballot(go && r.cur != label) == 0)
		{
			if ((unsigned)label >= (unsigned)nregions)
				return;
			unsigned cnt = go ? r.cnt : 0, sum = go ? r.sum : 0, amin = go ? r.amin : 0xFFFFFFFFu, amax = go ? r.amax : 0;
			unsigned long long sq = go ? r.sq : 0;
#pragma unroll
			for (int d = 32; d > 0; d >>= 1)
			{
				cnt += __shfl_xor(cnt, d);
				sum += __shfl_xor(sum, d);
				sq += __shfl_xor(sq, d);
				amin = min(amin, (unsigned)__shfl_xor(amin, d));
				amax = max(amax, (unsigned)__shfl_xor(amax, d));
			}
			if ((int)__lane_id() == lead)
				sink.put(label, cnt, sum, sq, rs_kmin(amin, base), rs_kmax(amax, base));
			return;
		}
		if (go && (unsigned)r.cur < (unsigned)nregions)
			sink.put(r.cur, r.cnt, r.sum, r.sq, rs_kmin(r.amin, base), rs_kmax(r.amax, base));
	}

	// 8 pixels from p (offset off in the item): each one either continues the run or flushes it and starts one of its own label.  Pixels at
	// or past `end` (checked steps only) leave the run as it is.
	template <bool LDS, bool CHECK>
	__device__ __forceinline__ void rs_chunk(RsRun &r, const uint16_t *__restrict__ f, const int32_t *__restrict__ l, int64_t p, int64_t end, unsigned off,
											 bool vec, int nregions, unsigned base, const RsSink<LDS> &sink)
	{
		unsigned v[RS_PX];
		int lab[RS_PX];
		if (!CHECK && vec)
		{
			const uint4 x = *reinterpret_cast<const uint4 *>(f + p);
			const int4 a = *reinterpret_cast<const int4 *>(l + p), b = *reinterpret_cast<const int4 *>(l + p + 4);
			const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
			for (int j = 0; j < 4; ++j)
			{
				v[2 * j] = w[j] & 0xFFFFu;
				v[2 * j + 1] = w[j] >> 16;
			}
			lab[0] = a.x, lab[1] = a.y, lab[2] = a.z, lab[3] = a.w, lab[4] = b.x, lab[5] = b.y, lab[6] = b.z, lab[7] = b.w;
		}
		else
		{
#pragma unroll
			for (int j = 0; j < RS_PX; ++j)
			{
				const bool in = !CHECK || p + j < end;
				v[j] = in ? f[p + j] : 0u;
				lab[j] = in ? l[p + j] : r.cur;
			}
		}
		bool same = true;
#pragma unroll
		for (int j = 0; j < RS_PX; ++j)
			same &= lab[j] == r.cur;
		if (__ballot(!same) == 0) // every lane's 8 pixels continue its run: no flush point
		{
#pragma unroll
			for (int j = 0; j < RS_PX; ++j)
				if (!CHECK || p + j < end)
					rs_pixel(r, v[j], off + j);
			return;
		}
#pragma unroll
		for (int j = 0; j < RS_PX; ++j)
		{
			const bool in = !CHECK || p + j < end;
			const bool go = in && lab[j] != r.cur;
			rs_flush<LDS>(go, r, nregions, base, sink);
			if (go)
				rs_reset(r, lab[j]);
			if (in)
				rs_pixel(r, v[j], off + j);
		}
	}

	template <bool LDS>
	__global__ __launch_bounds__(RS_BLOCK) void region_stats_accumulate(const uint16_t *__restrict__ frames, const int32_t *__restrict__ labels,
																		 int64_t npx, int per_frame, int nregions, int64_t items, int per_item_frame,
																		 int vec, int32_t *__restrict__ count, RsAcc *__restrict__ acc)
	{
		extern __shared__ unsigned long long rs_lds[];
		RsSink<LDS> sink{};
		if constexpr (LDS)
		{
			sink.sum = rs_lds;
			sink.sumsq = rs_lds + nregions;
			sink.kmin = rs_lds + 2 * nregions;
			sink.kmax = rs_lds + 3 * nregions;
			sink.cnt = reinterpret_cast<unsigned *>(rs_lds + 4 * nregions);
			for (int r = threadIdx.x; r < nregions; r += RS_BLOCK)
			{
				sink.sum[r] = sink.sumsq[r] = sink.kmin[r] = sink.kmax[r] = 0;
				sink.cnt[r] = 0;
			}
			__syncthreads();
		}
		for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
		{
			const int64_t fi = item / per_item_frame;
			const int64_t lo = (item - fi * per_item_frame) * RS_ITEM, hi = min(lo + RS_ITEM, npx);
			const uint16_t *f = frames + fi * npx;
			const int32_t *l = labels + (per_frame ? fi * npx : 0);
			if constexpr (!LDS)
			{
				sink.count = count + fi * nregions;
				sink.acc = acc + fi * nregions;
			}
			RsRun run;
			rs_reset(run, INT32_MIN);
			for (int64_t s = lo; s < hi; s += RS_STEP)
			{
				const int64_t p = s + threadIdx.x * RS_PX;
				const unsigned off = (unsigned)(p - lo);
				if (s + RS_STEP <= hi)
					rs_chunk<LDS, false>(run, f, l, p, hi, off, vec, nregions, (unsigned)lo, sink);
				else
					rs_chunk<LDS, true>(run, f, l, p, hi, off, vec, nregions, (unsigned)lo, sink);
			}
			rs_flush<LDS>(run.cnt != 0, run, nregions, (unsigned)lo, sink);
			if constexpr (LDS)
			{
				__syncthreads();
				int32_t *cf = count + fi * nregions;
				RsAcc *af = acc + fi * nregions;
				for (int r = threadIdx.x; r < nregions; r += RS_BLOCK)
				{
					const unsigned c = sink.cnt[r];
					if (c == 0)
						continue;
					rs_add(cf + r, (int32_t)c, __HIP_MEMORY_SCOPE_AGENT);
					rs_add(&af[r].sum, sink.sum[r], __HIP_MEMORY_SCOPE_AGENT);
					rs_add(&af[r].sumsq, sink.sumsq[r], __HIP_MEMORY_SCOPE_AGENT);
					rs_max(&af[r].kmin, sink.kmin[r], __HIP_MEMORY_SCOPE_AGENT);
					rs_max(&af[r].kmax, sink.kmax[r], __HIP_MEMORY_SCOPE_AGENT);
					sink.sum[r] = sink.sumsq[r] = sink.kmin[r] = sink.kmax[r] = 0;
					sink.cnt[r] = 0;
				}
				__syncthreads();
			}
		}
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
		int dev = 0, cus = 0;
		hipError_t e = hipGetDevice(&dev);
		if (e == hipSuccess)
			e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
		if (e != hipSuccess)
			return e;
		RsAcc *acc = static_cast<RsAcc *>(work);
		const int64_t cells = (int64_t)n * nregions;
		const unsigned fill_grid = (unsigned)std::min<int64_t>(RS_FILL_GRID, (cells + RS_BLOCK - 1) / RS_BLOCK);
		region_stats_init<<<fill_grid, RS_BLOCK, 0, st>>>(count, acc, cells);
		const int per_item_frame = (int)((npx + RS_ITEM - 1) / RS_ITEM);
		const int64_t items = (int64_t)n * per_item_frame;
		const int vec = npx % RS_PX == 0 && (uintptr_t)frames % 16 == 0 && (uintptr_t)labels % 16 == 0;
		if (nregions <= REGION_LDS_MAX)
		{
			const size_t lds = (size_t)nregions * (4 * sizeof(unsigned long long) + sizeof(unsigned));
			const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(RS_BLOCKS_PER_CU, RS_LDS_BYTES / lds));
			const unsigned grid = (unsigned)std::min<int64_t>(items, (int64_t)cus * per_cu);
			region_stats_accumulate<true><<<grid, RS_BLOCK, lds, st>>>(frames, labels, npx, per_frame, nregions, items, per_item_frame, vec, count, acc);
		}
		else
		{
			const unsigned grid = (unsigned)std::min<int64_t>(items, (int64_t)cus * RS_BLOCKS_PER_CU);
			region_stats_accumulate<false><<<grid, RS_BLOCK, 0, st>>>(frames, labels, npx, per_frame, nregions, items, per_item_frame, vec, count, acc);
		}
		region_stats_finish<<<fill_grid, RS_BLOCK, 0, st>>>(count, acc, cells, sum, sumsq, vmin, vmax, argmin, argmax);
		return hipGetLastError();
	}
} // namespace rir
