// Per-region geometry of int32 label maps, optionally weighted by a uint16 frame stack (the definition is with rir_region_geometry_device,
// include/rir_amd_device.h).  Two kernels:
//
//   region_geometry_init        writes the identities into the outputs: counts and sums 0, the four box words -1 (all bits set).
//   region_geometry_accumulate  <LDS, WEIGHTED> the walk of region_stats_accumulate (region_kernels.hip): a grid-stride loop over work items
//                               of GM_ITEM pixels of one frame, a thread takes 8 adjacent pixels per step (two 16-byte loads of labels, one
//                               of values) and keeps the run of its current label in registers.  A thread knows the (x, y) of its first
//                               pixel - one division per item, then x += GM_STEP % w, y += GM_STEP / w with one wrap per step - so a run
//                               carries the whole result: count, the box, the five moments and the three weighted sums.  Eight pixels of
//                               the run's label inside one row are added in closed form (sum of x = 8 x0 + 28, of x^2 = 8 x0^2 + 56 x0 +
//                               140, the y terms from y alone); eight pixels that cross a row end, a checked step and a step in which some
//                               lane's label changes go pixel by pixel.  A run is flushed where the label changes and at the end of the
//                               item; when at least GM_WAVE_ADD lanes of a complete wave flush the same label, the wave adds its runs with
//                               shuffles first and one lane flushes.  LDS form: flushes go to per-region LDS accumulators, and at the end
//                               of the item the regions with a non-zero count go to the outputs and are reset.  Global form (nregions >
//                               GEOMETRY_LDS_MAX): flushes go to the outputs directly.
//
// The outputs are the accumulators: every combination is an integer add, min or max (native ds_ / global_atomic add, add_x2, umin, umax and
// smax), so the result does not depend on the order the workgroups run in and there is no finishing pass.  xmin and ymin are unsigned minima
// over the identity 0xFFFFFFFF, xmax and ymax signed maxima over -1: an empty region keeps -1 in all four.
//
// Widths: a run and an item's LDS accumulators hold at most GM_ITEM pixels, so their count, sum of x, sum of y and sum of v fit 32 bits
// (16384 * 65535 < 2^30); the second-order sums are 64-bit everywhere (one row of 32768 pixels has a sum of x^2 of 1.2e13).  The products of
// one pixel fit 32 bits: x * x, x * y, y * y < 2^30 and v * x, v * y < 2^31.
#include <algorithm>

#include "geometry_kernels.h"

namespace rir
{
	constexpr int GM_BLOCK = 256;
	constexpr int GM_PX = 8;					// pixels per thread and step
	constexpr int GM_STEP = GM_BLOCK * GM_PX;	// pixels per workgroup and step
	constexpr int GM_ITEM = 16384;				// pixels per work item
	constexpr int GM_BLOCKS_PER_CU = 8;			// accumulate grid: at most this many workgroups per CU
	constexpr int GM_LDS_BYTES = 160 * 1024;	// LDS per CU
	constexpr int GM_REGION_BYTES = 5 * 8 + 8 * 4; // LDS per region: five 64-bit sums, four 32-bit sums, four box words
	constexpr int GM_FILL_GRID = 65536;			// init: workgroups at most (grid-stride)
	constexpr int GM_WAVE_ADD = 32;				// lanes that flush one label before the wave adds its runs first
	constexpr int GM_MAX_SIDE = 32768;			// w and h at most
	static_assert(GM_ITEM % GM_STEP == 0, "an item is whole steps");
	static_assert((long long)GM_ITEM * 65535 < (1ll << 32) && (long long)GM_ITEM * (GM_MAX_SIDE - 1) < (1ll << 32), "first-order sums of an item fit 32 bits");
	static_assert((long long)GEOMETRY_LDS_MAX * GM_REGION_BYTES * 2 <= GM_LDS_BYTES, "two workgroups per CU in the LDS form");

	struct GmRun // a thread's open run: pixels of label `cur` since the last flush (also: one region's accumulators read back from LDS)
	{
		int cur;
		unsigned cnt, sx, sy, sv;
		unsigned xmin, ymin, xmax, ymax;
		unsigned long long sxx, sxy, syy, svx, svy;
	};

	__device__ __forceinline__ void gm_reset(GmRun &r, int label)
	{
		r.cur = label;
		r.cnt = r.sx = r.sy = r.sv = 0;
		r.xmin = r.ymin = 0xFFFFFFFFu;
		r.xmax = r.ymax = 0;
		r.sxx = r.sxy = r.syy = r.svx = r.svy = 0;
	}

	template <bool WEIGHTED>
	__device__ __forceinline__ void gm_pixel(GmRun &r, unsigned v, unsigned x, unsigned y)
	{
		r.cnt += 1;
		r.sx += x;
		r.sy += y;
		r.sxx += (unsigned long long)(x * x);
		r.sxy += (unsigned long long)(x * y);
		r.syy += (unsigned long long)(y * y);
		r.xmin = min(r.xmin, x);
		r.xmax = max(r.xmax, x);
		r.ymin = min(r.ymin, y);
		r.ymax = max(r.ymax, y);
		if constexpr (WEIGHTED)
		{
			r.sv += v;
			r.svx += (unsigned long long)(v * x);
			r.svy += (unsigned long long)(v * y);
		}
	}

	// The 8 pixels (x0 .. x0 + 7, y) of one row, in closed form.
	template <bool WEIGHTED>
	__device__ __forceinline__ void gm_row8(GmRun &r, const unsigned (&v)[GM_PX], unsigned x0, unsigned y)
	{
		const unsigned sx8 = 8 * x0 + 28; // < 2^19
		r.cnt += 8;
		r.sx += sx8;
		r.sy += 8 * y;
		r.sxx += ((unsigned long long)(x0 * x0) << 3) + (56 * x0 + 140);
		r.sxy += (unsigned long long)y * sx8;
		r.syy += (unsigned long long)(y * y) << 3;
		r.xmin = min(r.xmin, x0);
		r.xmax = max(r.xmax, x0 + 7);
		r.ymin = min(r.ymin, y);
		r.ymax = max(r.ymax, y);
		if constexpr (WEIGHTED)
		{
			unsigned s = 0, js = 0; // sum of v_j < 2^19, sum of j * v_j < 2^21
#pragma unroll
			for (int j = 0; j < GM_PX; ++j)
			{
				s += v[j];
				js += j * v[j];
			}
			r.sv += s;
			r.svx += (unsigned long long)x0 * s + js;
			r.svy += (unsigned long long)y * s;
		}
	}

	template <class T>
	__device__ __forceinline__ void gm_add(T *p, T v, int scope)
	{
		if (scope == __HIP_MEMORY_SCOPE_WORKGROUP)
			__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		else
			__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	template <class T>
	__device__ __forceinline__ void gm_min(T *p, T v, int scope)
	{
		if (scope == __HIP_MEMORY_SCOPE_WORKGROUP)
			__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		else
			__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	template <class T>
	__device__ __forceinline__ void gm_max(T *p, T v, int scope)
	{
		if (scope == __HIP_MEMORY_SCOPE_WORKGROUP)
			__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		else
			__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}

	// One frame's rows of the outputs.
	struct GmOut
	{
		int32_t *count, *bbox; // [nregions], [nregions][4]
		int64_t *mom, *wgt;	   // [nregions][5], [nregions][3] (WEIGHTED)
	};

	// The sums and the box of `t` (cnt != 0) into region r of the outputs.
	template <bool WEIGHTED>
	__device__ __forceinline__ void gm_global_put(const GmOut &o, int r, const GmRun &t)
	{
		constexpr int G = __HIP_MEMORY_SCOPE_AGENT;
		gm_add(o.count + r, (int32_t)t.cnt, G);
		unsigned *ub = reinterpret_cast<unsigned *>(o.bbox + 4 * (int64_t)r);
		gm_min(ub + 0, t.xmin, G);
		gm_min(ub + 1, t.ymin, G);
		gm_max(o.bbox + 4 * (int64_t)r + 2, (int32_t)t.xmax, G);
		gm_max(o.bbox + 4 * (int64_t)r + 3, (int32_t)t.ymax, G);
		unsigned long long *m = reinterpret_cast<unsigned long long *>(o.mom + 5 * (int64_t)r);
		gm_add(m + 0, (unsigned long long)t.sx, G);
		gm_add(m + 1, (unsigned long long)t.sy, G);
		gm_add(m + 2, t.sxx, G);
		gm_add(m + 3, t.sxy, G);
		gm_add(m + 4, t.syy, G);
		if constexpr (WEIGHTED)
		{
			unsigned long long *q = reinterpret_cast<unsigned long long *>(o.wgt + 3 * (int64_t)r);
			gm_add(q + 0, (unsigned long long)t.sv, G);
			gm_add(q + 1, t.svx, G);
			gm_add(q + 2, t.svy, G);
		}
	}

	// Where flushes go.  LDS form: per-region arrays in LDS (SoA, GM_REGION_BYTES a region); global form: the frame's rows of the outputs.
	template <bool LDS>
	struct GmSink
	{
		unsigned long long *sxx, *sxy, *syy, *svx, *svy; // LDS form
		unsigned *cnt, *sx, *sy, *sv, *xmin, *ymin, *xmax, *ymax;
		GmOut out; // global form, and the target of the LDS form at the end of an item

		__device__ __forceinline__ void carve(unsigned long long *lds, int nregions)
		{
			sxx = lds, sxy = lds + nregions, syy = lds + 2 * nregions, svx = lds + 3 * nregions, svy = lds + 4 * nregions;
			cnt = reinterpret_cast<unsigned *>(lds + 5 * nregions);
			sx = cnt + nregions, sy = cnt + 2 * nregions, sv = cnt + 3 * nregions;
			xmin = cnt + 4 * nregions, ymin = cnt + 5 * nregions, xmax = cnt + 6 * nregions, ymax = cnt + 7 * nregions;
		}
		__device__ __forceinline__ void clear(int r) const
		{
			sxx[r] = sxy[r] = syy[r] = svx[r] = svy[r] = 0;
			cnt[r] = sx[r] = sy[r] = sv[r] = 0;
			xmin[r] = ymin[r] = 0xFFFFFFFFu;
			xmax[r] = ymax[r] = 0;
		}
		template <bool WEIGHTED>
		__device__ __forceinline__ void put(int r, const GmRun &t) const
		{
			if constexpr (LDS)
			{
				constexpr int S = __HIP_MEMORY_SCOPE_WORKGROUP;
				gm_add(cnt + r, t.cnt, S);
				gm_add(sx + r, t.sx, S);
				gm_add(sy + r, t.sy, S);
				gm_add(sxx + r, t.sxx, S);
				gm_add(sxy + r, t.sxy, S);
				gm_add(syy + r, t.syy, S);
				gm_min(xmin + r, t.xmin, S);
				gm_min(ymin + r, t.ymin, S);
				gm_max(xmax + r, t.xmax, S);
				gm_max(ymax + r, t.ymax, S);
				if constexpr (WEIGHTED)
				{
					gm_add(sv + r, t.sv, S);
					gm_add(svx + r, t.svx, S);
					gm_add(svy + r, t.svy, S);
				}
			}
			else
				gm_global_put<WEIGHTED>(out, r, t);
		}
	};

	// Flush the runs of the lanes with `go` (their label is about to change, or the item ends), called by the whole wave at one point.  When
	// the wave is complete and at least GM_WAVE_ADD lanes flush, all of them the same label, the runs are added across the wave and one lane
	// flushes.  Either way the same integers are added: the choice changes the cost, never the result.
	template <bool LDS, bool WEIGHTED>
	__device__ __forceinline__ void gm_flush(bool go, const GmRun &r, int nregions, const GmSink<LDS> &sink)
	{
		const unsigned long long m = __ballot(go);
		if (m == 0)
			return;
		const int lead = __ffsll((long long)m) - 1;
		const int label = __shfl(r.cur, lead);
		if (__popcll(m) >= GM_WAVE_ADD && __ballot(1) == ~0ull && __ballot(go && r.cur != label) == 0)
		{
			if ((unsigned)label >= (unsigned)nregions)
				return;
			GmRun t = r;
			if (!go)
				gm_reset(t, label);
#pragma unroll
			for (int d = 32; d > 0; d >>= 1)
			{
				t.cnt += __shfl_xor(t.cnt, d);
				t.sx += __shfl_xor(t.sx, d);
				t.sy += __shfl_xor(t.sy, d);
				t.sxx += __shfl_xor(t.sxx, d);
				t.sxy += __shfl_xor(t.sxy, d);
				t.syy += __shfl_xor(t.syy, d);
				t.xmin = min(t.xmin, (unsigned)__shfl_xor(t.xmin, d));
				t.ymin = min(t.ymin, (unsigned)__shfl_xor(t.ymin, d));
				t.xmax = max(t.xmax, (unsigned)__shfl_xor(t.xmax, d));
				t.ymax = max(t.ymax, (unsigned)__shfl_xor(t.ymax, d));
				if constexpr (WEIGHTED)
				{
					t.sv += __shfl_xor(t.sv, d);
					t.svx += __shfl_xor(t.svx, d);
					t.svy += __shfl_xor(t.svy, d);
				}
			}
			if ((int)__lane_id() == lead)
				sink.template put<WEIGHTED>(label, t);
			return;
		}
		if (go && (unsigned)r.cur < (unsigned)nregions)
			sink.template put<WEIGHTED>(r.cur, r);
	}

	// 8 pixels from p, the first at (x, y) of a frame w wide: each one either continues the run or flushes it and starts one of its own
	// label.  Pixels at or past `end` (checked steps only) leave the run as it is.
	template <bool LDS, bool WEIGHTED, bool CHECK>
	__device__ __forceinline__ void gm_chunk(GmRun &r, const uint16_t *__restrict__ f, const int32_t *__restrict__ l, int64_t p, int64_t end, unsigned x,
											 unsigned y, unsigned w, bool vec, int nregions, const GmSink<LDS> &sink)
	{
		unsigned v[GM_PX];
		int lab[GM_PX];
		if (!CHECK && vec)
		{
			const int4 a = *reinterpret_cast<const int4 *>(l + p), b = *reinterpret_cast<const int4 *>(l + p + 4);
			lab[0] = a.x, lab[1] = a.y, lab[2] = a.z, lab[3] = a.w, lab[4] = b.x, lab[5] = b.y, lab[6] = b.z, lab[7] = b.w;
			if constexpr (WEIGHTED)
			{
				const uint4 q = *reinterpret_cast<const uint4 *>(f + p);
				const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
				for (int j = 0; j < 4; ++j)
				{
					v[2 * j] = u[j] & 0xFFFFu;
					v[2 * j + 1] = u[j] >> 16;
				}
			}
		}
		else
		{
#pragma unroll
			for (int j = 0; j < GM_PX; ++j)
			{
				const bool in = !CHECK || p + j < end;
				lab[j] = in ? l[p + j] : r.cur;
				if constexpr (WEIGHTED)
					v[j] = in ? f[p + j] : 0u;
			}
		}
		if constexpr (!WEIGHTED)
		{
#pragma unroll
			for (int j = 0; j < GM_PX; ++j)
				v[j] = 0;
		}
		bool same = true;
#pragma unroll
		for (int j = 0; j < GM_PX; ++j)
			same &= lab[j] == r.cur;
		if (__ballot(!same) == 0) // every lane's 8 pixels continue its run: no flush point
		{
			if (!CHECK && x + GM_PX <= w)
			{
				gm_row8<WEIGHTED>(r, v, x, y);
				return;
			}
#pragma unroll
			for (int j = 0; j < GM_PX; ++j)
			{
				if (!CHECK || p + j < end)
					gm_pixel<WEIGHTED>(r, v[j], x, y);
				if (++x == w)
					x = 0, ++y;
			}
			return;
		}
#pragma unroll
		for (int j = 0; j < GM_PX; ++j)
		{
			const bool in = !CHECK || p + j < end;
			const bool go = in && lab[j] != r.cur;
			gm_flush<LDS, WEIGHTED>(go, r, nregions, sink);
			if (go)
				gm_reset(r, lab[j]);
			if (in)
				gm_pixel<WEIGHTED>(r, v[j], x, y);
			if (++x == w)
				x = 0, ++y;
		}
	}

	template <bool LDS, bool WEIGHTED>
	__global__ __launch_bounds__(GM_BLOCK) void region_geometry_accumulate(const int32_t *__restrict__ labels, const uint16_t *__restrict__ frames,
																			unsigned w, int64_t npx, int per_frame, int nregions, int64_t items,
																			int per_item_frame, int vec, int32_t *__restrict__ count,
																			int32_t *__restrict__ bbox, int64_t *__restrict__ mom, int64_t *__restrict__ wgt)
	{
		extern __shared__ unsigned long long gm_lds[];
		GmSink<LDS> sink{};
		if constexpr (LDS)
		{
			sink.carve(gm_lds, nregions);
			for (int r = threadIdx.x; r < nregions; r += GM_BLOCK)
				sink.clear(r);
			__syncthreads();
		}
		const unsigned step_dy = (unsigned)GM_STEP / w, step_dx = (unsigned)GM_STEP % w;
		for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
		{
			const int64_t fi = item / per_item_frame;
			const int64_t lo = (item - fi * per_item_frame) * GM_ITEM, hi = min(lo + GM_ITEM, npx);
			const uint16_t *f = WEIGHTED ? frames + fi * npx : nullptr;
			const int32_t *l = labels + (per_frame ? fi * npx : 0);
			sink.out = GmOut{count + fi * nregions, bbox + fi * nregions * 4, mom + fi * nregions * 5, WEIGHTED ? wgt + fi * nregions * 3 : nullptr};
			const unsigned p0 = (unsigned)lo + threadIdx.x * GM_PX; // < 2^31 + GM_ITEM
			unsigned y = p0 / w, x = p0 - y * w;
			GmRun run;
			gm_reset(run, INT32_MIN);
			for (int64_t s = lo; s < hi; s += GM_STEP)
			{
				const int64_t p = s + threadIdx.x * GM_PX;
				if (s + GM_STEP <= hi)
					gm_chunk<LDS, WEIGHTED, false>(run, f, l, p, hi, x, y, w, vec, nregions, sink);
				else
					gm_chunk<LDS, WEIGHTED, true>(run, f, l, p, hi, x, y, w, vec, nregions, sink);
				x += step_dx;
				y += step_dy;
				if (x >= w)
					x -= w, ++y;
			}
			gm_flush<LDS, WEIGHTED>(run.cnt != 0, run, nregions, sink);
			if constexpr (LDS)
			{
				__syncthreads();
				for (int r = threadIdx.x; r < nregions; r += GM_BLOCK)
				{
					const unsigned c = sink.cnt[r];
					if (c == 0)
						continue;
					GmRun t;
					t.cur = r;
					t.cnt = c, t.sx = sink.sx[r], t.sy = sink.sy[r], t.sv = sink.sv[r];
					t.xmin = sink.xmin[r], t.ymin = sink.ymin[r], t.xmax = sink.xmax[r], t.ymax = sink.ymax[r];
					t.sxx = sink.sxx[r], t.sxy = sink.sxy[r], t.syy = sink.syy[r], t.svx = sink.svx[r], t.svy = sink.svy[r];
					gm_global_put<WEIGHTED>(sink.out, r, t);
					sink.clear(r);
				}
				__syncthreads();
			}
		}
	}

	__global__ __launch_bounds__(GM_BLOCK) void region_geometry_init(int32_t *__restrict__ count, int32_t *__restrict__ bbox, int64_t *__restrict__ mom,
																	  int64_t *__restrict__ wgt, int64_t cells)
	{
		for (int64_t i = (int64_t)blockIdx.x * GM_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * GM_BLOCK)
		{
			count[i] = 0;
#pragma unroll
			for (int j = 0; j < 4; ++j)
				bbox[4 * i + j] = -1;
#pragma unroll
			for (int j = 0; j < 5; ++j)
				mom[5 * i + j] = 0;
			if (wgt)
			{
#pragma unroll
				for (int j = 0; j < 3; ++j)
					wgt[3 * i + j] = 0;
			}
		}
	}

	template <bool WEIGHTED>
	static void gm_launch(const int32_t *labels, const uint16_t *frames, int w, int64_t npx, int n, int per_frame, int nregions, int cus, int32_t *count,
						  int32_t *bbox, int64_t *mom, int64_t *wgt, hipStream_t st)
	{
		const int per_item_frame = (int)((npx + GM_ITEM - 1) / GM_ITEM);
		const int64_t items = (int64_t)n * per_item_frame;
		const int vec = npx % GM_PX == 0 && (uintptr_t)labels % 16 == 0 && (!WEIGHTED || (uintptr_t)frames % 16 == 0);
		if (nregions <= GEOMETRY_LDS_MAX)
		{
			const size_t lds = (size_t)nregions * GM_REGION_BYTES;
			const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(GM_BLOCKS_PER_CU, GM_LDS_BYTES / lds));
			const unsigned grid = (unsigned)std::min<int64_t>(items, (int64_t)cus * per_cu);
			region_geometry_accumulate<true, WEIGHTED>
				<<<grid, GM_BLOCK, lds, st>>>(labels, frames, (unsigned)w, npx, per_frame, nregions, items, per_item_frame, vec, count, bbox, mom, wgt);
		}
		else
		{
			const unsigned grid = (unsigned)std::min<int64_t>(items, (int64_t)cus * GM_BLOCKS_PER_CU);
			region_geometry_accumulate<false, WEIGHTED>
				<<<grid, GM_BLOCK, 0, st>>>(labels, frames, (unsigned)w, npx, per_frame, nregions, items, per_item_frame, vec, count, bbox, mom, wgt);
		}
	}

	hipError_t launch_region_geometry(const int32_t *labels, const uint16_t *frames, int w, int h, int n, int per_frame, int nregions, int32_t *count,
									  int32_t *bbox, int64_t *moments, int64_t *weighted, hipStream_t st)
	{
		if (n <= 0 || w <= 0 || h <= 0 || w > GM_MAX_SIDE || h > GM_MAX_SIDE || nregions <= 0 || (frames == nullptr) != (weighted == nullptr))
			return hipErrorInvalidValue;
		int dev = 0, cus = 0;
		hipError_t e = hipGetDevice(&dev);
		if (e == hipSuccess)
			e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
		if (e != hipSuccess)
			return e;
		const int64_t npx = (int64_t)w * h, cells = (int64_t)n * nregions;
		const unsigned fill_grid = (unsigned)std::min<int64_t>(GM_FILL_GRID, (cells + GM_BLOCK - 1) / GM_BLOCK);
		region_geometry_init<<<fill_grid, GM_BLOCK, 0, st>>>(count, bbox, moments, weighted, cells);
		if (frames)
			gm_launch<true>(labels, frames, w, npx, n, per_frame, nregions, cus, count, bbox, moments, weighted, st);
		else
			gm_launch<false>(labels, frames, w, npx, n, per_frame, nregions, cus, count, bbox, moments, weighted, st);
		return hipGetLastError();
	}
} // namespace rir
