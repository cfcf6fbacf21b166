// Per-region geometry of int32 label maps, optionally weighted by a uint16 frame stack (the definition is with rir_region_geometry_device,
// include/rir_amd_device.h).  Two kernels:
//
//   region_geometry_init        writes the identities into the outputs: counts and sums 0, the four box words -1 (all bits set).
//   region_geometry_accumulate  <LDS, WEIGHTED> the walk of region_walk.h, read by (x, y), so a run carries the whole result: count, the
//                               box, the five moments and the three weighted sums.  Eight pixels of the run's label inside one row are
//                               added in closed form (sum of x = 8 x0 + 28, of x^2 = 8 x0^2 + 56 x0 + 140, the y terms from y alone);
//                               eight pixels that cross a row end go pixel by pixel.  The wave adds its runs first only from GM_WAVE_ADD
//                               flushing lanes up.  LDS form: per-region LDS accumulators, GM_REGION_BYTES a region.  Global form
//                               (nregions > GEOMETRY_LDS_MAX): the outputs directly.
//
// The outputs are the accumulators: every combination is an integer add, min or max (native ds_ / global_atomic add, add_x2, umin, umax and
// smax), so the result does not depend on the order the workgroups run in and there is no finishing pass.  xmin and ymin are unsigned minima
// over the identity 0xFFFFFFFF, xmax and ymax signed maxima over -1: an empty region keeps -1 in all four.
//
// Widths: a run and an item's LDS accumulators hold at most WALK_ITEM pixels, so their count, sum of x, sum of y and sum of v fit 32 bits
// (16384 * 65535 < 2^30); the second-order sums are 64-bit everywhere (one row of 32768 pixels has a sum of x^2 of 1.2e13).  The products of
// one pixel fit 32 bits: x * x, x * y, y * y < 2^30 and v * x, v * y < 2^31.
#include "geometry_kernels.h"
#include "region_walk.h"

namespace rir
{
	constexpr int GM_BLOCK = WALK_BLOCK;
	constexpr int GM_PX = WALK_PX;
	constexpr int GM_REGION_BYTES = 5 * 8 + 8 * 4; // LDS per region: five 64-bit sums, four 32-bit sums, four box words
	constexpr int GM_FILL_GRID = 65536;			// init: workgroups at most (grid-stride)
	constexpr int GM_WAVE_ADD = 32;				// lanes that flush one label before the wave adds its runs first
	constexpr int GM_MAX_SIDE = 32768;			// w and h at most
	static_assert((long long)WALK_ITEM * (GM_MAX_SIDE - 1) < (1ll << 32), "first-order sums of an item fit 32 bits");
	static_assert((long long)GEOMETRY_LDS_MAX * GM_REGION_BYTES * 2 <= WALK_LDS_BYTES, "two workgroups per CU in the LDS form");

	struct GmRun // a thread's open run: pixels of label `cur` since the last flush (also: one region's accumulators read back from LDS)
	{
		int cur;
		unsigned cnt, sx, sy, sv;
		unsigned xmin, ymin, xmax, ymax;
		unsigned long long sxx, sxy, syy, svx, svy;
	};

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
		walk_add<G>(o.count + r, (int32_t)t.cnt);
		unsigned *ub = reinterpret_cast<unsigned *>(o.bbox + 4 * (int64_t)r);
		walk_min<G>(ub + 0, t.xmin);
		walk_min<G>(ub + 1, t.ymin);
		walk_max<G>(o.bbox + 4 * (int64_t)r + 2, (int32_t)t.xmax);
		walk_max<G>(o.bbox + 4 * (int64_t)r + 3, (int32_t)t.ymax);
		unsigned long long *m = reinterpret_cast<unsigned long long *>(o.mom + 5 * (int64_t)r);
		walk_add<G>(m + 0, (unsigned long long)t.sx);
		walk_add<G>(m + 1, (unsigned long long)t.sy);
		walk_add<G>(m + 2, t.sxx);
		walk_add<G>(m + 3, t.sxy);
		walk_add<G>(m + 4, t.syy);
		if constexpr (WEIGHTED)
		{
			unsigned long long *q = reinterpret_cast<unsigned long long *>(o.wgt + 3 * (int64_t)r);
			walk_add<G>(q + 0, (unsigned long long)t.sv);
			walk_add<G>(q + 1, t.svx);
			walk_add<G>(q + 2, t.svy);
		}
	}

	// The geometry policy of walk_regions.  LDS form: per-region arrays in LDS (SoA); `out` is the frame's rows of the outputs, the target of
	// the global form and of the LDS form at the end of an item.
	template <bool LDS, bool WEIGHTED>
	struct GmWalk
	{
		using Run = GmRun;
		static constexpr bool VALUES = WEIGHTED;
		static constexpr int WAVE_ADD = GM_WAVE_ADD;
		unsigned long long *sxx, *sxy, *syy, *svx, *svy; // LDS form
		unsigned *cnt, *sx, *sy, *sv, *xmin, *ymin, *xmax, *ymax;
		GmOut all, out; // all frames; this frame

		static __device__ __forceinline__ void reset(GmRun &r, int label)
		{
			r.cur = label;
			r.cnt = r.sx = r.sy = r.sv = 0;
			r.xmin = r.ymin = 0xFFFFFFFFu;
			r.xmax = r.ymax = 0;
			r.sxx = r.sxy = r.syy = r.svx = r.svy = 0;
		}
		static __device__ __forceinline__ void pixel(GmRun &r, unsigned v, const WalkPos &pos) { gm_pixel<WEIGHTED>(r, v, pos.x, pos.y); }
		static __device__ __forceinline__ bool chunk8(GmRun &r, const unsigned (&v)[GM_PX], const WalkPos &pos)
		{
			if (pos.x + GM_PX > pos.w)
				return false;
			gm_row8<WEIGHTED>(r, v, pos.x, pos.y);
			return true;
		}
		static __device__ __forceinline__ void combine(GmRun &t, int d)
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
		__device__ __forceinline__ void frame(int64_t fi, int nregions)
		{
			const int64_t at = fi * nregions;
			out = GmOut{all.count + at, all.bbox + at * 4, all.mom + at * 5, WEIGHTED ? all.wgt + at * 3 : nullptr};
		}
		__device__ __forceinline__ void put(int r, const GmRun &t, unsigned) const
		{
			if constexpr (LDS)
			{
				walk_add<WALK_WG>(cnt + r, t.cnt);
				walk_add<WALK_WG>(sx + r, t.sx);
				walk_add<WALK_WG>(sy + r, t.sy);
				walk_add<WALK_WG>(sxx + r, t.sxx);
				walk_add<WALK_WG>(sxy + r, t.sxy);
				walk_add<WALK_WG>(syy + r, t.syy);
				walk_min<WALK_WG>(xmin + r, t.xmin);
				walk_min<WALK_WG>(ymin + r, t.ymin);
				walk_max<WALK_WG>(xmax + r, t.xmax);
				walk_max<WALK_WG>(ymax + r, t.ymax);
				if constexpr (WEIGHTED)
				{
					walk_add<WALK_WG>(sv + r, t.sv);
					walk_add<WALK_WG>(svx + r, t.svx);
					walk_add<WALK_WG>(svy + r, t.svy);
				}
			}
			else
				gm_global_put<WEIGHTED>(out, r, t);
		}
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
		__device__ __forceinline__ void drain(int r) const
		{
			if (cnt[r] == 0)
				return;
			const GmRun t{r, cnt[r], sx[r], sy[r], sv[r], xmin[r], ymin[r], xmax[r], ymax[r], sxx[r], sxy[r], syy[r], svx[r], svy[r]};
			gm_global_put<WEIGHTED>(out, r, t);
			clear(r);
		}
	};

	template <bool LDS, bool WEIGHTED>
	__global__ __launch_bounds__(GM_BLOCK) void region_geometry_accumulate(const int32_t *__restrict__ labels, const uint16_t *__restrict__ frames,
																			unsigned w, int64_t npx, int per_frame, int nregions, int64_t items,
																			int per_item_frame, int vec, int32_t *__restrict__ count,
																			int32_t *__restrict__ bbox, int64_t *__restrict__ mom, int64_t *__restrict__ wgt)
	{
		GmWalk<LDS, WEIGHTED> walk{};
		walk.all = GmOut{count, bbox, mom, wgt};
		walk_regions<LDS>(walk, frames, labels, w, npx, per_frame, nregions, items, per_item_frame, vec);
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
		const size_t lds = nregions <= GEOMETRY_LDS_MAX ? (size_t)nregions * GM_REGION_BYTES : 0;
		const WalkShape s = walk_launch_shape(npx, n, lds, cus);
		const int vec = walk_vec(npx, labels, frames);
		if (lds)
			region_geometry_accumulate<true, WEIGHTED>
				<<<s.grid, GM_BLOCK, lds, st>>>(labels, frames, (unsigned)w, npx, per_frame, nregions, s.items, s.per_item_frame, vec, count, bbox, mom, wgt);
		else
			region_geometry_accumulate<false, WEIGHTED>
				<<<s.grid, GM_BLOCK, 0, st>>>(labels, frames, (unsigned)w, npx, per_frame, nregions, s.items, s.per_item_frame, vec, count, bbox, mom, wgt);
	}

	hipError_t launch_region_geometry(const int32_t *labels, const uint16_t *frames, int w, int h, int n, int per_frame, int nregions, int32_t *count,
									  int32_t *bbox, int64_t *moments, int64_t *weighted, hipStream_t st)
	{
		if (n <= 0 || w <= 0 || h <= 0 || w > GM_MAX_SIDE || h > GM_MAX_SIDE || nregions <= 0 || (frames == nullptr) != (weighted == nullptr))
			return hipErrorInvalidValue;
		int cus = 0;
		const hipError_t e = cu_count(&cus);
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
