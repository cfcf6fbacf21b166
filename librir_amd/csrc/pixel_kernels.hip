// Per-pixel statistics over time of a uint16 frame stack (the definition is with rir_pixel_stats_device, include/rir_amd_device.h).  Two kernels:
//
//   pixel_stats_slab  one workgroup per (tile of PS_TILE pixels, slab of frames).  A lane owns 8 adjacent pixels (one 16-byte load per frame);
//                     the four waves take the same pixels and every fourth frame of the slab each (walk_frames, time_walk.h), and keep per
//                     pixel a 32-bit sum, a 64-bit sum of squares and two 32-bit keys (value << 16 | frame index in the slab, the index
//                     complemented for the maximum so that the lowest index wins a tie).  The waves are combined in LDS, after which
//                     thread t holds pixels t and t + 256 of the tile: the stores are one element a lane, whatever the alignment.  With one
//                     slab (DIRECT) these go into the outputs, merged with what they hold when accumulating; else into the workspace.
//   pixel_stats_fold  (more than one slab) one thread a pixel walks the slabs' partials in order and writes or merges the outputs.
//
// Every combination is an integer add, a min / max of keys or a compare in a fixed order: no floating point, no atomics, nothing that
// depends on the order the workgroups run in.
#include <algorithm>

#include "pixel_kernels.h"
#include "time_walk.h"

namespace rir
{
	constexpr int PS_BLOCK = 256;
	constexpr int PS_WAVES = PS_BLOCK / 64;	  // the waves split the frames of a slab
	constexpr int PS_TILE = TW_TILE;		  // pixels per workgroup: its waves take the same ones
	constexpr int PS_SLAB_MAX = 65536;		  // frames per slab at most: the index fits 16 bits of a key and the sum 32 bits
	constexpr int PS_SLAB_MIN = 256;		  // frames per slab at least (unless the stack is shorter): bounds the partials' traffic
	static_assert((long long)PS_SLAB_MAX * 65535 < (1ll << 32), "a slab's sum fits 32 bits");
	static_assert(PS_TILE == 2 * PS_BLOCK, "after the LDS combine a thread holds two pixels of the tile");

	struct PsOut
	{
		int64_t *sum, *sumsq;
		int32_t *vmin, *vmax, *argmin, *argmax;
	};

	struct PsWork // partials [slabs][npx]
	{
		unsigned long long *sq;
		unsigned *sum, *kmin, *kmax;
	};

	struct PsAcc // a lane's 8 pixels over its wave's frames
	{
		unsigned sum[TW_PX];
		unsigned long long sq[TW_PX];
		unsigned kmin[TW_PX]; // min of value << 16 | index
		unsigned kmax[TW_PX]; // max of value << 16 | (0xFFFF - index)
	};

	// One frame.  PIN (the 16-byte loads): the sums stay one frame's adds - left free, the frames of a set are summed first, behind one wait
	// for all of them, at 1.5 to 1.7 times the registers.  Not with the 2-byte loads, where pinned sums have the second set's loads wait pair by pair.
	template <bool SUMS, bool EXTR, bool PIN>
	__device__ __forceinline__ void ps_frame(PsAcc &a, tw_v4u x, unsigned idx)
	{
		const unsigned idxc = 0xFFFFu - idx;
		if constexpr (SUMS && PIN)
		{
#pragma unroll
			for (int j = 0; j < TW_PX; ++j)
				asm("" : "+v"(a.sq[j]), "+v"(a.sum[j]));
		}
#pragma unroll
		for (int j = 0; j < 4; ++j)
		{
			const unsigned w = x[j], lo = w & 0xFFFFu, hi = w >> 16;
			if constexpr (SUMS)
			{
				a.sum[2 * j] += lo;
				a.sum[2 * j + 1] += hi;
				a.sq[2 * j] += (unsigned long long)(lo * lo); // 65535^2 < 2^32
				a.sq[2 * j + 1] += (unsigned long long)(hi * hi);
			}
			if constexpr (EXTR)
			{
				a.kmin[2 * j] = min(a.kmin[2 * j], w << 16 | idx);
				a.kmin[2 * j + 1] = min(a.kmin[2 * j + 1], (w & 0xFFFF0000u) | idx);
				a.kmax[2 * j] = max(a.kmax[2 * j], w << 16 | idxc);
				a.kmax[2 * j + 1] = max(a.kmax[2 * j + 1], (w & 0xFFFF0000u) | idxc);
			}
		}
	}

	// Write (or merge into) the outputs of pixel i: the sums, and the extremes with the times they were first seen at.
	template <bool SUMS, bool EXTR>
	__device__ __forceinline__ void ps_commit(const PsOut &o, int64_t i, int accumulate, unsigned long long sum, unsigned long long sq, int vmin,
											  int tmin, int vmax, int tmax)
	{
		if constexpr (SUMS)
		{
			if (accumulate)
			{
				sum += (unsigned long long)o.sum[i];
				sq += (unsigned long long)o.sumsq[i];
			}
			o.sum[i] = (int64_t)sum;
			o.sumsq[i] = (int64_t)sq;
		}
		if constexpr (EXTR)
		{
			if (accumulate)
			{
				const int omin = o.vmin[i], otmin = o.argmin[i], omax = o.vmax[i], otmax = o.argmax[i];
				if (omin >= 0 && (omin < vmin || (omin == vmin && otmin < tmin))) // -1: the empty state
					vmin = omin, tmin = otmin;
				if (omax >= 0 && (omax > vmax || (omax == vmax && otmax < tmax)))
					vmax = omax, tmax = otmax;
			}
			o.vmin[i] = vmin;
			o.argmin[i] = tmin;
			o.vmax[i] = vmax;
			o.argmax[i] = tmax;
		}
	}

	template <bool SUMS, bool EXTR, bool VEC, bool DIRECT>
	__global__ __launch_bounds__(PS_BLOCK) void pixel_stats_slab(const uint16_t *__restrict__ frames, int64_t npx, int n, int per_slab, int t0,
																 int accumulate, PsOut out, PsWork work)
	{
		// one array, used for the sums (12 bytes a wave and pixel) and then for the keys (8 bytes)
		__shared__ unsigned long long lds[PS_WAVES * PS_TILE * (SUMS ? 12 : 8) / 8];
		const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
		const int64_t f0 = (int64_t)blockIdx.y * per_slab, f1 = min(f0 + per_slab, (int64_t)n);
		const int cnt = f1 - f0 > wave ? (int)((f1 - f0 - wave + PS_WAVES - 1) / PS_WAVES) : 0; // this wave's frames: f0 + wave + PS_WAVES * k
		const int64_t tile = (int64_t)blockIdx.x * PS_TILE, p = tile + lane * TW_PX;

		unsigned off[TW_PX]; // what is loaded for a pixel past the end is never stored
		tw_offsets<VEC>(off, p, npx, npx);
		PsAcc a;
#pragma unroll
		for (int j = 0; j < TW_PX; ++j)
		{
			a.sum[j] = 0;
			a.sq[j] = 0;
			a.kmin[j] = 0xFFFFFFFFu;
			a.kmax[j] = 0;
		}
		walk_frames<VEC>( // the frame of step k is clamped to the wave's last one
			cnt, off, [&](int k) { return frames + (f0 + wave + (int64_t)PS_WAVES * min(k, cnt - 1)) * npx; },
			[&](tw_v4u x, int k) { ps_frame<SUMS, EXTR, VEC>(a, x, (unsigned)(wave + PS_WAVES * k)); });

		// combine the waves: afterwards thread t holds pixels t and t + 256 of the tile
		unsigned long long rsum[2] = {0, 0}, rsq[2] = {0, 0};
		unsigned rmin[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, rmax[2] = {0, 0};
		const int at = wave * PS_TILE + lane * TW_PX;
		if constexpr (SUMS)
		{
			unsigned long long *lsq = lds;
			unsigned *lsum = reinterpret_cast<unsigned *>(lds + PS_WAVES * PS_TILE);
#pragma unroll
			for (int j = 0; j < TW_PX; ++j)
			{
				lsq[at + j] = a.sq[j];
				lsum[at + j] = a.sum[j];
			}
			__syncthreads();
#pragma unroll
			for (int q = 0; q < 2; ++q)
#pragma unroll
				for (int w = 0; w < PS_WAVES; ++w)
				{
					rsum[q] += lsum[w * PS_TILE + q * PS_BLOCK + threadIdx.x];
					rsq[q] += lsq[w * PS_TILE + q * PS_BLOCK + threadIdx.x];
				}
			if constexpr (EXTR)
				__syncthreads();
		}
		if constexpr (EXTR)
		{
			unsigned *lmin = reinterpret_cast<unsigned *>(lds), *lmax = lmin + PS_WAVES * PS_TILE;
#pragma unroll
			for (int j = 0; j < TW_PX; ++j)
			{
				lmin[at + j] = a.kmin[j];
				lmax[at + j] = a.kmax[j];
			}
			__syncthreads();
#pragma unroll
			for (int q = 0; q < 2; ++q)
#pragma unroll
				for (int w = 0; w < PS_WAVES; ++w)
				{
					rmin[q] = min(rmin[q], lmin[w * PS_TILE + q * PS_BLOCK + threadIdx.x]);
					rmax[q] = max(rmax[q], lmax[w * PS_TILE + q * PS_BLOCK + threadIdx.x]);
				}
		}
#pragma unroll
		for (int q = 0; q < 2; ++q)
		{
			const int64_t i = tile + q * PS_BLOCK + threadIdx.x;
			if (i >= npx)
				continue;
			if constexpr (DIRECT) // one slab: f0 is 0, the keys' indices count from t0
				ps_commit<SUMS, EXTR>(out, i, accumulate, rsum[q], rsq[q], (int)(rmin[q] >> 16), t0 + (int)(rmin[q] & 0xFFFFu), (int)(rmax[q] >> 16),
									  t0 + (int)(0xFFFFu - (rmax[q] & 0xFFFFu)));
			else
			{
				const int64_t c = (int64_t)blockIdx.y * npx + i;
				if constexpr (SUMS)
				{
					work.sum[c] = (unsigned)rsum[q];
					work.sq[c] = rsq[q];
				}
				if constexpr (EXTR)
				{
					work.kmin[c] = rmin[q];
					work.kmax[c] = rmax[q];
				}
			}
		}
	}

	template <bool SUMS, bool EXTR>
	__global__ __launch_bounds__(PS_BLOCK) void pixel_stats_fold(PsWork work, int64_t npx, int slabs, int per_slab, int t0, int accumulate, PsOut out)
	{
		const int64_t i = (int64_t)blockIdx.x * PS_BLOCK + threadIdx.x;
		if (i >= npx)
			return;
		unsigned long long sum = 0, sq = 0;
		int vmin = 65536, tmin = 0, vmax = -1, tmax = 0;
		for (int s = 0; s < slabs; ++s) // in time order: an equal value in a later slab does not replace the earlier one
		{
			const int64_t c = (int64_t)s * npx + i;
			if constexpr (SUMS)
			{
				sum += __builtin_nontemporal_load(work.sum + c);
				sq += __builtin_nontemporal_load(work.sq + c);
			}
			if constexpr (EXTR)
			{
				const unsigned kmin = __builtin_nontemporal_load(work.kmin + c), kmax = __builtin_nontemporal_load(work.kmax + c);
				const int base = t0 + s * per_slab;
				if ((int)(kmin >> 16) < vmin)
					vmin = (int)(kmin >> 16), tmin = base + (int)(kmin & 0xFFFFu);
				if ((int)(kmax >> 16) > vmax)
					vmax = (int)(kmax >> 16), tmax = base + (int)(0xFFFFu - (kmax & 0xFFFFu));
			}
		}
		ps_commit<SUMS, EXTR>(out, i, accumulate, sum, sq, vmin, tmin, vmax, tmax);
	}

	PixelStatsPlan pixel_stats_plan(int64_t npx, int n)
	{
		const TimeSlabs t = time_slab_plan(npx, n, PS_SLAB_MIN, PS_SLAB_MAX);
		return PixelStatsPlan{t.slabs, t.per_slab};
	}

	size_t pixel_stats_workspace(int64_t npx, int n)
	{
		const PixelStatsPlan plan = pixel_stats_plan(npx, n);
		return plan.slabs > 1 ? (size_t)plan.slabs * (size_t)npx * 20 : 8;
	}

	namespace
	{
		template <bool SUMS, bool EXTR>
		void ps_launch(const uint16_t *frames, int64_t npx, int n, int t0, int accumulate, const PsOut &out, void *work, hipStream_t st)
		{
			const PixelStatsPlan plan = pixel_stats_plan(npx, n);
			const size_t cells = (size_t)plan.slabs * (size_t)npx;
			PsWork wk;
			wk.sq = static_cast<unsigned long long *>(work);
			wk.sum = reinterpret_cast<unsigned *>(wk.sq + cells);
			wk.kmin = wk.sum + cells;
			wk.kmax = wk.kmin + cells;
			const bool vec = frames_are_16_byte_aligned(npx, frames);
			const dim3 grid((unsigned)((npx + PS_TILE - 1) / PS_TILE), (unsigned)plan.slabs);
			if (plan.slabs == 1)
			{
				if (vec)
					pixel_stats_slab<SUMS, EXTR, true, true><<<grid, PS_BLOCK, 0, st>>>(frames, npx, n, plan.per_slab, t0, accumulate, out, wk);
				else
					pixel_stats_slab<SUMS, EXTR, false, true><<<grid, PS_BLOCK, 0, st>>>(frames, npx, n, plan.per_slab, t0, accumulate, out, wk);
				return;
			}
			if (vec)
				pixel_stats_slab<SUMS, EXTR, true, false><<<grid, PS_BLOCK, 0, st>>>(frames, npx, n, plan.per_slab, t0, accumulate, out, wk);
			else
				pixel_stats_slab<SUMS, EXTR, false, false><<<grid, PS_BLOCK, 0, st>>>(frames, npx, n, plan.per_slab, t0, accumulate, out, wk);
			pixel_stats_fold<SUMS, EXTR>
				<<<(unsigned)((npx + PS_BLOCK - 1) / PS_BLOCK), PS_BLOCK, 0, st>>>(wk, npx, plan.slabs, plan.per_slab, t0, accumulate, out);
		}
	} // namespace

	hipError_t launch_pixel_stats(const uint16_t *frames, int64_t npx, int n, int t0, int accumulate, int64_t *sum, int64_t *sumsq, int32_t *vmin,
								  int32_t *vmax, int32_t *argmin, int32_t *argmax, void *work, hipStream_t st)
	{
		const bool sums = sum != nullptr, extr = vmin != nullptr;
		if (n <= 0 || npx <= 0 || (!sums && !extr))
			return hipErrorInvalidValue;
		const PsOut out{sum, sumsq, vmin, vmax, argmin, argmax};
		if (sums && extr)
			ps_launch<true, true>(frames, npx, n, t0, accumulate, out, work, st);
		else if (sums)
			ps_launch<true, false>(frames, npx, n, t0, accumulate, out, work, st);
		else
			ps_launch<false, true>(frames, npx, n, t0, accumulate, out, work, st);
		return hipGetLastError();
	}
} // namespace rir
