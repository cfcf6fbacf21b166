// Spatial rank filters on frame stacks - gfx950 (CDNA4): the element of a given rank in a centred rectangle size_y x size_x (odd, 1..15)
// around every pixel of uint16, uint8 and bool frames [n][h][w]: medians, percentiles, majority filters.  An extension without an upstream
// counterpart; the definition is in include/rir_amd_device.h (rir_rank_filter_device).  All integer, bit-exact.
//
// The window is always FULL: a position outside the image (its first `rows` rows) takes the value of the nearest pixel - coordinates are
// clamped, as scipy's mode="nearest" does.  That is the difference to both neighbours of this unit: median3x3_kernel (filter_kernels.hip)
// shrinks its window along the border, the morphology unit clips it (which for a min or a max is the same as replicating, so ranks 0 and
// n - 1 are handed to launch_morphology; there is no third min / max kernel).
//
//   rank_median_wave_kernel<T, R>  the medians of 3x3 and 5x5 on frames of even width: the pair tile of pair_tile.h, two columns per lane
//                                  in registers.
//   rank_tile_kernel<T, RY>        every other size and rank, and every odd width: a workgroup tile with its halo in LDS, as bit planes;
//                                  each thread selects the values of 8 outputs by a binary search on the value, counting the window's
//                                  cells below the candidate a window row at a time.
//
// Every load is a plain load at an address clamped into the image, every store goes through a plain pointer: frames of 2 GiB and more
// take the same path as small ones.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "morphology_kernels.h"
#include "pair_tile.h"
#include "rank_kernels.h"
#include "rank_select.h"

namespace rir
{
	// ---- medians of 3x3 and 5x5: two columns per lane, in registers ------------------------------------------------------------------------
	// A wave's pair tile (pair_tile.h) with one halo lane on each side: 2 pixels, enough for 3x3 and 5x5.
	//   3x3: each column triple is sorted once (min, median, max of 3); the median of 9 is med3(max of the three column minima, median of the
	//        three column medians, min of the three column maxima), as in median3x3_kernel - on pairs, 30 instructions per pair.
	//   5x5: the five shifted copies of every loaded row are kept (5 x (TY + 4) registers); the 25 values of an output go through the
	//        selection network of rank_select.h, 129 exchanges = 258 packed instructions per pair.
	// A lane's pair column with REPLICATED borders: v[i] = the pixels (2 xp, 2 xp + 1) of row ytop + i of an image of wp pairs x rows rows,
	// every coordinate clamped into the image - a pair left of the image is the first pixel of the row twice, a pair right of it the last
	// pixel twice.  The loads are unconditional, at clamped addresses (the shape of load_column's branch for frames of 2 GiB and more), and
	// all in flight together; the row offsets are wave-uniform.  x_edge (wave-uniform): some lane of the wave lies outside the image.
	template <int NR, class T>
	__device__ __forceinline__ void load_pairs_replicated(const typename PixelPair<T>::type *__restrict__ s, int wp, int rows, int xp, int ytop, bool x_edge,
														  uint32_t (&v)[NR])
	{
		const typename PixelPair<T>::type *col = s + nearest(xp, wp);
#pragma unroll
		for (int i = 0; i < NR; ++i)
			v[i] = PixelPair<T>::widen(col[(int64_t)nearest(ytop + i, rows) * wp]);
		if (x_edge)
		{
#pragma unroll
			for (int i = 0; i < NR; ++i)
				v[i] = xp < 0 ? (v[i] & 0xffffu) * 0x10001u : xp >= wp ? (v[i] >> 16) * 0x10001u : v[i];
		}
	}

	constexpr int rank_wave_ty(int r) { return r == 1 ? 16 : 8; }

	template <class T, int R>
	__global__ __launch_bounds__(256) void rank_median_wave_kernel(const T *__restrict__ src, T *__restrict__ dst, int w, int h, int rows)
	{
		static_assert(R == 1 || R == 2, "3x3 or 5x5");
		typedef PackedPair O;
		constexpr int TY = rank_wave_ty(R), NR = TY + 2 * R;
		typedef typename PixelPair<T>::type P;
		const int lane = threadIdx.x & 63;
		const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
		const PairTile<T, TY, 1> t(lane, wv, w);
		if (t.y0 >= h)
			return;
		const P *s = t.frame(src, w, h);
		P *d = t.frame(dst, w, h);
		const bool out_lane = lane >= 1 && lane < 63 && t.xp < t.wp;
		if (t.y0 < rows)
		{
			uint32_t v[NR], res[TY];
			load_pairs_replicated<NR, T>(s, t.wp, rows, t.xp, t.y0 - R, t.xp0 < 0 || t.xp0 + 63 >= t.wp, v);
			// (all 64 lanes take part in the shifts; what is shifted in at the wave's ends only ever reaches the two halo lanes)
			if constexpr (R == 1)
			{
#pragma unroll
				for (int j = 0; j < TY; ++j)
				{
					const uint32_t ab_lo = O::lo(v[j], v[j + 1]), ab_hi = O::hi(v[j], v[j + 1]);
					const uint32_t lo = O::lo(ab_lo, v[j + 2]), hi = O::hi(ab_hi, v[j + 2]), mi = O::hi(ab_lo, O::lo(ab_hi, v[j + 2]));
					const uint32_t lo_l = left_pair(lo, wave_shr1(lo)), lo_r = right_pair(lo, wave_shl1(lo));
					const uint32_t mi_l = left_pair(mi, wave_shr1(mi)), mi_r = right_pair(mi, wave_shl1(mi));
					const uint32_t hi_l = left_pair(hi, wave_shr1(hi)), hi_r = right_pair(hi, wave_shl1(hi));
					res[j] = rank_med3<O>(O::hi(O::hi(lo_l, lo), lo_r), rank_med3<O>(mi_l, mi, mi_r), O::lo(O::lo(hi_l, hi), hi_r));
				}
			}
			else
			{
				uint32_t a[5][NR]; // a[dx][i]: row i shifted by dx - 2 pixels
#pragma unroll
				for (int i = 0; i < NR; ++i)
				{
					a[2][i] = v[i];
					a[0][i] = wave_shr1(v[i]);
					a[4][i] = wave_shl1(v[i]);
					a[1][i] = left_pair(v[i], a[0][i]);
					a[3][i] = right_pair(v[i], a[4][i]);
				}
#pragma unroll
				for (int j = 0; j < TY; ++j)
				{
					uint32_t in[25];
#pragma unroll
					for (int dy = 0; dy < 5; ++dy)
#pragma unroll
						for (int dx = 0; dx < 5; ++dx)
							in[dy * 5 + dx] = a[dx][j + dy];
					res[j] = rank_median<O, 25>(in);
				}
			}
			t.store(d, res, rows, out_lane);
		}
		t.copy_rest(s, d, h, rows, out_lane);
	}

	// ---- every other size and rank: a workgroup tile in LDS, as bit planes --------------------------------------------------------------
	// A workgroup owns RT_TW x RT_TH outputs and loads them with a halo of (size_x / 2, size_y / 2), each cell from the nearest pixel of the
	// image (pair_tile.h's nearest(), as in morph_tile_kernel's loader, whose cells are here what the definition asks for): unconditional
	// loads, all of a wave's in flight together.  The cells are not kept: a wave turns each row of 64 cells into one 64-bit mask per value
	// bit (a compare across the wave is that mask), so LDS holds the region as bit PLANES - plane b, row r: RT_WORDS dwords, bit x = bit b of the cell at column x.
	// A thread then finds the values of its outputs by a binary search on the value, most significant bit first.  With c = v | bit, the bit
	// is set exactly when at most `rank` cells of the window lie below c; those are the `below` cells known to lie below v's prefix plus,
	// among the cells whose higher bits equal that prefix (the candidates, a mask of size_x bits per window row), the ones whose bit b is 0.
	// A window row of a plane is 15 bits at most of two adjacent dwords: one funnel shift extracts it, an and-not and a population count
	// count its zeros among the candidates, an xor and an and narrow the candidates - 4 instructions per window ROW, output and step where
	// counting cell by cell takes 2 per window CELL.  After the last bit v is the largest value with at most `rank` cells below it, which is
	// the cell of that rank; ties need no care.  Integer instructions only, every register index a compile-time constant (RY = size_y / 2
	// is a template parameter).  A thread owns 8 vertically adjacent outputs and finds them in two strips of RT_STRIP; the outputs of a
	// strip share its extracted rows.  `top` is the highest value bit: 15 for uint16, 7 for uint8, 0 for bool (one step: the zeros against the rank).
	constexpr int RT_TW = 64, RT_TH = 32, RT_STRIP = 4, RT_WORDS = 3; // (64 + 14 columns: 78 bits of 96)

	template <class T, int RY>
	__global__ __launch_bounds__(256) void rank_tile_kernel(const T *__restrict__ src, T *__restrict__ dst, int w, int h, int rows, int rx, int rank,
															 int top)
	{
		constexpr int RH = RT_TH + 2 * RY, SY = 2 * RY + 1, NW = RT_STRIP + 2 * RY, LR = (RH + 3) / 4; // LR: region rows a wave loads
		static_assert(RT_TH == 4 * 2 * RT_STRIP, "four waves, two strips per thread");
		__shared__ uint32_t planes[16 * RH * RT_WORDS];
		const int lane = threadIdx.x & 63;
		const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
		const TileId id = tile_decode<false>(); // (vertically adjacent tiles share their halo rows)
		const int x0 = id.bx * RT_TW, y0 = id.by * RT_TH;
		const int64_t fbase = (int64_t)id.n * w * h;
		const T *s = src + fbase;
		T *d = dst + fbase;
		uint32_t v[2 * RT_STRIP];
#pragma unroll
		for (int k = 0; k < 2 * RT_STRIP; ++k)
			v[k] = 0;
		if (y0 < rows) // (the same for the whole workgroup)
		{
			// region row r = wv + 4 i of this wave: columns `lane` and 64 + `lane` (the second one a halo column for the first lanes only)
			const int xa = nearest(x0 - rx + lane, w), xb = nearest(x0 - rx + 64 + lane, w);
			const bool second = lane < 2 * rx;
			uint32_t a[LR], bq[LR];
#pragma unroll
			for (int i = 0; i < LR; ++i)
			{
				const T *row = s + (int64_t)nearest(y0 - RY + wv + 4 * i, rows) * w;
				a[i] = row[xa];
				bq[i] = row[xb];
			}
#pragma unroll
			for (int i = 0; i < LR; ++i)
			{
				const int r = wv + 4 * i;
				if (r < RH)
					for (int b = 0; b <= top; ++b)
					{
						const uint64_t m0 = __builtin_amdgcn_ballot_w64(((a[i] >> b) & 1u) != 0);
						const uint64_t m1 = __builtin_amdgcn_ballot_w64(second && ((bq[i] >> b) & 1u) != 0);
						if (lane < RT_WORDS)
							planes[(b * RH + r) * RT_WORDS + lane] = lane == 0 ? (uint32_t)m0 : lane == 1 ? (uint32_t)(m0 >> 32) : (uint32_t)m1;
					}
			}
			__syncthreads();
			const uint32_t full = (1u << (2 * rx + 1)) - 1u;
			const int word = lane >> 5, shift = lane & 31;
#pragma unroll
			for (int half = 0; half < 2; ++half)
			{
				const int r0 = wv * 2 * RT_STRIP + half * RT_STRIP; // the strip's first output row = its first window row in the region
				uint32_t cand[RT_STRIP][SY], below[RT_STRIP], val[RT_STRIP];
#pragma unroll
				for (int k = 0; k < RT_STRIP; ++k)
				{
					below[k] = 0;
					val[k] = 0;
#pragma unroll
					for (int j = 0; j < SY; ++j)
						cand[k][j] = full;
				}
				for (int b = top; b >= 0; --b)
				{
					const uint32_t *p = planes + (b * RH + r0) * RT_WORDS + word;
					uint32_t bits[NW]; // window row wr of the strip: bit dx = bit b of the cell dx columns into the window
#pragma unroll
					for (int wr = 0; wr < NW; ++wr)
						bits[wr] = __builtin_amdgcn_alignbit(p[wr * RT_WORDS + 1], p[wr * RT_WORDS], shift);
#pragma unroll
					for (int k = 0; k < RT_STRIP; ++k) // (output k's window is the rows k .. k + 2 RY of the strip)
					{
						uint32_t zeros = 0;
#pragma unroll
						for (int j = 0; j < SY; ++j)
							zeros += __builtin_popcount(~bits[k + j] & cand[k][j]);
						const bool one = below[k] + zeros <= (uint32_t)rank;
						const uint32_t flip = one ? 0u : ~0u;
#pragma unroll
						for (int j = 0; j < SY; ++j)
							cand[k][j] &= bits[k + j] ^ flip;
						below[k] += one ? zeros : 0u;
						val[k] |= one ? 1u << b : 0u;
					}
				}
#pragma unroll
				for (int k = 0; k < RT_STRIP; ++k)
					v[half * RT_STRIP + k] = val[k];
			}
		}
		const int x = x0 + lane;
		if (x >= w)
			return;
#pragma unroll
		for (int k = 0; k < 2 * RT_STRIP; ++k)
		{
			const int y = y0 + wv * 2 * RT_STRIP + k;
			if (y < h)
				d[(int64_t)y * w + x] = y < rows ? (T)v[k] : s[(int64_t)y * w + x];
		}
	}

	// ---- launchers ---------------------------------------------------------------------------------------------------------------------
	template <class T, int R>
	static void launch_median_wave(const T *src, T *dst, int w, int h, int n, int rows, hipStream_t st)
	{
		hipLaunchKernelGGL((rank_median_wave_kernel<T, R>), (pair_wave_grid<rank_wave_ty(R), 1>(w / 2, h, n)), dim3(256), 0, st, src, dst, w, h, rows);
	}

	template <class T, int RY>
	static void launch_tile(const T *src, T *dst, int w, int h, int n, int rows, int rx, int rank, int top, hipStream_t st)
	{
		dim3 block(256), grid((unsigned)((w + RT_TW - 1) / RT_TW), (unsigned)((h + RT_TH - 1) / RT_TH), (unsigned)n);
		hipLaunchKernelGGL((rank_tile_kernel<T, RY>), grid, block, 0, st, src, dst, w, h, rows, rx, rank, top);
	}

	template <class T>
	static hipError_t launch_rank_t(const T *src, T *dst, int w, int h, int nframes, int rank, int size_x, int size_y, int rows, int top, hipStream_t st)
	{
		// the pair kernels: the median of a 3x3 or 5x5 square on rows of whole, aligned pairs
		const bool pairs = size_x == size_y && (size_x == 3 || size_x == 5) && rank == size_x * size_y / 2 && rows_of_pairs(src, dst, w);
		const int rx = size_x / 2;
		return for_frame_chunks(src, dst, w, h, nframes, [=](const T *s, T *d, int n) {
			if (pairs && size_x == 3)
				launch_median_wave<T, 1>(s, d, w, h, n, rows, st);
			else if (pairs)
				launch_median_wave<T, 2>(s, d, w, h, n, rows, st);
			else
				switch (size_y / 2)
				{
				case 0:
					launch_tile<T, 0>(s, d, w, h, n, rows, rx, rank, top, st);
					break;
				case 1:
					launch_tile<T, 1>(s, d, w, h, n, rows, rx, rank, top, st);
					break;
				case 2:
					launch_tile<T, 2>(s, d, w, h, n, rows, rx, rank, top, st);
					break;
				case 3:
					launch_tile<T, 3>(s, d, w, h, n, rows, rx, rank, top, st);
					break;
				case 4:
					launch_tile<T, 4>(s, d, w, h, n, rows, rx, rank, top, st);
					break;
				case 5:
					launch_tile<T, 5>(s, d, w, h, n, rows, rx, rank, top, st);
					break;
				case 6:
					launch_tile<T, 6>(s, d, w, h, n, rows, rx, rank, top, st);
					break;
				default:
					launch_tile<T, 7>(s, d, w, h, n, rows, rx, rank, top, st);
					break;
				}
		});
	}

	hipError_t launch_rank_filter(int type, const void *src, void *dst, int w, int h, int nframes, int rank, int size_x, int size_y, int rows,
								  hipStream_t st)
	{
		// the two extreme ranks are the min and the max, which a replicated pixel does not change: the morphology unit's clipped windows
		if (rank == 0 || rank == size_x * size_y - 1)
			return launch_morphology(type, src, dst, w, h, nframes, rank == 0 ? MORPH_ERODE : MORPH_DILATE, size_x, size_y, rows, st);
		const int top = type == 'H' ? 15 : type == 'B' ? 7 : 0; // the highest value bit
		return with_pixel_type(type, src, dst, [=](auto *s, auto *d) { return launch_rank_t(s, d, w, h, nframes, rank, size_x, size_y, rows, top, st); });
	}
} // namespace rir
