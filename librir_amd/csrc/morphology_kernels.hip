// Flat grey-level morphology on frame stacks - gfx950 (CDNA4): erode, dilate, open, close, top-hat, black-hat, gradient with a centred
// rectangle size_y x size_x (odd, 1..15) on uint16, uint8 and bool frames [n][h][w].  An extension without an upstream counterpart; the
// definition is in include/rir_amd_device.h (rir_morphology_device).  All integer, bit-exact.
//
// Every call is ONE launch that reads the stack once and writes it once: the two stages of open / close (and the difference the hats and
// the gradient take) stay in registers or LDS.  The window is CLIPPED to the image (its first `rows` rows), never padded: a position
// outside the image is neutral for whichever stage looks at it - for the SECOND stage too, where the first stage's value at such a
// position (a min / max over the clamped part of a window that has no centre) must not be seen.
//
//   morph_wave_kernel<T, R, OP>  squares 3x3, 5x5, 7x7 on frames of even width: the pair tile of pair_tile.h, two columns per lane in
//                                registers.
//   morph_tile_kernel<T, RMAX>   every other size and every odd width: a workgroup tile with its halo in LDS, a row pass and a column pass
//                                per stage, radii as run-time bounds (<= RMAX = 1, 3, 5 or 7) clipped to the image.
//
// Frames of 2 GiB and more are correct in both: the tile kernel uses plain 64-bit indexed loads, the wave kernel's loader (load_column)
// falls back to them, and both store through plain pointers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "morphology_kernels.h"
#include "pair_tile.h"

namespace rir
{
	constexpr bool morph_two_stages(int op) { return op == MORPH_OPEN || op == MORPH_CLOSE || op == MORPH_TOPHAT || op == MORPH_BLACKHAT; }

	// ---- squares 3, 5, 7: two columns per lane, in registers ------------------------------------------------------------------------------
	// A wave's pair tile (pair_tile.h) is loaded with HALO rows above and below - the frame read as an image of w / 2 dwords through
	// load_column, which gives 0 for every pair outside the image (w is even: a pair is inside or outside as a whole).  A stage is a vertical
	// min / max over 2R + 1 registers, then a horizontal one over the pairs shifted by -R .. R pixels.
	// HALO = R (one stage) or 2R (two) pixels on every side; the outer ceil(HALO / 2) lanes of each side have no output.
	// Stores are plain, not streaming: a tile row is 248 / 240 / 232 bytes, so neighbouring tiles share 128-byte lines, which the default
	// policy completes in L2 (with the streaming policy every partial line goes to memory on its own: see the fused chain's store policy).
	constexpr int MORPH_TY = 16; // output rows per wave tile

	constexpr int morph_halo(int r, int op) { return morph_two_stages(op) ? 2 * r : r; }
	constexpr int morph_halo_lanes(int r, int op) { return (morph_halo(r, op) + 1) / 2; }

	// one flat (2R + 1)^2 stage: N rows of pairs in, N - 2R rows out (all 64 lanes take part in the shifts; what is shifted in at the wave's
	// ends only ever reaches halo lanes)
	template <bool MAX, int R, int N>
	__device__ __forceinline__ void morph_stage(const uint32_t (&a)[N], uint32_t (&o)[N - 2 * R])
	{
#pragma unroll
		for (int j = 0; j < N - 2 * R; ++j)
		{
			uint32_t c = a[j];
#pragma unroll
			for (int d = 1; d <= 2 * R; ++d)
				c = pk_pick<MAX>(c, a[j + d]);
			const uint32_t prev = wave_shr1(c), next = wave_shl1(c); // columns (x - 2, x - 1) and (x + 2, x + 3)
			uint32_t m = pk_pick<MAX>(c, pk_pick<MAX>(left_pair(c, prev), right_pair(c, next)));
			if constexpr (R >= 2)
				m = pk_pick<MAX>(m, pk_pick<MAX>(prev, next));
			if constexpr (R >= 3)
			{
				const uint32_t prev2 = wave_shr1(prev), next2 = wave_shl1(next);
				m = pk_pick<MAX>(m, pk_pick<MAX>(left_pair(prev, prev2), right_pair(next, next2)));
			}
			o[j] = m;
		}
	}

	// rows ytop .. ytop + N - 1 of the lane's pair: `fill` wherever the position lies outside the image
	template <int N>
	__device__ __forceinline__ void fill_outside(uint32_t (&a)[N], int ytop, int rows, bool xin, uint32_t fill)
	{
#pragma unroll
		for (int i = 0; i < N; ++i)
			a[i] = (xin && ytop + i >= 0 && ytop + i < rows) ? a[i] : fill;
	}

	template <class T, int R, int OP>
	__global__ __launch_bounds__(256) void morph_wave_kernel(const T *__restrict__ src, T *__restrict__ dst, int w, int h, int rows)
	{
		constexpr int TY = MORPH_TY, HALO = morph_halo(R, OP), HL = morph_halo_lanes(R, OP), NR = TY + 2 * HALO;
		constexpr uint32_t TOP = 0xffffffffu; // above every pixel of a pair: neutral for a min
		typedef typename PixelPair<T>::type P;
		const int lane = threadIdx.x & 63;
		const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
		const PairTile<T, TY, HL> t(lane, wv, w);
		const int y0 = t.y0;
		if (y0 >= h)
			return;
		const P *s = t.frame(src, w, h);
		P *d = t.frame(dst, w, h);
		const bool xin = t.xp >= 0 && t.xp < t.wp;
		const bool out_lane = lane >= HL && lane < 64 - HL && t.xp < t.wp;
		if (y0 < rows)
		{
			raw_px_t<P> raw[NR];
			// (the image is the first `rows` rows: what lies below reads as outside)
			const bool inside = load_column<NR, P, true, true>(s, t.wp, rows, t.xp0, lane, y0 - HALO, raw);
			uint32_t v[NR]; // 0 outside the image: neutral for a max
#pragma unroll
			for (int i = 0; i < NR; ++i)
				v[i] = PixelPair<T>::widen(raw[i]);
			uint32_t res[TY];
			if constexpr (OP == MORPH_DILATE)
				morph_stage<true, R, NR>(v, res);
			else if constexpr (OP == MORPH_ERODE || OP == MORPH_GRADIENT)
			{
				uint32_t lo[NR];
#pragma unroll
				for (int i = 0; i < NR; ++i)
					lo[i] = v[i];
				if (!inside)
					fill_outside(lo, y0 - HALO, rows, xin, TOP);
				morph_stage<false, R, NR>(lo, res);
				if constexpr (OP == MORPH_GRADIENT)
				{
					uint32_t hi[TY];
					morph_stage<true, R, NR>(v, hi);
#pragma unroll
					for (int j = 0; j < TY; ++j)
						res[j] = pk_sub(hi[j], res[j]);
				}
			}
			else
			{
				// two stages.  The first stage's values at positions outside the image are replaced by what is neutral for the second.
				constexpr bool MIN_FIRST = OP == MORPH_OPEN || OP == MORPH_TOPHAT;
				uint32_t a[NR], b[NR - 2 * R];
#pragma unroll
				for (int i = 0; i < NR; ++i)
					a[i] = v[i];
				if (MIN_FIRST && !inside)
					fill_outside(a, y0 - HALO, rows, xin, TOP);
				morph_stage<!MIN_FIRST, R, NR>(a, b);
				if (!inside)
					fill_outside(b, y0 - HALO + R, rows, xin, MIN_FIRST ? 0u : TOP);
				morph_stage<MIN_FIRST, R, NR - 2 * R>(b, res);
#pragma unroll
				for (int j = 0; j < TY; ++j)
				{
					if constexpr (OP == MORPH_TOPHAT)
						res[j] = pk_sub(v[j + HALO], res[j]);
					else if constexpr (OP == MORPH_BLACKHAT)
						res[j] = pk_sub(res[j], v[j + HALO]);
				}
			}
			t.store(d, res, rows, out_lane);
		}
		t.copy_rest(s, d, h, rows, out_lane);
	}

	// ---- every other size: a workgroup tile in LDS ------------------------------------------------------------------------------------
	// A workgroup owns G_TW x G_TH outputs and loads them with a halo of stages x radius on every side into LDS (uint16 cells for both
	// pixel types).  A stage is a row pass and a column pass between LDS buffers; every pass takes its min / max over the window CLIPPED to
	// the image, as the definition says - positions outside the image are never read, so no stage needs a neutral value - and to the loaded
	// region: what the region cuts off spoils one radius of halo per pass, which is the halo that was loaded for it.
	// A pass of radius r reads 2 RMAX + 1 cells whatever r <= RMAX is (RMAX = 1, 3, 5, 7 by the larger radius): the window's cells at
	// c - RMAX .. c + RMAX CLAMPED into the clipped window.  Cells read twice change no min / max, the reads do not depend on each other -
	// they are all in flight together, where a loop from the window's first cell to its last waits for every cell in turn (9x9 erode:
	// 1.44 -> 0.90 ms per 256 frames 640x512) - and their addresses never leave the region.  A pass of radius 0 is skipped.
	// Three buffers of the region's size, dynamic LDS: 92 x 60 cells each at most (15x15 in two stages: 33 120 bytes, four workgroups per
	// CU), 72 x 40 for a 9x9 erosion (17 280 bytes: the eight workgroups a CU has waves for) - the phases of a workgroup are separated by
	// barriers, and what hides one workgroup's wait is the other workgroups of the CU.
	constexpr int G_TW = 64, G_TH = 32;
	// cells of the region of a tile (its rows are stored back to back), rounded up to whole dwords
	__host__ __device__ constexpr int tile_cells(int op, int rx, int ry)
	{
		const int stages = morph_two_stages(op) ? 2 : 1;
		return ((G_TW + 2 * stages * rx) * (G_TH + 2 * stages * ry) + 1) & ~1;
	}

	template <bool MAX>
	__device__ __forceinline__ uint32_t pick(uint32_t a, uint32_t b)
	{
		return MAX ? max(a, b) : min(a, b);
	}

	// out[r][c] = min / max of in[r][c - rx .. c + rx], columns clipped to the image (region column c is image column gx0 + c) and the region
	// (a column outside the image has an empty window, lo > hi: it gets some cell of the region, and no clipped window reads it)
	template <bool MAX, int RMAX>
	__device__ __forceinline__ void row_pass(const uint16_t *in, uint16_t *out, int rw, int rh, int gx0, int w, int rx, int tid)
	{
		for (int c = tid & 63; c < rw; c += 64)
		{
			const int lo = max(max(c - rx, 0), -gx0), hi = min(min(c + rx, rw - 1), w - 1 - gx0);
			for (int r = tid >> 6; r < rh; r += 4)
			{
				uint32_t m = in[r * rw + min(max(c, lo), hi)];
#pragma unroll
				for (int d = 1; d <= RMAX; ++d)
				{
					m = pick<MAX>(m, in[r * rw + min(max(c - d, lo), hi)]);
					m = pick<MAX>(m, in[r * rw + min(max(c + d, lo), hi)]);
				}
				out[r * rw + c] = (uint16_t)m;
			}
		}
	}
	// out[r][c] = min / max of in[r - ry .. r + ry][c], rows clipped to the image (region row r is image row gy0 + r) and the region
	template <bool MAX, int RMAX>
	__device__ __forceinline__ void col_pass(const uint16_t *in, uint16_t *out, int rw, int rh, int gy0, int rows, int ry, int tid)
	{
		for (int r = tid >> 6; r < rh; r += 4)
		{
			const int lo = max(max(r - ry, 0), -gy0), hi = min(min(r + ry, rh - 1), rows - 1 - gy0); // (0 <= hi: the tile starts inside the image)
			for (int c = tid & 63; c < rw; c += 64)
			{
				uint32_t m = in[min(max(r, lo), hi) * rw + c];
#pragma unroll
				for (int d = 1; d <= RMAX; ++d)
				{
					m = pick<MAX>(m, in[min(max(r - d, lo), hi) * rw + c]);
					m = pick<MAX>(m, in[min(max(r + d, lo), hi) * rw + c]);
				}
				out[r * rw + c] = (uint16_t)m;
			}
		}
	}

	struct TileGeometry
	{
		int rw, rh, gx0, gy0, w, rows, rx, ry, tid;
	};
	// One stage from `in` into one of the two free buffers t1, t2 (t2 may be `in`, which is dead once the row pass has read it); returns the
	// buffer that holds the result.  A size of 1 along an axis has no pass there; 1 x 1 is a copy.
	template <bool MAX, int RMAX>
	__device__ __forceinline__ uint16_t *tile_stage(const uint16_t *in, uint16_t *t1, uint16_t *t2, const TileGeometry &g)
	{
		if (g.rx == 0 && g.ry != 0)
		{
			col_pass<MAX, RMAX>(in, t1, g.rw, g.rh, g.gy0, g.rows, g.ry, g.tid);
			__syncthreads();
			return t1;
		}
		row_pass<MAX, RMAX>(in, t1, g.rw, g.rh, g.gx0, g.w, g.rx, g.tid);
		__syncthreads();
		if (g.ry == 0)
			return t1;
		col_pass<MAX, RMAX>(t1, t2, g.rw, g.rh, g.gy0, g.rows, g.ry, g.tid);
		__syncthreads();
		return t2;
	}

	template <class T, int RMAX>
	__global__ __launch_bounds__(256) void morph_tile_kernel(const T *__restrict__ src, T *__restrict__ dst, int w, int h, int rows, int op, int rx, int ry)
	{
		extern __shared__ uint16_t morph_lds[]; // three buffers of tile_cells() cells (dynamic: what the op and the size need)
		const int tid = threadIdx.x;
		const TileId id = tile_decode<false>(); // (vertically adjacent tiles share their halo rows)
		const int stages = morph_two_stages(op) ? 2 : 1;
		const int hx = stages * rx, hy = stages * ry;
		const int x0 = id.bx * G_TW, y0 = id.by * G_TH;
		const TileGeometry g = {G_TW + 2 * hx, G_TH + 2 * hy, x0 - hx, y0 - hy, w, rows, rx, ry, tid};
		const int cells = tile_cells(op, rx, ry);
		uint16_t *A = morph_lds, *B = morph_lds + cells, *C = morph_lds + 2 * cells;
		const uint16_t *res = A, *low = A; // the result (the dilation, for the gradient), and what the gradient subtracts: the erosion
		const int64_t fbase = (int64_t)id.n * w * h;
		const T *s = src + fbase;
		T *d = dst + fbase;
		if (y0 < rows) // (the same for the whole workgroup)
		{
			// (no clipped window reads a cell outside the image: such a cell takes the nearest pixel, so that every load is unconditional and
			// the loads of a thread are in flight together - under a condition each of them waits for the one before)
			for (int c = tid & 63; c < g.rw; c += 64)
			{
				const T *col = s + nearest(g.gx0 + c, w);
#pragma unroll 8
				for (int r = tid >> 6; r < g.rh; r += 4)
					A[r * g.rw + c] = (uint16_t)col[(int64_t)nearest(g.gy0 + r, rows) * w];
			}
			__syncthreads();
			uint16_t *first;
			switch (op)
			{
			case MORPH_ERODE:
				res = tile_stage<false, RMAX>(A, B, C, g);
				break;
			case MORPH_DILATE:
				res = tile_stage<true, RMAX>(A, B, C, g);
				break;
			case MORPH_OPEN:
			case MORPH_TOPHAT:
				first = tile_stage<false, RMAX>(A, B, C, g);
				res = tile_stage<true, RMAX>(first, first == B ? C : B, first, g);
				break;
			case MORPH_CLOSE:
			case MORPH_BLACKHAT:
				first = tile_stage<true, RMAX>(A, B, C, g);
				res = tile_stage<false, RMAX>(first, first == B ? C : B, first, g);
				break;
			default: // MORPH_GRADIENT: the dilation, then the erosion into the buffers it left free (the input's own among them)
				first = tile_stage<true, RMAX>(A, B, C, g);
				res = first;
				low = tile_stage<false, RMAX>(A, first == B ? C : B, A, g);
				break;
			}
		}
		const int x = x0 + (tid & 63);
		if (x >= w)
			return;
		for (int r = tid >> 6; r < G_TH; r += 4)
		{
			const int y = y0 + r;
			if (y >= h)
				break;
			T val;
			if (y < rows)
			{
				const int i = (r + hy) * g.rw + (tid & 63) + hx;
				const uint32_t a = A[i], c = res[i];
				val = (T)(op == MORPH_TOPHAT ? a - c : op == MORPH_BLACKHAT ? c - a : op == MORPH_GRADIENT ? c - low[i] : c);
			}
			else
				val = s[(int64_t)y * w + x];
			d[(int64_t)y * w + x] = val;
		}
	}

	// ---- launchers ---------------------------------------------------------------------------------------------------------------------
	template <class T, int R, int OP>
	static void launch_wave(const T *src, T *dst, int w, int h, int nframes, int rows, hipStream_t st)
	{
		hipLaunchKernelGGL((morph_wave_kernel<T, R, OP>), (pair_wave_grid<MORPH_TY, morph_halo_lanes(R, OP)>(w / 2, h, nframes)), dim3(256), 0, st, src, dst, w,
						   h, rows);
	}
	template <class T, int R>
	static void launch_wave_op(const T *src, T *dst, int w, int h, int nframes, int op, int rows, hipStream_t st)
	{
		switch (op)
		{
		case MORPH_ERODE:
			return launch_wave<T, R, MORPH_ERODE>(src, dst, w, h, nframes, rows, st);
		case MORPH_DILATE:
			return launch_wave<T, R, MORPH_DILATE>(src, dst, w, h, nframes, rows, st);
		case MORPH_OPEN:
			return launch_wave<T, R, MORPH_OPEN>(src, dst, w, h, nframes, rows, st);
		case MORPH_CLOSE:
			return launch_wave<T, R, MORPH_CLOSE>(src, dst, w, h, nframes, rows, st);
		case MORPH_TOPHAT:
			return launch_wave<T, R, MORPH_TOPHAT>(src, dst, w, h, nframes, rows, st);
		case MORPH_BLACKHAT:
			return launch_wave<T, R, MORPH_BLACKHAT>(src, dst, w, h, nframes, rows, st);
		default:
			return launch_wave<T, R, MORPH_GRADIENT>(src, dst, w, h, nframes, rows, st);
		}
	}

	template <class T>
	static hipError_t launch_morphology_t(const T *src, T *dst, int w, int h, int nframes, int op, int size_x, int size_y, int rows, hipStream_t st)
	{
		// the pair kernel: a square 3, 5 or 7 on rows of whole, aligned pairs
		const bool pairs = size_x == size_y && size_x >= 3 && size_x <= 7 && rows_of_pairs(src, dst, w);
		return for_frame_chunks(src, dst, w, h, nframes, [=](const T *s, T *d, int n) {
			if (pairs && size_x == 3)
				launch_wave_op<T, 1>(s, d, w, h, n, op, rows, st);
			else if (pairs && size_x == 5)
				launch_wave_op<T, 2>(s, d, w, h, n, op, rows, st);
			else if (pairs)
				launch_wave_op<T, 3>(s, d, w, h, n, op, rows, st);
			else
			{
				dim3 block(256), grid((unsigned)((w + G_TW - 1) / G_TW), (unsigned)((h + G_TH - 1) / G_TH), (unsigned)n);
				const int rx = size_x / 2, ry = size_y / 2, rmax = std::max(rx, ry);
				const size_t lds = (size_t)3 * tile_cells(op, rx, ry) * sizeof(uint16_t); // (33 120 bytes at most: below the 64 KiB any launch may ask for)
				if (rmax <= 1)
					hipLaunchKernelGGL((morph_tile_kernel<T, 1>), grid, block, lds, st, s, d, w, h, rows, op, rx, ry);
				else if (rmax <= 3)
					hipLaunchKernelGGL((morph_tile_kernel<T, 3>), grid, block, lds, st, s, d, w, h, rows, op, rx, ry);
				else if (rmax <= 5)
					hipLaunchKernelGGL((morph_tile_kernel<T, 5>), grid, block, lds, st, s, d, w, h, rows, op, rx, ry);
				else
					hipLaunchKernelGGL((morph_tile_kernel<T, 7>), grid, block, lds, st, s, d, w, h, rows, op, rx, ry);
			}
		});
	}

	hipError_t launch_morphology(int type, const void *src, void *dst, int w, int h, int nframes, int op, int size_x, int size_y, int rows,
								 hipStream_t st)
	{
		if (op < 0 || op >= MORPH_OPS)
			return hipErrorInvalidValue;
		// (bool frames as bytes: min, max and the differences of 0 / 1 bytes are those of bools)
		return with_pixel_type(type, src, dst, [=](auto *s, auto *d) { return launch_morphology_t(s, d, w, h, nframes, op, size_x, size_y, rows, st); });
	}
} // namespace rir
