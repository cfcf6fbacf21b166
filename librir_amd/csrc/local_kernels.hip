// Local window statistics of frame stacks - gfx950 (CDNA4): the sum, the sum of squares and the rounded mean over a centred rectangle
// size_y x size_x (odd, 1..15) around every pixel of uint16, uint8 and bool frames [n][h][w], and the z-score mask built from them ("hot
// where the pixel stands more than k local standard deviations above its local mean").  An extension without an upstream counterpart; the
// definitions are in include/rir_amd_device.h (rir_local_stats_device, rir_local_threshold_device).  All integer, bit-exact; no float.
//
// The window is always FULL: a position outside the image (its first `rows` rows) takes the value of the nearest pixel, as in
// rank_kernels.hip.  The sums are separable and the window sizes are runtime values:
//
//   vertical    a wave owns a pair tile (pair_tile.h) of LOCAL_TY rows, a lane one column pair.  The lane keeps the COLUMN sums of its two
//               pixels over the window's rows (and of their squares) in registers and slides them down the tile: the row that enters is
//               added, the row that leaves - read again, an L1 / L2 hit - subtracted.  Rows are clamped into the image, so the slide is
//               exact at the border too.  O(1) per output row, no history of rows: nothing is indexed by a runtime value, so no scratch.
//   horizontal  per output row the column sums of the neighbouring lanes come in by DPP wave shifts, one lane further per step, (size_x / 2
//               + 1) / 2 steps; which of a neighbour's two columns belong to which of the lane's two windows is wave-uniform.  The outer
//               LOCAL_HL = 4 lanes of each side are halo (7 pixels reach 4 pairs far): they load their - replicated - columns and take part
//               in the shifts, and have no output.
//
// No LDS, no barrier, no workspace, no atomics.  Two forms of the same kernel, which differ in their loads and stores only:
//   PAIRS    rows of whole, aligned pairs (even width, every pointer aligned to a pair of its cells): one load per pair and row, one store
//            per pair, row and output.
//   general  every other width and alignment: each pixel of the pair is loaded and stored on its own, the second one of the last pair of an
//            odd width being a replicated pixel with no output.
// Squares: a uint16 square fills 32 bits, so their sums are 64-bit from the first addition (one v_mad_u64_u32 per pixel); the sums of uint8 /
// bool squares (at most 225 * 255^2 = 14 630 625) stay in 32 bits and are widened where they are stored.  A kernel that is not asked for
// squares (WANT_Q false: sum and mean only) carries none.
//
// Every load is a plain load at an address clamped into the image, every store goes through a plain pointer under its own bounds test.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "local_kernels.h"
#include "pair_tile.h"

namespace rir
{
	constexpr int LOCAL_TY = 16, LOCAL_HL = 4;

	template <class T>
	using local_sq_t = typename std::conditional<sizeof(T) == 2, uint64_t, uint32_t>::type; // what holds a sum of squares of T

	// The lane's pair column (pixels 2 xp, 2 xp + 1) of a frame of w columns, every coordinate clamped into the row: a pair left of the image
	// is the first pixel twice, one right of it the last pixel twice.
	template <class T, bool PAIRS>
	struct LocalColumn
	{
		typedef typename PixelPair<T>::type P;
		const T *s;
		int w, c0, c1; // PAIRS: c0 the pair's index in a row of w / 2 pairs, c1 < 0 / > 0: left / right of the image; general: the two columns
		__device__ __forceinline__ LocalColumn(const T *frame, int w, int xp) : s(frame), w(w)
		{
			if constexpr (PAIRS)
				c0 = nearest(xp, w >> 1), c1 = xp < 0 ? -1 : xp >= (w >> 1) ? 1 : 0;
			else
				c0 = nearest(2 * xp, w), c1 = nearest(2 * xp + 1, w);
		}
		__device__ __forceinline__ void load(int y, uint32_t &lo, uint32_t &hi) const
		{
			if constexpr (PAIRS)
			{
				const uint32_t raw = PixelPair<T>::widen(reinterpret_cast<const P *>(s)[(int64_t)y * (w >> 1) + c0]);
				const uint32_t a = raw & 0xffffu, b = raw >> 16;
				lo = c1 > 0 ? b : a;
				hi = c1 < 0 ? a : b;
			}
			else
			{
				const T *row = s + (int64_t)y * w;
				lo = row[c0];
				hi = row[c1];
			}
		}
	};

	// The window sums of the tile rows y0 .. yend - 1 (all inside the image, yend > y0) of this lane's pair: emit(y, S of the first pixel, S of
	// the second, Q of the first, Q of the second, the first pixel, the second) once per row, top down.  All 64 lanes of the wave walk
	// together (the shifts need them).  A row's three loads - its own pixels, the row that enters the window below it and the row that leaves
	// - are issued before its horizontal step and used after it, unconditionally (the addresses are clamped; what the last row loads for the
	// slide is not used), so their latency runs under the shifts.
	template <class T, bool PAIRS, bool WANT_Q, class Emit>
	__device__ __forceinline__ void local_walk(const LocalColumn<T, PAIRS> &col, int rows, int y0, int yend, int rx, int ry, Emit emit)
	{
		typedef local_sq_t<T> QT;
		uint32_t a = 0, b = 0; // the column sums over the window's rows: pixel 2 xp, pixel 2 xp + 1
		QT qa = 0, qb = 0;
		for (int dy = -ry; dy <= ry; ++dy)
		{
			uint32_t lo, hi;
			col.load(nearest(y0 + dy, rows), lo, hi);
			a += lo, b += hi;
			if constexpr (WANT_Q)
				qa += (QT)lo * lo, qb += (QT)hi * hi;
		}
		const int steps = (rx + 1) >> 1;
		for (int y = y0; y < yend; ++y)
		{
			uint32_t v_lo, v_hi, in_lo, in_hi, out_lo, out_hi;
			col.load(y, v_lo, v_hi);
			col.load(nearest(y + 1 + ry, rows), in_lo, in_hi);
			col.load(nearest(y - ry, rows), out_lo, out_hi);
			// the lane's own two columns, then the lanes k to the left (columns 2 xp - 2k, 2 xp - 2k + 1) and to the right (2 xp + 2k, 2 xp + 2k
			// + 1): the inner column of each is always inside both windows (2k - 1 <= rx), the others by `full` and `over`
			uint32_t s0 = a + (rx ? b : 0u), s1 = b + (rx ? a : 0u);
			QT q0 = qa + (rx ? qb : (QT)0), q1 = qb + (rx ? qa : (QT)0);
			uint32_t la = a, lb = b, ra = a, rb = b;
			QT lqa = qa, lqb = qb, rqa = qa, rqb = qb;
			for (int k = 1; k <= steps; ++k)
			{
				const bool full = 2 * k <= rx, over = 2 * k + 1 <= rx;
				lb = wave_shr1(lb), ra = wave_shl1(ra);
				if (full) // (false in the last step of a size_x of 3, 7, 11, 15, whose outer columns nothing asks for any more)
					la = wave_shr1(la), rb = wave_shl1(rb);
				s0 += lb + (full ? la + ra : 0u) + (over ? rb : 0u);
				s1 += ra + (full ? lb + rb : 0u) + (over ? la : 0u);
				if constexpr (WANT_Q)
				{
					lqb = wave_shr1(lqb), rqa = wave_shl1(rqa);
					if (full)
						lqa = wave_shr1(lqa), rqb = wave_shl1(rqb);
					q0 += lqb + (full ? lqa + rqa : (QT)0) + (over ? rqb : (QT)0);
					q1 += rqa + (full ? lqb + rqb : (QT)0) + (over ? lqa : (QT)0);
				}
			}
			emit(y, s0, s1, q0, q1, v_lo, v_hi);
			a += in_lo - out_lo, b += in_hi - out_hi; // (modulo 2^32 in between; the sums themselves fit)
			if constexpr (WANT_Q)
				qa += (QT)in_lo * in_lo - (QT)out_lo * out_lo, qb += (QT)in_hi * in_hi - (QT)out_hi * out_hi;
		}
	}

	// which of the lane's two pixels have an output: lanes HL .. 63 - HL, columns inside the image
	struct LocalLane
	{
		bool first, second;
		__device__ __forceinline__ LocalLane(int lane, int xp, int w) : first(lane >= LOCAL_HL && lane < 64 - LOCAL_HL && 2 * xp < w), second(first && 2 * xp + 1 < w) {}
	};

	// one cell of an output per pixel of the pair, (v0, v1), at row y: as one store of a pair (PAIRS) or pixel by pixel
	template <bool PAIRS, class C, class C2>
	__device__ __forceinline__ void local_store(C *frame, int w, int y, int xp, const LocalLane &out, C v0, C v1)
	{
		static_assert(sizeof(C2) == 2 * sizeof(C), "a pair of cells");
		C *cell = frame + (int64_t)y * w + 2 * xp;
		if constexpr (PAIRS)
		{
			if (out.first)
			{
				C2 both;
				both.x = v0, both.y = v1;
				*reinterpret_cast<C2 *>(cell) = both;
			}
		}
		else
		{
			if (out.first)
				cell[0] = v0;
			if (out.second)
				cell[1] = v1;
		}
	}

	struct LocalMean
	{
		uint32_t half, magic; // n / 2; floor(2^32 / n) + 1, or 0 for n = 1
		// (S + n / 2) / n: with e = magic n - 2^32 <= n <= 225 and x = S + n / 2 < 2^24, x e < 2^32, so the multiply-high is the exact quotient
		__device__ __forceinline__ uint32_t of(uint32_t S) const { return magic ? __umulhi(S + half, magic) : S; }
	};

	template <class T, bool PAIRS, bool WANT_Q>
	__global__ __launch_bounds__(256) void local_stats_kernel(const T *__restrict__ src, int32_t *__restrict__ sum, int64_t *__restrict__ sumsq,
															   T *__restrict__ mean, int w, int h, int rows, int rx, int ry, LocalMean div)
	{
		const int lane = threadIdx.x & 63;
		const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
		const PairTile<T, LOCAL_TY, LOCAL_HL> t(lane, wv, w);
		if (t.y0 >= h)
			return;
		const int64_t fbase = (int64_t)t.n * w * h;
		const T *s = src + fbase;
		int32_t *ds = sum ? sum + fbase : nullptr;
		int64_t *dq = WANT_Q ? sumsq + fbase : nullptr;
		T *dm = mean ? mean + fbase : nullptr;
		const int xp = t.xp;
		const LocalLane out(lane, xp, w);
		const LocalColumn<T, PAIRS> col(s, w, xp);
		const int yend = min(t.y0 + LOCAL_TY, rows);
		if (t.y0 < yend)
			local_walk<T, PAIRS, WANT_Q>(col, rows, t.y0, yend, rx, ry, [&](int y, uint32_t s0, uint32_t s1, local_sq_t<T> q0, local_sq_t<T> q1, uint32_t, uint32_t) {
				if (ds)
					local_store<PAIRS, int32_t, int2>(ds, w, y, xp, out, (int32_t)s0, (int32_t)s1);
				if constexpr (WANT_Q)
					local_store<PAIRS, int64_t, longlong2>(dq, w, y, xp, out, (int64_t)q0, (int64_t)q1);
				if (dm)
				{
					if constexpr (sizeof(T) == 2)
						local_store<PAIRS, uint16_t, ushort2>(dm, w, y, xp, out, (uint16_t)div.of(s0), (uint16_t)div.of(s1));
					else
						local_store<PAIRS, uint8_t, uchar2>(dm, w, y, xp, out, (uint8_t)div.of(s0), (uint8_t)div.of(s1));
				}
			});
		// the tile's rows below the image: the mean is the input, the sums are 0
		for (int y = max(t.y0, rows); y < min(t.y0 + LOCAL_TY, h); ++y)
		{
			if (ds)
				local_store<PAIRS, int32_t, int2>(ds, w, y, xp, out, 0, 0);
			if constexpr (WANT_Q)
				local_store<PAIRS, int64_t, longlong2>(dq, w, y, xp, out, 0, 0);
			if (dm)
			{
				uint32_t v0, v1;
				col.load(y, v0, v1);
				if constexpr (sizeof(T) == 2)
					local_store<PAIRS, uint16_t, ushort2>(dm, w, y, xp, out, (uint16_t)v0, (uint16_t)v1);
				else
					local_store<PAIRS, uint8_t, uchar2>(dm, w, y, xp, out, (uint8_t)v0, (uint8_t)v1);
			}
		}
	}

	struct LocalRule
	{
		uint32_t n;		   // cells of the window
		int32_t delta_n;   // delta n
		uint32_t kn2, kd2; // k_num^2, k_den^2
		int above, below;  // which signs of d pass the first test

		// The z-score test of pixel v in a window of sum S and sum of squares Q, in exact integers: d = n v - S is n times the pixel's distance
		// from the window's mean, V = n Q - S^2 >= 0 is n^2 times the window's variance.  Everything stays inside int64 because of the
		// limits of the parameters (n <= 225, v <= 65535, k_den <= 64, k_num <= 255), which are not to be widened:
		//   |d| <= 225 * 65535 = 14 745 375, so d^2 k_den^2 <= 14 745 375^2 * 64^2 = 8.9e17 < 2^63 = 9.22e18;
		//   V is largest on a window that is half 0 and half 65535 (113 of 225 cells: 225 Q - S^2 = 5.44e13), so k_num^2 V <= 255^2 * 5.44e13 =
		//   3.6e18 < 2^63; n Q <= 225 * 966 338 150 625 = 2.2e14 and S^2 <= 2.2e14 on the way there; delta n <= 65535 * 225 fits int32.
		__device__ __forceinline__ uint32_t hot(uint32_t v, uint32_t S, uint64_t Q) const
		{
			// (S and |d| are below 2^24 = 16 777 216: saying so - the masks change nothing - makes n v, S^2 and d^2 full-rate 24-bit products)
			const uint32_t S24 = S & 0xffffffu;
			const int32_t d = (int32_t)(n * v) - (int32_t)S24;
			const uint32_t size = (uint32_t)(d < 0 ? -d : d) & 0xffffffu;
			const uint64_t V = n * Q - (uint64_t)S24 * S24, d2 = (uint64_t)size * size;
			const bool side = (above & (d > delta_n)) | (below & (-d > delta_n)); // (no branches: the two pixels of a pair run side by side)
			return (side & (d2 * kd2 > V * kn2)) ? 1u : 0u;
		}
	};

	template <class T, bool PAIRS>
	__global__ __launch_bounds__(256) void local_threshold_kernel(const T *__restrict__ src, uint8_t *__restrict__ mask, int w, int h, int rows, int rx,
																   int ry, LocalRule rule)
	{
		const int lane = threadIdx.x & 63;
		const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
		const PairTile<T, LOCAL_TY, LOCAL_HL> t(lane, wv, w);
		if (t.y0 >= h)
			return;
		const int64_t fbase = (int64_t)t.n * w * h;
		const T *s = src + fbase;
		uint8_t *d = mask + fbase;
		const int xp = t.xp;
		const LocalLane out(lane, xp, w);
		const LocalColumn<T, PAIRS> col(s, w, xp);
		const int yend = min(t.y0 + LOCAL_TY, rows);
		if (t.y0 < yend)
			local_walk<T, PAIRS, true>(col, rows, t.y0, yend, rx, ry, [&](int y, uint32_t s0, uint32_t s1, local_sq_t<T> q0, local_sq_t<T> q1, uint32_t v0, uint32_t v1) {
				local_store<PAIRS, uint8_t, uchar2>(d, w, y, xp, out, (uint8_t)rule.hot(v0, s0, q0), (uint8_t)rule.hot(v1, s1, q1));
			});
		for (int y = max(t.y0, rows); y < min(t.y0 + LOCAL_TY, h); ++y)
			local_store<PAIRS, uint8_t, uchar2>(d, w, y, xp, out, 0, 0);
	}

	// ---- launchers ---------------------------------------------------------------------------------------------------------------------
	static dim3 local_grid(int w, int h, int n) { return pair_wave_grid<LOCAL_TY, LOCAL_HL>((w + 1) / 2, h, n); }

	template <class T, bool PAIRS, bool WANT_Q>
	static void launch_stats_kernel(const T *src, int32_t *sum, int64_t *sumsq, T *mean, int w, int h, int n, int rows, int rx, int ry, LocalMean div,
									hipStream_t st)
	{
		hipLaunchKernelGGL((local_stats_kernel<T, PAIRS, WANT_Q>), local_grid(w, h, n), dim3(256), 0, st, src, sum, sumsq, mean, w, h, rows, rx, ry, div);
	}

	template <class T>
	static hipError_t launch_local_stats_t(const T *src, T *mean, int w, int h, int nframes, int size_x, int size_y, int rows, int32_t *sum, int64_t *sumsq,
										   hipStream_t st)
	{
		// the pair form: rows of whole pairs of pixels, and every output aligned to a pair of its cells
		const bool pairs = rows_of_pairs(src, mean, w) && (uintptr_t)sum % 8 == 0 && (uintptr_t)sumsq % 16 == 0;
		const uint32_t n = (uint32_t)(size_x * size_y);
		const LocalMean div{n / 2, n > 1 ? (uint32_t)(0x100000000ull / n) + 1u : 0u};
		const int rx = size_x / 2, ry = size_y / 2;
		return for_frame_chunks(src, const_cast<T *>(src), w, h, nframes, [=](const T *s, T *, int count) {
			const int64_t at = s - src; // the chunk's first cell, in every output
			int32_t *ds = sum ? sum + at : nullptr;
			int64_t *dq = sumsq ? sumsq + at : nullptr;
			T *dm = mean ? mean + at : nullptr;
			if (pairs && dq)
				launch_stats_kernel<T, true, true>(s, ds, dq, dm, w, h, count, rows, rx, ry, div, st);
			else if (pairs)
				launch_stats_kernel<T, true, false>(s, ds, dq, dm, w, h, count, rows, rx, ry, div, st);
			else if (dq)
				launch_stats_kernel<T, false, true>(s, ds, dq, dm, w, h, count, rows, rx, ry, div, st);
			else
				launch_stats_kernel<T, false, false>(s, ds, dq, dm, w, h, count, rows, rx, ry, div, st);
		});
	}

	hipError_t launch_local_stats(int type, const void *src, int w, int h, int nframes, int size_x, int size_y, int rows, int32_t *sum, int64_t *sumsq,
								  void *mean, hipStream_t st)
	{
		return with_pixel_type(type, src, mean, [=](auto *s, auto *m) { return launch_local_stats_t(s, m, w, h, nframes, size_x, size_y, rows, sum, sumsq, st); });
	}

	template <class T>
	static hipError_t launch_local_threshold_t(const T *src, uint8_t *mask, int w, int h, int nframes, int size_x, int size_y, int rows, LocalRule rule,
											   hipStream_t st)
	{
		const bool pairs = rows_of_pairs(src, (const T *)nullptr, w) && (uintptr_t)mask % 2 == 0;
		const int rx = size_x / 2, ry = size_y / 2;
		return for_frame_chunks(src, const_cast<T *>(src), w, h, nframes, [=](const T *s, T *, int count) {
			uint8_t *d = mask + (s - src);
			if (pairs)
				hipLaunchKernelGGL((local_threshold_kernel<T, true>), local_grid(w, h, count), dim3(256), 0, st, s, d, w, h, rows, rx, ry, rule);
			else
				hipLaunchKernelGGL((local_threshold_kernel<T, false>), local_grid(w, h, count), dim3(256), 0, st, s, d, w, h, rows, rx, ry, rule);
		});
	}

	hipError_t launch_local_threshold(int type, const void *src, uint8_t *mask, int w, int h, int nframes, int size_x, int size_y, int rows, int k_num,
									  int k_den, int delta, int polarity, hipStream_t st)
	{
		const int n = size_x * size_y;
		const LocalRule rule{(uint32_t)n, delta * n, (uint32_t)(k_num * k_num), (uint32_t)(k_den * k_den), polarity != LOCAL_BELOW, polarity != LOCAL_ABOVE};
		return with_pixel_type(type, src, (void *)nullptr,
							   [=](auto *s, auto *) { return launch_local_threshold_t(s, mask, w, h, nframes, size_x, size_y, rows, rule, st); });
	}
} // namespace rir
