// Grey-level morphological reconstruction of a marker under a mask - gfx950 (CDNA4): geodesic dilation (or erosion) repeated to its fixed
// point, for h-domes, hole filling and seeded selection.  An extension without an upstream counterpart; the definition is in
// include/rir_amd_device.h (rir_reconstruct_device).  All integer, bit-exact: the fixed point is unique, so neither the order in which
// workgroups run nor the split of a stack into groups or calls shows in the result.
//
//   reconstruct_round_kernel<T, SOURCE, CONN8>  one ROUND.  A workgroup (four waves) owns a tile of 64 x 32 pixels and keeps it, with a halo of
//                                  one pixel, in LDS: the current values R and the mask G, 2 x 34 x 66 uint16.  It iterates there until
//                                  the tile no longer changes (at most 64 * 32 times), writes the tile back and raises its frame's flag if a
//                                  pixel moved.  The halo is read once and never written.  One iteration is one plain geodesic step,
//                                  r = min(G, max of R over the 3 x 3 window or the cross) - the connectivity asked for - and the tile is
//                                  stable when such a step changes nothing, which is the definition.  Short reach (noise) ends there
//                                  after a few steps.  Every fourth iteration adds, for long reach,
//                                    rows     every row of the tile, forwards and backwards, by a wave: a lane per pixel and a log-step scan
//                                    columns  every column, down and up, by half a wave: a lane per pixel and the same scan
//                                  The scan: along a line r[x] = min(G[x], max(r[x], r[x - 1])) is a clamp
//                                  v -> min(hi, max(lo, v)) of the value carried in, clamps are closed under composition and the composition
//                                  is associative, so the whole line propagates in log2(length) steps; a clamp is one dword (lo, hi) and
//                                  composing takes one packed max and one packed min (pair_tile.h).
//                                  SOURCE says where R comes from: the marker stack, the mask shifted by `param`, the mask on the image's
//                                  border (the first round; the halo comes from the same rule, dst is not read) or dst (every later round).
//   reconstruct_finish_kernel<T>   the rows outside the image (a copy of the mask) and the difference output, in place over dst.
//
// Erosion is dilation of the complemented images (v -> top - v = v ^ top), so the kernels complement what they load and what they store and
// know dilation only: the shifted marker max(0, G' - param), the border marker 0 inside and the difference G' - R' come out as the duals.
//
// Rounds work IN PLACE on dst.  Every value a round reads from another tile - old or already written by that tile in the same round, whole
// elements either way - is a lower bound of the result R and not below min(F, G), and every value a tile writes is the maximum of such
// values along paths under the mask: it never exceeds R and never goes down.  A tile is written by its own workgroup only.  So stale reads
// cost rounds, never correctness, and a round in which no tile wrote is a fixed point seen by every tile at once: the stop condition.  No
// workgroup waits for another.  The flags: frame f's flag of round k is flags[k % 3][f]; round k raises it, reads that of round k - 1 (a
// frame that was stable then returns at once) and clears that of round k + 1, which nothing else touches during round k.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pair_tile.h"
#include "reconstruct_kernels.h"
#include "runtime.h"

namespace rir
{
	constexpr int REC_TW = RECONSTRUCT_TILE_W, REC_TH = RECONSTRUCT_TILE_H;
	constexpr int REC_PITCH = REC_TW + 2, REC_CELLS = (REC_TH + 2) * REC_PITCH; // the tile with its halo
	constexpr int REC_THREADS = 256;
	constexpr int REC_FROM_MARKER = 0, REC_FROM_SHIFT = 1, REC_FROM_BORDER = 2, REC_FROM_DST = 3; // SOURCE (the first three: marker_mode)

	// a clamp v -> min(hi, max(lo, v)) as lo | hi << 16
	__device__ __forceinline__ uint32_t clamp_of(uint32_t lo, uint32_t hi) { return lo | (hi << 16); }
	// first a, then b: (b(a.lo), b(a.hi))
	__device__ __forceinline__ uint32_t clamp_then(uint32_t a, uint32_t b)
	{
		const uint32_t lo = (b & 0xffffu) * 0x10001u, hi = (b >> 16) * 0x10001u;
		return PackedPair::lo(PackedPair::hi(a, lo), hi);
	}

	// One line of N pixels, lane l (0 .. N - 1 within its group of N lanes) holding pixel l: r under g with `before` carried in ahead of
	// pixel 0 and `after` behind pixel N - 1 -> the line propagated forwards, then backwards
	template <int N>
	__device__ __forceinline__ uint32_t propagate_line(uint32_t r, uint32_t g, uint32_t before, uint32_t after, int l)
	{
		if (l == 0)
			r = min(g, max(r, before));
		uint32_t p = clamp_of(r, g);
#pragma unroll
		for (int d = 1; d < N; d <<= 1)
		{
			const uint32_t o = __shfl_up(p, d, N);
			if (l >= d)
				p = clamp_then(o, p);
		}
		r = p & 0xffffu; // the composition applied to 0
		if (l == N - 1)
			r = min(g, max(r, after));
		p = clamp_of(r, g);
#pragma unroll
		for (int d = 1; d < N; d <<= 1)
		{
			const uint32_t o = __shfl_down(p, d, N);
			if (l + d < N)
				p = clamp_then(o, p);
		}
		return p & 0xffffu;
	}

	// flags: [3][nframes] ints, see above.  flip: 0 for dilation, the type's maximum for erosion.  Grid: (tiles of a frame, 1, frames).
	template <class T, int SOURCE, bool CONN8>
	__global__ __launch_bounds__(REC_THREADS) void reconstruct_round_kernel(const T *__restrict__ mask, const T *__restrict__ marker, T *dst, int w, int h,
																			 int rows, int tiles_x, uint32_t flip, uint32_t param, int *flags, int nframes,
																			 int round)
	{
		__shared__ uint16_t R[REC_CELLS], G[REC_CELLS];
		const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
		const int f = blockIdx.z;
		int *const flag_now = flags + (round % 3) * nframes + f;
		if (blockIdx.x == 0 && t == 0)
			flags[((round + 1) % 3) * nframes + f] = 0;
		if (SOURCE == REC_FROM_DST && flags[((round + 2) % 3) * nframes + f] == 0) // (round - 1: nothing moved in this frame)
			return;
		const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * REC_TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * REC_TH;
		const int64_t base = (int64_t)f * w * h;
		mask += base, dst += base;
		if (SOURCE == REC_FROM_MARKER)
			marker += base;

		for (int i = t; i < REC_CELLS; i += REC_THREADS)
		{
			const int ty = i / REC_PITCH, tx = i - ty * REC_PITCH;
			const int y = y0 + ty - 1, x = x0 + tx - 1;
			uint32_t g = 0, r = 0; // outside the image: a cell that holds nothing and passes nothing on
			if (y >= 0 && y < rows && x >= 0 && x < w)
			{
				const int64_t at = (int64_t)y * w + x;
				g = (uint32_t)mask[at] ^ flip;
				if (SOURCE == REC_FROM_DST)
					r = (uint32_t)dst[at] ^ flip;
				else if (SOURCE == REC_FROM_MARKER)
					r = min((uint32_t)marker[at] ^ flip, g);
				else if (SOURCE == REC_FROM_SHIFT)
					r = g > param ? g - param : 0;
				else
					r = y == 0 || y == rows - 1 || x == 0 || x == w - 1 ? g : 0;
			}
			G[i] = (uint16_t)g, R[i] = (uint16_t)r;
		}
		__syncthreads();

		bool moved = false; // a pixel of the tile left the value it was loaded with
		for (int it = 0; it < REC_TW * REC_TH; ++it)
		{
			// one plain geodesic step, r = min(G, max of R over N): thread t has column t & 63 and rows wv * 8 .. + 7.  A neighbour read while
			// its owner writes it is its old or its new value - either is a lower bound of the result - and a pixel is written by its owner
			// only.  A step that changes nothing has read the tile as it is: the fixed point under this halo, the only way out of the loop.
			int changed = 0;
			int at = (1 + wv * (REC_TH / 4)) * REC_PITCH + 1 + lane;
			if (CONN8)
			{
				uint32_t above = max(max(R[at - REC_PITCH - 1], R[at - REC_PITCH]), R[at - REC_PITCH + 1]);
				uint32_t here = max(max(R[at - 1], R[at]), R[at + 1]);
				for (int j = 0; j < REC_TH / 4; ++j, at += REC_PITCH)
				{
					const uint32_t below = max(max(R[at + REC_PITCH - 1], R[at + REC_PITCH]), R[at + REC_PITCH + 1]);
					const uint32_t old = R[at], r = min((uint32_t)G[at], max(max(above, here), below));
					if (r != old)
						R[at] = (uint16_t)r, changed = 1;
					above = here, here = below;
				}
			}
			else
			{
				for (int j = 0; j < REC_TH / 4; ++j, at += REC_PITCH)
				{
					const uint32_t old = R[at];
					const uint32_t r = min((uint32_t)G[at], max(max(max(R[at - REC_PITCH], R[at + REC_PITCH]), max(R[at - 1], R[at + 1])), old));
					if (r != old)
						R[at] = (uint16_t)r, changed = 1;
				}
			}
			if (!__syncthreads_or(changed))
				break;
			moved = true;
			if ((it & 3) != 3)
				continue;
			// every fourth time, what plain steps take a step per pixel for: whole lines at once (the next plain step sees what they changed)
			// rows: wave wv has rows wv * 8 .. + 7 of the tile, lane = column
			for (int j = 0; j < REC_TH / 4; ++j)
			{
				const int row = (1 + wv * (REC_TH / 4) + j) * REC_PITCH;
				const uint32_t old = R[row + 1 + lane];
				const uint32_t r = propagate_line<64>(old, G[row + 1 + lane], R[row], R[row + REC_TW + 1], lane);
				if (r != old)
					R[row + 1 + lane] = (uint16_t)r;
			}
			__syncthreads();
			// columns: wave wv has columns wv * 16 .. + 15, two at a time, lane & 31 = row
			for (int j = 0; j < REC_TW / 8; ++j)
			{
				const int tx = 1 + wv * (REC_TW / 4) + j * 2 + (lane >> 5), l = lane & 31;
				const int cell = (1 + l) * REC_PITCH + tx;
				const uint32_t old = R[cell];
				const uint32_t r = propagate_line<32>(old, G[cell], R[tx], R[(REC_TH + 1) * REC_PITCH + tx], l);
				if (r != old)
					R[cell] = (uint16_t)r;
			}
			__syncthreads();
		}

		if (SOURCE != REC_FROM_DST || moved)
		{
			const int x = x0 + lane;
			for (int j = 0; j < REC_TH / 4; ++j)
			{
				const int ty = wv * (REC_TH / 4) + j, y = y0 + ty;
				if (y < rows && x < w)
					dst[(int64_t)y * w + x] = (T)(R[(1 + ty) * REC_PITCH + 1 + lane] ^ flip);
			}
		}
		if (moved && t == 0)
			atomicOr(flag_now, 1);
	}

	// rows >= rows: the mask; output 1: the difference, mask - dst (dilation) or dst - mask (erosion).  Grid: (256-pixel pieces of a frame, frames)
	template <class T>
	__global__ __launch_bounds__(256) void reconstruct_finish_kernel(const T *__restrict__ mask, T *dst, int w, int h, int rows, int method, int output)
	{
		const int64_t npx = (int64_t)w * h, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
		if (i >= npx)
			return;
		const int64_t at = (int64_t)blockIdx.y * npx + i;
		const T g = mask[at];
		if (i >= (int64_t)rows * w)
			dst[at] = g;
		else if (output)
			dst[at] = method ? (T)(dst[at] - g) : (T)(g - dst[at]);
	}

	// ---- launcher ---------------------------------------------------------------------------------------------------------------------------
	template <class T, bool CONN8>
	static void launch_round(int source, const T *mask, const T *marker, T *dst, int w, int h, int n, int rows, uint32_t flip, uint32_t param, int *flags,
							 int round, hipStream_t st)
	{
		const int tiles_x = (w + REC_TW - 1) / REC_TW, tiles_y = (rows + REC_TH - 1) / REC_TH;
		const dim3 grid((unsigned)(tiles_x * tiles_y), 1, (unsigned)n), block(REC_THREADS);
		switch (source)
		{
		case REC_FROM_MARKER:
			hipLaunchKernelGGL((reconstruct_round_kernel<T, REC_FROM_MARKER, CONN8>), grid, block, 0, st, mask, marker, dst, w, h, rows, tiles_x, flip, param,
							   flags, n, round);
			break;
		case REC_FROM_SHIFT:
			hipLaunchKernelGGL((reconstruct_round_kernel<T, REC_FROM_SHIFT, CONN8>), grid, block, 0, st, mask, marker, dst, w, h, rows, tiles_x, flip, param,
							   flags, n, round);
			break;
		case REC_FROM_BORDER:
			hipLaunchKernelGGL((reconstruct_round_kernel<T, REC_FROM_BORDER, CONN8>), grid, block, 0, st, mask, marker, dst, w, h, rows, tiles_x, flip, param,
							   flags, n, round);
			break;
		default:
			hipLaunchKernelGGL((reconstruct_round_kernel<T, REC_FROM_DST, CONN8>), grid, block, 0, st, mask, marker, dst, w, h, rows, tiles_x, flip, param,
							   flags, n, round);
		}
	}

	int reconstruct_group_frames(int nframes, size_t work_bytes)
	{
		const int fit = (int)std::min<size_t>(std::min<size_t>((size_t)nframes, work_bytes / RECONSTRUCT_FRAME_BYTES), MAX_GRID_Z);
		if (fit < 1)
			return 0;
		const int groups = (nframes + fit - 1) / fit;
		return (nframes + groups - 1) / groups; // groups of equal size, the fewest that fit
	}

	template <class T>
	static hipError_t launch_reconstruct_t(const T *mask, const T *marker, T *dst, int w, int h, int nframes, int method, int connectivity, int marker_mode,
										   int param, int output, int rows, uint32_t top, void *work, size_t work_bytes, int *h_flags, int *rounds,
										   bool *converged, hipStream_t st)
	{
		const int64_t npx = (int64_t)w * h;
		const int group = reconstruct_group_frames(nframes, work_bytes);
		if (group < 1)
			return hipErrorInvalidValue;
		const uint32_t flip = method ? top : 0;
		const int64_t cap = reconstruct_round_cap(w, rows);
		int *flags = static_cast<int *>(work);
		*rounds = 0, *converged = true;
		for (int o = 0; o < nframes; o += group)
		{
			const int n = std::min(group, nframes - o);
			const T *g_mask = mask + npx * o, *g_marker = marker ? marker + npx * o : nullptr;
			T *g_dst = dst + npx * o;
			int64_t round = 0;
			if (rows > 0)
			{
				hipError_t e = hipMemsetAsync(flags, 0, (size_t)3 * n * sizeof(int), st);
				if (e != hipSuccess)
					return e;
				bool stable = false;
				while (!stable && round < cap)
				{
					// one round before the first look at the flags, two before every later one: a frame that is stable returns at once
					for (int k = round < 1 ? 1 : 2; k > 0; --k, ++round)
					{
						if (connectivity == 8)
							launch_round<T, true>(round == 0 ? marker_mode : REC_FROM_DST, g_mask, g_marker, g_dst, w, h, n, rows, flip, (uint32_t)param, flags,
												  (int)(round % 3), st);
						else
							launch_round<T, false>(round == 0 ? marker_mode : REC_FROM_DST, g_mask, g_marker, g_dst, w, h, n, rows, flip, (uint32_t)param, flags,
												   (int)(round % 3), st);
					}
					if ((e = hipGetLastError()) != hipSuccess ||
						(e = hipMemcpyAsync(h_flags, flags + ((round - 1) % 3) * n, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
						(e = wait_stream(st)) != hipSuccess)
						return e;
					stable = std::all_of(h_flags, h_flags + n, [](int v) { return v == 0; });
				}
				if (!stable)
					*converged = false;
			}
			*rounds = (int)std::max<int64_t>(*rounds, round);
			if (output || rows < h)
				hipLaunchKernelGGL((reconstruct_finish_kernel<T>), dim3((unsigned)((npx + 255) / 256), (unsigned)n), dim3(256), 0, st, g_mask, g_dst, w, h, rows,
								   method, output);
		}
		return hipGetLastError();
	}

	hipError_t launch_reconstruct(int type, const void *mask, const void *marker, void *dst, int w, int h, int nframes, int method, int connectivity,
								  int marker_mode, int param, int output, int rows, void *work, size_t work_bytes, int *h_flags, int *rounds,
								  bool *converged, hipStream_t st)
	{
		switch (type)
		{
		case '?': // (bool frames as bytes 0 / 1)
		case 'B':
			return launch_reconstruct_t(static_cast<const uint8_t *>(mask), static_cast<const uint8_t *>(marker), static_cast<uint8_t *>(dst), w, h, nframes,
										method, connectivity, marker_mode, param, output, rows, type == '?' ? 1u : 255u, work, work_bytes, h_flags, rounds,
										converged, st);
		case 'H':
			return launch_reconstruct_t(static_cast<const uint16_t *>(mask), static_cast<const uint16_t *>(marker), static_cast<uint16_t *>(dst), w, h, nframes,
										method, connectivity, marker_mode, param, output, rows, 65535u, work, work_bytes, h_flags, rounds, converged, st);
		default:
			return hipErrorInvalidValue;
		}
	}
} // namespace rir
