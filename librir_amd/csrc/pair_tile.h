// The wave-tile scheme of wave_tile.h with TWO columns per lane, shared by the window-filter units (morphology_kernels.hip,
// rank_kernels.hip) — gfx950 (CDNA4) — and the host side of their launchers.  Include it from a .hip unit, inside no namespace.  The device
// parts are __forceinline__, so each unit's kernels carry their own copy.
//
// A wave owns 2 x OUT_LANES columns x TY rows of a frame of even width, lane i the column pair (x0 + 2i, x0 + 2i + 1) as one dword per row -
// two uint16 pixels, or two uint8 pixels widened on load - so every load, store and min / max works on a pair (v_pk_min_u16 /
// v_pk_max_u16); no LDS, no barrier.  Neighbouring columns come from the neighbouring lanes: an even shift is the next lane's pair (DPP
// wave shift), an odd one two neighbouring pairs funnel-shifted by 16 bits.  The outer HL lanes of each side are halo: they have no output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "wave_tile.h"

namespace rir
{
	// a pair of pixels in memory (`type`), and as the two uint16 halves of a dword
	template <class T>
	struct PixelPair;
	template <>
	struct PixelPair<uint16_t>
	{
		typedef uint32_t type;
		__device__ static uint32_t widen(uint32_t raw) { return raw; }
		__device__ static uint32_t narrow(uint32_t v) { return v; }
	};
	template <>
	struct PixelPair<uint8_t>
	{
		typedef uint16_t type;
		__device__ static uint32_t widen(uint32_t raw) { return (raw | (raw << 8)) & 0x00ff00ffu; }
		__device__ static uint16_t narrow(uint32_t v) { return (uint16_t)((v & 0xffu) | ((v >> 8) & 0xff00u)); }
	};

	// element-wise min / max / difference of two pairs; PackedPair is an `Ops` of rank_select.h
	typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
	__device__ __forceinline__ v2u16 pk_halves(uint32_t v) { return __builtin_bit_cast(v2u16, v); }
	__device__ __forceinline__ uint32_t pk_dword(v2u16 v) { return __builtin_bit_cast(uint32_t, v); }
	struct PackedPair
	{
		__device__ static __forceinline__ uint32_t lo(uint32_t a, uint32_t b) { return pk_dword(__builtin_elementwise_min(pk_halves(a), pk_halves(b))); }
		__device__ static __forceinline__ uint32_t hi(uint32_t a, uint32_t b) { return pk_dword(__builtin_elementwise_max(pk_halves(a), pk_halves(b))); }
	};
	template <bool MAX>
	__device__ __forceinline__ uint32_t pk_pick(uint32_t a, uint32_t b) { return MAX ? PackedPair::hi(a, b) : PackedPair::lo(a, b); }
	__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) { return pk_dword(pk_halves(a) - pk_halves(b)); }

	// the odd shifts: the pair one pixel to the left of c = (x, x + 1), from prev = (x - 2, x - 1): (x - 1, x); and the one to the right, from
	// next = (x + 2, x + 3): (x + 1, x + 2)
	__device__ __forceinline__ uint32_t left_pair(uint32_t c, uint32_t prev) { return __builtin_amdgcn_alignbit(c, prev, 16); }
	__device__ __forceinline__ uint32_t right_pair(uint32_t c, uint32_t next) { return __builtin_amdgcn_alignbit(next, c, 16); }

	// coordinate v clamped into 0 .. n - 1: the nearest pixel of the image
	__device__ __forceinline__ int nearest(int v, int n) { return min(max(v, 0), n - 1); }

	// The pair tile of this lane's wave in a launch of pair_wave_grid<TY, HL>: tile rows are not line-aligned, so column fastest.  A wave
	// whose y0 >= h has nothing to do, and returns before it asks for anything else.  Three things keep the kernels' code what it was with
	// all this written out in each of them (profiles/window_filters_refactor_resources.txt): the kernel reads threadIdx.x itself, nothing here
	// is computed before it is asked for, and the stores read the tile's members once, before their loops.  A kernel states its own lane
	// predicates (inside the image: 0 <= xp < wp; writing: HL <= lane < 64 - HL and xp < wp) for the same reason.
	template <class T, int TY, int HL>
	struct PairTile
	{
		typedef typename PixelPair<T>::type P;
		static constexpr int OUT_LANES = 64 - 2 * HL;
		int wp, xp0, xp, y0, n; // wp: pairs per row; the wave's first pair column and this lane's; the tile's first row; the frame

		// lane, wv: the thread's lane and (wave-uniform) wave, which the kernel reads itself
		__device__ __forceinline__ PairTile(int lane, int wv, int w)
		{
			const TileId id = tile_decode<true>();
			wp = w >> 1;
			xp0 = id.bx * OUT_LANES - HL, xp = xp0 + lane;
			y0 = (id.by * 4 + wv) * TY;
			n = id.n;
		}
		// the tile's frame of a stack, as pairs
		__device__ __forceinline__ const P *frame(const T *stack, int w, int h) const { return reinterpret_cast<const P *>(stack + (int64_t)n * w * h); }
		__device__ __forceinline__ P *frame(T *stack, int w, int h) const { return reinterpret_cast<P *>(stack + (int64_t)n * w * h); }
		// the tile's results, for its rows inside the image (the first `rows` rows)
		__device__ __forceinline__ void store(P *d, const uint32_t (&res)[TY], int rows, bool out_lane) const
		{
			const int wp = this->wp, xp = this->xp, y0 = this->y0;
			if (out_lane)
			{
#pragma unroll
				for (int j = 0; j < TY; ++j)
					if (y0 + j < rows)
						d[(int64_t)(y0 + j) * wp + xp] = PixelPair<T>::narrow(res[j]);
			}
		}
		// the tile's rows >= rows: copied
		__device__ __forceinline__ void copy_rest(const P *s, P *d, int h, int rows, bool out_lane) const
		{
			const int wp = this->wp, xp = this->xp, y0 = this->y0;
			if (out_lane)
				for (int y = max(y0, rows); y < min(y0 + TY, h); ++y)
					d[(int64_t)y * wp + xp] = s[(int64_t)y * wp + xp];
		}
	};

	// ---- host side ------------------------------------------------------------------------------------------------------------------------
	constexpr int MAX_GRID_Z = 65535;

	// f(src, dst) with the pointers typed by the ABI's type character; bool frames are 0 / 1 bytes and run as uint8
	template <class F>
	hipError_t with_pixel_type(int type, const void *src, void *dst, F f)
	{
		switch (type)
		{
		case 'H':
			return f((const uint16_t *)src, (uint16_t *)dst);
		case 'B':
		case '?':
			return f((const uint8_t *)src, (uint8_t *)dst);
		default:
			return hipErrorInvalidValue;
		}
	}

	// what a pair kernel needs: rows of whole, aligned pairs
	template <class T>
	bool rows_of_pairs(const T *src, const T *dst, int w)
	{
		return (w & 1) == 0 && (((uintptr_t)src | (uintptr_t)dst) & (2 * sizeof(T) - 1)) == 0;
	}

	// the grid of a pair wave kernel (256 threads: four waves, four row bands) over n frames of wp pairs x h rows
	template <int TY, int HL>
	dim3 pair_wave_grid(int wp, int h, int n)
	{
		constexpr int OUT_LANES = 64 - 2 * HL;
		return dim3((unsigned)((wp + OUT_LANES - 1) / OUT_LANES), (unsigned)((h + 4 * TY - 1) / (4 * TY)), (unsigned)n);
	}

	// launch(src, dst, n) over the stack in chunks of at most MAX_GRID_Z frames: what one grid holds
	template <class T, class F>
	hipError_t for_frame_chunks(const T *src, T *dst, int w, int h, int nframes, F launch)
	{
		const int64_t frame = (int64_t)w * h;
		for (int f0 = 0; f0 < nframes; f0 += MAX_GRID_Z)
		{
			launch(src + frame * f0, dst + frame * f0, std::min(MAX_GRID_Z, nframes - f0));
			const hipError_t e = hipGetLastError();
			if (e != hipSuccess)
				return e;
		}
		return hipSuccess;
	}
} // namespace rir
