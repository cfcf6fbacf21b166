// The wave-tile scheme shared by the frame-buffer units — gfx950 (CDNA4): filter_kernels.hip includes it itself, morphology_kernels.hip and
// rank_kernels.hip through pair_tile.h, which adds the form with two columns per lane.  Device code only: include it from a .hip unit,
// inside no namespace.  Everything here is __forceinline__, so each unit's kernels carry their own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace rir
{
	// XCD-aware workgroup order.  The dispatcher deals workgroups round-robin to the 8 XCDs of the MI355X, each
	// with its own L2: neighbours in the launch order never share a cache.  Re-reading the linear id "XCD-major"
	// (XCD k owns the k-th eighth of the logical order) makes logical neighbours - tiles that share halo rows or
	// split cache lines - run on the same XCD one after the other.  Measured: gaussian_filter 0.173 -> 0.131 ms per
	// 256 frames, translate (63-pixel tile rows, never line-aligned) 0.109 -> 0.097 ms; the 3x3 median, bound by
	// its instruction count, gains nothing and keeps the plain order.
	__device__ __forceinline__ unsigned xcd_major(unsigned id, unsigned total)
	{
		const unsigned per = total / 8u;
		return id < per * 8u ? (id % 8u) * per + id / 8u : id;
	}

	// ---- the wave-tile scheme -------------------------------------------------------------------
	// translate, the two gaussians, the fused chain, the 3x3 median, the 3x3 / 5x5 / 7x7 morphology and the 3x3 / 5x5 window medians work the
	// same way: a WAVE owns a
	// tile of 64 columns x TY rows, a lane one column - its pixels in registers, fetched with one raw-buffer load per row - and the
	// neighbouring columns come from the neighbouring lanes through DPP wave shifts: no LDS, no barrier.  The parts of the scheme are
	// written once, here.

	// The tile of a workgroup (its four waves take four consecutive row bands of it): XCD-major order, then (frame, ...) with
	// either index fastest.  Row band fastest: vertically adjacent tiles, which share their halo rows, run on the same XCD
	// back to back.  Column fastest, for tiles whose rows are not line-aligned (63- and 60-pixel rows): neighbours along x
	// split cache lines of the same rows - on one XCD, one after the other, the second half of a line is an L2 hit and the
	// two halves of a written line merge before they leave for HBM.
	struct TileId
	{
		int bx, by, n;
	};
	template <bool COLUMN_FASTEST>
	__device__ __forceinline__ TileId tile_decode()
	{
		const unsigned gx = gridDim.x, gy = gridDim.y;
		const unsigned id = xcd_major(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), gx * gy * gridDim.z);
		if constexpr (COLUMN_FASTEST)
			return {(int)(id % gx), (int)((id / gx) % gy), (int)(id / (gx * gy))};
		else
			return {(int)((id / gy) % gx), (int)(id % gy), (int)(id / (gy * gx))};
	}

	// lane i <- lane i + 1 (0 into lane 63) / lane i <- lane i - 1 (0 into lane 0), for 4- and 8-byte values
	template <int CTRL, class T>
	__device__ __forceinline__ T wave_shift1(T v)
	{
		static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two dwords");
		if constexpr (sizeof(T) == 4)
			return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
		else
		{
			const uint64_t b = __builtin_bit_cast(uint64_t, v);
			const uint32_t lo = wave_shift1<CTRL>((uint32_t)b), hi = wave_shift1<CTRL>((uint32_t)(b >> 32));
			return __builtin_bit_cast(T, (uint64_t)lo | ((uint64_t)hi << 32));
		}
	}
	template <class T>
	__device__ __forceinline__ T wave_shl1(T v) { return wave_shift1<0x130>(v); }
	template <class T>
	__device__ __forceinline__ T wave_shr1(T v) { return wave_shift1<0x138>(v); }

	// Raw-buffer descriptor over `bytes` bytes at p (wave-uniform; made scalar here).  An access whose byte offset lies outside
	// [0, bytes) reads as 0 and stores nothing - the range check the kernels below lean on; it covers the per-lane offset only,
	// the scalar offset is NOT checked.  A descriptor holds 32 bits of size: a frame of BUFFER_FRAME_LIMIT bytes or more
	// takes plain loads and stores instead.
	constexpr int64_t BUFFER_FRAME_LIMIT = (int64_t)1 << 31; // 2 GiB
	template <class T>
	__device__ __forceinline__ bool frame_fits_buffer(int w, int h)
	{
		return (int64_t)w * h * (int64_t)sizeof(T) < BUFFER_FRAME_LIMIT;
	}
	__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void *p, int bytes)
	{
		const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)p);
		const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)p >> 32));
		return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, bytes, 0x00020000);
	}
	template <class T>
	__device__ __forceinline__ T buffer_load_px(__amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff)
	{
		if constexpr (sizeof(T) == 1)
			return __builtin_bit_cast(T, (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)voff, (int)soff, 0));
		else if constexpr (sizeof(T) == 2)
			return __builtin_bit_cast(T, (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, (int)voff, (int)soff, 0));
		else if constexpr (sizeof(T) == 4)
			return __builtin_bit_cast(T, (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, (int)soff, 0));
		else
			return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)voff, (int)soff, 0));
	}

	// A lane's column: rows ytop .. ytop + NR - 1 of column x0 + lane of frame s, as raw values (a uint16 pixel as a uint32).
	// Returns whether the whole 64 x NR block lies inside the image (wave-uniform).  A pixel outside the image reads as 0 - what
	// such a pixel adds to a sum; without ZERO_OUTSIDE, for callers that never use it or drop it themselves, it is left
	// unspecified (frames of 2 GiB and more then give the nearest pixel of the frame, with no select behind the load).
	// Raw-buffer loads over the frame: a pixel outside the image has a byte offset outside the buffer (rows above: negative =
	// huge unsigned; rows below: past the end; columns outside: forced there) and the hardware returns 0 for it.  No branch,
	// no select, one add per row, and all NR loads are in flight together (a load under a condition becomes a branch with its
	// own wait: that many serial latencies).  INSIDE_BRANCH: a block inside the image gets a branch of its own with one lane
	// offset and the row steps on the scalar side.
	template <class T>
	using raw_px_t = typename std::conditional<sizeof(T) == 2, uint32_t, T>::type;
	template <int NR, class T, bool INSIDE_BRANCH, bool ZERO_OUTSIDE>
	__device__ __forceinline__ bool load_column(const T *__restrict__ s, int w, int h, int x0, int lane, int ytop, raw_px_t<T> (&v)[NR])
	{
		const int x = x0 + lane;
		const bool xin = x >= 0 && x < w;
		if (frame_fits_buffer<T>(w, h))
		{
			const __amdgpu_buffer_rsrc_t rs = buffer_rsrc(s, w * h * (int)sizeof(T));
			const uint32_t step = (uint32_t)w * (uint32_t)sizeof(T);
			if (INSIDE_BRANCH && x0 >= 0 && x0 + 63 < w && ytop >= 0 && ytop + NR <= h)
			{
				const uint32_t off = (uint32_t)((ytop * w + x) * (int)sizeof(T));
#pragma unroll
				for (int i = 0; i < NR; ++i)
					v[i] = buffer_load_px<T>(rs, off, (uint32_t)i * step);
				return true;
			}
			uint32_t off = xin ? (uint32_t)((ytop * w + x) * (int)sizeof(T)) : 0x80000000u;
#pragma unroll
			for (int i = 0; i < NR; ++i)
			{
				v[i] = buffer_load_px<T>(rs, off, 0);
				off += step;
			}
			return false;
		}
		// frames of 2 GiB and more: plain loads at addresses clamped into the frame
		const T *col = s + min(max(x, 0), w - 1);
#pragma unroll
		for (int i = 0; i < NR; ++i)
		{
			const int gy = ytop + i;
			const T val = col[(int64_t)min(max(gy, 0), h - 1) * w];
			v[i] = (!ZERO_OUTSIDE || (xin && gy >= 0 && gy < h)) ? val : T(0);
		}
		return false;
	}
} // namespace rir
