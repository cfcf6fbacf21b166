// Adaptive temporal downsampling of a uint16 frame stack (the definition is with rir_downsampler_push_device, include/rir_amd_device.h).
// Two streaming passes over the frames, the keep / drop recurrence runs on the host between them (downsample.cpp):
//
//   ds_pair_sums   one workgroup per (tile of DS_TILE pixels, slab of DS_SLAB frames).  A lane owns 8 adjacent pixels (one 16-byte load per
//                  frame) and walks the slab's frames in order (walk_frames, time_walk.h) with the previous frame's pixels in registers, so every frame is read once
//                  (the frame before a slab is read a second time: 1 / DS_SLAB more).  Per frame the lane has a 32-bit sum of |d| and a 64-bit
//                  sum of d^2 (8 * 65535^2 does not fit 32 bits); the wave adds them up with shuffles, the four waves meet in LDS, and the
//                  workgroup leaves one pair of int64 per frame in the partials [n][tiles][2].
//   ds_fold_sums   one wave per frame adds the tiles' partials into the table [n][2].
//   ds_max_hold    one workgroup per (tile, segment of the table): the per-pixel maximum of the segment's frames - packed 16-bit maxima, 8
//                  pixels a lane - for the first `size` pixels, the last frame's pixels after them; stored 16 bytes a lane into the kept image
//                  or, for the open run at the end of a push, into the carried maximum.  Each source frame is read once and each output
//                  written once.
//
// Integer adds and maxima only: no floating point, no atomics, nothing that depends on the order the workgroups run in.  The partials
// with a second kernel were chosen over one 64-bit atomic per workgroup and frame because they need no zeroed table and the fold takes
// 6 us beside the pass's 157 on 1 000 frames of 640x512.
#include <algorithm>

#include "downsample_kernels.h"
#include "time_walk.h"

namespace rir
{
	constexpr int DS_BLOCK = 256;
	constexpr int DS_WAVES = DS_BLOCK / 64;
	constexpr int DS_TILE = DS_BLOCK * TW_PX; // pixels per workgroup
	static_assert(DS_SLAB <= DS_BLOCK && DS_SLAB % (2 * TW_DEPTH) == 0, "a thread per frame of the slab writes the partials");

	typedef unsigned short ds_v8h __attribute__((ext_vector_type(8)));

	template <bool VEC>
	__global__ __launch_bounds__(DS_BLOCK) void ds_pair_sums(const uint16_t *__restrict__ frames, const uint16_t *__restrict__ prev, int64_t npx,
															 int64_t size, int n, int tiles, int64_t *__restrict__ partials)
	{
		__shared__ unsigned long long lds[DS_SLAB][DS_WAVES][2];
		const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
		const int f0 = blockIdx.y * DS_SLAB, cnt = min(DS_SLAB, n - f0);
		const int64_t p = (int64_t)blockIdx.x * DS_TILE + (int64_t)threadIdx.x * TW_PX;

		unsigned off[TW_PX];
		tw_offsets<VEC>(off, p, size, npx);
		tw_v4u mask; // the pixels below `size`: what is loaded for the others is masked out
#pragma unroll
		for (int j = 0; j < 4; ++j)
			mask[j] = (p + 2 * j < size ? 0xFFFFu : 0u) | (p + 2 * j + 1 < size ? 0xFFFF0000u : 0u);

		// frame k of the slab, clamped to its last one (loads past the end stay in bounds and are not used); k = -1: the frame before the
		// slab - the carried image ahead of the stack, and where there is none frame 0 itself, whose sums are then zero
		auto frame = [&](int k) {
			const int64_t f = (int64_t)f0 + min(k, cnt - 1);
			return f >= 0 ? frames + f * npx : (prev ? prev : frames);
		};
		tw_v4u before = tw_load<VEC>(frame(-1), off) & mask;
		auto step = [&](tw_v4u x, int k) {
			x &= mask;
			asm("" : "+v"(before)); // one frame at a time, behind its own wait
			unsigned sx = 0;
			unsigned long long sq = 0;
#pragma unroll
			for (int j = 0; j < 4; ++j)
			{
				const unsigned alo = x[j] & 0xFFFFu, ahi = x[j] >> 16, blo = before[j] & 0xFFFFu, bhi = before[j] >> 16;
				const unsigned dlo = alo > blo ? alo - blo : blo - alo, dhi = ahi > bhi ? ahi - bhi : bhi - ahi;
				sx += dlo + dhi;
				sq += (unsigned long long)(dlo * dlo); // 65535^2 < 2^32
				sq += (unsigned long long)(dhi * dhi);
			}
			before = x;
#pragma unroll
			for (int m = 32; m >= 1; m >>= 1)
			{
				sx += __shfl_xor(sx, m);
				sq += __shfl_xor(sq, m);
			}
			if (lane == 0)
			{
				lds[k][wave][0] = sx;
				lds[k][wave][1] = sq;
			}
		};

		walk_frames<VEC>(cnt, off, frame, step);
		__syncthreads();
		if ((int)threadIdx.x < cnt)
		{
			unsigned long long sx = 0, sq = 0;
#pragma unroll
			for (int w = 0; w < DS_WAVES; ++w)
			{
				sx += lds[threadIdx.x][w][0];
				sq += lds[threadIdx.x][w][1];
			}
			int64_t *at = partials + ((int64_t)(f0 + (int)threadIdx.x) * tiles + blockIdx.x) * 2;
			at[0] = (int64_t)sx;
			at[1] = (int64_t)sq;
		}
	}

	__global__ __launch_bounds__(64) void ds_fold_sums(const int64_t *__restrict__ partials, int tiles, int64_t *__restrict__ sums)
	{
		const int64_t *row = partials + (int64_t)blockIdx.x * tiles * 2;
		unsigned long long sx = 0, sq = 0;
		for (int t = threadIdx.x; t < tiles; t += 64)
		{
			sx += (unsigned long long)row[2 * t];
			sq += (unsigned long long)row[2 * t + 1];
		}
#pragma unroll
		for (int m = 32; m >= 1; m >>= 1)
		{
			sx += __shfl_xor(sx, m);
			sq += __shfl_xor(sq, m);
		}
		if (threadIdx.x == 0)
		{
			sums[2 * (int64_t)blockIdx.x] = (int64_t)sx;
			sums[2 * (int64_t)blockIdx.x + 1] = (int64_t)sq;
		}
	}

	template <bool VEC>
	__global__ __launch_bounds__(DS_BLOCK) void ds_max_hold(const uint16_t *__restrict__ frames, const uint16_t *__restrict__ max_in,
															uint16_t *__restrict__ max_out, uint16_t *__restrict__ out, int64_t npx, int64_t size,
															const DsSegment *__restrict__ segs)
	{
		const DsSegment sg = segs[blockIdx.y];
		const int cnt = sg.last - sg.first + 1;
		const uint16_t *first = frames + (int64_t)sg.first * npx, *last = frames + (int64_t)sg.last * npx;
		uint16_t *dst = sg.slot >= 0 ? out + (int64_t)sg.slot * npx : max_out;
		const int64_t tile = (int64_t)blockIdx.x * DS_TILE;
		if constexpr (VEC)
		{
			const int64_t p = tile + (int64_t)threadIdx.x * TW_PX;
			if (p >= npx) // npx is a multiple of 8 here: a lane's pixels are all inside or all outside
				return;
			ds_v8h m = 0;
			if (sg.carry)
				m = *reinterpret_cast<const ds_v8h *>(max_in + p);
			const uint16_t *at = first + p;
			int k = 0;
			for (; k + TW_DEPTH <= cnt; k += TW_DEPTH)
			{
				ds_v8h x[TW_DEPTH];
#pragma unroll
				for (int d = 0; d < TW_DEPTH; ++d)
					x[d] = __builtin_nontemporal_load(reinterpret_cast<const ds_v8h *>(at + (int64_t)(k + d) * npx));
#pragma unroll
				for (int d = 0; d < TW_DEPTH; ++d)
					m = __builtin_elementwise_max(m, x[d]);
			}
			for (; k < cnt; ++k)
				m = __builtin_elementwise_max(m, __builtin_nontemporal_load(reinterpret_cast<const ds_v8h *>(at + (int64_t)k * npx)));
			if (p + TW_PX > size) // the rows that are not held: the last frame's
			{
				const ds_v8h l = *reinterpret_cast<const ds_v8h *>(last + p);
#pragma unroll
				for (int j = 0; j < TW_PX; ++j)
					if (p + j >= size)
						m[j] = l[j];
			}
			__builtin_nontemporal_store(m, reinterpret_cast<ds_v8h *>(dst + p));
		}
		else
		{
#pragma unroll 1
			for (int j = 0; j < TW_PX; ++j)
			{
				const int64_t i = tile + j * DS_BLOCK + threadIdx.x;
				if (i >= npx)
					break;
				unsigned m;
				if (i < size)
				{
					m = sg.carry ? max_in[i] : 0;
					for (int k = 0; k < cnt; ++k)
						m = max(m, (unsigned)first[(int64_t)k * npx + i]);
				}
				else
					m = last[i];
				dst[i] = (uint16_t)m;
			}
		}
	}

	namespace
	{
		int64_t ds_tiles(int64_t px) { return (px + DS_TILE - 1) / DS_TILE; }
	} // namespace

	size_t downsample_partials_bytes(int64_t size, int n) { return (size_t)ds_tiles(size) * (size_t)n * 2 * sizeof(int64_t); }

	hipError_t launch_pair_sums(const uint16_t *frames, const uint16_t *prev, int64_t npx, int64_t size, int n, int64_t *partials, int64_t *sums,
								hipStream_t st)
	{
		const int64_t slabs = ((int64_t)n + DS_SLAB - 1) / DS_SLAB;
		if (n <= 0 || size < 1 || size > npx || npx >= (1ll << 31) || slabs > 65535)
			return hipErrorInvalidValue;
		const int tiles = (int)ds_tiles(size);
		const dim3 grid((unsigned)tiles, (unsigned)slabs);
		if (frames_are_16_byte_aligned(npx, frames, prev))
			ds_pair_sums<true><<<grid, DS_BLOCK, 0, st>>>(frames, prev, npx, size, n, tiles, partials);
		else
			ds_pair_sums<false><<<grid, DS_BLOCK, 0, st>>>(frames, prev, npx, size, n, tiles, partials);
		ds_fold_sums<<<(unsigned)n, 64, 0, st>>>(partials, tiles, sums);
		return hipGetLastError();
	}

	hipError_t launch_max_hold(const uint16_t *frames, const uint16_t *max_in, uint16_t *max_out, uint16_t *out, int64_t npx, int64_t size,
							   const DsSegment *segs, int nsegs, hipStream_t st)
	{
		if (nsegs <= 0 || size < 1 || size > npx || npx >= (1ll << 31))
			return hipErrorInvalidValue;
		const bool vec = frames_are_16_byte_aligned(npx, frames, max_in, max_out, out);
		for (int s0 = 0; s0 < nsegs; s0 += 65535) // (the grid's second dimension)
		{
			const dim3 grid((unsigned)ds_tiles(npx), (unsigned)std::min(65535, nsegs - s0));
			if (vec)
				ds_max_hold<true><<<grid, DS_BLOCK, 0, st>>>(frames, max_in, max_out, out, npx, size, segs + s0);
			else
				ds_max_hold<false><<<grid, DS_BLOCK, 0, st>>>(frames, max_in, max_out, out, npx, size, segs + s0);
		}
		return hipGetLastError();
	}
} // namespace rir
