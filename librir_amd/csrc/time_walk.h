// The walk along time that the per-pixel reducers share: statistics (pixel_stats_slab, pixel_kernels.hip), quantiles (pixel_quantiles_count,
// pixel_quantile_kernels.hip) and the pair sums of the downsampler (ds_pair_sums, downsample_kernels.hip).  Device templates plus a little
// host code; include from .hip files only.
//
// A lane owns TW_PX = 8 adjacent pixels of a uint16 stack [n][npx] and takes them from one frame with one non-temporal 16-byte load
// (tw_load<true>; the launcher has checked frames_are_16_byte_aligned) or, where the frames do not start on 16-byte boundaries, with eight
// 2-byte loads at the offsets of tw_offsets, which are clamped into the frame: what is loaded for a pixel past the end is discarded by the
// reducer.  walk_frames<VEC>(cnt, off, frame, step[, after_set]) runs the lane over `cnt` frame steps with two named sets of TW_DEPTH
// frames, so that no set is ever copied: while one set is reduced the other is in flight (TW_DEPTH to 2 * TW_DEPTH loads per wave), a
// scheduling barrier after each set of loads keeps them ahead of the arithmetic, and the compiler can wait for one frame at a time (counted
// waits).  Steps are reduced in the order k = 0 .. cnt - 1.  Fewer than 2 * TW_DEPTH steps at the end are a tail without hook: it issues
// one more set of loads and, where no step is left (cnt a multiple of 2 * TW_DEPTH), none.
//
// The reducer supplies what differs:
//   frame(k)        the address of the frame of step k, for k up to cnt - 1 + 2 * TW_DEPTH: the reducer clamps k to cnt - 1, so that the
//                   loads past the end stay in bounds; they are not used
//   step(x, k)      one frame: the lane's 8 pixels x (pixel 2j in the low, 2j + 1 in the high half of x[j]) of step k.  The three reducers
//                   pin what a step carries to the next one there, once a frame (an empty asm with "+v" operands): left free, the compiler
//                   sums the frames of a set first, behind one wait for all of them, and takes up to 1.7 times the registers
//   after_set()     optional: called after each set of TW_DEPTH steps of the main loop (not in the tail, which reduces up to
//                   2 * TW_DEPTH - 1 steps after the last call)
//
// Host side: time_slab_plan cuts a stack along time for the reducers whose workgroups take a tile of TW_TILE pixels and a slab of frames.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace rir
{
	constexpr int TW_PX = 8;			  // pixels per lane
	constexpr int TW_TILE = 64 * TW_PX;	  // pixels per wave
	constexpr int TW_DEPTH = 4;			  // frames per set; a wave has one or two sets in flight
	constexpr int TW_TARGET_BLOCKS = 1024; // slabs are added while the grid stays within 4 workgroups on each of 256 CUs

	typedef unsigned tw_v4u __attribute__((ext_vector_type(4)));

	// Where the lane's pixels p .. p + 7 are in a frame of npx pixels.  VEC (npx is a multiple of 8, so is p): off[0] alone is used, and is 0
	// for a lane that starts at or past `limit` - npx, or the fewer pixels the reducer wants.
	template <bool VEC>
	__device__ __forceinline__ void tw_offsets(unsigned (&off)[TW_PX], int64_t p, int64_t limit, int64_t npx)
	{
#pragma unroll
		for (int j = 0; j < TW_PX; ++j)
			off[j] = VEC ? (unsigned)(p < limit ? p : 0) : (unsigned)min(p + j, npx - 1);
	}

	// The lane's 8 pixels of one frame.
	template <bool VEC>
	__device__ __forceinline__ tw_v4u tw_load(const uint16_t *__restrict__ frame, const unsigned (&off)[TW_PX])
	{
		if constexpr (VEC)
			return __builtin_nontemporal_load(reinterpret_cast<const tw_v4u *>(frame + off[0]));
		else
		{
			tw_v4u x;
#pragma unroll
			for (int j = 0; j < 4; ++j)
				x[j] = (unsigned)__builtin_nontemporal_load(frame + off[2 * j]) | (unsigned)__builtin_nontemporal_load(frame + off[2 * j + 1]) << 16;
			return x;
		}
	}

	struct TwNoHook
	{
		__device__ __forceinline__ void operator()() const {}
	};

	template <bool VEC, class Frame, class Step, class AfterSet = TwNoHook>
	__device__ __forceinline__ void walk_frames(int cnt, const unsigned (&off)[TW_PX], Frame frame, Step step, AfterSet after_set = AfterSet())
	{
		if (cnt <= 0)
			return;
		tw_v4u a0[TW_DEPTH], b0[TW_DEPTH];
#pragma unroll
		for (int d = 0; d < TW_DEPTH; ++d)
			a0[d] = tw_load<VEC>(frame(d), off);
		int k = 0;
		for (; k + 2 * TW_DEPTH <= cnt; k += 2 * TW_DEPTH)
		{
#pragma unroll
			for (int d = 0; d < TW_DEPTH; ++d)
				b0[d] = tw_load<VEC>(frame(k + TW_DEPTH + d), off);
			__builtin_amdgcn_sched_barrier(0); // the loads stay ahead of the arithmetic
#pragma unroll
			for (int d = 0; d < TW_DEPTH; ++d)
				step(a0[d], k + d);
			after_set();
#pragma unroll
			for (int d = 0; d < TW_DEPTH; ++d)
				a0[d] = tw_load<VEC>(frame(k + 2 * TW_DEPTH + d), off);
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int d = 0; d < TW_DEPTH; ++d)
				step(b0[d], k + TW_DEPTH + d);
			after_set();
		}
		if (k == cnt)
			return;
		// 1 .. 2 * TW_DEPTH - 1 steps are left, the first TW_DEPTH of them loaded
#pragma unroll
		for (int d = 0; d < TW_DEPTH - 1; ++d)
			b0[d] = tw_load<VEC>(frame(k + TW_DEPTH + d), off);
#pragma unroll
		for (int d = 0; d < TW_DEPTH; ++d)
			if (k + d < cnt)
				step(a0[d], k + d);
#pragma unroll
		for (int d = 0; d < TW_DEPTH - 1; ++d)
			if (k + TW_DEPTH + d < cnt)
				step(b0[d], k + TW_DEPTH + d);
	}

	// Host side.

	// "Every frame starts on a 16-byte boundary": what tw_load<true> needs of a stack [n][npx] and of whatever else is read like a frame
	// (a null pointer passes: it is not read).
	template <class... P>
	inline bool frames_are_16_byte_aligned(int64_t npx, const P *...ptr)
	{
		return npx % TW_PX == 0 && (((uintptr_t)ptr % 16 == 0) && ...);
	}

	// How a stack of n frames of npx pixels is cut along time: `slabs` workgroups per tile of TW_TILE pixels, `per_slab` frames each (the last
	// one may be shorter).  Slabs are added while the grid stays within TW_TARGET_BLOCKS workgroups and a slab keeps slab_min frames; it holds
	// at most slab_max.
	struct TimeSlabs
	{
		int slabs, per_slab;
	};
	inline TimeSlabs time_slab_plan(int64_t npx, int n, int slab_min, int slab_max)
	{
		const int64_t tiles = (npx + TW_TILE - 1) / TW_TILE;
		const int64_t want = std::max<int64_t>(1, TW_TARGET_BLOCKS / tiles);
		const int64_t per_slab = std::min<int64_t>(std::max<int64_t>(((int64_t)n + want - 1) / want, slab_min), slab_max);
		return TimeSlabs{(int)std::max<int64_t>(1, ((int64_t)n + per_slab - 1) / per_slab), (int)per_slab};
	}
} // namespace rir
