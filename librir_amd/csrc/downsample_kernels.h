// Host-side launchers of the adaptive temporal downsampling (downsample_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	constexpr int DS_SLAB = 64; // frames a workgroup of the pair sums walks: a stack is cut along time every DS_SLAB frames
	constexpr int DS_MAX_FRAMES = 65535 * DS_SLAB; // the frames launch_pair_sums takes: its slabs are the grid's second dimension

	// One kept image (slot >= 0: image `slot` of the output) or the open trailing run (slot < 0: the carried maximum) of the max-hold:
	// source frames first .. last of this push, and whether the maximum carried in from the push before takes part.
	struct DsSegment
	{
		int first, last, slot, carry;
	};

	// int64 [n][tiles][2] partial sums between the two kernels of the pair sums
	size_t downsample_partials_bytes(int64_t size, int n);

	// sums[i] = { sum |d|, sum d^2 } over the first `size` pixels, d = frames[i] - frames[i - 1], frames[-1] = prev; without prev (the first
	// image of a stream) sums[0] = {0, 0}.  frames: uint16 [n][npx], n >= 1, 2 <= size <= npx < 2^31.
	hipError_t launch_pair_sums(const uint16_t *frames, const uint16_t *prev, int64_t npx, int64_t size, int n, int64_t *partials, int64_t *sums,
								hipStream_t st);

	// For every segment: the per-pixel maximum of its frames (and of max_in when it carries) over the first `size` pixels, the last frame's
	// pixels from there on, written to out[slot] or, for the open run, to max_out.  max_in != max_out; segs on the device.
	hipError_t launch_max_hold(const uint16_t *frames, const uint16_t *max_in, uint16_t *max_out, uint16_t *out, int64_t npx, int64_t size,
							   const DsSegment *segs, int nsegs, hipStream_t st);
} // namespace rir
