// Host-side launcher of the exact Euclidean distance transform (distance_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	constexpr int DISTANCE_MAX_SIDE = 16384; // w and h at most: every squared distance, 2 * 16383^2 at most, fits an int32
	constexpr int DIST2_NONE = 0x7fffffff;	 // dist2 of an image without a background pixel (RIR_DIST2_NONE)

	// what one frame takes of the workspace: the row pass's line offsets, int16 (the column pass keeps its stack in them and in dist2),
	// rounded up to the workspace's alignment
	inline size_t distance_frame_bytes(int w, int h) { return ((size_t)w * h * 2 + 7) & ~(size_t)7; }

	// dist2[n][h][w] (and index, unless null) of src[n][h][w] by the definition of rir_distance_transform_device (include/rir_amd_device.h).
	// type: '?' / 'B' (one byte), 'H' uint16, 'i' int32.  The stack is walked in groups of as many frames as `work` (8-byte aligned,
	// work_bytes >= distance_frame_bytes(w, h)) holds, two launches per group, all on `st`.  Arguments are checked by the caller;
	// hipErrorInvalidValue on an unknown type.
	hipError_t launch_distance_transform(int type, const void *src, int w, int h, int nframes, int background, int border, int rows, int *dist2,
										 int *index, void *work, size_t work_bytes, hipStream_t st);
} // namespace rir
