// Host-side launcher of the component tracking (track_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	// The bounds of a call: pixels of a frame and nodes (n * nlabels) both fit an int32 index with room for a workgroup's overshoot.
	constexpr int64_t TRACK_MAX_INDEX = 0x7FFF0000LL;

	// w, h >= 1 with w * h <= TRACK_MAX_INDEX, n >= 0, nlabels >= 1 with n * nlabels <= TRACK_MAX_INDEX.
	bool track_geometry_ok(int w, int h, int n, int nlabels);

	// Device scratch of one call (0: geometry refused): the forest and each node's final root (4 bytes a node each), the root bitmaps and
	// the per-wave and per-block root counts, plus 64 bytes to find a 64-byte boundary in an 8-byte aligned block.
	size_t track_workspace_bytes(int w, int h, int n, int nlabels);

	// Tracks of the components of labels[n][h][w] (the definition is with rir_track_components_device, include/rir_amd_device.h).  counts
	// and dst may be null; dst may be labels.  Arguments are checked by the caller (geometry, table_entries >= 1, no overlaps, work >=
	// track_workspace_bytes and 8-byte aligned).
	hipError_t launch_track_components(const int32_t *labels, const int32_t *counts, int w, int h, int n, int nlabels, int32_t *track_of, int32_t *info,
									   int32_t *first_frame, int32_t *last_frame, int32_t *first_label, int32_t *components, int table_entries,
									   int32_t *dst, void *work, hipStream_t st);
} // namespace rir
