// Host-side launcher of grey-level morphological reconstruction (reconstruct_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rir
{
	constexpr int RECONSTRUCT_TILE_W = 64, RECONSTRUCT_TILE_H = 32; // what one workgroup converges in LDS per round
	constexpr int RECONSTRUCT_MARKERS = 3;							 // marker_mode: 0 explicit, 1 the mask shifted by param, 2 the mask on the border

	// what one frame takes of the workspace: its "changed" flag of three consecutive rounds (int32 each), rounded up to 16 bytes
	constexpr size_t RECONSTRUCT_FRAME_BYTES = 16;

	// how many rounds a stack of w x rows images can take at most: a round does at least one plain 3x3 (or cross) iteration everywhere, the
	// plain iteration moves a value one pixel per step along a path that visits no pixel twice, and one more round finds nothing to write
	inline int64_t reconstruct_round_cap(int w, int rows) { return (int64_t)w * rows + 2; }

	// dst[n][h][w] by the definition of rir_reconstruct_device (include/rir_amd_device.h).  type: '?' / 'B' (one byte), 'H' uint16.  The
	// stack is walked in groups of as many frames as `work` (8-byte aligned, work_bytes >= RECONSTRUCT_FRAME_BYTES) holds; a group runs
	// rounds - one launch each, on `st` - until the flags of a round, read through `h_flags` (page-locked, as many ints as a group has
	// frames), say that no frame changed.  SYNCHRONOUS: it waits for `st` between rounds.  *rounds (never null): the largest number of
	// rounds a group took; *converged: false when a group reached reconstruct_round_cap().  Arguments are checked by the caller;
	// hipErrorInvalidValue on an unknown type.
	hipError_t launch_reconstruct(int type, const void *mask, const void *marker, void *dst, int w, int h, int nframes, int method, int connectivity,
								  int marker_mode, int param, int output, int rows, void *work, size_t work_bytes, int *h_flags, int *rounds,
								  bool *converged, hipStream_t st);
	// the frames of a group for a workspace of work_bytes: what h_flags must hold
	int reconstruct_group_frames(int nframes, size_t work_bytes);
} // namespace rir
