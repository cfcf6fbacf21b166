// Host-side launchers of the per-pixel quantiles over time (pixel_quantile_kernels.hip).  C++ linkage, internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "quantile_kernels.h"

namespace rir
{
	// An MSB-first radix select over the 16-bit value, 4 bits a pass: a sequence is streamed this many times.
	constexpr int PIXEL_QUANTILE_PASSES = 4;
	// Percents that one read of the frames counts for in passes 1 .. 3 (pass 0 counts once for all of them).
	constexpr int PIXEL_QUANTILE_GROUP = 4;
	// The state is uint32 [npercents][PIXEL_QUANTILE_ROWS][npx]: per percent 16 rows of digit counts of the open pass, the row of prefixes (the
	// high bits fixed so far) and the row of ranks left inside the prefix's bucket (0: the value is decided, 0 or -1).  Pass 0 counts into
	// the rows of percent 0 for all percents.  All zero is the empty state.
	constexpr int PIXEL_QUANTILE_ROWS = 18;

	size_t pixel_quantiles_state_bytes(int64_t npx, int npercents); // 72 * npercents * npx

	// Add the digit counts of frames[n][npx] (uint16) for pass `pass` into the state.  Arguments are checked by the caller (n >= 1,
	// npx < 2^31, 0 <= pass < PIXEL_QUANTILE_PASSES, 1 <= npercents <= 8, state 8-byte aligned, no overlap).
	hipError_t launch_pixel_quantiles_count(const uint16_t *frames, int64_t npx, int n, int npercents, int pass, void *state, hipStream_t st);

	// Close pass `pass` over `total` frames: extend every prefix by the digit that holds the rank and clear the counts; the last pass writes
	// values [npercents][npx] by the rule of rir_pixel_quantiles_device.
	hipError_t launch_pixel_quantiles_resolve(int64_t npx, const QuantilePercents &percents, int npercents, int pass, uint32_t total, void *state,
											  int32_t *values, hipStream_t st);
} // namespace rir
