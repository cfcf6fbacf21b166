// Per-pixel quantiles over time of a uint16 frame stack (the definition is with rir_pixel_quantiles_device, include/rir_amd_device.h): an
// MSB-first radix select over the 16-bit value, 4 bits a pass.  Per (percent, pixel) the state holds the prefix fixed so far and the rank
// left inside that prefix's bucket (pixel_quantile_kernels.h).  Each pass has two kernels:
//
//   pixel_quantiles_count    one workgroup per (tile of PQ_TILE pixels, slab of frames), for a group of G percents.  The walk of time_walk.h:
//                            a lane owns 8 adjacent pixels (one 16-byte load per frame), the waves take the same pixels and every
//                            WAVES-th frame of the slab each, TW_DEPTH to 2 * TW_DEPTH loads in flight per wave.  Per (percent, pixel) a
//                            lane keeps one 64-bit accumulator of sixteen 4-bit fields: a sample whose high bits equal the prefix adds
//                            1 << (4 * digit), no register is indexed at run time.  Every PQ_FLUSH_SETS * TW_DEPTH frames, before a field
//                            can wrap, the fields are added to the workgroup's 32-bit counters in LDS, laid out [percent][digit][pixel
//                            of the lane][lane] so that the bank is the lane (ds_add_u32, shared by the waves).  At the end the workgroup
//                            adds its non-zero counters to the state: plain loads and stores where the tile has one owner in the launch
//                            (one slab), native 32-bit atomic adds where the time axis is cut into slabs (few pixels, many frames).
//   pixel_quantiles_resolve  one thread a pixel, no frames: per percent it walks the 16 counts to the digit whose bucket holds the rank,
//                            subtracts what lies below, extends the prefix and clears the counts.  Pass 0 computes the rank t from the
//                            frame count (qt_rank: the only floating-point operation); the last pass writes the values.
//
// Every combination is a 32-bit integer add, so the result depends neither on the order the workgroups run in nor on how the sequence is
// split into calls.
#include <limits.h>

#include <algorithm>

#include "pixel_quantile_kernels.h"
#include "quantile_rank.h"
#include "time_walk.h"

namespace rir
{
	constexpr int PQ_TILE = TW_TILE;		// pixels per workgroup: its waves take the same ones
	constexpr int PQ_FLUSH_SETS = 3;		// sets between two flushes of the 4-bit fields
	constexpr int PQ_DIGITS = 16;			// buckets of a pass
	constexpr int PQ_SLAB_MIN = 512;		// frames per slab at least (unless the stack is shorter)
	constexpr int PQ_RESOLVE_BLOCK = 256;
	// between two flushes a field counts at most PQ_FLUSH_SETS * TW_DEPTH frames, or (PQ_FLUSH_SETS - 1) * TW_DEPTH and the tail of a wave
	static_assert(PQ_FLUSH_SETS * TW_DEPTH <= 15 && (PQ_FLUSH_SETS - 1) * TW_DEPTH + 2 * TW_DEPTH - 1 <= 15, "a 4-bit field cannot wrap");
	static_assert(PIXEL_QUANTILE_PASSES * 4 == 16 && PIXEL_QUANTILE_ROWS == PQ_DIGITS + 2, "4 bits a pass; counts, prefix, rank");
	static_assert(PIXEL_QUANTILE_GROUP == 4 && QUANTILE_MAX_PERCENTS == 8, "the launcher instantiates groups of 1 .. 4 percents");

	// threads of a counting workgroup: the LDS counters of G percents take G * 32 KiB, so one percent leaves room for five workgroups of
	// four waves on a CU, more percents for fewer, larger ones
	constexpr int pq_block(int G) { return G == 1 ? 256 : 512; }

	__device__ __forceinline__ uint32_t *pq_row(uint32_t *state, int64_t npx, int percent, int row)
	{
		return state + ((int64_t)percent * PIXEL_QUANTILE_ROWS + row) * npx;
	}

	// One frame: v >> shift is the sample's prefix and digit; it counts where the prefix is the pixel's (pre = prefix << 4).
	template <int G>
	__device__ __forceinline__ void pq_frame(unsigned long long (&acc)[G][TW_PX], const unsigned (&pre)[G][TW_PX], tw_v4u x, int shift)
	{
#pragma unroll
		for (int g = 0; g < G; ++g) // the fields stay one frame's adds: left free, the frames of a set are summed first, behind one wait for all
#pragma unroll
			for (int j = 0; j < TW_PX; ++j)
				asm("" : "+v"(acc[g][j]));
#pragma unroll
		for (int j = 0; j < 4; ++j)
		{
			const unsigned w = x[j], lo = (w & 0xFFFFu) >> shift, hi = w >> (16 + shift);
#pragma unroll
			for (int g = 0; g < G; ++g)
			{
				const unsigned a = lo ^ pre[g][2 * j], b = hi ^ pre[g][2 * j + 1]; // < 16: the digit, the prefix matches
				acc[g][2 * j] += (unsigned long long)(a < 16u ? 1u : 0u) << ((a & 15u) * 4u);
				acc[g][2 * j + 1] += (unsigned long long)(b < 16u ? 1u : 0u) << ((b & 15u) * 4u);
			}
		}
	}

	// Add the 4-bit fields to the workgroup's counters lds[g][digit][pixel of the lane][lane] and clear them.
	template <int G>
	__device__ __forceinline__ void pq_flush(unsigned long long (&acc)[G][TW_PX], uint32_t *lds, int lane)
	{
#pragma unroll 1
		for (int d = 0; d < PQ_DIGITS / 2; ++d) // digits d (low word) and d + 8 (high word)
		{
#pragma unroll
			for (int g = 0; g < G; ++g)
#pragma unroll
				for (int j = 0; j < TW_PX; ++j)
				{
					const uint32_t lo = ((uint32_t)acc[g][j] >> (4 * d)) & 15u, hi = ((uint32_t)(acc[g][j] >> 32) >> (4 * d)) & 15u;
					__hip_atomic_fetch_add(lds + ((g * PQ_DIGITS + d) * TW_PX + j) * 64 + lane, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					__hip_atomic_fetch_add(lds + ((g * PQ_DIGITS + d + 8) * TW_PX + j) * 64 + lane, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				}
		}
#pragma unroll
		for (int g = 0; g < G; ++g)
#pragma unroll
			for (int j = 0; j < TW_PX; ++j)
				acc[g][j] = 0;
	}

	// Counts of the digit (v >> shift) & 15 among the samples of percents j0 .. j0 + G - 1 whose higher bits equal the percent's prefix.
	template <int G, bool VEC, bool ATOMIC>
	__global__ __launch_bounds__(pq_block(G)) void pixel_quantiles_count(const uint16_t *__restrict__ frames, int64_t npx, int n, int per_slab, int shift,
																		  int j0, uint32_t *__restrict__ state)
	{
		constexpr int BLOCK = pq_block(G), WAVES = BLOCK / 64, CELLS = G * PQ_DIGITS * PQ_TILE;
		__shared__ uint32_t lds[CELLS];
		const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
		const int64_t f0 = (int64_t)blockIdx.y * per_slab, f1 = min(f0 + per_slab, (int64_t)n);
		const int cnt = f1 - f0 > wave ? (int)((f1 - f0 - wave + WAVES - 1) / WAVES) : 0; // this wave's frames: f0 + wave + WAVES * k
		const int64_t tile = (int64_t)blockIdx.x * PQ_TILE, p = tile + lane * TW_PX;

		for (int i = threadIdx.x; i < CELLS; i += BLOCK)
			lds[i] = 0;
		unsigned off[TW_PX];
		unsigned pre[G][TW_PX];
		unsigned long long acc[G][TW_PX];
		tw_offsets<VEC>(off, p, npx, npx);
#pragma unroll
		for (int j = 0; j < TW_PX; ++j)
		{
			const int64_t at = min(p + j, npx - 1); // a pixel past the end counts what the last one does, and is never stored
#pragma unroll
			for (int g = 0; g < G; ++g)
			{
				pre[g][j] = pq_row(state, npx, j0 + g, PQ_DIGITS)[at] << 4;
				acc[g][j] = 0;
			}
		}
		__syncthreads();

		int sets = 0; // sets counted since the last flush: at most PQ_FLUSH_SETS - 1 when the walk's tail begins
		walk_frames<VEC>( // the frame of step k is clamped to the wave's last one
			cnt, off, [&](int k) { return frames + (f0 + wave + (int64_t)WAVES * min(k, cnt - 1)) * npx; },
			[&](tw_v4u x, int) { pq_frame<G>(acc, pre, x, shift); },
			[&] {
				if (++sets == PQ_FLUSH_SETS)
				{
					pq_flush<G>(acc, lds, lane);
					sets = 0;
				}
			});
		if (cnt > 0)
			pq_flush<G>(acc, lds, lane);
		__syncthreads();

		// counter e = (g * 16 + digit) * PQ_TILE + q of pixel tile + q: consecutive threads, consecutive pixels
		for (int e = threadIdx.x; e < CELLS; e += BLOCK)
		{
			const int q = e % PQ_TILE, gd = e / PQ_TILE;
			const int64_t i = tile + q;
			if (i >= npx)
				continue;
			const uint32_t c = lds[(gd * TW_PX + q % TW_PX) * 64 + q / TW_PX];
			if (c == 0)
				continue;
			uint32_t *dst = pq_row(state, npx, j0 + gd / PQ_DIGITS, gd % PQ_DIGITS) + i;
			if constexpr (ATOMIC)
				__hip_atomic_fetch_add(dst, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			else
				*dst += c;
		}
	}

	__global__ __launch_bounds__(PQ_RESOLVE_BLOCK) void pixel_quantiles_resolve(uint32_t *__restrict__ state, int64_t npx, int nq, QuantilePercents pc,
																				 int pass, uint32_t total, int32_t *__restrict__ values)
	{
		const int64_t i = (int64_t)blockIdx.x * PQ_RESOLVE_BLOCK + threadIdx.x;
		if (i >= npx)
			return;
#pragma unroll
		for (int j = 0; j < QUANTILE_MAX_PERCENTS; ++j)
		{
			if (j >= nq)
				break;
			uint32_t c[PQ_DIGITS];
#pragma unroll
			for (int d = 0; d < PQ_DIGITS; ++d)
				c[d] = pq_row(state, npx, pass == 0 ? 0 : j, d)[i];
			uint32_t prefix, rank;
			if (pass == 0)
			{
				const uint32_t t = qt_rank(total, pc.p[j]);
				prefix = 0;
				rank = t >= 1 && t <= total ? t : 0; // 0: no frames, t == 0 or t > count - the value is decided
			}
			else
			{
				prefix = pq_row(state, npx, j, PQ_DIGITS)[i];
				rank = pq_row(state, npx, j, PQ_DIGITS + 1)[i];
			}
			if (rank != 0)
			{
				uint32_t digit = PQ_DIGITS - 1;
				bool found = false;
#pragma unroll
				for (int d = 0; d < PQ_DIGITS; ++d)
				{
					const bool here = !found && rank <= c[d];
					digit = here ? (uint32_t)d : digit;
					found |= here;
					rank -= found ? 0u : c[d];
				}
				prefix = prefix << 4 | digit;
			}
			pq_row(state, npx, j, PQ_DIGITS)[i] = prefix;
			pq_row(state, npx, j, PQ_DIGITS + 1)[i] = rank;
			if (pass == PIXEL_QUANTILE_PASSES - 1)
				values[(int64_t)j * npx + i] = rank == 0 ? (total == 0 ? -1 : 0) : prefix == 65535u ? 0 : (int32_t)prefix; // 65535 is in no bin
			if (pass != 0) // the counts of this percent are spent
			{
#pragma unroll
				for (int d = 0; d < PQ_DIGITS; ++d)
					pq_row(state, npx, j, d)[i] = 0;
			}
		}
		if (pass == 0) // every percent has read the shared counts
		{
#pragma unroll
			for (int d = 0; d < PQ_DIGITS; ++d)
				pq_row(state, npx, 0, d)[i] = 0;
		}
	}

	size_t pixel_quantiles_state_bytes(int64_t npx, int npercents) { return (size_t)npx * (size_t)npercents * PIXEL_QUANTILE_ROWS * 4; }

	namespace
	{
		template <int G>
		void pq_launch(const uint16_t *frames, int64_t npx, int n, int shift, int j0, uint32_t *state, hipStream_t st)
		{
			const TimeSlabs plan = time_slab_plan(npx, n, PQ_SLAB_MIN, INT_MAX); // no cap: the counters are 32-bit
			const bool vec = frames_are_16_byte_aligned(npx, frames);
			const dim3 grid((unsigned)((npx + PQ_TILE - 1) / PQ_TILE), (unsigned)plan.slabs);
			if (plan.slabs == 1)
			{
				if (vec)
					pixel_quantiles_count<G, true, false><<<grid, pq_block(G), 0, st>>>(frames, npx, n, plan.per_slab, shift, j0, state);
				else
					pixel_quantiles_count<G, false, false><<<grid, pq_block(G), 0, st>>>(frames, npx, n, plan.per_slab, shift, j0, state);
			}
			else if (vec)
				pixel_quantiles_count<G, true, true><<<grid, pq_block(G), 0, st>>>(frames, npx, n, plan.per_slab, shift, j0, state);
			else
				pixel_quantiles_count<G, false, true><<<grid, pq_block(G), 0, st>>>(frames, npx, n, plan.per_slab, shift, j0, state);
		}
	} // namespace

	hipError_t launch_pixel_quantiles_count(const uint16_t *frames, int64_t npx, int n, int npercents, int pass, void *state, hipStream_t st)
	{
		if (n <= 0 || npx <= 0 || npercents <= 0 || npercents > QUANTILE_MAX_PERCENTS || pass < 0 || pass >= PIXEL_QUANTILE_PASSES)
			return hipErrorInvalidValue;
		uint32_t *s = static_cast<uint32_t *>(state);
		const int shift = 4 * (PIXEL_QUANTILE_PASSES - 1 - pass);
		if (pass == 0) // no prefix yet: one set of counts serves every percent
			pq_launch<1>(frames, npx, n, shift, 0, s, st);
		else
			for (int j0 = 0; j0 < npercents; j0 += PIXEL_QUANTILE_GROUP)
				switch (std::min(PIXEL_QUANTILE_GROUP, npercents - j0))
				{
				case 1:
					pq_launch<1>(frames, npx, n, shift, j0, s, st);
					break;
				case 2:
					pq_launch<2>(frames, npx, n, shift, j0, s, st);
					break;
				case 3:
					pq_launch<3>(frames, npx, n, shift, j0, s, st);
					break;
				default:
					pq_launch<4>(frames, npx, n, shift, j0, s, st);
				}
		return hipGetLastError();
	}

	hipError_t launch_pixel_quantiles_resolve(int64_t npx, const QuantilePercents &percents, int npercents, int pass, uint32_t total, void *state,
											  int32_t *values, hipStream_t st)
	{
		if (npx <= 0 || npercents <= 0 || npercents > QUANTILE_MAX_PERCENTS || pass < 0 || pass >= PIXEL_QUANTILE_PASSES ||
			(pass == PIXEL_QUANTILE_PASSES - 1 && !values))
			return hipErrorInvalidValue;
		pixel_quantiles_resolve<<<(unsigned)((npx + PQ_RESOLVE_BLOCK - 1) / PQ_RESOLVE_BLOCK), PQ_RESOLVE_BLOCK, 0, st>>>(
			static_cast<uint32_t *>(state), npx, npercents, percents, pass, total, values);
		return hipGetLastError();
	}
} // namespace rir
