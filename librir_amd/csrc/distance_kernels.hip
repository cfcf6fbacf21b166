// Exact Euclidean distance transform of masks and label maps - gfx950 (CDNA4): for every pixel the squared distance to the nearest
// background pixel and, when asked for, that pixel's flat index.  An extension without an upstream counterpart; the definition is in
// include/rir_amd_device.h (rir_distance_transform_device).  All integer, bit-exact, the same bits for any split of a stack into calls.
//
// Two passes per group of frames, both linear in the length of the line they walk, with nothing on the host in between:
//
//   distance_rows_kernel<T>        a wave per row.  It reads the row once, left to right, 64 cells at a time, and keeps each step's ballot of
//                                  background cells in LDS with the x of the last background cell before it; it then walks back right to
//                                  left, where a lane's nearest background cell at or left of it and at or right of it are the bits of its
//                                  step's ballot (a count of leading / trailing zeros) or what the neighbouring steps carried in.  It writes
//                                  the signed offset qx - x of the nearest one (the left one on a tie) as int16, DISTANCE_NO_CELL for a row
//                                  without background.
//   distance_columns_kernel<INDEX> a lane per column, consecutive lanes on consecutive addresses.  Meijster's lower envelope of the parabolas
//                                  (y - s)^2 + offset(s)^2 over the rows s that have a background cell: integer sep() by division, strict
//                                  comparisons, so that of equal parabolas the earlier row stays - the lowest flat index.  The top of the
//                                  stack (row, start, offset) is in registers; entry k of the stack lies at row k of the column, in
//                                  dist2 and in the offsets plane (see there), so lanes at equal depth coalesce and the only workspace
//                                  is the offsets plane, 2 bytes a pixel.  The walk back writes dist2 and the index.
//
// The border switch is the definition's min(dist2, b^2), taken when a pixel is written: the outside never enters a pass, so an index
// is -1 exactly where the outside is strictly nearer.  Rows y >= rows are written by the column pass and read by nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "distance_kernels.h"

namespace rir
{
	constexpr int DISTANCE_NO_CELL = -32768; // the row pass's offset for a row without a background cell (offsets are -16383 .. 16383)
	constexpr int DISTANCE_ROWS_PER_BLOCK = 4;
	constexpr int DISTANCE_STEPS = DISTANCE_MAX_SIDE / 64; // 64-cell steps of the widest row
	constexpr int DISTANCE_FAR = 1 << 20;				   // the x of a background cell that does not exist: farther than any cell of a row

	// ---- pass 1: along rows -----------------------------------------------------------------------------------------------------------------
	template <class T>
	__global__ __launch_bounds__(64 * DISTANCE_ROWS_PER_BLOCK) void distance_rows_kernel(const T *__restrict__ src, int16_t *__restrict__ offs, int w, int h,
																						 int rows, T background)
	{
		// (each wave uses its own part and nothing of the others': no barrier)
		__shared__ uint64_t step_cells[DISTANCE_ROWS_PER_BLOCK][DISTANCE_STEPS]; // the ballot of background cells of every step of the row
		__shared__ int step_left[DISTANCE_ROWS_PER_BLOCK][DISTANCE_STEPS];		 // the x of the last background cell before the step
		const int lane = threadIdx.x & 63;
		const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
		const int y = blockIdx.x * DISTANCE_ROWS_PER_BLOCK + wv;
		if (y >= rows)
			return;
		const int64_t at = ((int64_t)blockIdx.y * h + y) * w;
		const T *row = src + at;
		int16_t *out = offs + at;
		const int steps = (w + 63) >> 6; // <= DISTANCE_STEPS: w <= DISTANCE_MAX_SIDE
		int last = -DISTANCE_FAR;
		for (int c = 0; c < steps; ++c)
		{
			const int x = c * 64 + lane;
			const bool bg = x < w && row[x] == background;
			const uint64_t m = __ballot(bg);
			step_cells[wv][c] = m; // (the same value from every lane)
			step_left[wv][c] = last;
			if (m)
				last = c * 64 + 63 - __clzll((long long)m);
		}
		__builtin_amdgcn_wave_barrier(); // (the wave's LDS accesses stay in program order)
		int next = DISTANCE_FAR;
		for (int c = steps - 1; c >= 0; --c)
		{
			const uint64_t m = step_cells[wv][c];
			const int x = c * 64 + lane;
			const uint64_t upto = m & (~0ull >> (63 - lane)), from = m >> lane; // the step's background cells at or left / at or right of the lane
			const int xl = upto ? c * 64 + 63 - __clzll((long long)upto) : step_left[wv][c];
			const int xr = from ? x + __ffsll((unsigned long long)from) - 1 : next;
			const int dl = x - xl, dr = xr - x;
			const int d = dl <= dr ? -dl : dr; // a tie inside a line: the lower coordinate
			if (x < w)
				out[x] = (int16_t)(min(dl, dr) >= DISTANCE_MAX_SIDE ? DISTANCE_NO_CELL : d);
			if (m)
				next = c * 64 + __ffsll((unsigned long long)m) - 1;
		}
	}

	// ---- pass 2: along columns --------------------------------------------------------------------------------------------------------------
	// The stack needs no memory of its own.  Entry k of a column's stack is kept at row k of the column: its (row, start) word in dist2, its
	// offset in the offsets plane.  Going down, the stack is never deeper than the rows consumed, so entry k lands on an offset that has been
	// read (the rows loaded ahead are in registers).  Going back up, starts grow strictly from entry 0's 0, so entry k starts at row k or
	// below: when row u is written, the entries still to come lie in rows < u, and the one in use is in registers.
	struct EnvelopeTop // the parabola on top of the stack: its row s, the first y where it is the lowest, its row-pass offset
	{
		int s, t, d;
	};

	__device__ __forceinline__ void envelope_store(int *dist2, int16_t *offs, int64_t at, const EnvelopeTop &e)
	{
		dist2[at] = (int)((uint32_t)e.s | ((uint32_t)e.t << 16));
		offs[at] = (int16_t)e.d;
	}
	__device__ __forceinline__ EnvelopeTop envelope_load(const int *dist2, const int16_t *offs, int64_t at)
	{
		const uint32_t st = (uint32_t)dist2[at];
		return {(int)(st & 0xffffu), (int)(st >> 16), (int)offs[at]};
	}

	template <bool INDEX>
	__global__ __launch_bounds__(64) void distance_columns_kernel(int16_t *offs, int *dist2, int *__restrict__ index, int w, int h, int rows, int border)
	{
		constexpr int AHEAD = 8; // rows of offsets loaded together, one such group ahead of the envelope that consumes them
		const int x = blockIdx.x * 64 + threadIdx.x;
		if (x >= w)
			return;
		const int64_t base = (int64_t)blockIdx.y * w * h + x;
		offs += base, dist2 += base;
		if (INDEX)
			index += base;
		int q = -1; // depth of the stack - 1; the top is also in `top`
		EnvelopeTop top = {0, 0, 0};
		int ahead[AHEAD], next[AHEAD];
#pragma unroll
		for (int i = 0; i < AHEAD; ++i)
			next[i] = rows > 0 ? (int)offs[(int64_t)min(i, rows - 1) * w] : DISTANCE_NO_CELL;
		for (int y0 = 0; y0 < rows; y0 += AHEAD)
		{
#pragma unroll
			for (int i = 0; i < AHEAD; ++i)
			{
				ahead[i] = next[i];
				next[i] = offs[(int64_t)min(y0 + AHEAD + i, rows - 1) * w]; // (past the image: some row's value, never used)
			}
#pragma unroll
			for (int i = 0; i < AHEAD; ++i)
			{
				const int u = y0 + i, du = ahead[i];
				if (u >= rows || du == DISTANCE_NO_CELL)
					continue; // a row without a background cell never enters the envelope
				const int fu = du * du;
				// parabolas that the new one undercuts where they start leave (strictly: of equal ones the earlier row stays)
				while (q >= 0 && (top.t - top.s) * (top.t - top.s) + top.d * top.d > (top.t - u) * (top.t - u) + fu)
					if (--q >= 0)
						top = envelope_load(dist2, offs, (int64_t)q * w);
				if (q < 0)
				{
					q = 0;
					top = {u, 0, du};
					envelope_store(dist2, offs, 0, top);
				}
				else
				{
					// sep(): the last y at which the top is not above the new parabola (>= top.t >= 0: the numerator is not negative)
					const uint32_t num = (uint32_t)(u * u - top.s * top.s + fu - top.d * top.d), den = (uint32_t)(2 * (u - top.s));
					const int start = 1 + (int)(num / den);
					if (start < rows)
					{
						++q;
						top = {u, start, du};
						envelope_store(dist2, offs, (int64_t)q * w, top);
					}
				}
			}
		}
		const int bx = min(x + 1, w - x);
		for (int u = rows - 1; u >= 0; --u)
		{
			int d2 = DIST2_NONE, idx = -1;
			if (q >= 0)
			{
				d2 = (u - top.s) * (u - top.s) + top.d * top.d;
				idx = top.s * w + x + top.d;
			}
			if (border)
			{
				const int b = min(bx, min(u + 1, rows - u));
				if (b * b < d2) // (b <= 8192)
					d2 = b * b, idx = -1;
			}
			const bool leave = q >= 0 && u == top.t;
			if (leave && --q >= 0)
				top = envelope_load(dist2, offs, (int64_t)q * w); // (row q < u: before row u is written)
			dist2[(int64_t)u * w] = d2;
			if (INDEX)
				index[(int64_t)u * w] = idx;
		}
		for (int y = rows; y < h; ++y) // outside the image: distance 0, the pixel itself
		{
			dist2[(int64_t)y * w] = 0;
			if (INDEX)
				index[(int64_t)y * w] = y * w + x;
		}
	}

	// ---- launcher ---------------------------------------------------------------------------------------------------------------------------
	template <class T>
	static hipError_t launch_distance_t(const T *src, int w, int h, int nframes, T background, int border, int rows, int *dist2, int *index, void *work,
										size_t work_bytes, hipStream_t st)
	{
		const size_t npx = (size_t)w * h;
		const int fit = (int)std::min<size_t>(std::min<size_t>((size_t)nframes, work_bytes / distance_frame_bytes(w, h)), 65535);
		if (fit < 1)
			return hipErrorInvalidValue;
		const int group = (nframes + (nframes + fit - 1) / fit - 1) / ((nframes + fit - 1) / fit); // groups of equal size, the fewest that fit
		int16_t *offs = static_cast<int16_t *>(work);
		for (int o = 0; o < nframes; o += group)
		{
			const int n = std::min(group, nframes - o);
			if (rows > 0)
				hipLaunchKernelGGL((distance_rows_kernel<T>), dim3((unsigned)((rows + DISTANCE_ROWS_PER_BLOCK - 1) / DISTANCE_ROWS_PER_BLOCK), (unsigned)n),
								   dim3(64 * DISTANCE_ROWS_PER_BLOCK), 0, st, src + npx * o, offs, w, h, rows, background);
			const dim3 grid((unsigned)((w + 63) / 64), (unsigned)n);
			if (index)
				hipLaunchKernelGGL((distance_columns_kernel<true>), grid, dim3(64), 0, st, offs, dist2 + npx * o, index + npx * o, w, h, rows, border);
			else
				hipLaunchKernelGGL((distance_columns_kernel<false>), grid, dim3(64), 0, st, offs, dist2 + npx * o, index, w, h, rows, border);
		}
		return hipGetLastError();
	}

	hipError_t launch_distance_transform(int type, const void *src, int w, int h, int nframes, int background, int border, int rows, int *dist2,
										 int *index, void *work, size_t work_bytes, hipStream_t st)
	{
		switch (type)
		{
		case '?': // (bool frames as bytes 0 / 1)
		case 'B':
			return launch_distance_t(static_cast<const uint8_t *>(src), w, h, nframes, (uint8_t)background, border, rows, dist2, index, work, work_bytes, st);
		case 'H':
			return launch_distance_t(static_cast<const uint16_t *>(src), w, h, nframes, (uint16_t)background, border, rows, dist2, index, work, work_bytes, st);
		case 'i':
			return launch_distance_t(static_cast<const int32_t *>(src), w, h, nframes, (int32_t)background, border, rows, dist2, index, work, work_bytes, st);
		default:
			return hipErrorInvalidValue;
		}
	}
} // namespace rir
