// Temporal median filter over a uint16 frame stack [n][h][w] (the definition is with rir_temporal_median_device,
// include/rir_amd_device.h).  Two kernels per window W, both templated on W so that the window lives in registers indexed by
// compile-time constants (no scratch):
//
//   temporal_median_run<W, V>   the interior outputs of a step-1 call (full windows).  A thread owns 2V adjacent pixels, packed two
//                               per 32-bit register, and walks a run of consecutive outputs, loading each input frame of the run once.
//                               Outputs go in pairs: t and t + 1 share the 2r frames t - r + 1 .. t + r, whose two middle values lo <= hi
//                               a selection network finds; the median of t is then clamp(frame t - r, lo, hi), that of t + 1
//                               clamp(frame t + r + 1, lo, hi).
//   temporal_median_edge<W, V>  every other output: the truncated windows at the ends of the stack and calls with step > 1.  One
//                               output per thread; the missing frames of a truncated window of c frames are filled with r - c / 2
//                               zeros and the rest 0xFFFF, so that the middle of the W slots is sorted(window)[c / 2].  W = 1 is a copy.
//
// The networks are Batcher's merge exchange for the key count, fully unrolled; the compiler drops the comparators whose results do
// not reach the middle.  Min and max of two packed pixels are one v_pk_min_u16 / v_pk_max_u16 each.
#include <array>
#include <utility>

#include "temporal_kernels.h"

namespace rir
{
	typedef unsigned short tm_u16x2 __attribute__((ext_vector_type(2)));

	constexpr int TM_BLOCK = 256;
	constexpr int TM_MAX_WINDOW = 63;
	constexpr int TM_GRID_Y = 32768; // outputs (edge) or runs (interior) per launch
	constexpr int TM_RUN = 64;		 // outputs per thread in the interior, halved for small calls down to TM_RUN_MIN
	constexpr int TM_RUN_MIN = 8;
	constexpr long long TM_MIN_THREADS = 1 << 18;

	// Batcher's merge exchange (Knuth, TAOCP vol. 3, 5.2.2, Algorithm M): a sorting network for any number of keys.
	struct TmNetwork
	{
		short a[600];
		short b[600];
		int size;
	};
	constexpr TmNetwork merge_exchange(int keys)
	{
		TmNetwork net{};
		net.size = 0;
		if (keys < 2)
			return net;
		int t = 0;
		while ((1 << t) < keys)
			++t;
		for (int p = 1 << (t - 1); p > 0; p >>= 1)
		{
			int q = 1 << (t - 1), r = 0, d = p;
			while (true)
			{
				for (int i = 0; i + d < keys; ++i)
					if ((i & p) == r)
					{
						net.a[net.size] = (short)i;
						net.b[net.size] = (short)(i + d);
						++net.size;
					}
				if (q == p)
					break;
				d = q - p;
				q >>= 1;
				r = p;
			}
		}
		return net;
	}
	template <int N>
	struct TmSortNet
	{
		static constexpr TmNetwork net = merge_exchange(N);
	};
	static_assert(TmSortNet<64>::net.size == 543, "merge exchange of 64 keys is Batcher's 543-comparator network");

	template <int V>
	__device__ __forceinline__ void tm_exchange(tm_u16x2 (&x)[V], tm_u16x2 (&y)[V])
	{
#pragma unroll
		for (int j = 0; j < V; ++j)
		{
			const tm_u16x2 lo = __builtin_elementwise_min(x[j], y[j]);
			y[j] = __builtin_elementwise_max(x[j], y[j]);
			x[j] = lo;
		}
	}
	template <int N, int V, int... I>
	__device__ __forceinline__ void tm_sort(tm_u16x2 (&k)[N][V], std::integer_sequence<int, I...>)
	{
		(tm_exchange<V>(k[TmSortNet<N>::net.a[I]], k[TmSortNet<N>::net.b[I]]), ...);
	}
	template <int N, int V>
	__device__ __forceinline__ void tm_sort(tm_u16x2 (&k)[N][V])
	{
		tm_sort<N, V>(k, std::make_integer_sequence<int, TmSortNet<N>::net.size>());
	}

	template <int V>
	struct TmWide;
	template <>
	struct TmWide<1>
	{
		typedef unsigned int T;
	};
	template <>
	struct TmWide<2>
	{
		typedef unsigned int T __attribute__((ext_vector_type(2)));
	};
	template <>
	struct TmWide<4>
	{
		typedef unsigned int T __attribute__((ext_vector_type(4)));
	};

	// pixels p0 .. p0 + 2V - 1 of frame f: one 4V-byte load where the stack allows it (vec), else pixel by pixel (0 past the frame's end)
	template <int V>
	__device__ __forceinline__ void tm_load(tm_u16x2 (&v)[V], const uint16_t *__restrict__ f, int64_t p0, int64_t npx, bool vec)
	{
		if (vec)
		{
			const typename TmWide<V>::T x = *reinterpret_cast<const typename TmWide<V>::T *>(f + p0);
			__builtin_memcpy(&v[0], &x, sizeof(x));
		}
		else
		{
#pragma unroll
			for (int j = 0; j < V; ++j)
			{
				const int64_t p = p0 + 2 * j;
				v[j].x = p < npx ? f[p] : (uint16_t)0;
				v[j].y = p + 1 < npx ? f[p + 1] : (uint16_t)0;
			}
		}
	}
	template <int V>
	__device__ __forceinline__ void tm_store(uint16_t *__restrict__ f, const tm_u16x2 (&v)[V], int64_t p0, int64_t npx, bool vec)
	{
		if (vec)
		{
			typename TmWide<V>::T x;
			__builtin_memcpy(&x, &v[0], sizeof(x));
			*reinterpret_cast<typename TmWide<V>::T *>(f + p0) = x;
		}
		else
		{
#pragma unroll
			for (int j = 0; j < V; ++j)
			{
				const int64_t p = p0 + 2 * j;
				if (p < npx)
					f[p] = v[j].x;
				if (p + 1 < npx)
					f[p + 1] = v[j].y;
			}
		}
	}

	// m = the median where it differs from the centre a by more than threshold and the pixel lies before `limit` (rows * w), else a
	template <int V>
	__device__ __forceinline__ void tm_rule(tm_u16x2 (&m)[V], const tm_u16x2 (&a)[V], int64_t p0, int64_t limit, int threshold)
	{
		if (threshold == 0 && p0 + 2 * V <= limit)
			return; // (with threshold 0 the rule keeps the median: a pixel equal to it is the same value)
#pragma unroll
		for (int j = 0; j < V; ++j)
		{
			const int64_t p = p0 + 2 * j;
			const int dx = (int)m[j].x - (int)a[j].x, dy = (int)m[j].y - (int)a[j].y;
			if (!(p < limit && (dx > threshold || -dx > threshold)))
				m[j].x = a[j].x;
			if (!(p + 1 < limit && (dy > threshold || -dy > threshold)))
				m[j].y = a[j].y;
		}
	}

	template <int W, int V>
	__global__ __launch_bounds__(TM_BLOCK) void temporal_median_run(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, int64_t npx, int ngroups,
																	int t_begin, int t_end, int run, int first, int threshold, int64_t limit, int vec)
	{
		constexpr int R = W / 2;
		const int g = blockIdx.x * TM_BLOCK + threadIdx.x;
		if (g >= ngroups)
			return;
		const int t0 = t_begin + (int)blockIdx.y * run;
		const int t1 = min(t0 + run, t_end);
		const int64_t p0 = (int64_t)g * 2 * V;
		tm_u16x2 win[W + 1][V]; // frames t - r .. t + r + 1
#pragma unroll
		for (int i = 0; i < W - 1; ++i)
			tm_load<V>(win[i], src + (int64_t)(t0 - R + i) * npx, p0, npx, vec);
		for (int t = t0; t < t1; t += 2)
		{
			const bool two = t + 1 < t1;
			tm_load<V>(win[W - 1], src + (int64_t)(t + R) * npx, p0, npx, vec);
			if (two)
				tm_load<V>(win[W], src + (int64_t)(t + R + 1) * npx, p0, npx, vec);
			tm_u16x2 c[W - 1][V];
#pragma unroll
			for (int i = 0; i < W - 1; ++i)
#pragma unroll
				for (int j = 0; j < V; ++j)
					c[i][j] = win[i + 1][j];
			tm_sort<W - 1, V>(c);
			tm_u16x2 m0[V], m1[V];
#pragma unroll
			for (int j = 0; j < V; ++j)
			{
				m0[j] = __builtin_elementwise_max(c[R - 1][j], __builtin_elementwise_min(win[0][j], c[R][j]));
				m1[j] = __builtin_elementwise_max(c[R - 1][j], __builtin_elementwise_min(win[W][j], c[R][j]));
			}
			tm_rule<V>(m0, win[R], p0, limit, threshold);
			tm_store<V>(dst + (int64_t)(t - first) * npx, m0, p0, npx, vec);
			if (two)
			{
				tm_rule<V>(m1, win[R + 1], p0, limit, threshold);
				tm_store<V>(dst + (int64_t)(t + 1 - first) * npx, m1, p0, npx, vec);
			}
#pragma unroll
			for (int i = 0; i < W - 1; ++i)
#pragma unroll
				for (int j = 0; j < V; ++j)
					win[i][j] = win[i + 2][j];
		}
	}

	template <int W, int V>
	__global__ __launch_bounds__(TM_BLOCK) void temporal_median_edge(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, int64_t npx, int ngroups,
																	 int n, int first, int step, int k0, int threshold, int64_t limit, int vec)
	{
		constexpr int R = W / 2;
		const int g = blockIdx.x * TM_BLOCK + threadIdx.x;
		if (g >= ngroups)
			return;
		const int k = k0 + (int)blockIdx.y;
		const int t = first + k * step;
		const int64_t p0 = (int64_t)g * 2 * V;
		const int below = max(0, R - t), above = max(0, t + R - (n - 1)); // slots outside the stack
		const int zeros = R - (W - below - above) / 2;					  // of which this many read 0, the others 0xFFFF
		tm_u16x2 key[W][V], centre[V];
#pragma unroll
		for (int s = 0; s < W; ++s)
		{
			if (s < below || s >= W - above)
			{
				const int m = s < below ? s : below + s - (W - above);
				const uint16_t fill = m < zeros ? (uint16_t)0 : (uint16_t)0xFFFF;
#pragma unroll
				for (int j = 0; j < V; ++j)
					key[s][j] = (tm_u16x2){fill, fill};
			}
			else
				tm_load<V>(key[s], src + (int64_t)(t - R + s) * npx, p0, npx, vec);
		}
#pragma unroll
		for (int j = 0; j < V; ++j)
			centre[j] = key[R][j];
		tm_sort<W, V>(key);
		tm_rule<V>(key[R], centre, p0, limit, threshold);
		tm_store<V>(dst + (int64_t)k * npx, key[R], p0, npx, vec);
	}

	template <int W>
	hipError_t launch_window(const uint16_t *src, uint16_t *dst, int w, int h, int n, int first, int count, int step, int threshold, int rows, hipStream_t st)
	{
		constexpr int R = W / 2;
		constexpr int V = W <= 9 ? 4 : W <= 31 ? 2 : 1; // packed registers per thread: the window (W + 1 of them per register) stays resident
		const int64_t npx = (int64_t)w * h;
		const int vec = npx % (2 * V) == 0 && ((uintptr_t)src | (uintptr_t)dst) % (4 * V) == 0;
		const int ngroups = (int)((npx + 2 * V - 1) / (2 * V));
		const unsigned bx = (unsigned)((ngroups + TM_BLOCK - 1) / TM_BLOCK);
		const int64_t limit = (int64_t)rows * w;
		int kb = 0, ke = 0; // outputs [kb, ke) have full windows and take the run kernel
		if (W > 1 && step == 1)
		{
			const int tb = max(first, R), te = min(first + count, n - R);
			if (tb < te)
				kb = tb - first, ke = te - first;
		}
		if constexpr (W > 1)
			if (ke > kb)
			{
				const int outputs = ke - kb;
				int run = TM_RUN;
				while (run > TM_RUN_MIN && (long long)ngroups * ((outputs + run - 1) / run) < TM_MIN_THREADS)
					run /= 2;
				const int runs = (outputs + run - 1) / run;
				for (int r0 = 0; r0 < runs; r0 += TM_GRID_Y)
				{
					const unsigned by = (unsigned)min(TM_GRID_Y, runs - r0);
					temporal_median_run<W, V><<<dim3(bx, by), TM_BLOCK, 0, st>>>(src, dst, npx, ngroups, first + kb + r0 * run, first + ke, run, first, threshold,
																				 limit, vec);
				}
			}
		const int ranges[2][2] = {{0, kb}, {ke, count}};
		for (const auto &rg : ranges)
			for (int k0 = rg[0]; k0 < rg[1]; k0 += TM_GRID_Y)
			{
				const unsigned by = (unsigned)min(TM_GRID_Y, rg[1] - k0);
				temporal_median_edge<W, V><<<dim3(bx, by), TM_BLOCK, 0, st>>>(src, dst, npx, ngroups, n, first, step, k0, threshold, limit, vec);
			}
		return hipGetLastError();
	}

	typedef hipError_t (*TmLaunch)(const uint16_t *, uint16_t *, int, int, int, int, int, int, int, int, hipStream_t);
	template <int... I>
	constexpr std::array<TmLaunch, sizeof...(I)> tm_launchers(std::integer_sequence<int, I...>)
	{
		return {&launch_window<2 * I + 1>...};
	}

	hipError_t launch_temporal_median(const uint16_t *src, uint16_t *dst, int w, int h, int n, int first, int count, int step, int window, int threshold,
									  int rows, hipStream_t st)
	{
		static constexpr std::array<TmLaunch, (TM_MAX_WINDOW + 1) / 2> launchers = tm_launchers(std::make_integer_sequence<int, (TM_MAX_WINDOW + 1) / 2>());
		if (window < 1 || window > TM_MAX_WINDOW || window % 2 == 0 || count <= 0)
			return hipErrorInvalidValue;
		return launchers[window / 2](src, dst, w, h, n, first, count, step, threshold, rows, st);
	}
} // namespace rir
