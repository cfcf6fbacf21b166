// Connected components tracked through time - gfx950 (CDNA4).  The definition is with rir_track_components_device
// (include/rir_amd_device.h): the components of a stack of per-frame label maps are nodes (node of component k of frame t = t * K + k),
// two components of adjacent frames are linked when they share a pixel, a track is a connected set of nodes, and tracks are numbered
// 1, 2, ... in the order of their lowest node.
//
// The forest of union_find.h over node indices builds the partition: a root is the lowest node of its tree, so numbering the roots by a
// prefix sum over the node indices gives the tracks' numbers whatever the order the workgroups ran in.  Integer work, six launches:
//
//   track_init_kernel     L[i] = i, the tables to their empty state, info zeroed.
//   track_link_kernel     the pass over the pixels.  A workgroup takes a strip of TK_STRIP pixels and a run of consecutive frame pairs; a
//                         thread keeps frame t's 4 adjacent labels in registers while it takes frame t + 1's (one 16-byte load each), so a
//                         run of R pairs reads R + 1 frames: 4 * npx * (1 + 1/R) bytes a frame.  A pixel contributes the pair (a, b) when
//                         both components exist; it is skipped when the pixel to its left holds the same pair (inside the thread, and
//                         against the left lane through a wave shift), and when every contributing lane of the wave holds one pair, one
//                         lane links it: frame t + 1's node is hung under a node of frame t's tree with one atomic (hang(), union_find.h).
//                         A wave without a contributing pixel - most of them, where the hot spots are few - leaves after the eight range
//                         checks of its labels.
//   track_flatten_kernel  one thread per node: does the component exist, and what is its final root; wave bitmaps of the roots and
//                         per-block root counts (the shape of ccl_flatten_kernel).
//   track_scan_kernel     one workgroup: block counts -> offsets, info[0] = tracks + 1, info[1] = frames whose components >= K were dropped.
//   track_number_kernel   track_of and the tables: first_frame and first_label from the root itself, last_frame by atomicMax and
//                         components by atomicAdd (integer, order-free), the lanes of a wave that share a track grouped first.
//   track_relabel_kernel  (only with a destination) dst = track_of[t][labels[t][p]], 16-byte loads and stores; a thread reads its labels
//                         before it writes them, so dst may be the labels themselves.
#include <algorithm>

#include "track_kernels.h"
#include "union_find.h"

namespace rir
{
	namespace
	{
		constexpr int kAgent = __HIP_MEMORY_SCOPE_AGENT;
		constexpr int TK_BLOCK = 256;							 // 4 wavefronts
		constexpr int TK_PX = 4;								 // labels per thread: one 16-byte load
		constexpr int TK_STRIP = TK_BLOCK * TK_PX;				 // pixels per workgroup
		constexpr int TK_RUN = 64;								 // frame pairs per work item, halved for small calls down to TK_RUN_MIN
		constexpr int TK_RUN_MIN = 8;							 // (the rule of the temporal median's runs)
		constexpr long long TK_MIN_THREADS = 1 << 18;			 // threads that fill the chip
		constexpr int TK_DEPTH = 4;								 // frames a thread loads ahead of the pairs it works on
		constexpr unsigned TK_GRID = 1u << 20;					 // workgroups at most (grid-stride loops over work items)
		constexpr int TK_SCAN_BLOCK = 1024;						 // the one workgroup of the scan
		static_assert(TK_RUN % TK_DEPTH == 0 && TK_RUN_MIN % TK_DEPTH == 0, "a run is whole load groups");

		// c - 1 for the number c of label values that name a component of frame t or the background: min(K, counts[t]), at least 1.
		// Label a names a component when (unsigned)a - 1 < c - 1.
		__device__ __forceinline__ unsigned tk_limit(const int32_t *__restrict__ counts, int t, int K)
		{
			return (unsigned)(counts ? max(1, min(K, counts[t])) : K) - 1u;
		}
		__device__ __forceinline__ bool tk_names(int a, unsigned limit) { return (unsigned)a - 1u < limit; }

		// 4 adjacent labels of one frame from pixel p on; past the frame's end (or where a 16-byte load is not possible) range-checked
		// scalar loads, 0 past the end.
		__device__ __forceinline__ int4 tk_load4(const int32_t *f, int64_t p, int64_t npx, bool vec)
		{
			if (vec && p + (TK_PX - 1) < npx)
				return *reinterpret_cast<const int4 *>(f + p);
			int4 v;
			v.x = p < npx ? f[p] : 0;
			v.y = p + 1 < npx ? f[p + 1] : 0;
			v.z = p + 2 < npx ? f[p + 2] : 0;
			v.w = p + 3 < npx ? f[p + 3] : 0;
			return v;
		}

		// What a wave remembers from the last pair that one lane linked for all: `node` (frame t + 1 then) was hung under `low`.
		struct TkHint
		{
			int node, low;
		};

		// The pairs of one thread's 4 pixels in frames t (A, nodes from na on) and t + 1 (B, nodes from nb on), called by the whole wave.
		// A link hangs the node of frame t + 1 - which nothing has linked before in most cases - under a node of frame t's tree with
		// hang(): one atomic, not two climbs and an atomic.  The node it is hung under is the parent of frame t's node (one load), or, where
		// the wave itself hung that node in the pair before, the node it hung it under (no load): a component that a wave follows through
		// its run costs one atomic round trip a frame, and all its nodes of the run hang under one node.
		__device__ __forceinline__ void tk_pairs(int *L, const int4 &A, const int4 &B, unsigned la, unsigned lb, int na, int nb, TkHint &hint)
		{
			const int a[TK_PX] = {A.x, A.y, A.z, A.w}, b[TK_PX] = {B.x, B.y, B.z, B.w};
			bool on[TK_PX], any = false;
#pragma unroll
			for (int j = 0; j < TK_PX; ++j)
			{
				on[j] = tk_names(a[j], la) && tk_names(b[j], lb);
				any |= on[j];
			}
			if (__ballot(any) == 0)
				return;
			const int lane = (int)(threadIdx.x & 63);
			const int left_a = __shfl_up(a[TK_PX - 1], 1), left_b = __shfl_up(b[TK_PX - 1], 1); // (lane 0 has no left lane: it contributes)
			bool same_as_left[TK_PX];
			same_as_left[0] = lane > 0 && a[0] == left_a && b[0] == left_b;
#pragma unroll
			for (int j = 1; j < TK_PX; ++j)
				same_as_left[j] = a[j] == a[j - 1] && b[j] == b[j - 1];
#pragma unroll
			for (int j = 0; j < TK_PX; ++j)
			{
				const bool go = on[j] && !same_as_left[j];
				const unsigned long long m = __ballot(go);
				if (m == 0)
					continue;
				const int lead = __ffsll((long long)m) - 1;
				const int pa = __shfl(a[j], lead), pb = __shfl(b[j], lead);
				if (__ballot(go && (a[j] != pa || b[j] != pb)) == 0)
				{
					const int x = na + pa, y = nb + pb;
					const bool known = x == hint.node;
					if (lane == lead)
						hang<kAgent>(L, known ? hint.low : link_load<kAgent>(&L[x]), y);
					hint.low = known ? hint.low : x;
					hint.node = y;
				}
				else if (go)
					hang<kAgent>(L, link_load<kAgent>(&L[na + a[j]]), nb + b[j]);
			}
		}

		__global__ __launch_bounds__(TK_BLOCK) void track_init_kernel(int *__restrict__ L, int nodes, int32_t *__restrict__ info, int info0,
																	  int32_t *__restrict__ first_frame, int32_t *__restrict__ last_frame,
																	  int32_t *__restrict__ first_label, int32_t *__restrict__ components, int table)
		{
			const int64_t stride = (int64_t)gridDim.x * TK_BLOCK, first = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
			for (int64_t i = first; i < nodes; i += stride)
				L[i] = (int)i;
			for (int64_t k = first; k < table; k += stride)
			{
				first_frame[k] = last_frame[k] = k == 0 ? -1 : 0;
				first_label[k] = 0;
				components[k] = 0;
			}
			if (first == 0)
			{
				info[0] = info0;
				info[1] = 0;
			}
		}

		__global__ __launch_bounds__(TK_BLOCK) void track_link_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ counts, int64_t npx,
																	  int n, int K, int strips, int run, int64_t items, int vec, int *L)
		{
			for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
			{
				const int64_t r = item / strips;
				const int strip = (int)(item - r * strips);
				const int t0 = (int)(r * run), t1 = min(t0 + run, n - 1); // the pairs (t, t + 1), t0 <= t < t1
				const int64_t p = (int64_t)strip * TK_STRIP + (int64_t)threadIdx.x * TK_PX;
				const int32_t *f = labels + (int64_t)t0 * npx;
				int4 cur = tk_load4(f, p, npx, vec);
				unsigned la = tk_limit(counts, t0, K);
				TkHint hint{-1, -1};
				for (int t = t0; t < t1; t += TK_DEPTH)
				{
					int4 next[TK_DEPTH];
#pragma unroll
					for (int u = 0; u < TK_DEPTH; ++u)
						next[u] = t + u < t1 ? tk_load4(f + (int64_t)(u + 1) * npx, p, npx, vec) : int4{0, 0, 0, 0};
#pragma unroll
					for (int u = 0; u < TK_DEPTH; ++u)
						if (t + u < t1)
						{
							const unsigned lb = tk_limit(counts, t + u + 1, K);
							tk_pairs(L, cur, next[u], la, lb, (t + u) * K, (t + u + 1) * K, hint);
							cur = next[u];
							la = lb;
						}
					f += (int64_t)TK_DEPTH * npx;
				}
			}
		}

		// R[i] = the final root of node i, -1 where the component does not exist (such a node was never linked: the link pass applies the
		// same rule).  The climb shortens the paths it walks; no unite() runs beside it.
		__global__ __launch_bounds__(TK_BLOCK) void track_flatten_kernel(int *L, const int32_t *__restrict__ counts, int nodes, int K, int *__restrict__ R,
																		 unsigned long long *__restrict__ root_bits, int *__restrict__ wave_before,
																		 int *__restrict__ block_roots)
		{
			__shared__ int wave_roots[TK_BLOCK / 64];
			const int i = (int)(blockIdx.x * (unsigned)TK_BLOCK + threadIdx.x);
			const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
			int r = -1;
			if (i < nodes)
			{
				const int t = i / K, k = i - t * K;
				if (tk_names(k, tk_limit(counts, t, K)))
					r = find_root<kAgent>(L, i);
				R[i] = r;
			}
			const unsigned long long roots = __ballot(r == i);
			if (lane == 0)
			{
				root_bits[i >> 6] = roots;
				wave_roots[wv] = __popcll(roots);
			}
			__syncthreads();
			if (lane == 0)
			{
				int before = 0;
				for (int q = 0; q < wv; ++q)
					before += wave_roots[q];
				wave_before[i >> 6] = before;
			}
			if (threadIdx.x == 0)
			{
				int s = 0;
				for (int q = 0; q < TK_BLOCK / 64; ++q)
					s += wave_roots[q];
				block_roots[blockIdx.x] = s;
			}
		}

		// Sum of v over the workgroup (every thread gets it); `part` holds one int per wavefront.
		__device__ __forceinline__ int tk_block_sum(int v, int *part)
		{
			for (int d = 32; d >= 1; d >>= 1)
				v += __shfl_xor(v, d);
			__syncthreads();
			if ((threadIdx.x & 63) == 0)
				part[threadIdx.x >> 6] = v;
			__syncthreads();
			int s = 0;
			for (int q = 0; q < TK_SCAN_BLOCK / 64; ++q)
				s += part[q];
			return s;
		}

		__global__ __launch_bounds__(TK_SCAN_BLOCK) void track_scan_kernel(int *__restrict__ block_roots, int nb, const int32_t *__restrict__ counts, int n,
																		   int K, int32_t *__restrict__ info)
		{
			__shared__ int wave_sum[TK_SCAN_BLOCK / 64];
			__shared__ int carry;
			const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
			if (threadIdx.x == 0)
				carry = 0;
			__syncthreads();
			for (int base = 0; base < nb; base += TK_SCAN_BLOCK)
			{
				const int k = base + (int)threadIdx.x;
				const int v = k < nb ? block_roots[k] : 0;
				int inc = v;
				for (int d = 1; d < 64; d <<= 1)
				{
					const int t = __shfl_up(inc, d);
					if (lane >= d)
						inc += t;
				}
				if (lane == 63)
					wave_sum[wv] = inc;
				__syncthreads();
				int before = carry;
				for (int q = 0; q < wv; ++q)
					before += wave_sum[q];
				if (k < nb)
					block_roots[k] = before + inc - v;
				__syncthreads();
				if (threadIdx.x == TK_SCAN_BLOCK - 1)
					carry = before + inc;
				__syncthreads();
			}
			int dropped = 0;
			if (counts)
				for (int t = (int)threadIdx.x; t < n; t += TK_SCAN_BLOCK)
					dropped += counts[t] > K ? 1 : 0;
			dropped = tk_block_sum(dropped, wave_sum);
			if (threadIdx.x == 0)
			{
				info[0] = carry + 1;
				info[1] = dropped;
			}
		}

		// A root's number = the roots before it among the nodes + 1.  Tracks >= table are not written (the rule of the label tables).
		// The nodes of a wave belong to few tracks where the components are large: up to TK_GROUPS times the wave's first remaining lane
		// speaks for every lane of its track (their count, and the frame of the highest lane: frames rise with the node index), and only
		// the lanes left after that use an atomic of their own.
		constexpr int TK_GROUPS = 4;
		__global__ __launch_bounds__(TK_BLOCK) void track_number_kernel(const int *__restrict__ R, int nodes, int K,
																		const unsigned long long *__restrict__ root_bits, const int *__restrict__ wave_before,
																		const int *__restrict__ block_before, int32_t *__restrict__ track_of,
																		int32_t *__restrict__ first_frame, int32_t *__restrict__ last_frame,
																		int32_t *__restrict__ first_label, int32_t *__restrict__ components, int table)
		{
			const int i = (int)(blockIdx.x * (unsigned)TK_BLOCK + threadIdx.x);
			const int lane = (int)(threadIdx.x & 63);
			const int r = i < nodes ? R[i] : -1;
			const int t = i / K;
			int k = 0;
			if (r >= 0)
				k = block_before[r / TK_BLOCK] + wave_before[r >> 6] + __popcll(root_bits[r >> 6] & ((1ull << (r & 63)) - 1ull)) + 1;
			if (i < nodes)
				track_of[i] = k;
			const bool listed = r >= 0 && k < table;
			if (listed && r == i)
			{
				first_frame[k] = t;
				first_label[k] = i - t * K;
			}
			unsigned long long todo = __ballot(listed);
			for (int round = 0; round < TK_GROUPS && todo != 0; ++round)
			{
				const int lead = __ffsll((long long)todo) - 1;
				const int lk = __shfl(k, lead);
				const unsigned long long group = __ballot(listed && k == lk) & todo;
				const int last = __shfl(t, 63 - __builtin_clzll(group));
				if (lane == lead)
				{
					atomicMax(&last_frame[lk], last);
					atomicAdd(&components[lk], __popcll(group));
				}
				todo &= ~group;
			}
			if ((todo >> lane) & 1ull)
			{
				atomicMax(&last_frame[k], t);
				atomicAdd(&components[k], 1);
			}
		}

		// (labels and dst may be one array: neither is __restrict__, and a thread's loads come before its stores)
		__global__ __launch_bounds__(TK_BLOCK) void track_relabel_kernel(const int32_t *labels, const int32_t *__restrict__ counts, int64_t npx, int K,
																		 int strips, int64_t items, int vec, const int32_t *__restrict__ track_of, int32_t *dst)
		{
			for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
			{
				const int64_t t = item / strips;
				const int strip = (int)(item - t * strips);
				const int64_t p = (int64_t)strip * TK_STRIP + (int64_t)threadIdx.x * TK_PX;
				if (p >= npx)
					continue;
				const unsigned limit = tk_limit(counts, (int)t, K);
				const int32_t *of = track_of + t * K;
				const int4 v = tk_load4(labels + t * npx, p, npx, vec);
				int4 o;
				o.x = tk_names(v.x, limit) ? of[v.x] : 0;
				o.y = tk_names(v.y, limit) ? of[v.y] : 0;
				o.z = tk_names(v.z, limit) ? of[v.z] : 0;
				o.w = tk_names(v.w, limit) ? of[v.w] : 0;
				int32_t *d = dst + t * npx + p;
				if (vec && p + (TK_PX - 1) < npx)
					*reinterpret_cast<int4 *>(d) = o;
				else
				{
					d[0] = o.x;
					if (p + 1 < npx)
						d[1] = o.y;
					if (p + 2 < npx)
						d[2] = o.z;
					if (p + 3 < npx)
						d[3] = o.w;
				}
			}
		}

		size_t align64(size_t b) { return (b + 63) & ~(size_t)63; }
		struct TkWork
		{
			int *L, *R, *wave_before, *block_roots;
			unsigned long long *root_bits;
			int nodes, nb;
		};
		size_t tk_blocks(size_t nodes) { return (nodes + TK_BLOCK - 1) / TK_BLOCK; }
		TkWork tk_carve(void *work, int n, int K)
		{
			TkWork k;
			k.nodes = n * K;
			k.nb = (int)tk_blocks((size_t)k.nodes);
			const size_t waves = (size_t)k.nb * (TK_BLOCK / 64);
			char *p = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(work) + 63) & ~(uintptr_t)63);
			k.L = reinterpret_cast<int *>(p);
			k.R = reinterpret_cast<int *>(p += align64((size_t)k.nodes * sizeof(int)));
			k.root_bits = reinterpret_cast<unsigned long long *>(p += align64((size_t)k.nodes * sizeof(int)));
			k.wave_before = reinterpret_cast<int *>(p += align64(waves * sizeof(unsigned long long)));
			k.block_roots = reinterpret_cast<int *>(p += align64(waves * sizeof(int)));
			return k;
		}
	} // namespace

	bool track_geometry_ok(int w, int h, int n, int nlabels)
	{
		return w > 0 && h > 0 && (int64_t)w * h <= TRACK_MAX_INDEX && n >= 0 && nlabels >= 1 && (int64_t)n * nlabels <= TRACK_MAX_INDEX;
	}

	size_t track_workspace_bytes(int w, int h, int n, int nlabels)
	{
		if (!track_geometry_ok(w, h, n, nlabels))
			return 0;
		const size_t nodes = (size_t)n * nlabels, nb = tk_blocks(nodes), waves = nb * (TK_BLOCK / 64);
		return 2 * align64(nodes * sizeof(int)) + align64(waves * sizeof(unsigned long long)) + align64(waves * sizeof(int)) + align64(nb * sizeof(int)) + 64;
	}

	hipError_t launch_track_components(const int32_t *labels, const int32_t *counts, int w, int h, int n, int nlabels, int32_t *track_of, int32_t *info,
									   int32_t *first_frame, int32_t *last_frame, int32_t *first_label, int32_t *components, int table_entries,
									   int32_t *dst, void *work, hipStream_t st)
	{
		if (!track_geometry_ok(w, h, n, nlabels) || table_entries < 1 || !info || !first_frame || !last_frame || !first_label || !components || !work ||
			(n > 0 && (!labels || !track_of)))
			return hipErrorInvalidValue;
		const TkWork k = tk_carve(work, n, nlabels);
		const int64_t cells = std::max<int64_t>(k.nodes, table_entries);
		const unsigned fill_grid = (unsigned)std::min<int64_t>(TK_GRID, (cells + TK_BLOCK - 1) / TK_BLOCK);
		track_init_kernel<<<fill_grid, TK_BLOCK, 0, st>>>(k.L, k.nodes, info, n == 0 ? 1 : 0, first_frame, last_frame, first_label, components, table_entries);
		if (n == 0)
			return hipGetLastError();
		const int64_t npx = (int64_t)w * h;
		const int strips = (int)((npx + TK_STRIP - 1) / TK_STRIP);
		if (n > 1)
		{
			const int pairs = n - 1;
			int run = TK_RUN;
			while (run > TK_RUN_MIN && (long long)strips * TK_BLOCK * ((pairs + run - 1) / run) < TK_MIN_THREADS)
				run /= 2;
			const int64_t items = (int64_t)strips * ((pairs + run - 1) / run);
			const int vec = npx % TK_PX == 0 && (uintptr_t)labels % 16 == 0;
			track_link_kernel<<<(unsigned)std::min<int64_t>(TK_GRID, items), TK_BLOCK, 0, st>>>(labels, counts, npx, n, nlabels, strips, run, items, vec, k.L);
		}
		track_flatten_kernel<<<(unsigned)k.nb, TK_BLOCK, 0, st>>>(k.L, counts, k.nodes, nlabels, k.R, k.root_bits, k.wave_before, k.block_roots);
		track_scan_kernel<<<1, TK_SCAN_BLOCK, 0, st>>>(k.block_roots, k.nb, counts, n, nlabels, info);
		track_number_kernel<<<(unsigned)k.nb, TK_BLOCK, 0, st>>>(k.R, k.nodes, nlabels, k.root_bits, k.wave_before, k.block_roots, track_of, first_frame,
																   last_frame, first_label, components, table_entries);
		if (dst)
		{
			const int64_t items = (int64_t)strips * n;
			const int vec = npx % TK_PX == 0 && (uintptr_t)labels % 16 == 0 && (uintptr_t)dst % 16 == 0;
			track_relabel_kernel<<<(unsigned)std::min<int64_t>(TK_GRID, items), TK_BLOCK, 0, st>>>(labels, counts, npx, nlabels, strips, items, vec, track_of,
																									dst);
		}
		return hipGetLastError();
	}
} // namespace rir
