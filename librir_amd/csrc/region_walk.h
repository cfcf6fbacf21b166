// The walk over labelled pixels that the per-region reducers share: statistics (region_kernels.hip) and geometry (geometry_kernels.hip) take
// walk_regions, the counting reducers - quantiles (quantile_kernels.hip) and histograms (histogram_kernels.hip) - walk_counters, further
// down; all share the constants, the atomics, load8 and the host helpers.  Device templates plus a little host code; include from .hip
// files only.
//
// walk_regions<LDS>(policy, ...) is a grid-stride loop over work items of WALK_ITEM pixels of one frame.  A thread takes 8 adjacent pixels
// per step (two 16-byte loads of labels, one of values) and keeps the run of its current label in registers.  It knows where its first pixel
// is, as a WalkPos: the offset in the item, the item's base, and (x, y) - one division per item, then x += WALK_STEP % w, y += WALK_STEP / w
// with one wrap per step; what a reducer does not read of it compiles away.  A step in which every lane's 8 pixels continue its run adds them
// without a flush point (in the policy's closed form where it has one); a checked step - the item's last, when the item ends inside it - and
// a step in which some lane's label changes go pixel by pixel.  A run is flushed where the thread's label changes and at the end of the
// item; when at least WAVE_ADD lanes of a complete wave flush, all of them the same label, the wave adds its runs with shuffles first and one
// lane flushes.  Either way the same integers are combined: the choice changes the cost, never the result.  LDS form: flushes go to
// per-region LDS accumulators, and at the end of the item the regions this item touched go to global memory and are reset.  Global form:
// flushes go to global memory directly.
//
// The policy supplies what differs between reducers:
//   Run                       the run type, with the label `int cur` and the pixel count `unsigned cnt`
//   VALUES, WAVE_ADD          whether the frames are read; the flushing lanes from which the wave adds first
//   reset(run, label)         the empty run of `label`
//   pixel(run, v, pos)        one pixel
//   chunk8(run, v, pos)       8 pixels of an unchecked step in closed form, or false to have them go one by one
//   combine(run, d)           run += the run of lane ^ d
//   frame(fi, nregions)       points the global accumulators at frame fi
//   put(r, run, base)         a flushed run into region r: LDS form into LDS, global form into global memory
//   carve(lds, nregions), clear(r), drain(r)    LDS form: lay out, zero, and move region r to global memory if touched (then zero it)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace rir
{
	constexpr int WALK_BLOCK = 256;
	constexpr int WALK_PX = 8;						 // pixels per thread and step
	constexpr int WALK_STEP = WALK_BLOCK * WALK_PX;	 // pixels per workgroup and step
	constexpr int WALK_ITEM = 16384;				 // pixels per work item
	constexpr int WALK_BLOCKS_PER_CU = 8;			 // walking grid: at most this many workgroups per CU
	constexpr int WALK_LDS_BYTES = 160 * 1024;		 // LDS per CU
	static_assert(WALK_ITEM % WALK_STEP == 0, "an item is whole steps");
	static_assert((long long)WALK_ITEM * 65535 < (1ll << 32), "the values of an item, so of any run or wave of runs in it, sum to less than 2^32");

	constexpr int WALK_WG = __HIP_MEMORY_SCOPE_WORKGROUP, WALK_AGENT = __HIP_MEMORY_SCOPE_AGENT; // LDS accumulators; global memory

	template <int SCOPE, class T>
	__device__ __forceinline__ void walk_add(T *p, T v)
	{
		__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE);
	}
	template <int SCOPE, class T>
	__device__ __forceinline__ void walk_min(T *p, T v)
	{
		__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE);
	}
	template <int SCOPE, class T>
	__device__ __forceinline__ void walk_max(T *p, T v)
	{
		__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, SCOPE);
	}

	// The 8 labels and, when VALUES, the 8 values at p (otherwise v is 0).  !CHECK: all 8 are inside, `vec` takes the 16-byte loads.  CHECK:
	// a pixel at or past `end` gets value 0 and the label `pad`.
	template <bool CHECK, bool VALUES>
	__device__ __forceinline__ void load8(const uint16_t *__restrict__ f, const int32_t *__restrict__ l, int64_t p, int64_t end, bool vec, int pad,
										  unsigned (&v)[WALK_PX], int (&lab)[WALK_PX])
	{
		if (!CHECK && vec)
		{
			typedef int v4i __attribute__((ext_vector_type(4)));
			v4i a = *reinterpret_cast<const v4i *>(l + p), b = *reinterpret_cast<const v4i *>(l + p + 4);
			if constexpr (!VALUES) // keeps the two loads whole: alone in the step, they were split into the other path's narrower loads
				asm("" : "+v"(a), "+v"(b));
			lab[0] = a.x, lab[1] = a.y, lab[2] = a.z, lab[3] = a.w, lab[4] = b.x, lab[5] = b.y, lab[6] = b.z, lab[7] = b.w;
			if constexpr (VALUES)
			{
				const uint4 q = *reinterpret_cast<const uint4 *>(f + p);
				const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
				for (int j = 0; j < 4; ++j)
				{
					v[2 * j] = u[j] & 0xFFFFu;
					v[2 * j + 1] = u[j] >> 16;
				}
			}
		}
		else
		{
#pragma unroll
			for (int j = 0; j < WALK_PX; ++j)
			{
				const bool in = !CHECK || p + j < end;
				lab[j] = in ? l[p + j] : pad;
				if constexpr (VALUES)
					v[j] = in ? f[p + j] : 0u;
			}
		}
		if constexpr (!VALUES)
		{
#pragma unroll
			for (int j = 0; j < WALK_PX; ++j)
				v[j] = 0;
		}
	}

	struct WalkPos // where a pixel is: item base + off in its frame, which is (x, y) of a frame w wide
	{
		unsigned off, base, x, y, w;

		__device__ __forceinline__ void next()
		{
			++off;
			if (++x == w)
				x = 0, ++y;
		}
	};

	// to = keep ? from : to, word by word: selects, where an `if` around a whole run compiles to a branch per flush point
	template <class R>
	__device__ __forceinline__ void walk_keep(bool keep, const R &from, R &to)
	{
		static_assert(sizeof(R) % 4 == 0, "a run is 32-bit words");
		unsigned a[sizeof(R) / 4], b[sizeof(R) / 4];
		__builtin_memcpy(a, &from, sizeof(R));
		__builtin_memcpy(b, &to, sizeof(R));
#pragma unroll
		for (unsigned i = 0; i < sizeof(R) / 4; ++i)
			b[i] = keep ? a[i] : b[i];
		__builtin_memcpy(&to, b, sizeof(R));
	}

	// Flush the runs of the lanes with `go` (their label is about to change, or the item ends), called by the whole wave at one point.
	template <class P>
	__device__ __forceinline__ void walk_flush(bool go, const typename P::Run &r, int nregions, unsigned base, const P &pol)
	{
		const unsigned long long m = __ballot(go);
		if (m == 0)
			return;
		const int lead = __ffsll((long long)m) - 1;
		const int label = __shfl(r.cur, lead);
		if ((P::WAVE_ADD <= 1 || __popcll(m) >= P::WAVE_ADD) && __ballot(1) == ~0ull && __ballot(go && r.cur != label) == 0)
		{
			if ((unsigned)label >= (unsigned)nregions)
				return;
			typename P::Run t;
			P::reset(t, label);
			walk_keep(go, r, t); // lanes that do not flush add the empty run
#pragma unroll
			for (int d = 32; d > 0; d >>= 1)
				P::combine(t, d);
			if ((int)__lane_id() == lead)
				pol.put(label, t, base);
			return;
		}
		if (go && (unsigned)r.cur < (unsigned)nregions)
			pol.put(r.cur, r, base);
	}

	// 8 pixels from p, the first at pos: each one either continues the run or flushes it and starts one of its own label.  Pixels at or past
	// `end` (checked steps only) leave the run as it is.
	template <bool CHECK, class P>
	__device__ __forceinline__ void walk_chunk(typename P::Run &r, const uint16_t *__restrict__ f, const int32_t *__restrict__ l, int64_t p, int64_t end,
											   WalkPos pos, bool vec, int nregions, const P &pol)
	{
		unsigned v[WALK_PX];
		int lab[WALK_PX];
		load8<CHECK, P::VALUES>(f, l, p, end, vec, r.cur, v, lab);
		bool same = true;
#pragma unroll
		for (int j = 0; j < WALK_PX; ++j)
			same &= lab[j] == r.cur;
		if (__ballot(!same) == 0) // every lane's 8 pixels continue its run: no flush point
		{
			if (!CHECK && P::chunk8(r, v, pos))
				return;
#pragma unroll
			for (int j = 0; j < WALK_PX; ++j, pos.next())
				if (!CHECK || p + j < end)
					P::pixel(r, v[j], pos);
			return;
		}
#pragma unroll
		for (int j = 0; j < WALK_PX; ++j, pos.next())
		{
			const bool in = !CHECK || p + j < end;
			const bool go = in && lab[j] != r.cur;
			walk_flush(go, r, nregions, pos.base, pol);
			if (go)
				P::reset(r, lab[j]);
			if (in)
				P::pixel(r, v[j], pos);
		}
	}

	// The whole accumulate kernel of a reducer.  frames [n][npx] (not read unless P::VALUES), labels [npx] or, per_frame, [n][npx]; w: the
	// frame width (1 where the policy reads no x, y); the rest is walk_launch_shape()'s and walk_vec()'s answer.
	template <bool LDS, class P>
	__device__ __forceinline__ void walk_regions(P &pol, const uint16_t *__restrict__ frames, const int32_t *__restrict__ labels, unsigned w, int64_t npx,
												 int per_frame, int nregions, int64_t items, int per_item_frame, int vec)
	{
		extern __shared__ unsigned long long walk_lds[];
		if constexpr (LDS)
		{
			pol.carve(walk_lds, nregions);
			for (int r = threadIdx.x; r < nregions; r += WALK_BLOCK)
				pol.clear(r);
			__syncthreads();
		}
		const unsigned step_dy = (unsigned)WALK_STEP / w, step_dx = (unsigned)WALK_STEP % w;
		for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
		{
			const int64_t fi = item / per_item_frame;
			const int64_t lo = (item - fi * per_item_frame) * WALK_ITEM, hi = min(lo + WALK_ITEM, npx);
			const uint16_t *f = P::VALUES ? frames + fi * npx : nullptr;
			const int32_t *l = labels + (per_frame ? fi * npx : 0);
			pol.frame(fi, nregions);
			WalkPos pos;
			pos.base = (unsigned)lo;
			pos.w = w;
			pos.y = (pos.base + threadIdx.x * WALK_PX) / w; // dividend < 2^31 + WALK_ITEM
			pos.x = pos.base + threadIdx.x * WALK_PX - pos.y * w;
			typename P::Run run;
			P::reset(run, INT32_MIN);
			for (int64_t s = lo; s < hi; s += WALK_STEP)
			{
				const int64_t p = s + threadIdx.x * WALK_PX;
				pos.off = (unsigned)(p - lo);
				if (s + WALK_STEP <= hi)
					walk_chunk<false>(run, f, l, p, hi, pos, vec, nregions, pol);
				else
					walk_chunk<true>(run, f, l, p, hi, pos, vec, nregions, pol);
				pos.x += step_dx;
				pos.y += step_dy;
				if (pos.x >= w)
					pos.x -= w, ++pos.y;
			}
			walk_flush(run.cnt != 0, run, nregions, pos.base, pol);
			if constexpr (LDS)
			{
				__syncthreads();
				for (int r = threadIdx.x; r < nregions; r += WALK_BLOCK)
					pol.drain(r);
				__syncthreads();
			}
		}
	}

	// The whole kernel of a counting reducer (the passes of quantile_kernels.hip, histogram_kernels.hip): every pixel becomes the key of a
	// counter, and a thread keeps the run of its current key in registers, so a counter is touched where the key changes.  A workgroup takes
	// a contiguous range of the work items (`items` of them, per_item_frame to a frame of npx walked pixels), so that it meets few frames:
	// where its range passes into another frame, and at its end, the open run is closed and the policy drains the counters it keeps in LDS.
	// A step in which a thread's 8 keys all continue its run adds 8 to it; otherwise the 8 pixels go one by one.  The policy supplies
	//   Key, NONE                  the key type and the key of a pixel that counts nowhere
	//   Run                        the run type, with the key `Key key`; the kernel starts from Run{} re-opened with NONE
	//   clear()                    zero the LDS counters (the kernel's first step, before a barrier)
	//   frame(fi)                  point the loads and the global counters at frame fi
	//   keys<CHECK>(p, end, k)     the keys of the 8 pixels at p; CHECK: a pixel at or past `end` gets NONE
	//   add(run, n)                n more pixels of the run
	//   flush(run, next)           close the run into its counter and open one of key `next`
	//   drain()                    between two barriers: the LDS counters of the open frame to global memory, and zero them
	template <class P>
	__device__ __forceinline__ void walk_counters(P &pol, int64_t npx, int64_t items, int per_item_frame)
	{
		pol.clear();
		__syncthreads();
		typename P::Run run{};
		pol.flush(run, P::NONE);
		const int64_t first = (int64_t)blockIdx.x * items / gridDim.x, last = ((int64_t)blockIdx.x + 1) * items / gridDim.x;
		int64_t open = -1; // the frame the counters and the run belong to
		for (int64_t item = first;; ++item)
		{
			const int64_t fi = item < last ? item / per_item_frame : -1;
			if (fi != open)
			{
				if (open >= 0)
				{
					pol.flush(run, P::NONE);
					__syncthreads();
					pol.drain();
					__syncthreads();
				}
				open = fi;
				if (fi >= 0)
					pol.frame(fi);
			}
			if (fi < 0)
				break; // past the range's last item
			const int64_t lo = (item - fi * per_item_frame) * WALK_ITEM, hi = min(lo + WALK_ITEM, npx);
			for (int64_t s = lo; s < hi; s += WALK_STEP)
			{
				const int64_t p = s + threadIdx.x * WALK_PX;
				typename P::Key key[WALK_PX];
				if (p + WALK_PX <= hi)
					pol.template keys<false>(p, hi, key);
				else
					pol.template keys<true>(p, hi, key);
				bool same = true;
#pragma unroll
				for (int j = 0; j < WALK_PX; ++j)
					same &= key[j] == run.key;
				if (same)
				{
					P::add(run, WALK_PX);
					continue;
				}
#pragma unroll
				for (int j = 0; j < WALK_PX; ++j)
				{
					if (key[j] != run.key)
						pol.flush(run, key[j]);
					P::add(run, 1);
				}
			}
		}
	}

	// Host side of a walking launch.

	inline hipError_t cu_count(int *cus)
	{
		int dev = 0;
		const hipError_t e = hipGetDevice(&dev);
		return e != hipSuccess ? e : hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
	}

	// Whether load8 may take its 16-byte loads: frames that are not read pass as nullptr.
	inline int walk_vec(int64_t npx, const int32_t *labels, const uint16_t *frames)
	{
		return npx % WALK_PX == 0 && (uintptr_t)labels % 16 == 0 && (uintptr_t)frames % 16 == 0;
	}

	struct WalkShape
	{
		int per_item_frame; // items per frame
		int64_t items;
		unsigned grid; // at most as many workgroups per CU as WALK_BLOCKS_PER_CU and their LDS (0: none) allow
	};
	inline WalkShape walk_launch_shape(int64_t npx, int n, size_t lds_bytes_per_block, int cus)
	{
		WalkShape s;
		s.per_item_frame = (int)((npx + WALK_ITEM - 1) / WALK_ITEM);
		s.items = (int64_t)n * s.per_item_frame;
		const size_t fit = lds_bytes_per_block ? std::max<size_t>(1, WALK_LDS_BYTES / lds_bytes_per_block) : WALK_BLOCKS_PER_CU;
		s.grid = (unsigned)std::min<int64_t>(s.items, (int64_t)cus * (int64_t)std::min<size_t>(WALK_BLOCKS_PER_CU, fit));
		return s;
	}
} // namespace rir
