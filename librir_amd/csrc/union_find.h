// Lock-free union-find forest over int32 indices in which a root is always the LOWEST index of its tree - device code shared by the
// units that build one: label_kernels.hip (pixels of an image) and track_kernels.hip (components of a label stack).  Internal linkage:
// every unit that includes this gets its own inlined copy of the routines, and there is one text of them and of their race argument.
#pragma once
#include <hip/hip_runtime.h>

namespace rir
{
	namespace
	{
		// The forests are read and written by many waves at once: a link is loaded and stored as one 32-bit access at the scope that
		// shares it (never a stale copy from the CU's vector cache, never torn).
		template <int SCOPE>
		__device__ __forceinline__ int link_load(const int *p)
		{
			return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
		}
		template <int SCOPE>
		__device__ __forceinline__ void link_store(int *p, int v)
		{
			__hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE);
		}

		// Root of i's tree; on the way every visited node is re-pointed at its grandparent (path splitting).  A link only ever moves to an
		// ancestor, so a reader that sees the older value still climbs the same tree.  Racing with unite(): a node that unite() found to
		// be a root (atomicMin returned the node itself) was a root until that instant, so no splitting store - which only touches nodes
		// read as non-roots - can overwrite the link unite() just made; when the atomicMin lands on a node that had stopped being a root,
		// unite() carries on with the parent it displaced, and whatever a splitting store does to that node stays inside one tree.
		template <int SCOPE>
		__device__ __forceinline__ int find_root(int *L, int i)
		{
			int p = link_load<SCOPE>(&L[i]);
			while (p != i)
			{
				const int g = link_load<SCOPE>(&L[p]);
				if (g != p)
					link_store<SCOPE>(&L[i], g);
				i = p;
				p = g;
			}
			return i;
		}

		// Joins the trees of a and b: the higher root is hung under the lower one, so a root is always the lowest index of its tree.
		// Every failed round lowers max(a, b) (the displaced parent is below the node it was read from), so the loop ends for every wave
		// whatever the others do.
		template <int SCOPE>
		__device__ __forceinline__ void unite(int *L, int a, int b)
		{
			for (;;)
			{
				a = find_root<SCOPE>(L, a);
				b = find_root<SCOPE>(L, b);
				if (a == b)
					return;
				if (a > b)
				{
					const int t = a;
					a = b;
					b = t;
				}
				const int old = atomicMin(&L[b], a);
				if (old == b)
					return;
				b = old;
			}
		}

		// Joins the tree of y with the tree of `low`, any node below y (not necessarily a root), in one atomic where y is still the root
		// of its tree - the case of a node that is linked for the first time: y is hung under `low` itself.  A root stays the lowest
		// index of its tree (every node of y's tree is at or above y, and low's root is at or below low).  Where y had a parent already, the
		// atomicMin leaves the lower of the two in the link and the other one is joined by unite(): this is unite()'s own case of an
		// atomicMin that lands on a node that has stopped being a root, and its race argument holds word for word.
		template <int SCOPE>
		__device__ __forceinline__ void hang(int *L, int low, int y)
		{
			const int old = atomicMin(&L[y], low);
			if (old != y && old != low)
				unite<SCOPE>(L, low, old);
		}
	} // namespace
} // namespace rir
