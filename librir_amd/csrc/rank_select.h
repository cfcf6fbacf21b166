// Selection networks of the spatial rank filters (rank_kernels.hip): the median of an odd number of values by min / max exchanges alone.
// Plain C++ templates over the value type V and its two operations Ops::lo / Ops::hi (element-wise min and max: a uint32 of two uint16
// pixels with the packed instructions on the device, a plain integer on the host), so that the network a kernel runs can be run on a CPU.
// Every index is a compile-time constant: on the device the values stay in registers.
#pragma once

#ifdef __HIPCC__
#define RIR_RANK_HD __host__ __device__ __forceinline__
#else
#define RIR_RANK_HD inline
#endif

namespace rir
{
	// a <- min, b <- max
	template <class Ops, class V>
	RIR_RANK_HD void rank_exchange(V &a, V &b)
	{
		const V t = Ops::lo(a, b);
		b = Ops::hi(a, b);
		a = t;
	}
	template <class Ops, class V>
	RIR_RANK_HD V rank_med3(V a, V b, V c)
	{
		return Ops::hi(Ops::lo(a, b), Ops::lo(Ops::hi(a, b), c));
	}

	// p[0 .. N - 1] stays the same multiset, with its minimum at p[0] and its maximum at p[N - 1]: N / 2 exchanges split it into a low and a
	// high half (an odd N leaves the middle value in both), a chain over each half brings the extreme to its end.
	template <class Ops, int N, class V, int M>
	RIR_RANK_HD void rank_extremes(V (&p)[M])
	{
		static_assert(N >= 2 && N <= M, "a prefix of p");
#pragma unroll
		for (int i = 0; i < N / 2; ++i)
			rank_exchange<Ops>(p[i], p[N - 1 - i]);
#pragma unroll
		for (int i = 1; i < (N + 1) / 2; ++i)
			rank_exchange<Ops>(p[0], p[i]);
#pragma unroll
		for (int i = N / 2; i < N - 1; ++i)
			rank_exchange<Ops>(p[i], p[N - 1]);
	}

	// One step of the selection below on the N values p[0 .. N - 1]; in[NEXT] is the next value that has not been looked at.
	template <class Ops, int N, int NEXT, int C, class V>
	RIR_RANK_HD V rank_forget(V (&p)[C / 2 + 2], const V (&in)[C])
	{
		if constexpr (N == 3)
			return rank_med3<Ops>(p[0], p[1], p[2]);
		else
		{
			rank_extremes<Ops, N>(p);
			p[0] = in[NEXT]; // (the minimum is forgotten; so is the maximum, p[N - 1], which the next step leaves out)
			return rank_forget<Ops, N - 1, NEXT + 1, C>(p, in);
		}
	}

	// The median (rank C / 2) of C values, C odd: among any C / 2 + 2 of them neither the smallest nor the largest can be the median - each
	// has C / 2 + 1 values on one side -, so both are dropped and one new value joins; every later step drops two more in the same way (what
	// was dropped before still counts on its side), until three values are left, whose median is the answer.  Equal values need no care: a
	// value dropped as an extreme while equal to the median leaves an equal one behind.  129 exchanges for C = 25, 17 for C = 9.
	template <class Ops, int C, class V>
	RIR_RANK_HD V rank_median(const V (&in)[C])
	{
		static_assert(C % 2 == 1 && C >= 3, "an odd count");
		constexpr int K = C / 2 + 2;
		V p[K];
#pragma unroll
		for (int i = 0; i < K; ++i)
			p[i] = in[i];
		return rank_forget<Ops, K, K, C>(p, in);
	}
} // namespace rir
