// Lossless block codec for 16-bit IR frames — gfx950 (CDNA4) kernels.  Format "RIRB1", DESIGN.md §3.
//
// Replaces, behind the librir C ABI, what libx264 does for the reference saver/loader
// (reference: src/cpp/video_io/h264.cpp:1022-1131 AddFrame, :3096-3229 GetFrame; byte-plane
// split :1066-1082 / merge :3016-3051).  The bitstream is this build's own; the parity contract is
// the reference tests' identity decode(encode(x)) == x plus bit-exact equality with the CPU
// restatement in oracle/rir_oracle.c.
//
// Mapping to the machine
//   * one 64-lane wavefront owns one TILE of 512 consecutive pixels (1 KiB: one 16-byte load per
//     lane, fully coalesced) for every frame of a chunk, and walks the time axis in registers:
//     the previous frame never leaves VGPRs, so every raw pixel crosses HBM exactly once;
//   * residual = prediction error minus its tile minimum (DPP min-reduce), so it is an unsigned
//     range [0, max-min];
//   * the bit-planes of the 8 residual slots are produced by two 64x64 BIT-MATRIX TRANSPOSES
//     across the wavefront (v_permlane32_swap + 5 butterfly stages of {cross-lane move,
//     v_alignbit, v_bfi}): afterwards lane 16j+b holds plane b of slot j, a ballot of the
//     non-zero planes gives the 8 widths on the scalar unit, and each lane stores its own word.
//     No LDS, no barriers, no data-dependent branches, fixed instruction count per record;
//   * decode is the mirror image (the transpose is an involution);
//   * 4 independent waves per 256-thread workgroup; grid = (ntiles/4) x nchunks >> 256 CUs.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "codec_format.h"
#include "filter_kernels.h"
#include "runtime.h"

namespace rir
{

	// Cache policy of each traffic class (aux operand of the buffer instructions: 2 = nt, "streaming"; 16 = sc1, write-through to
	// the fabric; 18 = both).  What decides it is what a kernel leaves behind: L2 is private to an XCD, so a line that is dirty in
	// L2 when a kernel ends is written back by the release at its end - while the chip does nothing else - and the next kernel,
	// whose workgroups run on any XCD, cannot use it where it lay.  nt is a replacement hint, not write-through.
	//   raw frames, read once by the encoders                     nt loads: they must not evict what the next kernel reads
	//   raw frames, written once by the decoders                  nt stores (FRAME_STORE_AUX; the packed decoder's own constant
	//                                                             PACKED_FRAME_STORE_AUX, measured apart: DESIGN.md section 3)
	//   the packed encoder's payload, headers, seg_pos/seg_words  read by the NEXT kernel from the Infinity Cache: PAYLOAD_STORE_AUX /
	//                                                             TABLE_STORE_SC1, whole 128-byte lines per store instruction where
	//                                                             the policy is write-through (a line written by two write-through
	//                                                             instructions goes to the fabric twice)
	//   the slots of rirb1_encode_tiles, the dense stream         default: written and read in L2-sized pieces by neighbouring launches
	//   stream loads of the decoders                              default
	// The legs measured on the packed step are in profiles/packed_wt_time.txt.
	constexpr int FRAME_LOAD_AUX = 2;
	constexpr int FRAME_STORE_AUX = 2;
	constexpr int PACKED_FRAME_STORE_AUX = 2; // rirb1_decode_packed's frame stores
	constexpr int SPARSE_STORE_AUX = 0;
	constexpr int STREAM_LOAD_AUX = 0;
	constexpr int PAYLOAD_STORE_AUX = 16;	  // rirb1_encode_packed's copy-out of a segment
	constexpr bool TABLE_STORE_SC1 = true;	  // the staged encoders' headers, rirb1_encode_packed's seg_pos / seg_words

	typedef short short2v __attribute__((ext_vector_type(2)));
	typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));

	// ---- packed 2 x u16 arithmetic (low half = even pixel) -----------------------------------
	__device__ __forceinline__ uint32_t pk_sub16(uint32_t a, uint32_t b)
	{
		return __builtin_bit_cast(uint32_t, __builtin_bit_cast(ushort2v, a) - __builtin_bit_cast(ushort2v, b));
	}
	__device__ __forceinline__ uint32_t pk_add16(uint32_t a, uint32_t b)
	{
		return __builtin_bit_cast(uint32_t, __builtin_bit_cast(ushort2v, a) + __builtin_bit_cast(ushort2v, b));
	}
	__device__ __forceinline__ uint32_t pk_min_i16(uint32_t a, uint32_t b)
	{
		return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b)));
	}
	__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
	{
		return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(ushort2v, a), __builtin_bit_cast(ushort2v, b)));
	}

	// ---- wave reductions / scans ------------------------------------------------------------------
	// DPP row shifts inside the four 16-lane rows, then the two row broadcasts; lane 63 has the total.
	__device__ __forceinline__ int32_t wave_min_i32(int32_t v)
	{
		const int32_t id = 0x7fffffff;
		v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x111, 0xf, 0xf, false)); // row_shr:1
		v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x112, 0xf, 0xf, false)); // row_shr:2
		v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x114, 0xf, 0xf, false)); // row_shr:4
		v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x118, 0xf, 0xf, false)); // row_shr:8
		v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xa, 0xf, false)); // row_bcast:15
		v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x143, 0xc, 0xf, false)); // row_bcast:31
		return __builtin_amdgcn_readlane(v, 63);
	}
	__device__ __forceinline__ uint32_t wave_or(uint32_t v)
	{
		v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
		v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
		v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
		v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
		v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true);
		v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true);
		return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
	}
	// inclusive add-scan over the 64 lanes (rare paths only)
	__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v, int lane)
	{
#pragma unroll
		for (int d = 1; d < 64; d <<= 1)
		{
			uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
			if (lane >= d)
				v += o;
		}
		return v;
	}

	__device__ __forceinline__ uint32_t bitlen32(uint32_t v) { return v ? 32u - (uint32_t)__builtin_clz(v) : 0u; }

	// ---- 64x64 bit-matrix transpose across the wavefront ----------------------------------------
	// Lane l holds row l as (lo, hi); afterwards lane q holds column q: bit l of the result = bit q
	// of lane l's input.  Recursive block swap: distance 32 is one v_permlane32_swap, distances
	// 16..1 exchange with lane l^s and merge with a per-lane rotate amount and select mask.
	struct TransposeConsts
	{
		uint32_t k16, k8, k4, k2, k1; // select mask: bits taken from the partner
		uint32_t a16, a8, a4, a2, a1; // right-rotate amount applied to the partner's dword
	};
	__device__ __forceinline__ TransposeConsts make_transpose_consts(int lane)
	{
		TransposeConsts c;
		c.k16 = (lane & 16) ? 0x0000ffffu : 0xffff0000u;
		c.k8 = (lane & 8) ? 0x00ff00ffu : 0xff00ff00u;
		c.k4 = (lane & 4) ? 0x0f0f0f0fu : 0xf0f0f0f0u;
		c.k2 = (lane & 2) ? 0x33333333u : 0xccccccccu;
		c.k1 = (lane & 1) ? 0x55555555u : 0xaaaaaaaau;
		c.a16 = 16;
		c.a8 = (lane & 8) ? 8 : 24;
		c.a4 = (lane & 4) ? 4 : 28;
		c.a2 = (lane & 2) ? 2 : 30;
		c.a1 = (lane & 1) ? 1 : 31;
		return c;
	}
	// (mask & a) | (~mask & b) in one VALU op: v_bitop3_b32 with the truth table of a 3-input mux
	__device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) { return __builtin_amdgcn_bitop3_b32(mask, a, b, 0xCA); }

#define RIR_XOR16(x) ((uint32_t)__builtin_amdgcn_ds_swizzle((int)(x), (16 << 10) | 0x1f))
#define RIR_XOR8(x) ((uint32_t)__builtin_amdgcn_mov_dpp((int)(x), 0x128, 0xf, 0xf, false)) /* row_ror:8 */
#define RIR_XOR4(x) ((uint32_t)__builtin_amdgcn_ds_swizzle((int)(x), (4 << 10) | 0x1f))
#define RIR_XOR2(x) ((uint32_t)__builtin_amdgcn_mov_dpp((int)(x), 0x4e, 0xf, 0xf, false)) /* quad_perm:[2,3,0,1] */
#define RIR_XOR1(x) ((uint32_t)__builtin_amdgcn_mov_dpp((int)(x), 0xb1, 0xf, 0xf, false)) /* quad_perm:[1,0,3,2] */
#define RIR_TSTAGE2(X, K, A)                                    \
	{                                                           \
		const uint32_t t0 = X(a0), t1 = X(a1), t2 = X(b0), t3 = X(b1); \
		a0 = bfi(K, __builtin_amdgcn_alignbit(t0, t0, A), a0);   \
		a1 = bfi(K, __builtin_amdgcn_alignbit(t1, t1, A), a1);   \
		b0 = bfi(K, __builtin_amdgcn_alignbit(t2, t2, A), b0);   \
		b1 = bfi(K, __builtin_amdgcn_alignbit(t3, t3, A), b1);   \
	}

	// two independent transposes, stage by stage (4 independent dword chains fill the DPP/LDS latency)
	__device__ __forceinline__ void transpose64x2(uint32_t &a0, uint32_t &a1, uint32_t &b0, uint32_t &b1, const TransposeConsts &c)
	{
		auto ra = __builtin_amdgcn_permlane32_swap(a0, a1, false, false); // lo[32..63] <-> hi[0..31]
		auto rb = __builtin_amdgcn_permlane32_swap(b0, b1, false, false);
		a0 = ra[0];
		a1 = ra[1];
		b0 = rb[0];
		b1 = rb[1];
		RIR_TSTAGE2(RIR_XOR16, c.k16, c.a16)
		RIR_TSTAGE2(RIR_XOR8, c.k8, c.a8)
		RIR_TSTAGE2(RIR_XOR4, c.k4, c.a4)
		RIR_TSTAGE2(RIR_XOR2, c.k2, c.a2)
		RIR_TSTAGE2(RIR_XOR1, c.k1, c.a1)
	}

	// 32x32 bit-matrix transpose inside each 32-lane half of the wave (one dword per lane): lane q of a
	// half ends with bit l = bit q of that half's lane l.  Same butterfly, without the 32-lane stage.
	__device__ __forceinline__ uint32_t transpose32(uint32_t x, const TransposeConsts &c)
	{
		uint32_t t;
		t = RIR_XOR16(x);
		x = bfi(c.k16, __builtin_amdgcn_alignbit(t, t, c.a16), x);
		t = RIR_XOR8(x);
		x = bfi(c.k8, __builtin_amdgcn_alignbit(t, t, c.a8), x);
		t = RIR_XOR4(x);
		x = bfi(c.k4, __builtin_amdgcn_alignbit(t, t, c.a4), x);
		t = RIR_XOR2(x);
		x = bfi(c.k2, __builtin_amdgcn_alignbit(t, t, c.a2), x);
		t = RIR_XOR1(x);
		x = bfi(c.k1, __builtin_amdgcn_alignbit(t, t, c.a1), x);
		return x;
	}

	// ---- tile I/O ------------------------------------------------------------------------------------
	struct Px8
	{
		uint32_t d[4]; // 8 x u16, d[k] = pixels 2k (low) and 2k+1 (high)
	};

	// 8 consecutive pixels of frame `f` starting at flat index p0 (zero past the end of the frame)
	__device__ __forceinline__ Px8 load8(const uint16_t *__restrict__ frames, int64_t f, int64_t npx, int64_t p0, bool vec_ok)
	{
		Px8 r;
		const uint16_t *src = frames + f * npx + p0;
		if (vec_ok)
		{
			uint4 v = *reinterpret_cast<const uint4 *>(src);
			r.d[0] = v.x;
			r.d[1] = v.y;
			r.d[2] = v.z;
			r.d[3] = v.w;
		}
		else
		{
#pragma unroll
			for (int k = 0; k < 4; ++k)
			{
				uint32_t lo = (p0 + 2 * k < npx) ? src[2 * k] : 0u;
				uint32_t hi = (p0 + 2 * k + 1 < npx) ? src[2 * k + 1] : 0u;
				r.d[k] = lo | (hi << 16);
			}
		}
		return r;
	}

	__device__ __forceinline__ void store8(uint16_t *__restrict__ frames, int64_t f, int64_t npx, int64_t p0, bool vec_ok, const Px8 &r)
	{
		uint16_t *dst = frames + f * npx + p0;
		if (vec_ok)
		{
			uint4 v;
			v.x = r.d[0];
			v.y = r.d[1];
			v.z = r.d[2];
			v.w = r.d[3];
			*reinterpret_cast<uint4 *>(dst) = v;
		}
		else
		{
#pragma unroll
			for (int k = 0; k < 4; ++k)
			{
				if (p0 + 2 * k < npx)
					dst[2 * k] = (uint16_t)(r.d[k] & 0xffffu);
				if (p0 + 2 * k + 1 < npx)
					dst[2 * k + 1] = (uint16_t)(r.d[k] >> 16);
			}
		}
	}

	// ---- buffer-resource addressing -------------------------------------------------------------
	// Every vector-memory operation of the steady-state loops is an UNCONDITIONAL raw-buffer access:
	// lanes that must not touch memory get an out-of-range offset (the hardware drops the store /
	// returns 0 for the load), so no branch surrounds a memory instruction and the compiler can keep
	// exact s_waitcnt vmcnt(N) counts - which is what lets three frames stay in flight per wave.
	typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
	typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));
#define RIR_BUF_FLAGS 0x00020000 /* raw buffer, 32-bit data format (gfx942/gfx950 descriptor word 3) */
#define RIR_OOB 0x40000000u		 /* beyond any num_records used here */
#define RIR_NONE 0xffffffffu	 /* "no plane" as a word index */

	__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, uint32_t bytes)
	{
		// the base is wave-uniform by construction; readfirstlane makes that provable
		const uint64_t b = (uint64_t)base;
		const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
		const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
		return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, (int)bytes, RIR_BUF_FLAGS);
	}
	__device__ __forceinline__ Px8 buf_load8(const void *tile_base, uint32_t lane_off)
	{
		const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(make_rsrc(tile_base, RIRB1_TILE_PX * 2), lane_off, 0, FRAME_LOAD_AUX);
		Px8 r;
		r.d[0] = v.x;
		r.d[1] = v.y;
		r.d[2] = v.z;
		r.d[3] = v.w;
		return r;
	}
	template <int AUX = FRAME_STORE_AUX>
	__device__ __forceinline__ void buf_store8(void *tile_base, uint32_t lane_off, const Px8 &r)
	{
		v4u32 v;
		v.x = r.d[0];
		v.y = r.d[1];
		v.z = r.d[2];
		v.w = r.d[3];
		__builtin_amdgcn_raw_buffer_store_b128(v, make_rsrc(tile_base, RIRB1_TILE_PX * 2), lane_off, 0, AUX);
	}

	// tile minimum of the 8 packed values of every lane -> wave-uniform 16-bit base
	__device__ __forceinline__ uint32_t tile_base(const Px8 &d, bool is_signed)
	{
		int32_t v;
		if (is_signed)
		{
			const uint32_t m = pk_min_i16(pk_min_i16(d.d[0], d.d[1]), pk_min_i16(d.d[2], d.d[3]));
			v = min((int32_t)(int16_t)(m & 0xffffu), (int32_t)m >> 16);
		}
		else
		{
			const uint32_t m = pk_min_u16(pk_min_u16(d.d[0], d.d[1]), pk_min_u16(d.d[2], d.d[3]));
			v = (int32_t)min(m & 0xffffu, m >> 16);
		}
		return (uint32_t)wave_min_i32(v) & 0xffffu;
	}

	// left-delta prediction error inside a tile (MODE_LEFT): d[i] = p[i] - p[i-1], p[-1] = 0
	__device__ __forceinline__ Px8 left_delta(const Px8 &cur, int lane)
	{
		uint32_t prev_last = (uint32_t)__shfl_up((int)(cur.d[3] >> 16), 1, 64);
		if (lane == 0)
			prev_last = 0;
		Px8 d;
		d.d[0] = pk_sub16(cur.d[0], (cur.d[0] << 16) | prev_last);
		d.d[1] = pk_sub16(cur.d[1], (cur.d[1] << 16) | (cur.d[0] >> 16));
		d.d[2] = pk_sub16(cur.d[2], (cur.d[2] << 16) | (cur.d[1] >> 16));
		d.d[3] = pk_sub16(cur.d[3], (cur.d[3] << 16) | (cur.d[2] >> 16));
		return d;
	}

	// sum over the 8 slots of the bit length of the OR of the slot's residuals (payload words)
	__device__ __forceinline__ uint32_t payload_words(const Px8 &r)
	{
		uint32_t tot = 0;
#pragma unroll
		for (int k = 0; k < 4; ++k)
		{
			const uint32_t o = wave_or(r.d[k]);
			tot += bitlen32(o & 0xffffu) + bitlen32(o >> 16);
		}
		return tot;
	}

	// ---- per-lane bookkeeping of a record (no scalar-unit work) ---------------------------------
	// After the transposes lane 16q+k holds plane k of slot q (half A) and of slot 4+q (half B).
	struct LaneConsts
	{
		uint32_t bit;	 // k = lane & 15
		uint32_t bitp1;	 // k + 1
		uint32_t onehot; // 1 << k
		uint32_t sh4;	 // 4 * q   (base nibble of this row)
		uint32_t sh16;	 // 16 * (q & 1)
		bool row_hi;	 // q >= 2 : this row's header field is in the high dword
		bool row0;		 // q == 0
		// narrow tier (all widths <= 4): lane (lane & 31) = 4*slot + plane, the two 32-lane halves
		// hold the low / high dword of the plane word
		uint32_t n_bit;	   // plane = lane & 3
		uint32_t n_sh;	   // 4 * slot : position of the slot's planes in the 32-bit non-zero mask
		uint32_t n_half;   // byte offset of this half inside the 64-bit word (0 or 4)
		uint32_t n_hsh;	   // bit position of the slot's width inside its header dword
		bool n_hhi;		   // the slot's width lives in the high header dword
		bool n_first;	   // plane 0 of its slot
		// narrow tier, packed-nibble order (see emit_words_narrow): nibble n of the packed dword holds slot
		// NIB_SLOT[n] = {0,4,2,6,1,5,3,7}; lane (lane & 31) = 4n + b holds plane b of that slot
		uint32_t p_before; // mask of the lanes whose plane words precede this lane's word in the stream
		uint32_t p_hshw;   // header lane 16q+k: left shift that brings its bit of the width word W to bit 31
		uint32_t p_hshb;   // same for the base/mode word
	};
	__device__ __forceinline__ LaneConsts make_lane_consts(int lane)
	{
		LaneConsts c;
		const uint32_t q = (uint32_t)lane >> 4;
		c.bit = lane & 15;
		c.bitp1 = c.bit + 1;
		c.onehot = 1u << c.bit;
		c.sh4 = 4 * q;
		c.sh16 = 16 * (q & 1);
		c.row_hi = q >= 2;
		c.row0 = q == 0;
		const uint32_t slot = ((uint32_t)lane & 31u) >> 2;
		c.n_bit = lane & 3;
		c.n_sh = 4 * slot;
		c.n_half = ((uint32_t)lane >> 5) * 4;
		c.n_hsh = 16 * (slot & 1) + (slot >= 4 ? 5 : 0);
		c.n_hhi = (slot & 2) != 0;
		c.n_first = (lane & 3) == 0;
		{
			const uint32_t nib_slot[8] = {0, 4, 2, 6, 1, 5, 3, 7};
			const uint32_t n = ((uint32_t)lane & 31u) >> 2, b = lane & 3;
			uint32_t before = ((1u << b) - 1u) << (4 * n);
			for (uint32_t m = 0; m < 8; ++m)
				if (nib_slot[m] < nib_slot[n])
					before |= 0xfu << (4 * m);
			c.p_before = before;
			// header field q = w_q | w_{4+q} << 5 | base nibble q << 10 | mode << 14 (q == 0); lane 16q+k tests bit k.
			// Slot q sits in nibble nq = {0,4,2,6}[q] of W, slot 4+q in nibble nq+1; widths are <= 4 (3 bits).
			const uint32_t k = lane & 15, nq = (q & 1) * 4 + (q >> 1) * 2;
			uint32_t bw = 3; // a bit of W that is always 0
			if (k < 3)
				bw = 4 * nq + k;
			else if (k >= 5 && k < 8)
				bw = 4 * (nq + 1) + (k - 5);
			c.p_hshw = 31 - bw;
			uint32_t bb = 31; // a bit of (base | mode << 16) that is always 0
			if (k >= 10 && k < 14)
				bb = 4 * q + (k - 10);
			else if (k >= 14 && q == 0)
				bb = 16 + (k - 14);
			c.p_hshb = 31 - bb;
		}
		return c;
	}

	// max over the 16 lanes of a row, result in every lane (4 DPP rotations)
	__device__ __forceinline__ uint32_t row_allmax(uint32_t v)
	{
		v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x121, 0xf, 0xf, false)); // row_ror:1
		v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x122, 0xf, 0xf, false)); // row_ror:2
		v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xf, 0xf, false)); // row_ror:4
		v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xf, 0xf, false)); // row_ror:8
		return v;
	}
	// w: row-uniform value.  Returns the inclusive sum over rows 0..q (row-uniform); row 3 holds the total.
	__device__ __forceinline__ uint32_t rows_inclusive_sum(uint32_t w)
	{
		const uint32_t s = w + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x142, 0xa, 0xf, false); // row_bcast:15 -> rows 1,3
		return s + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x143, 0xc, 0xf, false);			  // row_bcast:31 -> rows 2,3
	}

	// inclusive sum over the 32 lanes of each half (DPP row shifts + one row broadcast)
	__device__ __forceinline__ uint32_t half_inclusive_sum(uint32_t v)
	{
		v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true); // row_shr:1
		v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true); // row_shr:2
		v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true); // row_shr:4
		v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true); // row_shr:8
		v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15 -> rows 1,3
		return v;
	}
	// bit length of a value < 2^31 without a zero test: bitlen(2f+1) = bitlen(f)+1
	__device__ __forceinline__ uint32_t bitlen_nz(uint32_t f) { return 31u - (uint32_t)__builtin_clz((f << 1) | 1u); }

	// ---- the plane words of a record -----------------------------------------------------------------
	// The two plane words of a lane and where they go.  A position is (index of the word in the wave's payload) * SCALE, or NONE for a
	// lane without a plane: each target asks for the form it consumes as it is - the direct slot for byte offsets of buffer stores
	// (SCALE 8, RIR_OOB), the staged target for word indices (SCALE 1, RIR_NONE) - so neither converts after the fact.
	// The words are stored by the sink, outside the wave-uniform tier branch: the direct sink's two 8-byte stores of a record are
	// unconditional, so that the compiler keeps exact s_waitcnt vmcnt(N) counts (a store inside the branch made it fall back to vmcnt(0)
	// on half of the steps); the staged sink writes LDS only.
	struct RecordWords
	{
		v2u32 va, vb;
		uint32_t pa, pb;
	};

	// Narrow tier: every residual < 16.  The 8 nibbles of a lane are packed in one dword (3 shift-ors, nibble
	// order r0 r4 r2 r6 r1 r5 r3 r7) and ONE 32x32 transpose per half-wave produces the 32 candidate planes
	// (lane 4n+b: plane b of the slot in nibble n; the upper half holds bits 32..63 of the same plane word).
	// Everything after the ballot is wave-uniform and runs on the scalar unit: M = the mask of stored planes
	// (non-zero mask smeared down inside each nibble), W = per-nibble popcount of M = the 8 widths.  A lane's
	// word index is a popcount of M under a per-lane constant mask; the header is two ballots of per-lane
	// bit tests of W and of (base | mode << 16).
	template <uint32_t SCALE, uint32_t NONE>
	__device__ __forceinline__ uint64_t emit_words_narrow(const Px8 &r, uint32_t mode, uint32_t base, RecordWords &rw, uint32_t pos,
														  const LaneConsts &lc, const TransposeConsts &tc, uint32_t *words)
	{
		uint32_t x = (r.d[0] | (r.d[1] << 8)) | ((r.d[2] | (r.d[3] << 8)) << 4);
		x = transpose32(x, tc);
		const uint64_t nz64 = __ballot(x != 0);
		const uint32_t nz = (uint32_t)nz64 | (uint32_t)(nz64 >> 32); // bit 4n+b: plane b of nibble n is not empty
		uint32_t M = nz | ((nz >> 1) & 0x77777777u);
		M |= (M >> 2) & 0x33333333u; // nibble n = (1 << w) - 1
		uint32_t W = M - ((M >> 1) & 0x55555555u);
		W = (W & 0x33333333u) + ((W >> 2) & 0x33333333u); // nibble n = w (0..4)
		*words = (uint32_t)__builtin_popcount(M);
		// lower-half lanes assemble the 64-bit plane word (their dword | the partner lane's dword << 32)
		auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false); // sw[1] lower lanes = x of lane + 32
		rw.va.x = x, rw.va.y = sw[1];
		const uint32_t at = (pos + (uint32_t)__builtin_popcount(M & lc.p_before)) * SCALE;
		rw.pa = __builtin_amdgcn_inverse_ballot_w64((uint64_t)M) ? at : NONE; // lane l < 32 has a word iff bit l of M
		rw.vb = rw.va, rw.pb = NONE;
		const uint32_t B = base | (mode << 16);
		const uint64_t hw = __ballot((int32_t)(W << lc.p_hshw) < 0) & 0x00E700E700E700E7ull;
		const uint64_t hb = __ballot((int32_t)(B << lc.p_hshb) < 0) & 0x3C003C003C00FC00ull;
		return hw | hb;
	}

	// Wide tier (any width up to 16): two 64x64 transposes, lane 16q+k holds plane k of slots q and 4+q.
	template <uint32_t SCALE, uint32_t NONE>
	__device__ __forceinline__ uint64_t emit_words_wide(const Px8 &r, uint32_t mode, uint32_t base, RecordWords &rw, uint32_t pos,
														const LaneConsts &lc, const TransposeConsts &tc, uint32_t *words)
	{
		uint32_t alo = r.d[0], ahi = r.d[1], blo = r.d[2], bhi = r.d[3];
		transpose64x2(alo, ahi, blo, bhi, tc);
		const uint32_t wa = row_allmax((alo | ahi) != 0 ? lc.bitp1 : 0u); // width of slot q
		const uint32_t wb = row_allmax((blo | bhi) != 0 ? lc.bitp1 : 0u); // width of slot 4+q
		const uint32_t ia = rows_inclusive_sum(wa), ib = rows_inclusive_sum(wb);
		const uint32_t tot_a = (uint32_t)__builtin_amdgcn_readlane((int)ia, 63);
		const uint32_t tot_b = (uint32_t)__builtin_amdgcn_readlane((int)ib, 63);
		// one word per half; lanes without a plane have none
		rw.va.x = alo, rw.va.y = ahi, rw.vb.x = blo, rw.vb.y = bhi;
		rw.pa = lc.bit < wa ? (pos + ia - wa + lc.bit) * SCALE : NONE;
		rw.pb = lc.bit < wb ? (pos + tot_a + ib - wb + lc.bit) * SCALE : NONE;
		*words = tot_a + tot_b;
		// header = ballot of the row's 16-bit field (w_q | w_{4+q} << 5 | base nibble q << 10 | mode << 14)
		const uint32_t nib = (base >> lc.sh4) & 15u;
		const uint32_t field = ((nib << 10) | (lc.row0 ? mode << 14 : 0u)) | ((wb << 5) | wa);
		return __ballot((field & lc.onehot) != 0);
	}

	// The payload of one record: residuals r (packed pairs) -> plane words at positions pos .. pos + words.  Returns the header.
	// The tier is a property of the data (wave-uniform branch), the bitstream is the same either way.
	template <uint32_t SCALE, uint32_t NONE>
	__device__ __forceinline__ uint64_t emit_words(const Px8 &r, uint32_t mode, uint32_t base, RecordWords &rw, uint32_t pos, const LaneConsts &lc,
												   const TransposeConsts &tc, uint32_t *words)
	{
		const uint32_t any = (r.d[0] | r.d[1]) | (r.d[2] | r.d[3]);
		if (__ballot((any & 0xfff0fff0u) != 0) == 0)
			return emit_words_narrow<SCALE, NONE>(r, mode, base, rw, pos, lc, tc, words);
		return emit_words_wide<SCALE, NONE>(r, mode, base, rw, pos, lc, tc, words);
	}

	// A word of a table the NEXT kernel reads (a header, seg_pos, seg_words).  STAGED (the single-pass encoders) and TABLE_STORE_SC1: the
	// store is write-through (an agent-scope relaxed store is the sc1 form of the same global store instruction), so the line is not left
	// dirty in L2 for the release at the kernel's end; otherwise the plain store.
	template <bool STAGED, class T>
	__device__ __forceinline__ void store_table_word(T *p, T v)
	{
		if (STAGED && TABLE_STORE_SC1)
			__hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		else
			*p = v;
	}

	// ---- where a record's words go: the two sinks of encode_run ------------------------------------------
	// sink.emit<DIR>(residuals, mode, base, pos, ...) files the record that begins at word `pos` of what the wave has produced so far
	// and returns its header.  GUARDED_STEPS tells the frame walk whether a record's work may sit under a condition: not the direct sink's,
	// which issues two unconditional buffer stores per record (out of range for a lane without a plane); the staged sink's, which issues none.
	//
	// The direct sink: the segment's slot in the workspace (rirb1_encode_tiles), filled from word 0 in the order of production.
	struct DirectSink
	{
		static constexpr bool GUARDED_STEPS = false; // its stores must not sit under a condition
		__amdgpu_buffer_rsrc_t out;
		__device__ __forceinline__ void keep_key(const v4u32 &, int) {} // (walks forwards only)
		__device__ __forceinline__ v4u32 kept_key(int) { return v4u32{}; }
		template <int DIR>
		__device__ __forceinline__ uint64_t emit(const Px8 &r, uint32_t mode, uint32_t base, uint32_t pos, const LaneConsts &lc,
												 const TransposeConsts &tc, uint32_t *words)
		{
			static_assert(DIR > 0, "a slot is filled in frame order from word 0: the direct sink only walks forwards");
			RecordWords rw;
			const uint64_t h = emit_words<8u, RIR_OOB>(r, mode, base, rw, pos, lc, tc, words);
			__builtin_amdgcn_raw_buffer_store_b64(rw.va, out, rw.pa, 0, SPARSE_STORE_AUX);
			__builtin_amdgcn_raw_buffer_store_b64(rw.vb, out, rw.pb, 0, SPARSE_STORE_AUX);
			return h;
		}
	};

	// first word of an extent of `need` words, ~0 when the arena is full (the launch is marked); wave-uniform
	__device__ __noinline__ uint64_t staging_take_extent(unsigned long long *cursor, uint32_t need, uint64_t arena_words, uint32_t *error_word)
	{
		// (the lane from the execution mask: threadIdx would be one more register that the caller has to hand over)
		const bool first_lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0;
		unsigned long long off = 0;
		if (first_lane)
			off = __hip_atomic_fetch_add(cursor, (unsigned long long)need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)off);
		const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(off >> 32));
		off = ((unsigned long long)hi << 32) | lo;
		if (off + need > arena_words)
		{ // no room: the caller keeps no extent and stores nothing
			if (first_lane)
				__hip_atomic_fetch_or(error_word, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			return ~0ull;
		}
		return off;
	}

	// The flush of the staged sink: the n words at `src` (the wave's LDS region) go to dst (its spill area), with coalesced 8-byte stores
	// as in copy_wave_words.  Out of line, and a word at a time: the registers it uses are registers the frame loop cannot keep across
	// the call.
	typedef const __attribute__((address_space(3))) uint64_t *lds_words_ptr;
	typedef __attribute__((address_space(1))) uint64_t *global_words_ptr;
	__device__ __noinline__ void staging_flush(global_words_ptr dst, lds_words_ptr src, uint32_t n)
	{
#pragma unroll 1
		for (uint32_t j = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); j < n; j += 64)
			dst[j] = src[j];
	}

	// The staged sink (single-pass encoders): every record is filed in the wave's LDS region and emit() issues no vector-memory
	// operation.  When a record does not fit, staging_flush() copies what the region holds - the records the wave produced FIRST - to
	// the wave's spill area in the workspace and the region is empty again; a record is at most RIRB1_REC_MAX_WORDS <= the region, so
	// one flush always makes room.
	// Two kinds of spill area.  STATIC (cursor == nullptr): `area` is the wave's own worst-case slot, there from the start
	// (rirb1_encode_dense).  DYNAMIC (rirb1_encode_packed): nothing is reserved; the wave that flushes for the first time takes an
	// extent of `need` words - the worst case of its share of the chunk - from a bump cursor in the workspace, once.
	// DIR > 0: the wave walks its frames forwards and fills its region and its area upwards from word 0; its words in stream order are
	// area, then region.  DIR < 0: it walks them backwards and fills both DOWNWARDS from the top, each flush below the one before, so
	// that what it leaves is still its records in frame order: region (ending at its top), then area (ending at its top).  The word
	// indices of a record are taken relative to the record and the wave-uniform first word of the record is added to them.
	struct Staging
	{
		static constexpr bool GUARDED_STEPS = true;
		uint64_t *lds; // this wave's region
		uint32_t cap;  // its capacity in words
		uint32_t fill; // words it holds now
		uint32_t need; // words of the spill area: the worst case of the wave's share of the chunk
		uint64_t *area; // the static area, or the arena
		uint64_t extent; // first word of the wave's part of `area`: 0 (static), its extent once granted, else ~0
		// dynamic spill extents
		unsigned long long *cursor; // words handed out so far; nullptr: static
		uint64_t arena_words;
		uint32_t *error_word;
		v4u32 *key_lds; // 64 x 16 bytes for the key frame of a wave that walks backwards

		// wave w's region of `cap` words, empty, and no spill area (the caller sets `area` and `extent` = 0, or the arena's fields)
		__device__ __forceinline__ Staging(uint64_t *lds_all, int w, int cap_, int nrec)
			: lds(lds_all + (size_t)w * cap_), cap((uint32_t)cap_), fill(0), need((uint32_t)(nrec > 0 ? nrec : 0) * RIRB1_REC_MAX_WORDS), area(nullptr),
			  extent(~0ull), cursor(nullptr), arena_words(0), error_word(nullptr), key_lds(nullptr)
		{
		}
		__device__ __forceinline__ void keep_key(const v4u32 &v, int lane) { key_lds[lane] = v; }
		__device__ __forceinline__ v4u32 kept_key(int lane) { return key_lds[lane]; }

		// pos: words the wave has produced so far; pos - fill of them have been flushed
		template <int DIR>
		__device__ __forceinline__ uint64_t emit(const Px8 &r, uint32_t mode, uint32_t base, uint32_t pos, const LaneConsts &lc, const TransposeConsts &tc,
												 uint32_t *words)
		{
			RecordWords rw;
			const uint64_t h = emit_words<1u, RIR_NONE>(r, mode, base, rw, 0u, lc, tc, words);
			if (fill + *words > cap)
			{ // rare: flush what the region holds, below (backwards) or above (forwards) what was flushed before
				const uint32_t flushed = pos - fill;
				if (cursor != nullptr && flushed == 0)
				{ // (what comes back from a call is in vector registers, "divergent" for the compiler; it is wave-uniform: say so)
					const uint64_t ext = staging_take_extent(cursor, need, arena_words, error_word);
					extent = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ext >> 32)) << 32) |
							 (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ext);
				}
				if (extent != ~0ull)
					staging_flush((global_words_ptr)(area + extent + (DIR > 0 ? flushed : need - flushed - fill)),
								  (lds_words_ptr)(DIR > 0 ? lds : lds + (cap - fill)), fill);
				fill = 0;
			}
			uint64_t *rec = DIR > 0 ? lds + fill : lds + (cap - fill - *words);
			if (rw.pa != RIR_NONE)
				rec[rw.pa] = ((uint64_t)rw.va.y << 32) | rw.va.x;
			if (rw.pb != RIR_NONE)
				rec[rw.pb] = ((uint64_t)rw.vb.y << 32) | rw.vb.x;
			fill += *words;
			return h;
		}
	};

	// ---- the frame walk -----------------------------------------------------------------------------------
	// One wave packs the records of a run of frames of a chunk for one tile: every encoder kernel calls it.  `nload` frames are LOADED,
	// from frame `frame_first` on: the key frame first when has_key, else the frame before the wave's first record.  hdr_first: table
	// entry of that first loaded frame (headers of records go to hdr_first[1..] / hdr_first[0] for the key frame).
	// DIR > 0: the wave walks its frames forwards.  DIR < 0: backwards - it loads its LAST frame first and its records come out
	// last to first, the key record at the very end.  A record is frame f minus frame f - 1 either way, so every header and payload
	// word is the same; only the order in which the wave produces them differs (and the staged sink files them in frame order).
	// The ring is indexed by the ORDER OF LOADING k (slot k % 4): step k packs what was loaded k-th against what was loaded (k-1)-th.
	// Returns the number of payload words produced.
	template <bool FAST, int DIR, class Sink>
	__device__ __forceinline__ uint32_t encode_run(const uint16_t *__restrict__ frames, int64_t npx, int nload, int64_t frame_first, bool has_key,
												   int tile, int lane, uint64_t *__restrict__ hdr_first, Sink &sink)
	{
		constexpr bool BACK = DIR < 0;
		const int64_t p0 = (int64_t)tile * RIRB1_TILE_PX + lane * 8;
		const TransposeConsts tc = make_transpose_consts(lane);
		const LaneConsts lc = make_lane_consts(lane);
		const uint32_t lane_off = (uint32_t)lane * 16u;
		// FAST: whole tile inside the frame and 16-byte aligned rows -> raw-buffer loads, unconditional.  They are compiler-visible
		// builtins: the waits are the compiler's own counted s_waitcnt, which stay exact because no vector-memory operation of the
		// frame loop sits inside a branch (the staged sink's flush is out of line, behind a call).  Frames are loaded strictly in order (of time, or against it: 0,1,2,3 up front, then the
		// (k+3)-th at step k), so the address is a running wave-uniform pointer (2 scalar adds per load instead of a 64-bit multiply
		// chain); a request past the wave's last frame is an out-of-range offset: the instruction is issued (the waits stay counted)
		// and touches no memory.
		const uint16_t *next_ptr = frames + (frame_first + (BACK ? nload - 1 : 0)) * npx + (int64_t)tile * RIRB1_TILE_PX;
		auto load = [&](int k, v4u32 &dst) { // the k-th load of the wave
			if (FAST)
			{
				const Px8 p = buf_load8(next_ptr, k < nload ? lane_off : RIR_OOB);
				dst.x = p.d[0], dst.y = p.d[1], dst.z = p.d[2], dst.w = p.d[3];
				next_ptr = BACK ? next_ptr - npx : next_ptr + npx;
			}
			else
			{
				const int i = min(k, nload - 1);
				const Px8 p = load8(frames, frame_first + (BACK ? nload - 1 - i : i), npx, p0, false);
				dst.x = p.d[0], dst.y = p.d[1], dst.z = p.d[2], dst.w = p.d[3];
			}
		};
		auto as_px8 = [](const v4u32 &v) {
			Px8 p;
			p.d[0] = v.x, p.d[1] = v.y, p.d[2] = v.z, p.d[3] = v.w;
			return p;
		};
		uint32_t pos = 0;
		uint64_t hdr_reg = 0; // lane (k - 1) & 63 keeps the header of step k until the 64-step flush
		// key frame: RAW, or LEFT when its payload is strictly smaller
		auto key_record = [&](const Px8 &cur) {
			const uint32_t base_raw = tile_base(cur, false);
			const uint32_t b2 = base_raw | (base_raw << 16);
			Px8 r_raw;
#pragma unroll
			for (int k = 0; k < 4; ++k)
				r_raw.d[k] = pk_sub16(cur.d[k], b2);
			const Px8 dl = left_delta(cur, lane);
			const uint32_t base_left = tile_base(dl, true);
			const uint32_t bl2 = base_left | (base_left << 16);
			Px8 r_left;
#pragma unroll
			for (int k = 0; k < 4; ++k)
				r_left.d[k] = pk_sub16(dl.d[k], bl2);
			const bool use_left = payload_words(r_left) < payload_words(r_raw);
			Px8 r_sel;
#pragma unroll
			for (int k = 0; k < 4; ++k)
				r_sel.d[k] = use_left ? r_left.d[k] : r_raw.d[k];
			uint32_t words;
			const uint32_t key_mode = use_left ? RIRB1_MODE_LEFT : RIRB1_MODE_RAW;
			const uint64_t h = sink.template emit<DIR>(r_sel, key_mode, use_left ? base_left : base_raw, pos, lc, tc, &words);
			if (lane == 0)
				store_table_word<Sink::GUARDED_STEPS>(hdr_first, h);
			pos += words;
		};
		// Ring of 4 frame slots: what was loaded k-th lives in slot k % 4, three frames are in flight ahead of the one being packed.
		// The loop is unrolled by 4 so that slots are fixed registers (a register copy of a loaded value would force an early wait
		// on the load): every load must go into the registers of the frame it replaces.
		v4u32 s0, s1, s2, s3;
		// (in this order: a wait counts the loads issued AFTER the one it needs, and the scheduler is otherwise free to issue slot 1's
		// load last - then the wait at the loop's head is vmcnt(0) for good)
		load(0, s0);
		if (Sink::GUARDED_STEPS)
			__builtin_amdgcn_sched_barrier(0);
		load(1, s1);
		if (Sink::GUARDED_STEPS)
			__builtin_amdgcn_sched_barrier(0);
		load(2, s2);
		if (Sink::GUARDED_STEPS)
			__builtin_amdgcn_sched_barrier(0);
		load(3, s3);
		if (Sink::GUARDED_STEPS)
			__builtin_amdgcn_sched_barrier(0);
		if (!BACK && has_key)
			key_record(as_px8(s0));
		// step K: NEW was loaded K-th, OLD (K-1)-th; forwards NEW is the record's frame and OLD the one before it, backwards OLD is
		// the record's frame and NEW the one before it.  OLD's slot is free afterwards: the (K+3)-th load goes there.  The load is
		// issued whatever LIVE says; the record's work - which holds no vector-memory operation for a sink without stores of its own -
		// only when LIVE (wave-uniform).  The empty asm is no instruction: it keeps the difference in front of the load.  Without it
		// the compiler sinks the difference into the LIVE branch, behind the load, which then cannot reuse OLD's registers: the slots
		// wander through eight register quads, come back with copies (and a drain) at the loop's edge, and 64 registers no longer do.  Backwards the key frame is the NEW of the last live step: the sink keeps it (in LDS: four
		// more registers across the loop do not fit 64), because the loads of the steps that are not live go on overwriting the slots.
#define RIR_ENC_STEP(K, NEW, OLD, LIVE)                                                       \
	{                                                                                          \
		const int k_ = (K);                                                                    \
		Px8 d;                                                                                 \
		{                                                                                      \
			const Px8 c_ = as_px8(BACK ? OLD : NEW), p_ = as_px8(BACK ? NEW : OLD);            \
			_Pragma("unroll") for (int k = 0; k < 4; ++k) d.d[k] = pk_sub16(c_.d[k], p_.d[k]); \
		}                                                                                      \
		if (Sink::GUARDED_STEPS)                                                               \
			asm volatile("" : "+v"(d.d[0]), "+v"(d.d[1]), "+v"(d.d[2]), "+v"(d.d[3]));        \
		load(k_ + 3, OLD);                                                                     \
		if (LIVE)                                                                              \
		{                                                                                      \
			if (BACK && Sink::GUARDED_STEPS && has_key && k_ == nload - 1)                     \
				sink.keep_key(NEW, lane);                                                      \
			const uint32_t base = tile_base(d, true);                                          \
			const uint32_t b2 = base | (base << 16);                                           \
			_Pragma("unroll") for (int k = 0; k < 4; ++k) d.d[k] = pk_sub16(d.d[k], b2);      \
			uint32_t words;                                                                    \
			const uint64_t h = sink.template emit<DIR>(d, RIRB1_MODE_TEMPORAL, base, pos, lc, tc, &words); \
			if (lane == ((k_ - 1) & 63))                                                       \
				hdr_reg = h;                                                                   \
			pos += words;                                                                      \
		}                                                                                      \
	}
		// Steps come in groups of 64 (one header per lane of hdr_reg, flushed with one coalesced store per group).  What lets the
		// compiler keep counted waits - the loads of the next frames in flight across the packing of the current one - is that no
		// vector-memory operation of the loop sits under a condition.
		int fb = 1;
		while (fb < nload)
		{
			const int g0 = fb, gend = min(fb + 64, nload); // this group: steps [g0, gend), header of step k in lane k - g0
			if (Sink::GUARDED_STEPS)
			{
				// A sink without stores: ONE loop whose steps past the group's end only issue their (out-of-range) loads.  There is no
				// remainder code, so every wait before the use of a frame - the loop's head included - allows the two younger loads, and
				// the ring is never drained.  64 % 4 == 0: the slot rotation stays aligned.
				for (; fb < gend; fb += 4)
				{
					RIR_ENC_STEP(fb, s1, s0, true)
					RIR_ENC_STEP(fb + 1, s2, s1, fb + 1 < gend)
					RIR_ENC_STEP(fb + 2, s3, s2, fb + 2 < gend)
					RIR_ENC_STEP(fb + 3, s0, s3, fb + 3 < gend)
				}
			}
			else
			{
				// A sink with two stores per record: they stay unconditional in whole iterations of 4 steps, and up to three left-over
				// steps follow the run's last group (64 % 4 == 0: the slot rotation stays aligned)
				for (; fb + 3 < gend; fb += 4)
				{
					RIR_ENC_STEP(fb, s1, s0, true)
					RIR_ENC_STEP(fb + 1, s2, s1, true)
					RIR_ENC_STEP(fb + 2, s3, s2, true)
					RIR_ENC_STEP(fb + 3, s0, s3, true)
				}
				if (fb < gend)
				{
					RIR_ENC_STEP(fb, s1, s0, true)
					if (fb + 1 < gend)
					{
						RIR_ENC_STEP(fb + 1, s2, s1, true)
						if (fb + 2 < gend)
							RIR_ENC_STEP(fb + 2, s3, s2, true)
					}
				}
			}
			fb = gend;
			// lane l holds the header of step g0 + l: the record of frame g0 + l forwards, of frame nload - (g0 + l) backwards
			if (g0 + lane < gend)
				store_table_word<Sink::GUARDED_STEPS>(hdr_first + (BACK ? nload - (g0 + lane) : g0 + lane), hdr_reg);
			hdr_reg = 0;
		}
#undef RIR_ENC_STEP
		if (BACK && has_key)
		{ // the key frame was loaded last, (nload - 1)-th: the run's only frame, or what the last step gave the sink to keep
			key_record(as_px8(nload > 1 ? sink.kept_key(lane) : s0));
		}
		return pos;
	}

	// ---- encode -----------------------------------------------------------------------------
	//
	// grid  = (ceil(tile_count/4), nchunks), block = 256 (4 independent waves); tiles [tile_first, tile_first + tile_count)
	// hdr       [nchunks][ntiles][gop]      u64  record headers
	// seg_words [nchunks][ntiles]           u32  segment length (sum over the chunk's frames)
	// sparse    [nchunks][ntiles][gop*128]  u64, only the first seg_words words of a slot are written
	// One wave = one tile over all the frames of one chunk: the walk with the key frame, forwards, into the segment's slot.
	// Two kernels: FAST for tiles that lie whole inside 16-byte aligned frames (every tile but the last one of a frame whose
	// size is not a multiple of 512 pixels) - unconditional raw-buffer loads, 64 registers, no scratch - and the ragged form
	// (element-wise loads with bounds tests) for the rest; as one kernel the ragged instantiation's spills cost the fast path
	// its scratch set-up.
	// 8 waves per SIMD (<= 64 VGPRs; the allocator's natural choice was 71 -> 7 waves): 12 800 waves then take 1.56
	// rounds instead of 1.79 and the run-to-run spread of the kernel (141 / 154 us) collapses onto the fast mode
	template <bool FAST>
	__attribute__((amdgpu_waves_per_eu(8, 8))) __global__ __launch_bounds__(256) void rirb1_encode_tiles(const uint16_t *__restrict__ frames, int64_t npx, int ntiles,
																 int tile_first, int tile_count, int nframes, int gop,
																 uint64_t *__restrict__ hdr_table, uint32_t *__restrict__ seg_words,
																 uint64_t *__restrict__ sparse)
	{
		const int lane = threadIdx.x & 63;
		const int ti = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		if (ti >= tile_count)
			return;
		const int tile = tile_first + ti;
		const int chunk = blockIdx.y;
		const int f_begin = chunk * gop;
		const int nf = min(gop, nframes - f_begin);
		const int64_t slot = (int64_t)chunk * ntiles + tile;
		uint64_t *my_hdr = hdr_table + slot * gop;
		DirectSink sink{make_rsrc(sparse + slot * RIRB1_SLOT_WORDS(gop), (uint32_t)gop * RIRB1_REC_MAX_WORDS * 8u)};
		const uint32_t words = encode_run<FAST, 1>(frames, npx, nf, f_begin, true, tile, lane, my_hdr, sink);
		for (int f = nf + lane; f < gop; f += 64)
			my_hdr[f] = 0; // short last chunk: the unused table entries are defined
		if (lane == 0)
			seg_words[slot] = words;
	}

	// ---- offsets ------------------------------------------------------------------------------
	// grid = nchunks, block = 256.  tile_off[c][0..ntiles] = exclusive scan of seg_words[c][*],
	// chunk_words[c] = total.
	__global__ __launch_bounds__(256) void rirb1_scan_tiles(const uint32_t *__restrict__ seg_words, int ntiles,
														   uint32_t *__restrict__ tile_off, uint64_t *__restrict__ chunk_words)
	{
		__shared__ uint32_t wave_tot[4];
		__shared__ uint32_t carry_s;
		const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
		const uint32_t *in = seg_words + (int64_t)c * ntiles;
		uint32_t *off = tile_off + (int64_t)c * (ntiles + 1);
		if (tid == 0)
			carry_s = 0;
		__syncthreads();
		for (int base = 0; base < ntiles; base += 256)
		{
			const int i = base + tid;
			const uint32_t v = i < ntiles ? in[i] : 0u;
			const uint32_t inc = wave_scan_add(v, lane);
			if (lane == 63)
				wave_tot[wv] = inc;
			__syncthreads();
			uint32_t pre = carry_s;
			for (int k = 0; k < wv; ++k)
				pre += wave_tot[k];
			if (i < ntiles)
				off[i] = pre + inc - v;
			__syncthreads();
			if (tid == 255)
				carry_s = pre + inc;
			__syncthreads();
		}
		if (tid == 0)
		{
			off[ntiles] = carry_s;
			chunk_words[c] = carry_s;
		}
	}

	// grid = (ntiles, nchunks), block = 256: gathers the sparse slots into the dense stream and
	// publishes chunk_off[c] (first word of chunk c in the stream; chunk_off[nchunks] = total).
	__global__ __launch_bounds__(256) void rirb1_compact(const uint64_t *__restrict__ sparse, const uint32_t *__restrict__ tile_off,
														const uint64_t *__restrict__ chunk_words, int ntiles, int nchunks, int gop,
														uint64_t *__restrict__ chunk_off, uint64_t *__restrict__ stream)
	{
		const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
		// every wave derives the chunk's base itself (sum of the preceding chunks' lengths): no LDS, no barrier,
		// and the loads of the table entries are in flight while the reduction runs
		const uint32_t *off = tile_off + (int64_t)c * (ntiles + 1);
		const uint32_t o0 = off[t], o1 = off[t + 1];
		uint64_t s = 0;
		for (int i = tid & 63; i < c; i += 64)
			s += chunk_words[i];
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1)
			s += (uint64_t)__shfl_xor((long long)s, d, 64);
		if (t == 0 && tid == 0)
		{
			chunk_off[c] = s;
			if (c == nchunks - 1)
				chunk_off[nchunks] = s + chunk_words[c];
		}
		const uint32_t n = o1 - o0;
		const uint64_t *src = sparse + ((int64_t)c * ntiles + t) * RIRB1_SLOT_WORDS(gop);
		uint64_t *dst = stream + s + o0;
		uint32_t i = tid;
		for (; i + 768 < n; i += 1024)
		{ // four independent 8-byte copies per thread and iteration
			const uint64_t v0 = __builtin_nontemporal_load(src + i);
			const uint64_t v1 = __builtin_nontemporal_load(src + i + 256);
			const uint64_t v2 = __builtin_nontemporal_load(src + i + 512);
			const uint64_t v3 = __builtin_nontemporal_load(src + i + 768);
			dst[i] = v0, dst[i + 256] = v1, dst[i + 512] = v2, dst[i + 768] = v3;
		}
		for (; i < n; i += 256)
			dst[i] = __builtin_nontemporal_load(src + i);
	}

	// ==== single-pass dense encoder ===================================================================
	//
	// One WORKGROUP owns one (chunk, tile) segment; its WAVES waves split the chunk's frames in time (wave 0 takes the
	// key frame, a later wave loads the frame before its first one as its starting `prev`).  The payload words of the
	// segment are staged in LDS (R words per wave; what does not fit goes to a spill slot in the workspace - noisy data
	// degrades to the traffic of a two-pass layout, the reference's recipe never spills).  When a workgroup has packed
	// its frames it knows the length of its segment, publishes it, and looks back for the lengths of the segments in
	// front of it (decoupled look-back): the sum is its place in the dense stream, to which it copies its words from LDS.
	// The stream, tile_off and chunk_off are bit-identical to the two-pass layout (scan + gather) this replaces.
	//
	// Look-back state (control block in the workspace, zeroed by a memset node before every launch):
	//   gran   [chunk][tile]    u64  TAG | segment length                        published by the segment's workgroup
	//   gtotal [chunk][tile/64] u64  TAG | sum of the lengths of a group of 64   published by the group's last arriver
	//   P      [chunk]          u64  TAG | first word of the chunk in the stream published by the previous chunk's last arriver
	//   gcount [chunk][tile/64], ccount [chunk]  u64  arrivals << 40 | sum: returning agent-scope atomic adds that find the
	//          last arriver of a group / of a chunk; on lines of their own, never polled
	// Every POLLED word is written once, by one sc1 store, and carries its own data (granule = flag).  What is polled is
	// never what is added to (counters that 64 workgroups add to while hundreds poll them serialise on their cache line:
	// 60 ns per add, 770 us per launch), and no published word depends on another one except P[c + 1] on P[c] (prefixes
	// chained through the groups cost 200 hops of 2.5 us).
	// Workgroup (c, t) needs  A = sum of lengths of tiles < t in chunk c  (= its tile_off) and P[c]: it polls the granules of
	// the tiles in front of it in its own group of 64, the totals of the groups in front and P[c] - 63 + ntiles / 64 + 1
	// words at most, by ONE wave, with relaxed agent-scope loads (sc1: served by L2 / memory, never a stale L1 line).  No
	// payload is handed between workgroups inside the launch (the stream is read by the NEXT kernel).
	// Forward progress: segments are dealt by tickets (8 heads, head = blockIdx % 8, segment = ticket * 8 + head), so a
	// workgroup only ever waits for segments whose workgroups have taken their ticket earlier on the same head or are
	// not behind it in dispatch; every spin is bounded by a 2 s clock and a shared error word, a wait that gives up
	// raises the error instead of hanging.
#define RIR_LB_TAG (1ull << 63)
#define RIR_LB_TIMEOUT_TICKS 200000000ull /* s_memrealtime runs at 100 MHz: 2 s */
	constexpr int LB_SLEEP = 8; // s_sleep between two polls of a look-back

	__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
	{
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1)
			v += (uint64_t)__shfl_xor((long long)v, d, 64);
		return v;
	}

	// Look-back of workgroup (c, t), run by ONE wave.  A = sum of the lengths of tiles < t of chunk c, Pc = first word of
	// chunk c.  false: gave up (clock or error word); the error word is raised.
	__device__ __noinline__ bool encode_lookback(const uint64_t *P, const uint64_t *gtotal, const uint64_t *gran, uint32_t *error_word, int c, int t,
												 int ntiles, int ngroups, int lane, uint64_t *A_out, uint64_t *P_out)
	{
		const int g = t >> 6, e1 = t & 63, E = e1 + g + (c > 0 ? 1 : 0);
		uint64_t accA = 0, accP = 0;
		const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
		for (int e0 = 0; e0 < E; e0 += 64)
		{
			const int e = e0 + lane;
			const bool valid = e < E;
			int kind = 2;
			const uint64_t *ptr = P + c;
			if (e < e1)
				kind = 0, ptr = gran + (int64_t)c * ntiles + ((int64_t)g << 6) + e;
			else if (e < e1 + g)
				kind = 1, ptr = gtotal + (int64_t)c * ngroups + (e - e1);
			uint64_t v = 0;
			bool done = !valid;
			for (uint32_t spins = 0;; ++spins)
			{
				if (!done)
				{
					v = __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					done = (v >> 63) != 0;
				}
				if (__ballot(!done) == 0)
					break;
				if ((spins & 15u) == 15u)
				{
					const uint32_t err = __hip_atomic_load(error_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (err != 0 || __builtin_amdgcn_s_memrealtime() - t_start > RIR_LB_TIMEOUT_TICKS)
					{
						if (lane == 0)
							__hip_atomic_store(error_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						return false;
					}
				}
				__builtin_amdgcn_s_sleep(LB_SLEEP);
			}
			if (valid)
			{
				if (kind == 2)
					accP = v & ~RIR_LB_TAG;
				else
					accA += v & ~RIR_LB_TAG;
			}
		}
		*A_out = wave_sum_u64(accA);
		*P_out = wave_sum_u64(accP);
		return true;
	}

	// frames of wave w when nf frames are split over `waves` waves with the key frame counted twice: [enc_split(w), enc_split(w + 1))
	__device__ __host__ __forceinline__ int enc_split(int w, int waves, int nf)
	{
		if (w <= 0)
			return 0;
		if (w >= waves)
			return nf;
		const int b = (w * (nf + 1) + waves / 2) / waves - 1;
		return b < 1 ? (nf < 1 ? nf : 1) : (b > nf ? nf : b);
	}

	// The packed encoder's waves walk in mirrored pairs: an even wave walks its share backwards, the odd wave after it forwards, so both
	// start on the frame where their shares meet and ask for it at the same moment, from the same CU - the frame crosses the fabric once.
	__device__ __host__ __forceinline__ bool enc_walks_back(int w) { return (w & 1) == 0; }
	// Its cuts: enc_split's, but with four waves the third cut gives waves 1 and 2 the same number of records.  They meet at the middle
	// boundary from both sides at the END of their walks, and reach it in step only when they have equally far to go.
	__device__ __host__ __forceinline__ int enc_split_mirrored(int w, int waves, int nf)
	{
		if (waves == 4 && w == 3)
		{
			const int c = 2 * enc_split(2, waves, nf) - enc_split(1, waves, nf);
			return c > nf ? nf : c;
		}
		return enc_split(w, waves, nf);
	}

	// control block: 8 ticket heads on lines of their own, the error word, then P / group / gran
	__device__ __host__ __forceinline__ int64_t enc_ctrl_words64(int nchunks, int ntiles)
	{
		const int64_t ngroups = (ntiles + 63) / 64;
		return 8 * 16 + 16 + ((int64_t)nchunks + 1) + (int64_t)nchunks * ngroups + (((int64_t)nchunks * ntiles + 15) & ~(int64_t)15) +
			   (int64_t)nchunks * ngroups + nchunks + 16;
	}

	// ---- what the two staged encoders share ---------------------------------------------------------------------
	// Wave w's share of a chunk of nf frames under the cuts CUT (enc_split or enc_split_mirrored): records [rec0, rec0 + nrec).  It loads
	// nload frames from frame first_load of the chunk on: the key frame first (wave 0), else the frame before its first record.
	struct WaveShare
	{
		int rec0, nrec, first_load, nload;
		bool has_key;
	};
	template <int (*CUT)(int, int, int)>
	__device__ __forceinline__ WaveShare wave_share(int w, int waves, int nf)
	{
		WaveShare s;
		const int rec1 = CUT(w + 1, waves, nf);
		s.rec0 = CUT(w, waves, nf);
		s.nrec = rec1 - s.rec0;
		s.has_key = w == 0;
		s.first_load = s.has_key ? 0 : s.rec0 - 1;
		s.nload = s.nrec > 0 ? rec1 - s.first_load : 0;
		return s;
	}

	// The end of a wave's walk, before the barrier: the workgroup defines the table entries a short last chunk leaves unused, the wave
	// publishes its words and how many of them are in LDS, and what it flushed has left it before another wave reads it.
	template <int WAVES>
	__device__ __forceinline__ void staged_publish(uint64_t *__restrict__ my_hdr, int nf, int gop, const Staging &sg, uint32_t pos, int w, int lane,
												   uint32_t *sh_words, uint32_t *sh_lds_words)
	{
		for (int f = nf + (int)threadIdx.x; f < gop; f += WAVES * 64)
			store_table_word<true>(my_hdr + f, (uint64_t)0);
		if (lane == 0)
		{
			sh_words[w] = pos;
			sh_lds_words[w] = sg.fill;
		}
		if (sg.fill != pos)
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	}

	// Copies one wave's n_all words to dst in frame order: n_lds of them are in its LDS region (`cap` words), the rest - the records it
	// produced first - in its spill area, which spill_area(need) describes (its size in words goes to `need`) and which is asked for
	// only when there is a rest.  A forward wave's words: its area from word 0, then its region from word 0.  A backward wave's: its
	// region (the EARLIER records, which it packed last) up to the region's end, then its area up to the area's end.
	// AUX: the policy of its stores (0: plain pointer stores, else buffer stores with that aux operand).
	template <int AUX, class SpillArea>
	__device__ __forceinline__ void copy_wave_words(uint64_t *__restrict__ dst, const uint64_t *region, uint32_t cap, uint32_t n_all, uint32_t n_lds, bool back,
													int lane, SpillArea spill_area)
	{
		const uint32_t n_ext = n_all - n_lds;
		const uint64_t *src = region + (back ? cap - n_lds : 0u);
		uint64_t *dst_lds = dst + (back ? 0u : n_ext);
		const __amdgpu_buffer_rsrc_t out = make_rsrc(dst, n_all * 8u); // (AUX != 0)
		auto put = [&](uint64_t *base, uint32_t j, uint64_t v) {
			if (AUX == 0)
				base[j] = v;
			else
				__builtin_amdgcn_raw_buffer_store_b64(v2u32{(uint32_t)v, (uint32_t)(v >> 32)}, out, (uint32_t)(base - dst + j) * 8u, 0, AUX);
		};
		uint32_t j = (uint32_t)lane;
		for (; j + 192 < n_lds; j += 256)
		{
			const uint64_t v0 = src[j], v1 = src[j + 64], v2 = src[j + 128], v3 = src[j + 192];
			put(dst_lds, j, v0), put(dst_lds, j + 64, v1), put(dst_lds, j + 128, v2), put(dst_lds, j + 192, v3);
		}
		for (; j < n_lds; j += 64)
			put(dst_lds, j, src[j]);
		if (n_ext > 0)
		{ // what the wave flushed comes back from the workspace (sc1 loads: from L2, where its stores went)
			uint32_t need;
			const __amdgpu_buffer_rsrc_t sp = spill_area(need);
			const uint32_t first = back ? need - n_ext : 0u;
			uint64_t *dst_ext = dst + (back ? n_lds : 0u);
			for (uint32_t q = (uint32_t)lane; q < n_ext; q += 64)
			{
				const v2u32 v = __builtin_amdgcn_raw_buffer_load_b64(sp, (first + q) * 8u, 0, 16 /* sc1 */);
				put(dst_ext, q, ((uint64_t)v.y << 32) | v.x);
			}
		}
	}

	// The copy-out of a segment no wave of which spilled: words [0, total) of the segment lie in the WAVES regions of `lds` (`cap` words
	// each) - wave i's n[i] words at the bottom of its region, or at its top when back(i) - and go to dst as ONE run, cut by the 128-byte
	// lines of memory instead of by the waves: the words in front of the first line boundary and those behind the last whole line as
	// 8-byte stores (one instruction for both ends), the lines between as 16 bytes per lane, so that every body instruction writes eight
	// whole lines and no line is written by two instructions.  That is what a write-through policy needs (AUX 16 / 18): a line two
	// instructions write goes to the fabric twice, and neighbouring segments share lines only at their ends.  A lane's two words may lie
	// in two waves' regions: a word of the segment is found from the running sums of n.  LDS is read 8 bytes at a time.
	template <int WAVES, int AUX, class Back>
	__device__ __forceinline__ void copy_segment_lines(uint64_t *__restrict__ dst, const uint64_t *lds, uint32_t cap, const uint32_t *n, uint32_t total, int lane,
													   Back back)
	{
		uint32_t end[WAVES], delta[WAVES]; // word q < end[i] (and >= end[i - 1]) of the segment is lds[q + delta[i]]
		uint32_t sum = 0;
#pragma unroll
		for (int i = 0; i < WAVES; ++i)
		{
			delta[i] = (uint32_t)i * cap + (back(i) ? cap - n[i] : 0u) - sum;
			sum += n[i];
			end[i] = sum;
		}
		// (as a telescoping sum, not as a chain of selects between elements of delta: the compiler turns such a chain into a select
		// between their addresses, and the array into scratch)
		auto word = [&](uint32_t q) {
			uint32_t d = delta[WAVES - 1];
#pragma unroll
			for (int i = WAVES - 2; i >= 0; --i)
				d += q < end[i] ? delta[i] - delta[i + 1] : 0u;
			return lds[q + d];
		};
		const __amdgpu_buffer_rsrc_t out = make_rsrc(dst, total * 8u);
		const uint32_t to_line = (16u - (uint32_t)(((uintptr_t)dst >> 3) & 15u)) & 15u;
		const uint32_t head = min(to_line, total);			   // words in front of the first line boundary
		const uint32_t pairs = ((total - head) >> 4) << 3;	   // 16-byte pieces of the whole lines behind it
		const uint32_t tail0 = head + 2u * pairs, tail = total - tail0; // the rest: < 16 words
		{ // both ends: lanes [0, head) and [16, 16 + tail)
			const uint32_t l = (uint32_t)lane;
			const bool on = l < 16u ? l < head : l - 16u < tail;
			const uint32_t q = l < 16u ? l : tail0 + (l - 16u);
			const uint64_t v = on ? word(q) : 0ull;
			__builtin_amdgcn_raw_buffer_store_b64(v2u32{(uint32_t)v, (uint32_t)(v >> 32)}, out, on ? q * 8u : RIR_OOB, 0, AUX);
		}
		auto piece = [&](uint32_t j) { // (a piece past the end reads words 0 and 1 of a segment of at least 16, and is stored nowhere)
			const uint32_t q = j < pairs ? head + 2u * j : 0u;
			const uint64_t a = word(q), b = word(q + 1u);
			return v4u32{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
		};
		auto put = [&](uint32_t j, const v4u32 &v) {
			__builtin_amdgcn_raw_buffer_store_b128(v, out, j < pairs ? (head + 2u * j) * 8u : RIR_OOB, 0, AUX);
		};
		uint32_t j0 = 0; // (wave-uniform loops: 1 KiB, eight whole lines, per store instruction)
		for (; j0 + 256 <= pairs; j0 += 256)
		{
			const uint32_t j = j0 + (uint32_t)lane;
			const v4u32 v0 = piece(j), v1 = piece(j + 64), v2 = piece(j + 128), v3 = piece(j + 192);
			put(j, v0), put(j + 64, v1), put(j + 128, v2), put(j + 192, v3);
		}
		for (; j0 < pairs; j0 += 64)
			put(j0 + (uint32_t)lane, piece(j0 + (uint32_t)lane));
	}

	template <int WAVES>
	__attribute__((amdgpu_waves_per_eu(8, 8))) __global__ __launch_bounds__(WAVES * 64) void rirb1_encode_dense(
		const uint16_t *__restrict__ frames, int64_t npx, int ntiles, int nframes, int gop, int nchunks, uint64_t *__restrict__ hdr_table,
		uint32_t *__restrict__ tile_off, uint64_t *__restrict__ chunk_off, uint64_t *__restrict__ stream, uint64_t *__restrict__ ctrl,
		uint64_t *__restrict__ spill, int cap)
	{
		extern __shared__ __attribute__((aligned(16))) uint64_t enc_lds[];
		uint64_t *sh_base = enc_lds + (size_t)WAVES * cap;				   // [0] segment's first word in the stream
		uint32_t *sh_u32 = reinterpret_cast<uint32_t *>(sh_base + 1); // [0..WAVES) words of each wave, [WAVES] segment index, [WAVES + 2..] words of each wave in LDS
		const int lane = threadIdx.x & 63;
		const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		const int ngroups = (ntiles + 63) >> 6;
		uint32_t *heads = reinterpret_cast<uint32_t *>(ctrl);
		uint32_t *error_word = reinterpret_cast<uint32_t *>(ctrl + 8 * 16);
		uint64_t *P = ctrl + 8 * 16 + 16;
		uint64_t *gtotal = P + nchunks + 1;
		uint64_t *gran = gtotal + (int64_t)nchunks * ngroups;
		uint64_t *gcount = gran + (((int64_t)nchunks * ntiles + 15) & ~(int64_t)15); // counters: on lines of their own
		uint64_t *ccount = gcount + (int64_t)nchunks * ngroups;

		if (threadIdx.x == 0)
		{
			const uint32_t head = blockIdx.x & 7u;
			const uint32_t ticket = __hip_atomic_fetch_add(heads + head * 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			sh_u32[WAVES] = ticket * 8u + head;
		}
		__syncthreads();
		const int seg = __builtin_amdgcn_readfirstlane((int)sh_u32[WAVES]);
		const int chunk = seg / ntiles, tile = seg - chunk * ntiles;
		const int f_begin = chunk * gop;
		const int nf = min(gop, nframes - f_begin);
		uint64_t *my_hdr = hdr_table + (int64_t)seg * gop;

		// a wave's spill area: its share of the segment's worst-case slot
		auto spill_area = [&](const WaveShare &s, uint32_t &need) {
			need = (uint32_t)s.nrec * RIRB1_REC_MAX_WORDS;
			return make_rsrc(spill + (int64_t)seg * RIRB1_SLOT_WORDS(gop) + (int64_t)s.rec0 * RIRB1_REC_MAX_WORDS, need * 8u);
		};
		const WaveShare sh = wave_share<enc_split>(w, WAVES, nf);
		Staging sg(enc_lds, w, cap, sh.nrec);
		sg.area = spill + (int64_t)seg * RIRB1_SLOT_WORDS(gop) + (int64_t)sh.rec0 * RIRB1_REC_MAX_WORDS, sg.extent = 0; // (spill_area's words)
		uint32_t pos = 0;
		if (sh.nrec > 0)
		{
			const bool fast = ((npx & 7) == 0) && ((int64_t)(tile + 1) * RIRB1_TILE_PX <= npx) && ((((uintptr_t)frames) & 15) == 0);
			if (fast)
				pos = encode_run<true, 1>(frames, npx, sh.nload, (int64_t)f_begin + sh.first_load, sh.has_key, tile, lane, my_hdr + sh.first_load, sg);
			else
				pos = encode_run<false, 1>(frames, npx, sh.nload, (int64_t)f_begin + sh.first_load, sh.has_key, tile, lane, my_hdr + sh.first_load, sg);
		}
		staged_publish<WAVES>(my_hdr, nf, gop, sg, pos, w, lane, sh_u32, sh_u32 + WAVES + 2);
		__syncthreads();
		// Only wave 0 goes on: the segment is complete in LDS (+ spill), what is left is to wait for its place in the stream and
		// to copy it there.  The other waves END here - a workgroup that waits holds one wave slot, not four, so the CU can
		// start the next workgroup's waves while this one looks back.
		if (w != 0)
			return;
		uint32_t total = 0;
#pragma unroll
		for (int i = 0; i < WAVES; ++i)
			total += sh_u32[i];
		bool chunk_last = false; // this workgroup completed its chunk (lane 0 knows)
		uint64_t chunk_words = 0;
		if (lane == 0)
		{ // publish first, then look back
			__hip_atomic_store(gran + (int64_t)chunk * ntiles + tile, RIR_LB_TAG | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			const int g = tile >> 6, gsize = min(64, ntiles - (g << 6));
			const uint64_t one = 1ull << 40, sum_mask = one - 1ull;
			const uint64_t og = __hip_atomic_fetch_add(gcount + (int64_t)chunk * ngroups + g, one | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if ((int)(og >> 40) == gsize - 1)
			{ // last arriver of its group: the group's total becomes visible; it may complete the chunk too
				const uint64_t gsum = (og & sum_mask) + total;
				__hip_atomic_store(gtotal + (int64_t)chunk * ngroups + g, RIR_LB_TAG | gsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				const uint64_t oc = __hip_atomic_fetch_add(ccount + chunk, one | gsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if ((int)(oc >> 40) == ngroups - 1)
					chunk_last = true, chunk_words = (oc & sum_mask) + gsum;
			}
		}
		uint64_t A = 0, Pc = 0;
		const bool ok = encode_lookback(P, gtotal, gran, error_word, chunk, tile, ntiles, ngroups, lane, &A, &Pc);
		if (!ok)
			return; // the look-back gave up: the error word is raised, nothing is copied
		if (lane == 0)
		{
			tile_off[(int64_t)chunk * (ntiles + 1) + tile] = (uint32_t)A;
			if (seg == 0)
				chunk_off[0] = 0;
			if (chunk_last)
			{ // the chunk's length is known and so is its first word: the next chunk's first word follows
				tile_off[(int64_t)chunk * (ntiles + 1) + ntiles] = (uint32_t)chunk_words;
				__hip_atomic_store(P + chunk + 1, RIR_LB_TAG | (Pc + chunk_words), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				chunk_off[chunk + 1] = Pc + chunk_words;
			}
		}
		uint64_t *dst = stream + (Pc + A);
		for (int i = 0; i < WAVES; ++i)
		{
			const uint32_t n_all = sh_u32[i];
			// (the ordered stream is not what the packed step reads: it keeps the per-wave copy and plain stores)
			copy_wave_words<0>(dst, enc_lds + (size_t)i * cap, (uint32_t)cap, n_all, sh_u32[WAVES + 2 + i], false, lane,
							[&](uint32_t &need) { return spill_area(wave_share<enc_split>(i, WAVES, nf), need); });
			dst += n_all;
		}
	}

	// ==== packed form: the dense stream without the order ===============================================
	//
	// What made the single-pass DENSE encoder slow was not the staging but the ORDER: a segment's place is the sum of all
	// lengths in front of it, so every workgroup waits for the slowest of its predecessors.  The
	// reference's own ZFile container does not order its records by anything either: it keeps a table of positions
	// (ZFile.cpp:434-447).  The PACKED form does the same on the device: a segment is packed into LDS exactly as above, and
	// when its length is known ONE returning atomic add on a cursor hands it the next free words of the stream - first come,
	// first placed, nobody waits for anybody.  The batch is
	//   hdr       [nchunks][ntiles][gop]  u64   record headers (as everywhere)
	//   seg_pos   [nchunks][ntiles]       u64   first word of the segment in `stream`
	//   seg_words [nchunks][ntiles]       u32   its length
	//   stream    cursor words, no holes: the segments in order of arrival
	// i.e. exactly C bytes of payload plus tables - what can be kept, sent or written - from ONE pass over the frames.  The
	// layout differs from run to run (arrival order); every segment's words are the oracle's.
	// ONE cursor is not enough: 12 800 returning atomic adds on one address take 16 ns each at the memory side - 205 us, longer
	// than the kernel (measured: 207 us with one cursor, 162-165 with two or more or with none).  So there are TWO, and so that
	// they share the caller's capacity instead of halving it they work from its two ends: segments with an even (tile + chunk)
	// are placed upwards from word 0, the others downwards from word `capacity`.  The batch is two extents without holes,
	// [0, low) and [capacity - high, capacity); it fits when low + high <= capacity.
	// ctrl (a line each): [0] low cursor, [16] high cursor, [32] spill cursor, [48] error word (u32): bit 1 = the spill arena was
	// exceeded; [64..68] the status line; [80] the meeting word (u32).
	// The launch leaves its control block as it found it - zero - so the next launch needs no fill before it: a stream cursor counts
	// its segments in its top bits (each add is `words | 1 << 40`), and the workgroup that brings a cursor's count to the number of
	// segments on that side knows it is the last there (no ticket of its own: 12 800 more returning atomics on few addresses would
	// cost what the second cursor saved).  The last of each side meets the other at [80]; the second to arrive swaps every word of the
	// block with 0 and writes what it took to the status line: [64] low, [65] high, [66] spill words asked for, [67] error word, [68]
	// the capacity the launch was given (rir_codec_encode_packed_status: a segment did not fit its side, or the extents cross, when
	// low + high > capacity).  Each workgroup's spill atomics are complete before its cursor add (returning, or waited for), so the
	// swaps see every one.
#define RIR_PACKED_COUNT_SHIFT 40
#define RIR_PACKED_WORDS_MASK ((1ull << RIR_PACKED_COUNT_SHIFT) - 1)
	// the last workgroup of one side (wave-uniform call): meet the other side's last, and the second of the two empties the block
	__device__ __noinline__ void packed_finish(uint64_t *ctrl, uint64_t capacity_words, uint32_t sides)
	{
		if ((threadIdx.x & 63u) != 0)
			return;
		uint32_t *meet = reinterpret_cast<uint32_t *>(ctrl + 80);
		if (sides > 1 && __hip_atomic_fetch_add(meet, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 < sides)
			return;
		unsigned long long *c = reinterpret_cast<unsigned long long *>(ctrl);
		const uint64_t low = __hip_atomic_exchange(c, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & RIR_PACKED_WORDS_MASK;
		const uint64_t high = __hip_atomic_exchange(c + 16, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & RIR_PACKED_WORDS_MASK;
		const uint64_t spill = __hip_atomic_exchange(c + 32, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const uint32_t err = __hip_atomic_exchange(reinterpret_cast<uint32_t *>(ctrl + 48), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_store(meet, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		ctrl[64] = low, ctrl[65] = high, ctrl[66] = spill, ctrl[67] = err, ctrl[68] = capacity_words;
	}
	// Two kernels, as for rirb1_encode_tiles: FAST for the tiles that lie whole inside 16-byte aligned frames, the ragged form for
	// the last tile of a frame whose size is not a multiple of 512 pixels.  grid = (tile_count, nchunks).
	template <int WAVES, bool FAST>
	__attribute__((amdgpu_waves_per_eu(8, 8))) __global__ __launch_bounds__(WAVES * 64) void rirb1_encode_packed(
		const uint16_t *__restrict__ frames, int64_t npx, int ntiles, int tile_first, int nframes, int gop, uint64_t *__restrict__ hdr_table,
		uint64_t *__restrict__ seg_pos, uint32_t *__restrict__ seg_words, uint64_t *__restrict__ stream, uint64_t capacity_words,
		uint64_t *__restrict__ ctrl, uint64_t *__restrict__ arena, uint64_t arena_words, int cap)
	{
		extern __shared__ __attribute__((aligned(16))) uint64_t enc_lds[];
		v4u32 *key_lds = reinterpret_cast<v4u32 *>(enc_lds + (size_t)WAVES * cap); // the key frame while wave 0 walks back to it (1 KiB)
		uint64_t *sh_u64 = enc_lds + (size_t)WAVES * cap + 128;	  // [0] segment's first word in the stream, [1 + w] wave w's spill extent
		uint32_t *sh_u32 = reinterpret_cast<uint32_t *>(sh_u64 + 1 + WAVES); // [0..WAVES) words of each wave, [WAVES..2 WAVES) of them in LDS
		const int lane = threadIdx.x & 63;
		const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		const int chunk = blockIdx.y, tile = tile_first + blockIdx.x;
		const bool downwards = ((tile + chunk) & 1) != 0;
		unsigned long long *cursor = reinterpret_cast<unsigned long long *>(ctrl) + (downwards ? 16 : 0);
		unsigned long long *spill_cursor = reinterpret_cast<unsigned long long *>(ctrl + 32);
		uint32_t *error_word = reinterpret_cast<uint32_t *>(ctrl + 48);

		const int64_t seg = (int64_t)chunk * ntiles + tile;
		const int f_begin = chunk * gop;
		const int nf = min(gop, nframes - f_begin);
		uint64_t *my_hdr = hdr_table + seg * gop;

		const WaveShare sh = wave_share<enc_split_mirrored>(w, WAVES, nf);
		Staging sg(enc_lds, w, cap, sh.nrec);
		sg.key_lds = key_lds;
		sg.area = arena, sg.cursor = spill_cursor, sg.arena_words = arena_words, sg.error_word = error_word;
		uint32_t pos = 0;
		if (sh.nrec > 0)
		{
			if (enc_walks_back(w))
				pos = encode_run<FAST, -1>(frames, npx, sh.nload, (int64_t)f_begin + sh.first_load, sh.has_key, tile, lane, my_hdr + sh.first_load, sg);
			else
				pos = encode_run<FAST, 1>(frames, npx, sh.nload, (int64_t)f_begin + sh.first_load, sh.has_key, tile, lane, my_hdr + sh.first_load, sg);
		}
		if (lane == 0)
			sh_u64[1 + w] = sg.extent;
		staged_publish<WAVES>(my_hdr, nf, gop, sg, pos, w, lane, sh_u32, sh_u32 + WAVES);
		__syncthreads();
		// the segment is complete in LDS (+ extents): one wave places and copies it, the others make room (the alternative, every
		// wave copying its own words after one more barrier, is RIR_PACKED_COPY_ALL_WAVES in 02807a8)
		if (w != 0)
			return;
		uint32_t total = 0, n_wave[WAVES];
		bool lost = false;	  // a wave of this segment wanted an extent and got none
		bool spilled = false; // a wave of this segment has words outside LDS
#pragma unroll
		for (int i = 0; i < WAVES; ++i)
		{
			const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh_u32[i]);
			n_wave[i] = n;
			total += n;
			spilled |= n != sh_u32[WAVES + i];
			lost |= n > sh_u32[WAVES + i] && sh_u64[1 + i] == ~0ull;
		}
		unsigned long long at = 0;
		if (lane == 0)
			at = __hip_atomic_fetch_add(cursor, (unsigned long long)total | (1ull << RIR_PACKED_COUNT_SHIFT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)at);
		const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(at >> 32));
		// segments placed on this side before this one: the last of them all leaves the control block clean
		const uint32_t arrived = hi >> (RIR_PACKED_COUNT_SHIFT - 32);
		const uint64_t nseg = (uint64_t)gridDim.y * (uint32_t)ntiles; // (both launches: every segment of the batch)
		const uint64_t on_side = downwards ? nseg / 2 : (nseg + 1) / 2; // (tile + chunk) odd / even
		if ((uint64_t)arrived + 1 == on_side)
			packed_finish(ctrl, capacity_words, nseg < 2 ? 1u : 2u);
		at = ((unsigned long long)hi << 32 | lo) & RIR_PACKED_WORDS_MASK;
		const bool fits = at + total <= capacity_words; // (a segment that does not fit leaves its cursor beyond the capacity)
		if (downwards)
			at = capacity_words - at - total; // (unused when it does not fit)
		if (lane == 0)
		{
			store_table_word<true>(seg_pos + seg, (uint64_t)at);
			store_table_word<true>(seg_words + seg, total);
			sh_u64[0] = (fits && !lost) ? at : ~0ull;
		}
		if (!fits || lost)
			return;
		uint64_t *dst = stream + at;
		if (!spilled)
		{ // the common case (every segment of the reference's recipe): one copy of the whole segment, cut by the lines of memory
			copy_segment_lines<WAVES, PAYLOAD_STORE_AUX>(dst, enc_lds, (uint32_t)cap, n_wave, total, lane, [](int i) { return enc_walks_back(i); });
			return;
		}
		// a wave spilled: wave by wave, each from its region and its extent, under the same policy
		for (int i = 0; i < WAVES; ++i)
		{
			const uint32_t n_all = sh_u32[i]; // (not n_wave[i]: a register array indexed by a loop that is not unrolled is scratch)
			copy_wave_words<PAYLOAD_STORE_AUX>(dst, enc_lds + (size_t)i * cap, (uint32_t)cap, n_all, sh_u32[WAVES + i], enc_walks_back(i), lane, [&](uint32_t &need) {
				need = (uint32_t)wave_share<enc_split_mirrored>(i, WAVES, nf).nrec * RIRB1_REC_MAX_WORDS;
				return make_rsrc(arena + sh_u64[1 + i], need * 8u); // its extent
			});
			dst += n_all;
		}
	}

	// ---- decode -----------------------------------------------------------------------------
	// One record in flight: header + the two plane words of this lane.
	struct Fetched
	{
		uint64_t hdr;
		v2u32 a, b; // wide tier: the two plane words of this lane; narrow tier: a = plane word (lanes 0..31)
		uint32_t words;
		bool bad;
		bool narrow; // every width <= 4 (wave-uniform)
	};

	// true when every 5-bit width field of the header is <= 4 (scalar-unit arithmetic on the uniform header)
	__device__ __forceinline__ bool header_is_narrow(uint64_t hdr)
	{
		const uint64_t m0 = 0x0021002100210021ull; // bit 0 of w_q and of w_{4+q} in each 16-bit field
		const uint64_t hi = hdr & (m0 * 0x18u);	   // bits 3,4 of any width
		const uint64_t b2 = (hdr >> 2) & m0;
		const uint64_t lo = (hdr | (hdr >> 1)) & m0;
		return (hi | (b2 & lo)) == 0;
	}

	__device__ __forceinline__ Fetched fetch_record(uint64_t hdr, __amdgpu_buffer_rsrc_t in, uint32_t pos, uint32_t seg_len, const LaneConsts &lc)
	{
		Fetched r;
		r.hdr = hdr;
		r.narrow = header_is_narrow(hdr);
		const bool hdr_bad = ((hdr & 0xC000C000C0000000ull) != 0) || (((hdr >> 14) & 3u) == 3u);
		// Offsets depend on the tier; the two loads below do not (no branch around a memory operation,
		// no copy of an in-flight load result: the ring keeps its counted waits).  Lanes without a plane
		// - and every lane of a malformed record - point out of range and read 0; the descriptor's
		// num_records is the segment length, so nothing outside the segment is ever touched.
		uint32_t oa, ob;
		if (r.narrow)
		{ // lanes 0..31: lane 4*slot + plane reads the whole 64-bit plane word
			const uint32_t w = ((lc.n_hhi ? (uint32_t)(hdr >> 32) : (uint32_t)hdr) >> lc.n_hsh) & 31u;
			const uint32_t incl = half_inclusive_sum(lc.n_first ? w : 0u);
			r.words = (uint32_t)__builtin_amdgcn_readlane((int)incl, 31);
			r.bad = hdr_bad || (pos + r.words > seg_len);
			oa = (!r.bad && lc.n_half == 0 && lc.n_bit < w) ? (pos + incl - w + lc.n_bit) * 8u : RIR_OOB;
			ob = RIR_OOB;
		}
		else
		{ // wide tier: this row's header field is w_q | w_{4+q} << 5 | base nibble << 10 | mode << 14
			const uint32_t field = ((lc.row_hi ? (uint32_t)(hdr >> 32) : (uint32_t)hdr) >> lc.sh16) & 0xffffu;
			const uint32_t wa = field & 31u, wb = (field >> 5) & 31u;
			const uint32_t ia = rows_inclusive_sum(wa), ib = rows_inclusive_sum(wb);
			const uint32_t tot_a = (uint32_t)__builtin_amdgcn_readlane((int)ia, 63);
			const uint32_t tot_b = (uint32_t)__builtin_amdgcn_readlane((int)ib, 63);
			r.words = tot_a + tot_b;
			const bool too_wide = __ballot(wa > 16u || wb > 16u) != 0;
			r.bad = hdr_bad || too_wide || (pos + r.words > seg_len);
			oa = (!r.bad && lc.bit < wa) ? (pos + ia - wa + lc.bit) * 8u : RIR_OOB;
			ob = (!r.bad && lc.bit < wb) ? (pos + tot_a + ib - wb + lc.bit) * 8u : RIR_OOB;
		}
		// exactly two loads per record, whatever the tier (the consumer's wait counts younger loads)
		r.a = __builtin_amdgcn_raw_buffer_load_b64(in, oa, 0, STREAM_LOAD_AUX);
		r.b = __builtin_amdgcn_raw_buffer_load_b64(in, ob, 0, STREAM_LOAD_AUX);
		return r;
	}

	// residuals of one record back in pixel order (packed pairs), from the fetched plane words
	__device__ __forceinline__ Px8 planes_to_residuals(v2u32 a, v2u32 b, bool narrow, const TransposeConsts &tc)
	{
		Px8 r;
		if (narrow)
		{
			// upper-half lanes take the high dword of their partner's plane word
			auto sw = __builtin_amdgcn_permlane32_swap(a.x, a.y, false, false);
			const uint32_t x = transpose32(sw[0], tc); // nibble j = residual of pixel j
			const uint32_t lo = x & 0x0f0f0f0fu, hi = (x >> 4) & 0x0f0f0f0fu; // bytes r0,r2,r4,r6 / r1,r3,r5,r7
			r.d[0] = __builtin_amdgcn_perm(hi, lo, 0x0c040c00u);
			r.d[1] = __builtin_amdgcn_perm(hi, lo, 0x0c050c01u);
			r.d[2] = __builtin_amdgcn_perm(hi, lo, 0x0c060c02u);
			r.d[3] = __builtin_amdgcn_perm(hi, lo, 0x0c070c03u);
		}
		else
		{
			uint32_t alo = a.x, ahi = a.y, blo = b.x, bhi = b.y;
			transpose64x2(alo, ahi, blo, bhi, tc);
			r.d[0] = alo, r.d[1] = ahi, r.d[2] = blo, r.d[3] = bhi;
		}
		return r;
	}

	__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l)
	{
		return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l) |
			   ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32);
	}

	// MODE_LEFT reconstruction: inclusive prefix sum (mod 2^16) over the tile, lane-local then across lanes
	__device__ __forceinline__ Px8 left_integrate(const Px8 &d, int lane)
	{
		uint32_t a[8];
#pragma unroll
		for (int k = 0; k < 4; ++k)
		{
			a[2 * k] = d.d[k] & 0xffffu;
			a[2 * k + 1] = d.d[k] >> 16;
		}
#pragma unroll
		for (int i = 1; i < 8; ++i)
			a[i] = (a[i] + a[i - 1]) & 0xffffu;
		const uint32_t incl = wave_scan_add(a[7], lane);
		const uint32_t carry = (incl - a[7]) & 0xffffu;
		Px8 o;
#pragma unroll
		for (int k = 0; k < 4; ++k)
			o.d[k] = ((a[2 * k] + carry) & 0xffffu) | (((a[2 * k + 1] + carry) & 0xffffu) << 16);
		return o;
	}

	// where decode_tile puts a reconstructed record: every frame of the chunk at its place in `frames`; AUX: the policy of the FAST stores
	// (1 KiB per wave instruction: whole 128-byte lines when the frames are 128-byte aligned)
	template <int AUX = FRAME_STORE_AUX>
	struct ChunkSink
	{
		uint16_t *frames, *tile0;
		int64_t npx, frame0, p0;
		uint32_t lane_off;
		__device__ __forceinline__ ChunkSink(uint16_t *frames_, int64_t npx_, int64_t frame0_, int tile, int lane)
			: frames(frames_), tile0(frames_ + frame0_ * npx_ + (int64_t)tile * RIRB1_TILE_PX), npx(npx_), frame0(frame0_),
			  p0((int64_t)tile * RIRB1_TILE_PX + lane * 8), lane_off((uint32_t)lane * 16u)
		{
		}
		template <bool FAST>
		__device__ __forceinline__ void put(int f, const Px8 &o)
		{
			if (FAST)
				buf_store8<AUX>(tile0 + (int64_t)f * npx, lane_off, o);
			else
				store8(frames, frame0 + f, npx, p0, false, o);
		}
	};

	// The record walk of one tile over frames 0 .. nf - 1 of a chunk; sink.put<FAST>(f, pixels) takes each reconstructed frame.
	// check_end: the walk covers the whole segment, so it must end exactly at its last word (a walk that stops early - the selective
	// decode - checks every record it reads against the segment, not what lies behind the last one).
	template <bool FAST, class Sink>
	__device__ __forceinline__ void decode_tile(const uint64_t *__restrict__ my_hdr, const uint64_t *__restrict__ in_ptr, uint32_t seg_len,
												int nf, bool check_end, int lane, Sink &sink, int *__restrict__ error_flag)
	{
		const TransposeConsts tc = make_transpose_consts(lane);
		const LaneConsts lc = make_lane_consts(lane);
		const __amdgpu_buffer_rsrc_t in = make_rsrc(in_ptr, seg_len * 8u);

		Px8 prev;
		prev.d[0] = prev.d[1] = prev.d[2] = prev.d[3] = 0;
		uint32_t pos = 0;  // fetch position: words of every record requested so far
		bool err = false; // malformed input seen (wave-uniform); reported once, at the end
		for (int f0 = 0; f0 < nf; f0 += 64)
		{
			const int nr = min(64, nf - f0);
			const uint64_t my_h = lane < nr ? my_hdr[f0 + lane] : 0ull; // 64 headers, one coalesced load
			// Ring of 4 records in flight (fixed registers, loop unrolled by 4, see the encoder).
			// Requests past the end of the round use an all-zero header = empty record (no memory
			// touched); a malformed record points every lane out of range, so the loop body has no
			// data-dependent branch and the compiler keeps counted s_waitcnt vmcnt(N).
			Fetched r0 = fetch_record(readlane64(my_h, 0), in, pos, seg_len, lc);
			pos += r0.words;
			Fetched r1 = fetch_record(nr > 1 ? readlane64(my_h, 1) : 0ull, in, pos, seg_len, lc);
			pos += r1.words;
			Fetched r2 = fetch_record(nr > 2 ? readlane64(my_h, 2) : 0ull, in, pos, seg_len, lc);
			pos += r2.words;
			Fetched r3 = fetch_record(nr > 3 ? readlane64(my_h, 3) : 0ull, in, pos, seg_len, lc);
			pos += r3.words;
#define RIR_DEC_STEP(FR, R)                                                                                          \
	if ((FR) < nr)                                                                                                   \
	{                                                                                                                \
		const int fr = (FR);                                                                                         \
		const uint64_t hdr = R.hdr;                                                                                  \
		err |= R.bad;                                                                                                \
		const v2u32 wa_ = R.a, wb_ = R.b;                                                                             \
		const bool narrow_ = R.narrow;                                                                               \
		/* refill the slot with the record four frames ahead */                                                       \
		R = fetch_record(fr + 4 < nr ? readlane64(my_h, fr + 4) : 0ull, in, pos, seg_len, lc);                        \
		pos += R.words;                                                                                              \
		const Px8 res = planes_to_residuals(wa_, wb_, narrow_, tc);                                                  \
		const uint32_t mode = (uint32_t)(hdr >> 14) & 3u;                                                            \
		const uint32_t base = ((uint32_t)(hdr >> 10) & 0xfu) | ((uint32_t)(hdr >> 22) & 0xf0u) |                     \
							  ((uint32_t)(hdr >> 34) & 0xf00u) | ((uint32_t)(hdr >> 46) & 0xf000u);                  \
		const uint32_t b2 = base | (base << 16);                                                                     \
		Px8 o;                                                                                                       \
		_Pragma("unroll") for (int k = 0; k < 4; ++k) o.d[k] = pk_add16(res.d[k], b2);                              \
		if (f0 + fr == 0)                                                                                            \
		{ /* key frame: RAW or LEFT */                                                                               \
			if (mode == RIRB1_MODE_LEFT)                                                                             \
				o = left_integrate(o, lane);                                                                         \
			err |= (mode == RIRB1_MODE_TEMPORAL);                                                                    \
		}                                                                                                            \
		else                                                                                                         \
		{ /* TEMPORAL (or RAW); LEFT is only legal on the key frame */                                               \
			const uint32_t keep = (mode == RIRB1_MODE_TEMPORAL) ? 0xffffffffu : 0u;                                  \
			_Pragma("unroll") for (int k = 0; k < 4; ++k) o.d[k] = pk_add16(prev.d[k] & keep, o.d[k]);              \
			err |= (mode == RIRB1_MODE_LEFT);                                                                        \
		}                                                                                                            \
		sink.template put<FAST>(f0 + fr, o);                                                                         \
		prev = o;                                                                                                    \
	}
			for (int fb = 0; fb < nr; fb += 4)
			{
				RIR_DEC_STEP(fb, r0)
				RIR_DEC_STEP(fb + 1, r1)
				RIR_DEC_STEP(fb + 2, r2)
				RIR_DEC_STEP(fb + 3, r3)
			}
#undef RIR_DEC_STEP
		}
		if ((err || (check_end && pos != seg_len)) && lane == 0)
			atomicExch(error_flag, 1);
	}

	// grid = (ceil(ntiles/4), nchunks), block = 256 (4 independent waves)
	// Two layouts of the payload, one record format (the third, packed, has a kernel of its own: rirb1_decode_packed):
	//   dense   (seg_words == NULL)  segment (c, t) = stream[chunk_off[c] + tile_off[c][t] ...) - the file form, tables untrusted
	//   slotted (seg_words != NULL)  segment (c, t) = stream[(c * ntiles + t) * RIRB1_SLOT_WORDS(gop) ...), seg_words[c][t] words
	//            long - what rirb1_encode_tiles leaves in its workspace: every segment's place is known before anything is
	//            packed, so the encoder needs no second pass and the decoder no offsets (tile_off / chunk_off unused).
	__global__ __launch_bounds__(256) void rirb1_decode_tiles(const uint64_t *__restrict__ hdr_table, const uint32_t *__restrict__ tile_off,
															 const uint64_t *__restrict__ chunk_off, const uint64_t *__restrict__ stream,
															 uint64_t stream_words, int64_t npx, int ntiles, int nframes, int gop,
															 const int64_t *__restrict__ chunk_frames, const uint32_t *__restrict__ seg_words,
															 uint16_t *__restrict__ frames, int *__restrict__ error_flag)
	{
		const int lane = threadIdx.x & 63;
		const int tile = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		if (tile >= ntiles)
			return;
		const int chunk = blockIdx.y;
		// chunk -> frames of the output: consecutive runs of `gop` frames, or (chunk_frames != NULL, nframes = capacity of
		// `frames`) an explicit (first frame, frame count) pair per chunk - chunks gathered from several shards decode
		// straight to their place in the reassembled stream
		int64_t f_begin = (int64_t)chunk * gop;
		int nf = (int)min((int64_t)gop, (int64_t)nframes - f_begin);
		if (chunk_frames)
		{
			const int64_t cf = chunk_frames[2 * chunk], cn = chunk_frames[2 * chunk + 1];
			if (cn == 0)
				return; // padding entry
			if (cf < 0 || cn < 0 || cn > gop || cf > (int64_t)nframes - cn)
			{
				if (lane == 0)
					atomicExch(error_flag, 1);
				return;
			}
			f_begin = cf, nf = (int)cn;
		}
		const int64_t slot = (int64_t)chunk * ntiles + tile;
		const uint64_t *my_hdr = hdr_table + slot * gop;
		uint32_t seg_len;
		const uint64_t *in;
		if (seg_words)
		{ // slotted: the slot's place is fixed, its length comes from the encoder's table (clamped to the slot all the same)
			const uint64_t base = (uint64_t)slot * (uint64_t)RIRB1_SLOT_WORDS(gop);
			seg_len = min(seg_words[slot], (uint32_t)gop * RIRB1_REC_MAX_WORDS);
			if (base > stream_words || (uint64_t)seg_len > stream_words - base)
			{
				if (lane == 0)
					atomicExch(error_flag, 1);
				return;
			}
			in = stream + base;
		}
		else
		{
			const uint32_t t0 = tile_off[(int64_t)chunk * (ntiles + 1) + tile];
			const uint32_t t1 = tile_off[(int64_t)chunk * (ntiles + 1) + tile + 1];
			const uint64_t c0 = chunk_off[chunk], c1 = chunk_off[chunk + 1];
			// The tables are untrusted (they come from a file): the segment [c0 + t0, c0 + t1) must lie inside the chunk
			// [c0, c1) and the chunk inside the stream allocation BEFORE a descriptor is built on it - the descriptor's
			// num_records only bounds accesses relative to its base.
			if (c0 > c1 || c1 > stream_words || t1 < t0 || (uint64_t)t1 > c1 - c0)
			{ // malformed offsets tables
				if (lane == 0)
					atomicExch(error_flag, 1);
				return;
			}
			seg_len = min(t1 - t0, (uint32_t)gop * RIRB1_REC_MAX_WORDS);
			in = stream + c0 + t0;
		}
		const bool fast = ((npx & 7) == 0) && ((int64_t)(tile + 1) * RIRB1_TILE_PX <= npx) && ((((uintptr_t)frames) & 15) == 0);
		ChunkSink<> sink(frames, npx, f_begin, tile, lane);
		if (fast)
			decode_tile<true>(my_hdr, in, seg_len, nf, true, lane, sink, error_flag);
		else
			decode_tile<false>(my_hdr, in, seg_len, nf, true, lane, sink, error_flag);
	}

	// The packed layout: segment (c, t) = stream[seg_pos[c][t] ...), seg_words[c][t] words long - what rirb1_encode_packed leaves, a stream
	// without holes whose segments lie in order of arrival.  Both tables are untrusted (a batch received from another device): the segment
	// must lie inside the stream before a descriptor is built on it.  A kernel of its own, specialised like the encoder: FAST for tiles
	// [tile0, tile_end) that lie whole inside the frame of 16-byte aligned frames, the ragged form for the rest.  Without the other
	// layouts' tables and branches its registers admit 8 workgroups per CU (<= 80 SGPRs) where rirb1_decode_tiles' admit 6; how many
	// run at once is set by the launch (launch_decode_packed).
	// grid = (ceil((tile_end - tile0) / 4), nchunks), block = 256 (4 independent waves)
	template <bool FAST>
	__attribute__((amdgpu_waves_per_eu(8, 8))) __global__ __launch_bounds__(256) void rirb1_decode_packed(
		const uint64_t *__restrict__ hdr_table, const uint64_t *__restrict__ seg_pos, const uint32_t *__restrict__ seg_words,
		const uint64_t *__restrict__ stream, uint64_t stream_words, int64_t npx, int ntiles, int tile0, int tile_end, int nframes, int gop,
		uint16_t *__restrict__ frames, int *__restrict__ error_flag)
	{
		const int lane = threadIdx.x & 63;
		const int tile = tile0 + blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		if (tile >= tile_end)
			return;
		const int chunk = blockIdx.y;
		const int64_t f_begin = (int64_t)chunk * gop;
		const int nf = (int)min((int64_t)gop, (int64_t)nframes - f_begin);
		const int64_t slot = (int64_t)chunk * ntiles + tile;
		const uint64_t base = seg_pos[slot];
		const uint32_t seg_len = min(seg_words[slot], (uint32_t)gop * RIRB1_REC_MAX_WORDS);
		if (base > stream_words || (uint64_t)seg_len > stream_words - base)
		{
			if (lane == 0)
				atomicExch(error_flag, 1);
			return;
		}
		ChunkSink<PACKED_FRAME_STORE_AUX> sink(frames, npx, f_begin, tile, lane);
		decode_tile<FAST>(hdr_table + slot * gop, stream + base, seg_len, nf, true, lane, sink, error_flag);
	}

	// ---- selective decode into the caller's buffer (rir_load_images_device) ----------------------------------------------
	// Where decode_tile puts a record of the selective decode: frame f of the walk is stored when it is the next one the entry selects
	// (first, first + step, ...), at its output slot - the store of a skipped frame points out of range (no branch around it, the walk
	// keeps its counted waits).  MIN_T (IRFileLoader.cpp:1173-1179) is added to the first min_px pixels of every stored frame, after the
	// reconstruction (the next frame is predicted from the stored value without it); F32: the value converted exactly (load_imageF).
	template <bool F32>
	struct SelectSink
	{
		char *cur;		 // this wave's tile in the output frame the next stored frame goes to
		int64_t fbytes;	 // bytes of an output frame
		int next, step;	 // next local frame to store, distance to the one after it
		int npx, p0;	 // pixels of a frame (< 2^31: ChunkCodec::prepare), first pixel of this lane
		uint32_t lane_off, min_t;
		int nmin;		 // pixels of this lane's eight that get min_t
		__device__ __forceinline__ Px8 add_min(Px8 o) const
		{
			if (min_t)
			{
#pragma unroll
				for (int k = 0; k < 4; ++k)
					o.d[k] = pk_add16(o.d[k], (2 * k < nmin ? min_t : 0u) | (2 * k + 1 < nmin ? min_t << 16 : 0u));
			}
			return o;
		}
		// (the walk ends at the last selected frame, so a skipped frame always lies before a selected one: `cur` is inside the output)
		template <bool FAST>
		__device__ __forceinline__ void put(int f, const Px8 &r)
		{
			const bool sel = f == next; // (wave-uniform)
			const Px8 o = add_min(r);
			if (FAST)
			{
				if (F32)
				{
					v4u32 a, b;
					a.x = __builtin_bit_cast(uint32_t, (float)(o.d[0] & 0xffffu)), a.y = __builtin_bit_cast(uint32_t, (float)(o.d[0] >> 16));
					a.z = __builtin_bit_cast(uint32_t, (float)(o.d[1] & 0xffffu)), a.w = __builtin_bit_cast(uint32_t, (float)(o.d[1] >> 16));
					b.x = __builtin_bit_cast(uint32_t, (float)(o.d[2] & 0xffffu)), b.y = __builtin_bit_cast(uint32_t, (float)(o.d[2] >> 16));
					b.z = __builtin_bit_cast(uint32_t, (float)(o.d[3] & 0xffffu)), b.w = __builtin_bit_cast(uint32_t, (float)(o.d[3] >> 16));
					const __amdgpu_buffer_rsrc_t r4 = make_rsrc(cur, RIRB1_TILE_PX * 4);
					__builtin_amdgcn_raw_buffer_store_b128(a, r4, sel ? lane_off * 2u : RIR_OOB, 0, FRAME_STORE_AUX);
					__builtin_amdgcn_raw_buffer_store_b128(b, r4, sel ? lane_off * 2u + 16u : RIR_OOB, 0, FRAME_STORE_AUX);
				}
				else
				{
					v4u32 v;
					v.x = o.d[0], v.y = o.d[1], v.z = o.d[2], v.w = o.d[3];
					__builtin_amdgcn_raw_buffer_store_b128(v, make_rsrc(cur, RIRB1_TILE_PX * 2), sel ? lane_off : RIR_OOB, 0, FRAME_STORE_AUX);
				}
			}
			else if (sel)
			{
#pragma unroll
				for (int k = 0; k < 8; ++k)
				{
					const uint32_t v = (o.d[k >> 1] >> (16 * (k & 1))) & 0xffffu;
					if (p0 + k < npx)
					{
						if (F32)
							reinterpret_cast<float *>(cur)[lane_off / 2u + k] = (float)v;
						else
							reinterpret_cast<uint16_t *>(cur)[lane_off / 2u + k] = (uint16_t)v;
					}
				}
			}
			if (sel)
				next += step, cur += fbytes;
		}
	};

	// grid = (ceil(ntiles/4), entries), block = 256.  Entry e (RirbSelect, filter_kernels.h) names a chunk of the batch - its tables at
	// hdr_table + chunk * ntiles * gop, tile_off + chunk * (ntiles + 1), its payload at stream[chunk_off[chunk] ...) - and the frames
	// of it to store.  Tables and entries are untrusted like the file they come from: every check of the dense form, plus the entry's
	// own (a walk inside the chunk and inside the hdr table, output slots inside `out`); a failed check or a malformed record raises
	// *error_flag.  The walk stops at the last selected frame: frames behind it are neither decoded nor read.
	// FAST: tiles [tile0, tile_end) lie whole inside the frame, npx is a multiple of 8 and `out` 16-byte aligned (the host launches the
	// tiles that do so with FAST, the rest - the frame's last, cut tile - without).
	template <bool F32, bool FAST>
	__attribute__((amdgpu_waves_per_eu(8, 8))) __global__ __launch_bounds__(256) void rirb1_decode_select(
		const uint64_t *__restrict__ hdr_table, const uint32_t *__restrict__ tile_off, const uint64_t *__restrict__ chunk_off, const uint64_t *__restrict__ stream,
		uint64_t stream_words, int64_t npx, int ntiles, int tile0, int tile_end, int gop, int nchunks, const RirbSelect *__restrict__ table, int out_frames,
		void *__restrict__ out, int min_px, uint32_t min_t, int *__restrict__ error_flag)
	{
		const int lane = threadIdx.x & 63;
		const int tile = tile0 + blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		if (tile >= tile_end)
			return;
		const RirbSelect e = table[blockIdx.y];
		if (e.count == 0)
			return;
		const int64_t walk = (int64_t)e.first + (int64_t)(e.count - 1) * e.step + 1;
		if (e.chunk < 0 || e.chunk >= nchunks || e.nframes <= 0 || e.nframes > gop || e.first < 0 || e.count < 0 || e.step < 1 || walk > e.nframes ||
			e.out_first < 0 || e.out_first > out_frames - e.count)
		{
			if (lane == 0)
				atomicExch(error_flag, 1);
			return;
		}
		const int chunk = e.chunk;
		const uint32_t t0 = tile_off[(int64_t)chunk * (ntiles + 1) + tile];
		const uint32_t t1 = tile_off[(int64_t)chunk * (ntiles + 1) + tile + 1];
		const uint64_t c0 = chunk_off[chunk], c1 = chunk_off[chunk + 1];
		if (c0 > c1 || c1 > stream_words || t1 < t0 || (uint64_t)t1 > c1 - c0)
		{ // (the checks of rirb1_decode_tiles' dense form)
			if (lane == 0)
				atomicExch(error_flag, 1);
			return;
		}
		const uint32_t seg_len = min(t1 - t0, (uint32_t)gop * RIRB1_REC_MAX_WORDS);
		const int tpx = tile * RIRB1_TILE_PX;
		SelectSink<F32> sink;
		sink.fbytes = npx * (F32 ? 4 : 2);
		sink.cur = static_cast<char *>(out) + (int64_t)e.out_first * sink.fbytes + (int64_t)tpx * (F32 ? 4 : 2);
		sink.next = e.first, sink.step = e.step;
		sink.npx = (int)npx, sink.p0 = tpx + lane * 8;
		sink.lane_off = (uint32_t)lane * 16u, sink.min_t = min_t & 0xffffu;
		sink.nmin = max(0, min(8, min_px - sink.p0));
		decode_tile<FAST>(hdr_table + ((int64_t)chunk * ntiles + tile) * gop, stream + c0 + t0, seg_len, (int)walk, walk == e.nframes, lane, sink, error_flag);
	}

	// ---- windowed decode into the caller's buffer (rir_load_window_device) ------------------------------------------------
	// Where decode_tile puts a record of the windowed decode: SelectSink's choice of frames and its MIN_T, but of a stored frame only the
	// pixels inside the window, in an output frame of h x w.  A lane's eight pixels keep their place from frame to frame, so where they
	// go is worked out once, before the walk (rirb1_decode_window): relative to `cur`, the first window row this tile touches in the
	// output frame the next stored frame goes to - a frame only moves `cur` on.
	//   FAST     the eight pixels lie in one window row or outside the window: `off`, their byte offset (RIR_OOB outside); the store of
	//            a lane outside, as of a skipped frame, points out of range
	//   general  `off` is the element pixel 0 would go to (modulo 2^32: a lane may begin above the tile's first window row); pixel k is
	//            stored when bit k of `code` is set, at element off + k - rows * gap, rows (bits 8 + 3k .. 10 + 3k of `code`) being the
	//            frame rows between pixel 0 and pixel k, each of which skips gap = W - w elements of the output
	template <bool F32>
	struct WindowSink
	{
		char *cur;
		int64_t fbytes;	 // bytes of an output frame
		uint32_t room;	 // bytes of the output frame this tile's rows take from `cur` on
		int next, step;	 // next local frame to store, distance to the one after it
		uint32_t off, code, gap;
		uint32_t min_t;
		int nmin; // pixels of this lane's eight that get min_t
		__device__ __forceinline__ Px8 add_min(Px8 o) const
		{
			if (min_t)
			{
#pragma unroll
				for (int k = 0; k < 4; ++k)
					o.d[k] = pk_add16(o.d[k], (2 * k < nmin ? min_t : 0u) | (2 * k + 1 < nmin ? min_t << 16 : 0u));
			}
			return o;
		}
		template <bool FAST>
		__device__ __forceinline__ void put(int f, const Px8 &r)
		{
			const bool sel = f == next; // (wave-uniform)
			const Px8 o = add_min(r);
			if (FAST)
			{
				const __amdgpu_buffer_rsrc_t rs = make_rsrc(cur, room);
				const uint32_t at = sel ? off : RIR_OOB;
				if (F32)
				{
					v4u32 a, b;
					a.x = __builtin_bit_cast(uint32_t, (float)(o.d[0] & 0xffffu)), a.y = __builtin_bit_cast(uint32_t, (float)(o.d[0] >> 16));
					a.z = __builtin_bit_cast(uint32_t, (float)(o.d[1] & 0xffffu)), a.w = __builtin_bit_cast(uint32_t, (float)(o.d[1] >> 16));
					b.x = __builtin_bit_cast(uint32_t, (float)(o.d[2] & 0xffffu)), b.y = __builtin_bit_cast(uint32_t, (float)(o.d[2] >> 16));
					b.z = __builtin_bit_cast(uint32_t, (float)(o.d[3] & 0xffffu)), b.w = __builtin_bit_cast(uint32_t, (float)(o.d[3] >> 16));
					__builtin_amdgcn_raw_buffer_store_b128(a, rs, at, 0, FRAME_STORE_AUX);
					__builtin_amdgcn_raw_buffer_store_b128(b, rs, sel ? off + 16u : RIR_OOB, 0, FRAME_STORE_AUX); // (off = RIR_OOB: + 16 is out of range too)
				}
				else
				{
					v4u32 v;
					v.x = o.d[0], v.y = o.d[1], v.z = o.d[2], v.w = o.d[3];
					__builtin_amdgcn_raw_buffer_store_b128(v, rs, at, 0, FRAME_STORE_AUX);
				}
			}
			else
			{
				const __amdgpu_buffer_rsrc_t rs = make_rsrc(cur, room);
				// the eight places are worked out again for every frame: kept across the walk they would cost more registers than a wave
				// has at this residency (the compiler would, so the two words they come from are hidden from it)
				uint32_t d0 = off, cd = code;
				asm volatile("" : "+v"(d0), "+v"(cd));
				const uint32_t on = sel ? cd : 0u;
#pragma unroll
				for (int k = 0; k < 8; ++k)
				{
					const uint32_t v = (o.d[k >> 1] >> (16 * (k & 1))) & 0xffffu;
					// (a pixel outside may have a meaningless place, before `cur` say: it is not looked at)
					const uint32_t at = ((on >> k) & 1u) ? (d0 + (uint32_t)k - ((cd >> (8 + 3 * k)) & 7u) * gap) * (F32 ? 4u : 2u) : RIR_OOB;
					if (F32)
						__builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, (float)v), rs, at, 0, FRAME_STORE_AUX);
					else
						__builtin_amdgcn_raw_buffer_store_b16((short)v, rs, at, 0, FRAME_STORE_AUX);
				}
			}
			if (sel)
				next += step, cur += fbytes;
		}
	};

	// grid = (ceil((tile_end - tile0) / 4), entries), block = 256: rirb1_decode_select for a window of the frame.  `win` is the window of
	// frames of npx pixels in rows of fw, `out` is [out_frames][win.h][win.w].  The tables are the dense form's, restricted to the tiles
	// [t_lo, t_lo + ntiles_win) the host read from the file: headers at hdr_table + (chunk * ntiles_win + tile - t_lo) * gop, ntiles_win + 1
	// tile offsets a chunk, and a chunk's payload slice stream[chunk_off[chunk] ...) begins at its first tile offset.  Every check of
	// rirb1_decode_select, restated for the slice (the segment inside the slice, the slice inside the stream, the entry's own), and the
	// window's: inside the frame, not empty, the tiles asked for among those of the tables; a failed check raises *error_flag and
	// stores nothing.  A tile of the run that holds no pixel of the window (rows of two tiles or more, a window in one half) returns
	// before it reads a header or a payload word.
	// FAST: fw, win.x0 and win.w are multiples of 8, `out` is 16-byte aligned and the tiles [tile0, tile_end) lie whole inside the frame.
	template <bool F32, bool FAST>
	__attribute__((amdgpu_waves_per_eu(8, 8))) __global__ __launch_bounds__(256) void rirb1_decode_window(
		const uint64_t *__restrict__ hdr_table, const uint32_t *__restrict__ tile_off, const uint64_t *__restrict__ chunk_off, const uint64_t *__restrict__ stream,
		uint64_t stream_words, int64_t npx, int fw, RirbWindow win, int t_lo, int ntiles_win, int tile0, int tile_end, int gop, int nchunks,
		const RirbSelect *__restrict__ table, int out_frames, void *__restrict__ out, int min_px, uint32_t min_t, int *__restrict__ error_flag)
	{
		constexpr int ESZ = F32 ? 4 : 2;
		const int lane = threadIdx.x & 63;
		const int tile = tile0 + blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		if (tile >= tile_end)
			return;
		// the frame, the window in it, the tiles of the tables (fw <= 2^24: what a tile's rows take of the output stays far below RIR_OOB)
		bool bad = fw < 1 || fw > (1 << 24) || npx < fw || npx > 0x7fffffff || npx % fw != 0 || win.y0 < 0 || win.x0 < 0 || win.h < 1 || win.w < 1;
		bad = bad || win.x0 > fw - win.w || win.y0 > (int)(npx / fw) - win.h || t_lo < 0 || ntiles_win < 1 || tile < t_lo || tile_end - t_lo > ntiles_win ||
			  (int64_t)tile * RIRB1_TILE_PX >= npx;
		if (FAST)
			bad = bad || ((fw | win.x0 | win.w) & 7) != 0 || (((uintptr_t)out) & 15) != 0 || (int64_t)(tile + 1) * RIRB1_TILE_PX > npx;
		if (bad)
		{
			if (lane == 0)
				atomicExch(error_flag, 1);
			return;
		}
		// the frame rows [ya, yb] of this tile, those of them in the window [ra, rb]; the first and the last may be cut by the tile's ends
		const int tpx = tile * RIRB1_TILE_PX, tlast = (int)min((int64_t)tpx + RIRB1_TILE_PX, npx) - 1;
		const int ya = tpx / fw, yb = tlast / fw;
		const int ra = max(ya, win.y0), rb = min(yb, win.y0 + win.h - 1);
		if (ra > rb)
			return;
		{
			const int xa0 = ra == ya ? tpx - ya * fw : 0, xa1 = ra == yb ? tlast - yb * fw : fw - 1; // the tile's pixels of row ra
			const int xb0 = rb == ya ? tpx - ya * fw : 0, xb1 = rb == yb ? tlast - yb * fw : fw - 1; // ... and of row rb
			const int x1 = win.x0 + win.w - 1;
			if (rb - ra < 2 && !(xa0 <= x1 && xa1 >= win.x0) && !(xb0 <= x1 && xb1 >= win.x0))
				return; // (with a row between ra and rb the tile holds that row whole)
		}
		const RirbSelect e = table[blockIdx.y];
		if (e.count == 0)
			return;
		const int64_t walk = (int64_t)e.first + (int64_t)(e.count - 1) * e.step + 1;
		if (e.chunk < 0 || e.chunk >= nchunks || e.nframes <= 0 || e.nframes > gop || e.first < 0 || e.count < 0 || e.step < 1 || walk > e.nframes ||
			e.out_first < 0 || e.out_first > out_frames - e.count)
		{
			if (lane == 0)
				atomicExch(error_flag, 1);
			return;
		}
		const int chunk = e.chunk;
		const uint32_t *toff = tile_off + (int64_t)chunk * (ntiles_win + 1);
		const uint32_t tb = toff[0], t0 = toff[tile - t_lo], t1 = toff[tile - t_lo + 1];
		const uint64_t c0 = chunk_off[chunk], c1 = chunk_off[chunk + 1];
		if (c0 > c1 || c1 > stream_words || t0 < tb || t1 < t0 || (uint64_t)(t1 - tb) > c1 - c0)
		{ // (the checks of the dense form, the positions taken from the slice's first word)
			if (lane == 0)
				atomicExch(error_flag, 1);
			return;
		}
		const uint32_t seg_len = min(t1 - t0, (uint32_t)gop * RIRB1_REC_MAX_WORDS);
		WindowSink<F32> sink;
		sink.fbytes = (int64_t)win.h * win.w * ESZ;
		sink.cur = static_cast<char *>(out) + (int64_t)e.out_first * sink.fbytes + (int64_t)(ra - win.y0) * win.w * ESZ;
		sink.room = (uint32_t)(rb - ra + 1) * (uint32_t)win.w * ESZ;
		sink.next = e.first, sink.step = e.step;
		sink.min_t = min_t & 0xffffu;
		const int p0 = tpx + lane * 8;
		sink.nmin = max(0, min(8, min_px - p0));
		sink.gap = (uint32_t)(fw - win.w);
		int y = p0 / fw, x = p0 - y * fw;
		sink.off = (uint32_t)((y - ra) * win.w + (x - win.x0));
		sink.code = 0;
		if (FAST)
			sink.off = (y >= ra && y <= rb && x >= win.x0 && x < win.x0 + win.w) ? sink.off * ESZ : RIR_OOB;
		else
		{
			uint32_t below = 0;
#pragma unroll
			for (int k = 0; k < 8; ++k)
			{
				if (y >= ra && y <= rb && x >= win.x0 && x < win.x0 + win.w)
					sink.code |= 1u << k;
				sink.code |= below << (8 + 3 * k);
				if (++x == fw)
					x = 0, ++y, ++below;
			}
		}
		decode_tile<FAST>(hdr_table + ((int64_t)chunk * ntiles_win + (tile - t_lo)) * gop, stream + c0 + (t0 - tb), seg_len, (int)walk, walk == e.nframes, lane,
						  sink, error_flag);
	}

	// ---- host launchers --------------------------------------------------------------------------------

	// The FAST-then-ragged pair of every kernel that has the two forms: launch(fast, t0, t1) for the tiles [0, nfast) that lie whole
	// inside 16-byte aligned frames at `frames`, launch(ragged, t0, t1) for the rest (no launch for an empty range).
	template <class KFast, class KRagged, class Launch>
	static void launch_fast_then_ragged(const void *frames, int64_t npx, int ntiles, KFast fast, KRagged ragged, Launch launch)
	{
		const bool aligned = ((npx & 7) == 0) && ((((uintptr_t)frames) & 15) == 0);
		const int nfast = aligned ? (int)std::min<int64_t>(ntiles, npx / RIRB1_TILE_PX) : 0;
		if (nfast > 0)
			launch(fast, 0, nfast);
		if (ntiles > nfast)
			launch(ragged, nfast, ntiles);
	}

	// LDS words per wave of a staged encoder whose `waves` waves pack one segment: 14.4 KB per workgroup - 11 workgroups per CU, in the
	// dense encoder 7 packing (28 waves) while 4 wait for their offsets (1 wave each); the packed encoder adds 1 KiB for the key frame of
	// its backward wave: 10 per CU, of which 8 can pack.  The reference's recipe needs 290-355 words per wave of four - and never more
	// than the worst case of the wave's share of the chunk
	static int staged_lds_words(int gop, int waves)
	{
		const int share = (gop + 1 + waves - 1) / waves + 1;
		return std::min(448 * 4 / waves, share * RIRB1_REC_MAX_WORDS);
	}

	// stage 1: one pass over the raw frames -> headers, per-tile segment lengths, sparse payload
	hipError_t launch_encode_tiles(const uint16_t *d_frames, int64_t npx, int ntiles, int nframes, int gop, uint64_t *d_hdr,
								   uint32_t *d_seg_words, uint64_t *d_sparse, hipStream_t st)
	{
		const int nchunks = (nframes + gop - 1) / gop;
		launch_fast_then_ragged(d_frames, npx, ntiles, rirb1_encode_tiles<true>, rirb1_encode_tiles<false>, [&](auto kernel, int t0, int t1) {
			hipLaunchKernelGGL(kernel, dim3((t1 - t0 + 3) / 4, nchunks), dim3(256), 0, st, d_frames, npx, ntiles, t0, t1 - t0, nframes, gop, d_hdr, d_seg_words,
							   d_sparse);
		});
		return hipGetLastError();
	}

	// stage 2: offsets (exclusive scans) + gather of the sparse slots into the compact stream
	hipError_t launch_encode_compact(int ntiles, int nframes, int gop, const uint32_t *d_seg_words, const uint64_t *d_sparse,
									 uint32_t *d_tile_off, uint64_t *d_chunk_words, uint64_t *d_chunk_off, uint64_t *d_stream, hipStream_t st)
	{
		const int nchunks = (nframes + gop - 1) / gop;
		dim3 block(256);
		hipLaunchKernelGGL(rirb1_scan_tiles, dim3(nchunks), block, 0, st, d_seg_words, ntiles, d_tile_off, d_chunk_words);
		hipLaunchKernelGGL(rirb1_compact, dim3(ntiles, nchunks), block, 0, st, d_sparse, d_tile_off, d_chunk_words, ntiles, nchunks, gop,
						   d_chunk_off, d_stream);
		return hipGetLastError();
	}

	// single-pass dense encode: control block zeroed by a memset node, then one kernel.  d_ctrl: enc_ctrl_words64() x 8 bytes at
	// the start of an allocation; d_spill: one RIRB1_SLOT_WORDS(gop) slot per (chunk, tile).
	int64_t encode_ctrl_bytes(int nchunks, int ntiles) { return enc_ctrl_words64(nchunks, ntiles) * 8; }
	hipError_t launch_encode_dense(const uint16_t *d_frames, int64_t npx, int ntiles, int nframes, int gop, uint64_t *d_hdr, uint32_t *d_tile_off,
								   uint64_t *d_chunk_off, uint64_t *d_stream, uint64_t *d_ctrl, uint64_t *d_spill, hipStream_t st)
	{
		const int nchunks = (nframes + gop - 1) / gop;
		const int64_t ctrl_bytes = (encode_ctrl_bytes(nchunks, ntiles) + 15) & ~(int64_t)15;
		hipError_t e = hipMemsetAsync(d_ctrl, 0, (size_t)ctrl_bytes, st);
		if (e != hipSuccess)
			return e;
		constexpr int WAVES = 4;
		const int cap = staged_lds_words(gop, WAVES);
		const size_t lds = (size_t)WAVES * cap * 8 + 8 + (2 * WAVES + 2) * 4;
		const int64_t total = (int64_t)nchunks * ntiles;
		// its workgroups wait for the segments in front of them (dealt by tickets, so any grid size makes progress on its own - but
		// not beside a launch that holds the chip waiting for ITS missing workgroups): through the process-wide gate (runtime.h)
		ResidentGate gate(st);
		if (!gate.ok())
			return hipErrorUnknown;
		hipLaunchKernelGGL(rirb1_encode_dense<WAVES>, dim3((unsigned)total), dim3(WAVES * 64), lds, st, d_frames, npx, ntiles, nframes, gop, nchunks, d_hdr,
						   d_tile_off, d_chunk_off, d_stream, d_ctrl, d_spill, cap);
		return hipGetLastError();
	}

	hipError_t launch_decode(const uint64_t *d_hdr, const uint32_t *d_tile_off, const uint64_t *d_chunk_off, const uint64_t *d_stream,
							 uint64_t stream_words, int64_t npx, int ntiles, int nframes, int gop, const int64_t *d_chunk_frames, int nchunks_tab,
							 uint16_t *d_frames, int *d_error, hipStream_t st)
	{
		const int nchunks = d_chunk_frames ? nchunks_tab : (nframes + gop - 1) / gop;
		dim3 grid((ntiles + 3) / 4, nchunks), block(256);
		hipLaunchKernelGGL(rirb1_decode_tiles, grid, block, 0, st, d_hdr, d_tile_off, d_chunk_off, d_stream, stream_words, npx, ntiles, nframes, gop,
						   d_chunk_frames, (const uint32_t *)nullptr, d_frames, d_error);
		return hipGetLastError();
	}
	// the slotted form: d_slots = the encoder's slot array ([nchunks][ntiles] slots of RIRB1_SLOT_WORDS(gop) words), d_seg_words its lengths
	hipError_t launch_decode_slots(const uint64_t *d_hdr, const uint32_t *d_seg_words, const uint64_t *d_slots, int64_t npx, int ntiles, int nframes,
								   int gop, uint16_t *d_frames, int *d_error, hipStream_t st)
	{
		const int nchunks = (nframes + gop - 1) / gop;
		dim3 grid((ntiles + 3) / 4, nchunks), block(256);
		hipLaunchKernelGGL(rirb1_decode_tiles, grid, block, 0, st, d_hdr, (const uint32_t *)nullptr, (const uint64_t *)nullptr, d_slots,
						   (uint64_t)nchunks * ntiles * (uint64_t)RIRB1_SLOT_WORDS(gop), npx, ntiles, nframes, gop, (const int64_t *)nullptr,
						   d_seg_words, d_frames, d_error);
		return hipGetLastError();
	}

	// the packed form.  d_ctrl: RIRB1_PACKED_CTRL_BYTES at the start of the workspace (zeroed here when `reset`; the kernel leaves it
	// zero), d_arena: the rest of it.
	constexpr int PACKED_WAVES = 4; // waves that pack one segment between them
	hipError_t launch_encode_packed(const uint16_t *d_frames, int64_t npx, int ntiles, int nframes, int gop, uint64_t *d_hdr, uint64_t *d_seg_pos,
									uint32_t *d_seg_words, uint64_t *d_stream, uint64_t capacity_words, uint64_t *d_ctrl, uint64_t *d_arena,
									uint64_t arena_words, bool reset, hipStream_t st)
	{
		const int nchunks = (nframes + gop - 1) / gop;
		if (reset)
		{
			hipError_t e = hipMemsetAsync(d_ctrl, 0, RIRB1_PACKED_CTRL_BYTES, st);
			if (e != hipSuccess)
				return e;
		}
		constexpr int WAVES = PACKED_WAVES;
		const int cap = staged_lds_words(gop, WAVES);
		const size_t lds = (size_t)WAVES * cap * 8 + 1024 + (1 + WAVES) * 8 + 2 * WAVES * 4;
		launch_fast_then_ragged(d_frames, npx, ntiles, rirb1_encode_packed<WAVES, true>, rirb1_encode_packed<WAVES, false>, [&](auto kernel, int t0, int t1) {
			hipLaunchKernelGGL(kernel, dim3(t1 - t0, nchunks), dim3(WAVES * 64), lds, st, d_frames, npx, ntiles, t0, nframes, gop, d_hdr, d_seg_pos, d_seg_words,
							   d_stream, capacity_words, d_ctrl, d_arena, arena_words, cap);
		});
		return hipGetLastError();
	}
	hipError_t launch_decode_packed(const uint64_t *d_hdr, const uint64_t *d_seg_pos, const uint32_t *d_seg_words, const uint64_t *d_stream,
									uint64_t stream_words, int64_t npx, int ntiles, int nframes, int gop, uint16_t *d_frames, int *d_error, hipStream_t st)
	{
		const int nchunks = (nframes + gop - 1) / gop;
		// The kernel uses no LDS and its registers admit 8 workgroups per CU, but the decoder is bound by the HBM writes of the frames,
		// not by latency: with more of its waves writing at once the step is slower (DESIGN.md §3, 8 / 7 / 6 / 5 / 4 / 3 / 2 workgroups
		// per CU measured).  The launch reserves LDS it does not use so that 5 share a CU: 160 KiB / 32 KiB.
		constexpr unsigned lds_reserve = 32768;
		launch_fast_then_ragged(d_frames, npx, ntiles, rirb1_decode_packed<true>, rirb1_decode_packed<false>, [&](auto kernel, int t0, int t1) {
			hipLaunchKernelGGL(kernel, dim3((t1 - t0 + 3) / 4, nchunks), dim3(256), lds_reserve, st, d_hdr, d_seg_pos, d_seg_words, d_stream, stream_words, npx,
							   ntiles, t0, t1, nframes, gop, d_frames, d_error);
		});
		return hipGetLastError();
	}

	hipError_t launch_decode_select(const uint64_t *hdr, const uint32_t *tile_off, const uint64_t *chunk_off, const uint64_t *stream, uint64_t stream_words,
									int64_t npx, int ntiles, int gop, int nchunks, const RirbSelect *table, int entries, int out_frames, bool f32, void *out,
									int min_px, uint32_t min_t, int *d_error, hipStream_t st)
	{
		if (entries <= 0)
			return hipSuccess;
		auto go = [&](auto kernel, int t0, int t1) {
			hipLaunchKernelGGL(kernel, dim3((t1 - t0 + 3) / 4, entries), dim3(256), 0, st, hdr, tile_off, chunk_off, stream, stream_words, npx, ntiles, t0, t1,
							   gop, nchunks, table, out_frames, out, min_px, min_t, d_error);
		};
		if (f32)
			launch_fast_then_ragged(out, npx, ntiles, rirb1_decode_select<true, true>, rirb1_decode_select<true, false>, go);
		else
			launch_fast_then_ragged(out, npx, ntiles, rirb1_decode_select<false, true>, rirb1_decode_select<false, false>, go);
		return hipGetLastError();
	}

	// The FAST-then-ragged pair again, over the tiles [t_lo, t_lo + ntiles_win) of the window: FAST needs more than whole tiles of aligned
	// frames here (the window's columns on 8-pixel lanes too), so the split is made here and not by launch_fast_then_ragged.
	hipError_t launch_decode_window(const uint64_t *hdr, const uint32_t *tile_off, const uint64_t *chunk_off, const uint64_t *stream, uint64_t stream_words,
									int64_t npx, int fw, RirbWindow win, int t_lo, int ntiles_win, int gop, int nchunks, const RirbSelect *table, int entries,
									int out_frames, bool f32, void *out, int min_px, uint32_t min_t, int *d_error, hipStream_t st)
	{
		if (entries <= 0)
			return hipSuccess;
		if (fw < 1 || fw > (1 << 24) || npx < fw || npx > 0x7fffffff || npx % fw != 0 || win.y0 < 0 || win.x0 < 0 || win.h < 1 || win.w < 1 ||
			win.x0 > fw - win.w || win.y0 > (int)(npx / fw) - win.h || t_lo < 0 || ntiles_win < 1 ||
			(int64_t)(t_lo + ntiles_win - 1) * RIRB1_TILE_PX >= npx)
			return hipErrorInvalidValue;
		const bool aligned = (((fw | win.x0 | win.w) & 7) == 0) && ((((uintptr_t)out) & 15) == 0);
		const int t_hi = t_lo + ntiles_win;
		const int fast_end = aligned ? std::max(t_lo, (int)std::min<int64_t>(t_hi, npx / RIRB1_TILE_PX)) : t_lo;
		auto go = [&](auto kernel, int t0, int t1) {
			if (t1 > t0)
				hipLaunchKernelGGL(kernel, dim3((t1 - t0 + 3) / 4, entries), dim3(256), 0, st, hdr, tile_off, chunk_off, stream, stream_words, npx, fw, win, t_lo,
								   ntiles_win, t0, t1, gop, nchunks, table, out_frames, out, min_px, min_t, d_error);
		};
		if (f32)
			go(rirb1_decode_window<true, true>, t_lo, fast_end), go(rirb1_decode_window<true, false>, fast_end, t_hi);
		else
			go(rirb1_decode_window<false, true>, t_lo, fast_end), go(rirb1_decode_window<false, false>, fast_end, t_hi);
		return hipGetLastError();
	}

	// The window of whole frames (a windowed read behind a read-back filter, which needs whole frames): dst[f][y][x] = src[f][y0 + y][x0 + x],
	// uint16 or (F32) the value converted exactly; one element per thread and turn
	template <bool F32>
	__global__ __launch_bounds__(256) void crop_window_kernel(const uint16_t *__restrict__ src, int64_t npx, int fw, int y0, int x0, int h, int w,
															   void *__restrict__ dst, int64_t total)
	{
		for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
		{
			const int64_t row = i / w; // (frame, window row)
			const int x = (int)(i - row * w);
			const int64_t f = row / h;
			const int y = (int)(row - f * h);
			const uint16_t v = src[f * npx + (int64_t)(y0 + y) * fw + x0 + x];
			if (F32)
				static_cast<float *>(dst)[i] = (float)v;
			else
				static_cast<uint16_t *>(dst)[i] = v;
		}
	}
	hipError_t launch_crop_window(const uint16_t *src, int fw, int fh, int y0, int x0, int h, int w, int nframes, bool f32, void *dst, hipStream_t st)
	{
		const int64_t total = (int64_t)nframes * h * w;
		if (total <= 0)
			return hipSuccess;
		if (y0 < 0 || x0 < 0 || h < 1 || w < 1 || y0 > fh - h || x0 > fw - w)
			return hipErrorInvalidValue;
		const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
		if (f32)
			hipLaunchKernelGGL(crop_window_kernel<true>, dim3(blocks), dim3(256), 0, st, src, (int64_t)fw * fh, fw, y0, x0, h, w, dst, total);
		else
			hipLaunchKernelGGL(crop_window_kernel<false>, dim3(blocks), dim3(256), 0, st, src, (int64_t)fw * fh, fw, y0, x0, h, w, dst, total);
		return hipGetLastError();
	}
} // namespace rir
