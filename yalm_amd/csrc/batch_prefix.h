// batch_prefix.h — batched decode attention over a SHARED prompt prefix, on the matrix cores.
//
// The sequences of a batch that continue one prompt share cache rows [0, prefix): those rows stay
// in the decoder's own caches and every sequence attends to them there; rows from `prefix` on are
// the sequence's own. Two launches per layer, and no workgroup of either waits for another:
//
//  1. attn_prefix_part_kernel. One wave owns (kv head g, segment, key split). Segment 0 is the
//     shared prefix: its query rows are ALL n_seq * G heads of the kv head (row r = sequence r / G,
//     head g G + r % G), so a shared K / V row is read from HBM once per kv head and step, whatever
//     the sequence count. Segment s + 1 is sequence s's own rows [prefix, kv_len[s]) with that
//     sequence's G rows. The rows are padded to the 32 of v_mfma_f32_32x32x16_f16; dead rows
//     compute on q = 0 and are never stored. Split i of a segment with S splits takes the segment's
//     64-key tiles i, i + S, ..; a split without a tile writes nothing. Per tile, in the prefill
//     attention's "swapped" form (prefill.h attn_prefill_kernel, SPLIT):
//       S^T = K Q^T   A = K rows straight from global memory (lane (key, half) reads 16 bytes of
//                     its key's row per k-step: the contraction over d needs no transpose),
//                     B = the f32 q rows staged once in LDS as f16 hi and lo (q = hi + lo);
//       f32 online softmax with the query on the lane (keys in registers, one permlane32 swap),
//       in log2 units, keys at or past the segment's end set to -inf BY INDEX (their loads are
//       clamped to the segment's last row, so a poisoned or unallocated row is never read);
//       O^T += V^T P^T  A = V^T through LDS (16-byte row writes, swizzled; ds_read_b64_tr_b16
//                     transposed reads), B = P^T as f16 hi and lo straight from the S^T registers.
//     The next tile's K and V loads are issued before the current tile is computed. The wave ends
//     with plain stores of (unnormalised o[D], max, sum) per live row into
//     part[sequence][head][slot][D + 4], slot = the split for segment 0, S0 + the split for a
//     sequence's own segment.
//  2. attn_prefix_merge_kernel. One wave per (sequence, head) folds that head's partials in slot
//     order (prefix splits, then own splits; the counts are computed from prefix and kv_len as the
//     first launch computes them, so a slot nobody wrote is never read) and writes the normalised
//     row. The order is fixed: the same input gives the same bits.
// q beyond the f16 range (|q| > 65504) is not representable by the hi half; the QKV epilogue's
// rows are far inside it.
#pragma once

#include <float.h>

#include "attention.h"
#include "batch.h"
#include "device_common.h"

typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef short pfx_short4_t __attribute__((ext_vector_type(4)));
#define PFX_LDS __attribute__((address_space(3)))

#define PFX_TILE 64                // keys per tile
#define PFX_ROWS 32                // query rows of a workgroup (the MFMA's 32)
#define PFX_SPLITS ATTN_SPLITS     // key splits of the shared prefix per kv head
#define PFX_OWN_SPLITS 8           // key splits of a sequence's own rows per kv head

// the slots of one (sequence, head) and the floats of one slot: o[D], max, sum, 2 of padding
// (16-byte stores of o)
__host__ __device__ constexpr int pfx_stride(int D) { return D + 4; }
__host__ __device__ inline int pfx_tiles(int rows) { return (rows + PFX_TILE - 1) / PFX_TILE; }
// S0: splits of the prefix; S1: of every own segment (sized for the rows the window leaves)
__host__ __device__ inline int pfx_s0(int prefix) {
	const int t = pfx_tiles(prefix);
	return t < PFX_SPLITS ? t : PFX_SPLITS;
}
__host__ __device__ inline int pfx_s1(int prefix, int cache_rows) {
	const int t = pfx_tiles(cache_rows - prefix);
	return t < 1 ? 1 : t < PFX_OWN_SPLITS ? t : PFX_OWN_SPLITS;
}
// floats of the partial buffer of a batch: every prefix, every window
static inline size_t pfx_part_floats(int n_seq, int n_heads, int D) {
	return (size_t)n_seq * n_heads * (PFX_SPLITS + PFX_OWN_SPLITS) * pfx_stride(D);
}

struct PfxArgs {
	const float *q;               // [n_seq] rows, q_stride floats apart
	float *out;                   // the same shape
	int q_stride;
	const uint16_t *ks, *vs;      // the shared caches: rows [0, prefix)
	BatchKV kv;                   // every sequence's own caches: rows [prefix, kv_len[s])
	const StepState *steps;       // kv_len of every sequence
	float *part;
	int n_seq, prefix, n_heads, n_kv, S0, S1;
};

__device__ __forceinline__ void pfx_lds_fence() { // LDS writes and reads of this wave, in program order
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

template <int D>
__global__ __launch_bounds__(YALM_WAVE) void attn_prefix_part_kernel(const PfxArgs a) {
	static_assert(D == 64 || D == 128, "head_dim");
	constexpr int DCH = D / 8, KS = D / 16, NJ = PFX_TILE / 32, NV = PFX_TILE * DCH / YALM_WAVE;
	constexpr int QSTR = D + 8; // halves per staged q row: 16 bytes of padding spread the rows over the banks
	__shared__ __attribute__((aligned(16))) uint16_t Qh[PFX_ROWS * QSTR], Ql[PFX_ROWS * QSTR], Vs[PFX_TILE * D];
	const int lane = threadIdx.x & 63, l32 = lane & 31, hh = lane >> 5;
	const int G = a.n_heads / a.n_kv, kv_dim = a.n_kv * D;
	// unit -> (kv head, segment, split): the prefix splits of every kv head, then the own splits
	const int g = (int)blockIdx.x % a.n_kv, v = (int)blockIdx.x / a.n_kv;
	const bool own = v >= a.S0;
	const int seq0 = own ? (v - a.S0) / a.S1 : 0;        // the first (own: the only) sequence of the rows
	const int split = own ? (v - a.S0) % a.S1 : v, S = own ? a.S1 : a.S0;
	const int nrows = own ? G : a.n_seq * G;              // live query rows
	const int beg = own ? a.prefix : 0;
	const int end = __builtin_amdgcn_readfirstlane(own ? a.steps[seq0].kv_len : a.prefix);
	const int ntiles = pfx_tiles(end - beg);
	if (split >= ntiles)
		return; // an empty split writes nothing (the merge does not read it)
	const uint16_t *kc = a.ks, *vc = a.vs;
	if (own) {
		kc = seq0 == 0 ? a.kv.k[0] : seq0 == 1 ? a.kv.k[1] : seq0 == 2 ? a.kv.k[2] : a.kv.k[3];
		vc = seq0 == 0 ? a.kv.v[0] : seq0 == 1 ? a.kv.v[1] : seq0 == 2 ? a.kv.v[2] : a.kv.v[3];
	}
	kc += g * D, vc += g * D;

	// ---- q rows -> LDS as f16 hi | lo; dead rows are zero
	for (int e = lane; e < PFX_ROWS * D / 4; e += YALM_WAVE) {
		const int r = e / (D / 4), d = 4 * (e % (D / 4));
		float4_t x = {0.0f, 0.0f, 0.0f, 0.0f};
		if (r < nrows)
			x = *(const float4_t *)(a.q + (size_t)(seq0 + r / G) * a.q_stride + (size_t)(g * G + r % G) * D + d);
		uint16_t hi[4], lo[4];
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const _Float16 h = (_Float16)x[i], l = (_Float16)(x[i] - (float)h);
			__builtin_memcpy(&hi[i], &h, 2);
			__builtin_memcpy(&lo[i], &l, 2);
		}
		*(uint2 *)(Qh + r * QSTR + d) = make_uint2(hi[0] | ((uint32_t)hi[1] << 16), hi[2] | ((uint32_t)hi[3] << 16));
		*(uint2 *)(Ql + r * QSTR + d) = make_uint2(lo[0] | ((uint32_t)lo[1] << 16), lo[2] | ((uint32_t)lo[3] << 16));
	}

	// a tile's loads; rows at or past `end` read the segment's last row instead (masked below)
	auto load_k = [&](int key0, u32x4_t (&kf)[NJ][KS]) {
#pragma unroll
		for (int j = 0; j < NJ; ++j) {
			const uint16_t *p = kc + (size_t)min(key0 + 32 * j + l32, end - 1) * kv_dim + 8 * hh;
#pragma unroll
			for (int s = 0; s < KS; ++s)
				kf[j][s] = load16(p + 16 * s);
		}
	};
	auto load_v = [&](int key0, u32x4_t (&vr)[NV]) {
#pragma unroll
		for (int i = 0; i < NV; ++i) {
			const int idx = i * YALM_WAVE + lane, r = idx / DCH, c = idx % DCH;
			vr[i] = load16(vc + (size_t)min(key0 + r, end - 1) * kv_dim + 8 * c);
		}
	};

	const float sl2 = 1.4426950408889634f / sqrtf((float)D); // scores in log2 units
	f32x16_t o[D / 32]; // O^T: rows d = 32 jd + crow(reg), column = the query row l32
#pragma unroll
	for (int jd = 0; jd < D / 32; ++jd)
		o[jd] = f32x16_t{};
	float m = -FLT_MAX, l = 0.0f;
	// transposed-read lane geometry (ds_read_b64_tr_b16: 16-lane groups, 4 rows x 16 columns)
	const int gi = lane & 15, gq = gi >> 2, gp = gi & 3, dgrp = 16 * ((lane >> 4) & 1);

	u32x4_t kf[NJ][KS], kn[NJ][KS], vr[NV];
	load_k(beg + split * PFX_TILE, kf);
	load_v(beg + split * PFX_TILE, vr);
	for (int t = split; t < ntiles; t += S) {
		const int key0 = beg + t * PFX_TILE;
		pfx_lds_fence(); // the last tile's V reads (and the first tile's q writes) are done
#pragma unroll
		for (int i = 0; i < NV; ++i) { // chunk c of row r at chunk c ^ ((r & 3) << 1): the 4 rows of a transposed read on distinct banks
			const int idx = i * YALM_WAVE + lane, r = idx / DCH, c = idx % DCH;
			*(u32x4_t *)(Vs + r * D + 8 * (c ^ ((r & 3) << 1))) = vr[i];
		}
		pfx_lds_fence();
		const bool more = t + S < ntiles;
		if (more) { // the next tile's loads fly under this tile's math
			load_k(key0 + S * PFX_TILE, kn);
			load_v(key0 + S * PFX_TILE, vr);
		}
		// ---- S^T = K Q^T: register r of block j is key key0 + 32 j + crow(r), column = query row
		f32x16_t st[NJ];
#pragma unroll
		for (int j = 0; j < NJ; ++j)
			st[j] = f32x16_t{};
#pragma unroll
		for (int s = 0; s < KS; ++s) {
			const half8_t qh = *(const half8_t *)(Qh + l32 * QSTR + 16 * s + 8 * hh);
			const half8_t ql = *(const half8_t *)(Ql + l32 * QSTR + 16 * s + 8 * hh);
#pragma unroll
			for (int j = 0; j < NJ; ++j) {
				const half8_t ka = __builtin_bit_cast(half8_t, kf[j][s]);
				st[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka, qh, st[j], 0, 0, 0);
				st[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka, ql, st[j], 0, 0, 0);
			}
		}
		if (key0 + PFX_TILE > end) { // the segment's last tile: mask by index
#pragma unroll
			for (int j = 0; j < NJ; ++j)
#pragma unroll
				for (int r = 0; r < 16; ++r)
					if (key0 + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * hh >= end)
						st[j][r] = -INFINITY;
		}
		float mx = st[0][0];
#pragma unroll
		for (int j = 0; j < NJ; ++j)
#pragma unroll
			for (int r = (j == 0 ? 1 : 0); r < 16; ++r)
				mx = fmaxf(mx, st[j][r]);
		mx = fmaxf(mx, xor32(mx)) * sl2; // the other lane half holds the other keys (a tile has a live key: finite)
		const float mn = fmaxf(m, mx), alpha = __builtin_amdgcn_exp2f(m - mn);
		m = mn;
		l *= alpha;
#pragma unroll
		for (int jd = 0; jd < D / 32; ++jd)
			o[jd] *= alpha;
		half8_t pb[NJ][2], pl[NJ][2]; // P^T fragments [block j][k-step s], hi and lo
		float ls = 0.0f;
#pragma unroll
		for (int j = 0; j < NJ; ++j)
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const float p = __builtin_amdgcn_exp2f(fmaf(st[j][r], sl2, -m));
				ls += p;
				const _Float16 ph = (_Float16)p;
				pb[j][r >> 3][r & 7] = ph;
				pl[j][r >> 3][r & 7] = (_Float16)(p - (float)ph);
			}
		ls += xor32(ls);
		l += ls;
		// ---- O^T += V^T P^T: element e of lane half hh is key 32 j + 16 s + 8 (e >> 2) + 4 hh + (e & 3)
#pragma unroll
		for (int j = 0; j < NJ; ++j)
#pragma unroll
			for (int s = 0; s < 2; ++s) {
				const int klo = 32 * j + 16 * s + 4 * hh + gq;
#pragma unroll
				for (int jd = 0; jd < D / 32; ++jd) {
					const int d = 32 * jd + dgrp + 4 * gp;
					const pfx_short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
					    (PFX_LDS pfx_short4_t *)(Vs + klo * D + 8 * ((d >> 3) ^ ((klo & 3) << 1)) + (d & 7)));
					const pfx_short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((PFX_LDS pfx_short4_t *)(
					    Vs + (klo + 8) * D + 8 * ((d >> 3) ^ (((klo + 8) & 3) << 1)) + (d & 7)));
					half8_t va;
#pragma unroll
					for (int e = 0; e < 4; ++e) {
						va[e] = __builtin_bit_cast(_Float16, (short)lo[e]);
						va[4 + e] = __builtin_bit_cast(_Float16, (short)hi[e]);
					}
					o[jd] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb[j][s], o[jd], 0, 0, 0);
					o[jd] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pl[j][s], o[jd], 0, 0, 0);
				}
			}
		if (more) {
#pragma unroll
			for (int j = 0; j < NJ; ++j)
#pragma unroll
				for (int s = 0; s < KS; ++s)
					kf[j][s] = kn[j][s];
		}
	}
	// ---- the partial of every live row: o[D] (d = 32 jd + 8 r4 + 4 hh + e), then (max, sum)
	if (l32 < nrows) {
		const int slot = own ? a.S0 + split : split;
		float *dst = a.part + (((size_t)(seq0 + l32 / G) * a.n_heads + (g * G + l32 % G)) * (a.S0 + a.S1) + slot) *
		                          pfx_stride(D);
#pragma unroll
		for (int jd = 0; jd < D / 32; ++jd)
#pragma unroll
			for (int r4 = 0; r4 < 4; ++r4) {
				float4_t x;
#pragma unroll
				for (int e = 0; e < 4; ++e)
					x[e] = o[jd][4 * r4 + e];
				*(float4_t *)(dst + 32 * jd + 8 * r4 + 4 * hh) = x;
			}
		if (hh == 0) {
			dst[D] = m;
			dst[D + 1] = l;
		}
	}
}

// One wave per (sequence, head): lane d (and d + 64) folds dimension d of the head's partials.
template <int D>
__global__ __launch_bounds__(YALM_WAVE) void attn_prefix_merge_kernel(const PfxArgs a) {
	const int lane = threadIdx.x & 63;
	const int s = (int)blockIdx.x / a.n_heads, h = (int)blockIdx.x % a.n_heads;
	const int n0 = min(pfx_tiles(a.prefix), a.S0), n1 = max(0, min(pfx_tiles(a.steps[s].kv_len - a.prefix), a.S1));
	const float *p = a.part + ((size_t)s * a.n_heads + h) * (a.S0 + a.S1) * pfx_stride(D);
	constexpr int ND = (D + 63) / 64;
	float M = -FLT_MAX;
	for (int i = 0; i < n0 + n1; ++i) // slot order: prefix splits, then own splits
		M = fmaxf(M, p[(size_t)(i < n0 ? i : a.S0 + i - n0) * pfx_stride(D) + D]);
	float L = 0.0f, acc[ND] = {};
	for (int i = 0; i < n0 + n1; ++i) {
		const float *ps = p + (size_t)(i < n0 ? i : a.S0 + i - n0) * pfx_stride(D);
		const float w = __builtin_amdgcn_exp2f(ps[D] - M);
		L = fmaf(ps[D + 1], w, L);
#pragma unroll
		for (int u = 0; u < ND; ++u)
			acc[u] = fmaf(ps[lane + 64 * u], w, acc[u]);
	}
	const float inv = 1.0f / L;
	float *out = a.out + (size_t)s * a.q_stride + (size_t)h * D;
#pragma unroll
	for (int u = 0; u < ND; ++u)
		out[lane + 64 * u] = acc[u] * inv;
}
