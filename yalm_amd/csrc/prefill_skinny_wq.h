// prefill_skinny_wq.h — the short-prompt split-K GEMM (prefill_skinny.h) over weights in
// their stored format: fp8 (E5M2), e4m3 (row-scaled OCP E4M3) and q4 (4-bit groups of 32).
// The prefill of such a model otherwise upcasts each layer to f16 in memory first (prefill.h
// *_to_f16_kernel) and streams the copy: 5 (fp8, e4m3) to 8 (q4) times the model's own bytes.
// Here the raw bytes are the stream and become f16 MFMA fragments in registers.
//
// Same product as skinny_gemm_lds_kernel, bit for bit: tokens are the A operand (sk_stage_a),
// 16 weight rows per wave the B operand of v_mfma_f32_16x16x32_f16, lane (n, q) of step j
// holds elements 32 j + 8 q .. + 7 of row n, converted by the upcast kernels' own (exact)
// arithmetic. Same K split, same partials, same reduce: the MFMA sees the operands the f16
// copy would have given it, in the same order.
//
// Weight movement: per wave a ring of SKQ_NS stages of SKQ_KS = 256 K columns of its 16
// rows, filled by LDS-DMA (global_load_lds_dwordx4), no workgroup barrier in the loop, one
// counted vmcnt per stage. A stage row is RB bytes:
//   fp8 / e4m3  256 B (16 chunks of 16 B): 4 DMA instructions of 4 rows x 256 B, the f16
//               form's geometry byte for byte; a step's fragment is 8 B of chunk 2 j + (q >> 1)
//   q4          128 B (8 nibble blocks = 8 scale groups): 2 DMA instructions of 8 rows x 128 B
//               plus one dword DMA that brings the 8 f16 scales of each of the 16 rows (16 B
//               per row, lane l: row l >> 2, dword l & 3); a step is block j = one scale
//               group, the lane's fragment its word q
// The 16-byte chunks of a row are XOR-swizzled on the source side (slot s holds chunk
// s ^ swz(row)) so the 16-row fragment reads cover all 64 banks: swz = row & 15 for 256-byte
// rows, (row >> 1) & 7 for 128-byte rows (rows r and r + 1 are 32 banks apart there).
// LDS: the A chunk (<= 32 KB) + 48 KB (fp8, e4m3) or 27 KB (q4): two workgroups per CU.
#pragma once

#include "prefill_skinny.h"

namespace pf {

// B row policies over rows of `rb` bytes (yalm_row_bytes of the format): prefill_gemm.h's
// BRowsPlain (q | k | v segments end to end) and BRowsGlu (W1 / W3 rows interleaved per wave)
struct BRowsPlainQ {
	BSrc src;
	size_t rb;
	static constexpr int COLS_PER_TILE_DIV = 1;
	__device__ __forceinline__ const char *row(int n0, int r) const {
		const int n = n0 + r;
		const int s = n < src.end[0] ? 0 : (n < src.end[1] ? 1 : 2);
		const int start = s == 0 ? 0 : src.end[s - 1];
		return (const char *)src.p[s] + (size_t)(n - start) * rb;
	}
};
template <int TN>
struct BRowsGluQ {
	const char *w1, *w3;
	size_t rb;
	static constexpr int COLS_PER_TILE_DIV = 2;
	__device__ __forceinline__ const char *row(int h0, int r) const {
		const int wc = r / TN, within = r % TN;
		const int hc = h0 + wc * (TN / 2) + within % (TN / 2);
		return (within / (TN / 2) ? w3 : w1) + (size_t)hc * rb;
	}
};

constexpr int SKQ_KS = 256; // K columns per stage
constexpr int SKQ_NS = 3;   // ring stages
template <class WT>
struct SkqGeo {
	static constexpr int RB = WT::Q4 ? SKQ_KS / 2 : SKQ_KS; // stage bytes per row
	static constexpr int CPR = RB / 16;                      // 16-byte chunks per stage row
	static constexpr int RPI = 64 / CPR;                     // rows per DMA instruction
	static constexpr int NI = 16 / RPI;                      // DMA instructions per wave stage
	static constexpr int STAGE = SK_ROWS * RB;               // bytes per stage
	static constexpr int SCALES = WT::Q4 ? SK_ROWS * 16 : 0; // q4: bytes of scales per stage
	static constexpr size_t RING_BYTES = (size_t)SKQ_NS * (STAGE + SCALES);
	__device__ static __forceinline__ int swz(int row) { return CPR == 16 ? row & 15 : (row >> 1) & 7; }
};

__device__ __forceinline__ half8_t skq_pack(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
	const u32x4_t v = {a, b, c, d};
	return __builtin_bit_cast(half8_t, v);
}
// 8 E5M2 codes (lo: elements 0..3, hi: 4..7) -> 8 f16: the byte b is the f16 with bits b << 8
__device__ __forceinline__ half8_t skq_frag_e5m2(uint32_t lo, uint32_t hi) {
	return skq_pack(((lo & 0xffu) << 8) | ((lo & 0xff00u) << 16), ((lo & 0xff0000u) >> 8) | (lo & 0xff000000u),
	                ((hi & 0xffu) << 8) | ((hi & 0xff00u) << 16), ((hi & 0xff0000u) >> 8) | (hi & 0xff000000u));
}
// 8 E4M3 codes of a row with scale sc -> f16(code * sc), the arithmetic of e4m3_to_f16_kernel
__device__ __forceinline__ half8_t skq_frag_e4m3(uint32_t lo, uint32_t hi, float sc) {
	const float2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
	const float2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
	return skq_pack((uint32_t)f2h(a[0] * sc) | ((uint32_t)f2h(a[1] * sc) << 16),
	                (uint32_t)f2h(b[0] * sc) | ((uint32_t)f2h(b[1] * sc) << 16),
	                (uint32_t)f2h(c[0] * sc) | ((uint32_t)f2h(c[1] * sc) << 16),
	                (uint32_t)f2h(d[0] * sc) | ((uint32_t)f2h(d[1] * sc) << 16));
}
// one q4 word (8 nibbles) of a group with f16 scale bits s -> (u - 8) * s, the arithmetic of q4_to_f16_kernel
__device__ __forceinline__ half8_t skq_frag_q4(uint32_t w, uint16_t s) {
	const _Float16 sh = __builtin_bit_cast(_Float16, s);
	const half2_t s2 = {sh, sh};
	half2_t h[4];
	q4_pairs(w, h);
	return skq_pack(__builtin_bit_cast(uint32_t, h[0] * s2), __builtin_bit_cast(uint32_t, h[1] * s2),
	                __builtin_bit_cast(uint32_t, h[2] * s2), __builtin_bit_cast(uint32_t, h[3] * s2));
}

// C[:, c0 .. c0 + N) partials as skinny_gemm_lds_kernel leaves them; bm: a *Q row policy over
// rows of format WT (WF8, WE4M3, WQ4), kb elements wide. KC % SKQ_KS == 0 (the host's K split).
template <int MT, class BMAP, class WT>
__global__ __launch_bounds__(256) void skinny_gemm_wq_kernel(const uint16_t *__restrict__ A, int lda, int T, int K,
                                                             int kb, BMAP bm, int N, int KC, int c0, int Np,
                                                             float *__restrict__ part) {
	extern __shared__ __attribute__((aligned(16))) uint16_t sm[];
	using G = SkqGeo<WT>;
	constexpr int TP = 16 * MT;
	constexpr bool Q4 = WT::Q4;
	uint16_t *const as = sm;                              // [TP][KC], swizzled as skinny_gemm_kernel
	char *const ring = (char *)(sm + (size_t)TP * KC);    // [SKQ_NS][64 rows][RB]
	char *const sring = ring + SKQ_NS * G::STAGE;         // q4: [SKQ_NS][64 rows][8 f16 scales]
	const int nblk = N / SK_ROWS;
	const int nb = blockIdx.x % nblk, ks = blockIdx.x / nblk;
	const int k0 = ks * KC;
	const int tid = threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int cb = c0 + nb * SK_ROWS;       // the workgroup's first B row (output column)
	const int col = cb + 16 * wave;         // the wave's
	const int kw0 = k0 < kb ? k0 : k0 - kb; // B wrap (a K chunk never straddles kb)
	const int nst = KC / SKQ_KS;
	const int n = lane & 15, q = lane >> 4;
	const int tile = cb / BMAP::COLS_PER_TILE_DIV;
	// e4m3: the row's f32 scale sits behind its kb codes
	float rscale = 1.0f;
	if constexpr (WT::ROW_SCALE)
		rscale = *(const float *)(bm.row(tile, 16 * wave + n) + kb);
	// DMA geometry: instruction i of a stage covers the wave's rows RPI i .. RPI i + RPI - 1, lane
	// l row RPI i + l / CPR, LDS slot l % CPR <- source chunk (l % CPR) ^ swz(row)
	const char *src[G::NI];
#pragma unroll
	for (int i = 0; i < G::NI; ++i) {
		const int rr = G::RPI * i + lane / G::CPR;
		src[i] = bm.row(tile, 16 * wave + rr) + (Q4 ? kw0 >> 1 : kw0) + 16 * ((lane % G::CPR) ^ G::swz(rr));
	}
	// q4: the scales of group kw0 / 32 + 8 st .. + 7 of row l >> 2, dword l & 3 of their 16 bytes
	const char *ssrc = nullptr;
	if constexpr (Q4)
		ssrc = bm.row(tile, 16 * wave + (lane >> 2)) + WQ4::scale_off(kb, kw0 >> 5) + 4 * (lane & 3);
	char *const wring = ring + wave * 16 * G::RB; // this wave's rows in every stage
	char *const wsring = sring + wave * 16 * 16;
	auto issue = [&](int st, int slot) { // stage st (clamped: past the chunk it re-reads the last stage, an L2 hit)
		const int sc = st < nst ? st : nst - 1;
		char *dst = wring + slot * G::STAGE;
#pragma unroll
		for (int i = 0; i < G::NI; ++i)
			__builtin_amdgcn_global_load_lds((const void *)(src[i] + sc * G::RB), (YALM_LDS void *)(dst + i * 1024), 16, 0,
			                                 0);
		if constexpr (Q4)
			__builtin_amdgcn_global_load_lds((const void *)(ssrc + sc * 16), (YALM_LDS void *)(wsring + slot * G::SCALES),
			                                 4, 0, 0);
	};
	issue(0, 0);
	issue(1, 1);
	sk_stage_a<MT>(as, A, lda, T, k0, KC);
	__syncthreads();
	f32x4_t acc[MT];
#pragma unroll
	for (int m = 0; m < MT; ++m)
		acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
	int slot = 0, fill = 2; // stage st sits in slot st % SKQ_NS, stage st + 2 goes to (st + 2) % SKQ_NS
	for (int st = 0; st < nst; ++st) {
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // stage st - 1's B reads are done...
		issue(st + 2, fill);                               // ...before its slot is re-staged
		if constexpr (Q4)
			asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); // stage st landed (2 stages x 3 behind it)
		else
			asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); // (2 stages x 4)
		const char *bst = wring + slot * G::STAGE + n * G::RB;
		u32x4_t sv = {0u, 0u, 0u, 0u};
		if constexpr (Q4)
			sv = *(const u32x4_t *)(wsring + slot * G::SCALES + 16 * n);
#pragma unroll
		for (int j = 0; j < SKQ_KS / 32; ++j) {
			half8_t b;
			if constexpr (Q4) {
				const uint32_t w = *(const uint32_t *)(bst + 16 * (j ^ G::swz(n)) + 4 * q);
				const uint32_t s = sv[j >> 1];
				b = skq_frag_q4(w, (uint16_t)(j & 1 ? s >> 16 : s));
			} else {
				const uint2 w = *(const uint2 *)(bst + 16 * ((2 * j + (q >> 1)) ^ G::swz(n)) + 8 * (q & 1));
				if constexpr (WT::ROW_SCALE)
					b = skq_frag_e4m3(w.x, w.y, rscale);
				else
					b = skq_frag_e5m2(w.x, w.y);
			}
#pragma unroll
			for (int m = 0; m < MT; ++m) {
				const half8_t a = sk_afrag<MT>(as, KC, 16 * m + n, st * SKQ_KS + 32 * j + 8 * q);
				acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[m], 0, 0, 0);
			}
		}
		slot = slot + 1 == SKQ_NS ? 0 : slot + 1;
		fill = fill + 1 == SKQ_NS ? 0 : fill + 1;
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the clamped tail stages, before the wave exits
	float *pp = part + (size_t)ks * TP * Np;
#pragma unroll
	for (int m = 0; m < MT; ++m)
#pragma unroll
		for (int r = 0; r < 4; ++r)
			pp[(size_t)(16 * m + crow16(r, lane)) * Np + col + n] = acc[m][r];
}

} // namespace pf
