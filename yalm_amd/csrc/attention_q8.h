// attention_q8.h — decode attention over the opt-in 8-bit shadow of the KV cache ("q8 KV",
// DESIGN.md §22), and the quantiser that fills the shadow.
//
// Format: every (cache row, kv head) has head_dim codes and one f32 scale, for K and for V. In
// float32: a = max|x| over the head's row, inv = 127 / a, c = clamp(rint(x * inv), -127, 127),
// s = a / 127 (a == 0: s = 0 and every c = 0); the value is c * s. A code is stored offset-binary,
// c + 128 in one byte. Per layer: codes [max_seq_len][n_kv_heads][head_dim] u8 and scales
// [max_seq_len][n_kv_heads] f32. models.kv_q8_quantize is the same statement in numpy.
//
// attn_decode_q8_kernel computes what attn_decode_kernel (attention.h) computes; only the rows it
// reads differ. Rows < kv_sink (rotated in place in f16 by every step's QKV launch) and the step's
// own row kv_pos come from the f16 cache, every other live row from the shadow. Head mode, key
// mode, the per-chunk buffer descriptors, the {value, tag} partials and the merger
// (attn_merge_body, as it stands) are attention.h's.
//
// Data movement: a row of head_dim codes is head_dim / 16 lanes x 16 bytes, so a 64-key chunk of
// head_dim 128 is two 16-byte loads per lane for K and two for V (the f16 kernel: four and four),
// plus one 4-byte scale per row. A lane unpacks its 16 codes to f32 (v_cvt_f32_ubyte0..3 and one
// subtract: exact), runs the G dot products of its 16 dims on the VALU and the row's lanes meet
// by DPP; the K scale and 1 / sqrt(head_dim) are applied once per key to the reduced dot, the V
// scale is folded into the key's probability, so no value is ever multiplied by its scale.
// The three f16 rows at most (two sinks, kv_pos) replace their lane's unpacked codes inside a
// divergent branch that only the lanes owning such a row enter.
//
// Unit 0 of every kv head also quantises row kv_pos into the shadow for the later steps; no
// workgroup of the launch uses that shadow row, so there is no hand-off inside the launch.
#pragma once

#include "attention.h"

// lanes per row (16 codes each), rows per wave-instruction, rows per workgroup-instruction,
// rows per lane and chunk
template <int D>
struct Q8Geo {
	static_assert(D == 64 || D == 128, "q8 kv: head_dim 64 or 128");
	static constexpr int LPK = D / 16, KPW = 64 / LPK, RSTEP = ATTN_WAVES * KPW, NK = attn_chunk<D>() / RSTEP;
};

// the 16 codes of one 16-byte piece as exact f32 values c = byte - 128
__device__ __forceinline__ void q8_unpack(const u32x4_t &w, float *o) {
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const uint32_t v = w[i];
		o[4 * i + 0] = (float)(v & 0xFFu) - 128.0f;
		o[4 * i + 1] = (float)((v >> 8) & 0xFFu) - 128.0f;
		o[4 * i + 2] = (float)((v >> 16) & 0xFFu) - 128.0f;
		o[4 * i + 3] = (float)(v >> 24) - 128.0f;
	}
}

// 16 consecutive f16 values at p (16-byte aligned) as f32
__device__ __forceinline__ void q8_load_f16x16(const uint16_t *p, float *o) {
	const u32x4_t a = load16(p), b = load16(p + 8);
	WF16::unpack(a, o);
	WF16::unpack(b, o + 8);
}

// One (row, kv head) of the f16 caches into the shadow, by one whole wave: lanes 0 .. D/16 - 1
// take K, lanes 16 .. 16 + D/16 - 1 take V, 16 values each; the row's absmax meets by DPP inside
// the lanes' 16-lane row (idle lanes hold zeros and only follow along), the codes leave as one
// 16-byte store per lane. Every lane of the wave must call it.
template <int D>
__device__ __forceinline__ void kvq8_quant_row(const uint16_t *kc, const uint16_t *vc, uint8_t *kq, float *ks,
                                               uint8_t *vq, float *vs, int n_kv_heads, int row, int g) {
	constexpr int LPK = Q8Geo<D>::LPK;
	const int lane = threadIdx.x & 63, piece = lane & 15;
	const bool isv = lane & 16, active = lane < 32 && piece < LPK;
	const size_t hr = (size_t)row * n_kv_heads + g;
	const size_t o = hr * D + (size_t)(active ? piece : 0) * 16;
	float x[16];
#pragma unroll
	for (int e = 0; e < 16; ++e)
		x[e] = 0.0f;
	if (active)
		q8_load_f16x16((isv ? vc : kc) + o, x);
	float a = 0.0f;
#pragma unroll
	for (int e = 0; e < 16; ++e)
		a = fmaxf(a, fabsf(x[e]));
	a = fmaxf(a, dpp<0xB1>(a)); // quad_perm xor 1, xor 2, then (8 lanes) row_half_mirror
	a = fmaxf(a, dpp<0x4E>(a));
	if constexpr (LPK == 8)
		a = fmaxf(a, dpp<0x141>(a));
	const float inv = __fdiv_rn(127.0f, a);
	u32x4_t w;
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		uint32_t p = 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const float r = fminf(fmaxf(rintf(x[4 * j + k] * inv), -127.0f), 127.0f);
			const int c = a > 0.0f ? (int)r : 0;
			p |= (uint32_t)(c + 128) << (8 * k);
		}
		w[j] = p;
	}
	if (active) {
		*(u32x4_t *)((isv ? vq : kq) + o) = w;
		if (piece == 0)
			(isv ? vs : ks)[hr] = a > 0.0f ? __fdiv_rn(a, 127.0f) : 0.0f;
	}
}

// Rows [r0, r0 + n) of one layer's f16 caches into its shadow: one wave per (row, kv head).
template <int D>
__global__ __launch_bounds__(ATTN_THREADS) void kv_quant_rows_kernel(const uint16_t *__restrict__ kc,
                                                                     const uint16_t *__restrict__ vc,
                                                                     uint8_t *__restrict__ kq, float *__restrict__ ks,
                                                                     uint8_t *__restrict__ vq, float *__restrict__ vs,
                                                                     int n_kv_heads, int r0, int n) {
	const int w = blockIdx.x * ATTN_WAVES + (threadIdx.x >> 6);
	if (w >= n * n_kv_heads)
		return; // (the whole wave)
	kvq8_quant_row<D>(kc, vc, kq, ks, vq, vs, n_kv_heads, r0 + w / n_kv_heads, w % n_kv_heads);
}

// One lane's shadow rows of a 64-key chunk: KvRows (attention.h) over the codes, with a second
// descriptor pair for the rows' scales. Each chunk gets its own descriptors, num_records = the
// chunk's rows inside the cache (0 when the chunk is not live): rows past the cache read zero.
template <int D>
struct KvRowsQ8 {
	static constexpr int LPK = Q8Geo<D>::LPK, KPW = Q8Geo<D>::KPW, RSTEP = Q8Geo<D>::RSTEP, NK = Q8Geo<D>::NK;
	const char *kb, *vb, *ksb, *vsb;
	uint32_t rowb, srowb, msl; // bytes per row of codes / of scales, rows per layer
	uint32_t voff[NK], soff[NK];
	__device__ __forceinline__ KvRowsQ8(const uint8_t *kq, const float *ks, const uint8_t *vq, const float *vs,
	                                    int n_kv_heads, int max_seq_len, int g) {
		const int lane = threadIdx.x & 63;
		const int tl0 = (threadIdx.x >> 6) * KPW + lane / LPK, piece = lane % LPK;
		auto uni = [](const void *p) { // provably wave-uniform descriptor inputs (KvRows)
			const uint64_t a = (uint64_t)p;
			const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
			const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
			return (const char *)(((uint64_t)hi << 32) | lo);
		};
		rowb = (uint32_t)__builtin_amdgcn_readfirstlane(n_kv_heads * D);
		srowb = (uint32_t)__builtin_amdgcn_readfirstlane(n_kv_heads * 4);
		msl = (uint32_t)__builtin_amdgcn_readfirstlane(max_seq_len);
		kb = uni(kq), vb = uni(vq), ksb = uni(ks), vsb = uni(vs);
#pragma unroll
		for (int i = 0; i < NK; ++i) {
			voff[i] = (uint32_t)(tl0 + i * RSTEP) * rowb + (uint32_t)(g * D + piece * 16);
			soff[i] = (uint32_t)(tl0 + i * RSTEP) * srowb + (uint32_t)g * 4;
		}
	}
	// the chunk at row t0 (nothing when !live); t0 and live from scalar values (KvRows::load)
	__device__ __forceinline__ void load(int t0, bool live, u32x4_t (&kw)[NK], u32x4_t (&vw)[NK], float (&ksc)[NK],
	                                     float (&vsc)[NK]) const {
		const uint32_t t = (uint32_t)t0;
		const int rows = min((int)msl - t0, attn_chunk<D>());
		const int nrec = live ? rows * (int)rowb : 0, nsrec = live ? rows * (int)srowb : 0;
		const uint64_t o = (uint64_t)t * rowb, so = (uint64_t)t * srowb;
		const __amdgpu_buffer_rsrc_t kr = __builtin_amdgcn_make_buffer_rsrc((void *)(kb + o), (short)0, nrec, 0x00020000);
		const __amdgpu_buffer_rsrc_t vr = __builtin_amdgcn_make_buffer_rsrc((void *)(vb + o), (short)0, nrec, 0x00020000);
		const __amdgpu_buffer_rsrc_t ksr = __builtin_amdgcn_make_buffer_rsrc((void *)(ksb + so), (short)0, nsrec, 0x00020000);
		const __amdgpu_buffer_rsrc_t vsr = __builtin_amdgcn_make_buffer_rsrc((void *)(vsb + so), (short)0, nsrec, 0x00020000);
#pragma unroll
		for (int i = 0; i < NK; ++i) {
			kw[i] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(kr, voff[i], 0, 0));
			vw[i] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(vr, voff[i], 0, 0));
			ksc[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ksr, soff[i], 0, 0));
			vsc[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(vsr, soff[i], 0, 0));
		}
	}
};

// The caches and the step's row indices an attention workgroup works on.
struct Q8Caches {
	const uint16_t *kc, *vc; // f16 caches: rows < kv_sink and row kv_pos
	const uint8_t *kq, *vq;  // shadow codes
	const float *ks, *vs;    // shadow scales
};

// attn_core (attention.h) over the shadow: query heads hq0 .. hq0 + Gh - 1 of kv head g over the
// key chunks c_first, c_first + cstride, ... < ns; the head outputs (final_out) or one partial per
// head at split s_part. Lane (row group, piece) holds 16 dims of NK rows; per wave a running
// (max, sum, P.V) with the flash-decoding rescale, the next chunk's rows loaded before the
// current one is computed, one barrier at the end to combine the 4 waves.
template <int D, int GT, int GQ>
__device__ __forceinline__ void attn_q8_core(int g, int hq0, int Gh, int c_first, int cstride, int ns, bool final_out,
                                             int s_part, const float4_t (&qv)[(GQ * D + 255) / 256],
                                             u32x4_t (&kA)[Q8Geo<D>::NK], u32x4_t (&vA)[Q8Geo<D>::NK],
                                             float (&ksA)[Q8Geo<D>::NK], float (&vsA)[Q8Geo<D>::NK], int kv_len,
                                             int kv_sink, int kv_pos, const Q8Caches &cc, int n_heads, int n_kv_heads,
                                             int max_seq_len, int nsplit, unsigned long long *part, unsigned ptag,
                                             float *out) {
	constexpr int CHUNK = attn_chunk<D>();
	constexpr int LPK = Q8Geo<D>::LPK, KPW = Q8Geo<D>::KPW, RSTEP = Q8Geo<D>::RSTEP, NK = Q8Geo<D>::NK;
	constexpr int QL = (GQ * D + 255) / 256;
	c_first = __builtin_amdgcn_readfirstlane(c_first);
	cstride = __builtin_amdgcn_readfirstlane(cstride);
	ns = __builtin_amdgcn_readfirstlane(ns);
	kv_len = __builtin_amdgcn_readfirstlane(kv_len);
	kv_sink = __builtin_amdgcn_readfirstlane(kv_sink);
	kv_pos = __builtin_amdgcn_readfirstlane(kv_pos);
	__shared__ __attribute__((aligned(16))) float qs[ATTN_WAVES][GQ * D];
	__shared__ float wsum[ATTN_WAVES][GT][D]; // per-wave P.V sums
	__shared__ float wml[ATTN_WAVES][GT][2];  // per-wave (max, sum of exp)

	const int G = n_heads / n_kv_heads;
	const int hb = g * G + hq0;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
	const int sub = lane / LPK, piece = lane % LPK;
	const int tl0 = wave * KPW + sub;

	const KvRowsQ8<D> rows(cc.kq, cc.ks, cc.vq, cc.vs, n_kv_heads, max_seq_len, g);
	auto load_kv = [&](int t0, u32x4_t (&kw)[NK], u32x4_t (&vw)[NK], float (&ksc)[NK], float (&vsc)[NK]) {
		rows.load(t0, t0 < kv_len, kw, vw, ksc, vsc);
	};
	// q through this wave's own LDS copy (attn_core): dims piece * 16 .. + 16 of every head
	const int gq = G * D;
#pragma unroll
	for (int j = 0; j < QL; ++j)
		if ((j * 64 + lane) * 4 < gq)
			*(float4_t *)&qs[wave][(j * 64 + lane) * 4] = qv[j];
	float qr[GT][16];
#pragma unroll
	for (int h = 0; h < GT; ++h) {
		const float *qp = &qs[wave][(hq0 + (h < Gh ? h : 0)) * D + piece * 16];
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const float4_t a = *(const float4_t *)(qp + 4 * j);
			qr[h][4 * j] = a[0], qr[h][4 * j + 1] = a[1], qr[h][4 * j + 2] = a[2], qr[h][4 * j + 3] = a[3];
		}
	}
	const float sq = sqrtf((float)D);
	// this lane's 16 dims of f16 cache row t (a sink row or kv_pos)
	const size_t hoff = (size_t)g * D + piece * 16;
	auto f16_row = [&](const uint16_t *c, int t, float *o) { q8_load_f16x16(c + (size_t)t * n_kv_heads * D + hoff, o); };

	float acc[GT * 16]; // element e of head h at dim piece * 16 + e, not yet reduced across row groups
#pragma unroll
	for (int k = 0; k < GT * 16; ++k)
		acc[k] = 0.0f;
	float mw[GT], lw[GT];
#pragma unroll
	for (int h = 0; h < GT; ++h)
		mw[h] = -FLT_MAX, lw[h] = 0.0f;

	auto chunk = [&](auto first, const u32x4_t (&kw)[NK], const u32x4_t (&vw)[NK], const float (&ksc)[NK],
	                 const float (&vsc)[NK], int t0) {
		constexpr bool FIRST = decltype(first)::value;
		const int nt = min(CHUNK, kv_len - t0);
		float sv[NK][GT];
		bool valid[NK], exact[NK];
#pragma unroll
		for (int i = 0; i < NK; ++i) {
			const int tl = tl0 + i * RSTEP, t = t0 + tl;
			valid[i] = tl < nt;
			exact[i] = valid[i] && (t < kv_sink || t == kv_pos); // this row is read from the f16 cache
			float kf[16], s = ksc[i];
			q8_unpack(kw[i], kf);
			if (exact[i]) {
				f16_row(cc.kc, t, kf);
				s = 1.0f;
			}
#pragma unroll
			for (int h = 0; h < GT; ++h) {
				float d = 0.0f;
#pragma unroll
				for (int e = 0; e < 16; ++e)
					d = fmaf(qr[h][e], kf[e], d);
				sv[i][h] = attn_row_sum<LPK>(d) * s / sq; // (rows past kv_len: anything, masked below)
			}
		}
#pragma unroll
		for (int h = 0; h < GT; ++h) {
			float m = -FLT_MAX;
#pragma unroll
			for (int i = 0; i < NK; ++i)
				m = valid[i] ? fmaxf(m, sv[i][h]) : m;
			m = attn_wave_red<LPK, true>(m);
			const float Mn = FIRST ? m : fmaxf(mw[h], m);
			float l = 0.0f;
#pragma unroll
			for (int i = 0; i < NK; ++i) {
				sv[i][h] = valid[i] ? expf(sv[i][h] - Mn) : 0.0f;
				l += sv[i][h];
			}
			l = attn_wave_red<LPK, false>(l);
			if constexpr (FIRST) {
				lw[h] = l;
			} else {
				const float corr = expf(mw[h] - Mn);
				lw[h] = fmaf(lw[h], corr, l);
#pragma unroll
				for (int e = 0; e < 16; ++e)
					acc[h * 16 + e] *= corr;
			}
			mw[h] = Mn;
		}
#pragma unroll
		for (int i = 0; i < NK; ++i) {
			float vf[16], s = valid[i] ? vsc[i] : 0.0f; // (codes are finite whatever the bytes; the scale may not be)
			q8_unpack(vw[i], vf);
			if (exact[i]) {
				f16_row(cc.vc, t0 + tl0 + i * RSTEP, vf);
				s = 1.0f;
			}
#pragma unroll
			for (int h = 0; h < GT; ++h) {
				const float p = sv[i][h] * s; // the V scale folded into the key's probability
#pragma unroll
				for (int e = 0; e < 16; ++e)
					acc[h * 16 + e] = fmaf(p, vf[e], acc[h * 16 + e]);
			}
		}
	};

	// chunks c_first, c_first + cstride, ...: the next chunk's rows are requested before the current
	// one is computed; the loads stay unconditional (a dead one moves no data), as in attn_core
	using T_ = std::true_type;
	using F_ = std::false_type;
	if (c_first + cstride >= ns) {
		chunk(T_{}, kA, vA, ksA, vsA, c_first * CHUNK);
	} else {
		u32x4_t kB[NK], vB[NK];
		float ksB[NK], vsB[NK];
		load_kv((c_first + cstride) * CHUNK, kB, vB, ksB, vsB);
		chunk(T_{}, kA, vA, ksA, vsA, c_first * CHUNK);
		for (int c = c_first + cstride;; c += 2 * cstride) { // the B registers hold chunk c
			load_kv((c + cstride) * CHUNK, kA, vA, ksA, vsA);
			chunk(F_{}, kB, vB, ksB, vsB, c * CHUNK);
			if (c + cstride >= ns)
				break;
			load_kv((c + 2 * cstride) * CHUNK, kB, vB, ksB, vsB);
			chunk(F_{}, kA, vA, ksA, vsA, (c + cstride) * CHUNK);
			if (c + 2 * cstride >= ns)
				break;
		}
	}

	// ---- this wave's (max, sum) and its P.V sums over its row groups, into LDS: the row groups
	// inside each DPP row first, then across the 4 DPP rows transposed (sum4_rows): for value
	// group k, lane `piece` of DPP row r holds value 4 k + r of that piece summed over the wave
	if (lane < Gh) {
		float m = mw[0], l = lw[0];
#pragma unroll
		for (int h = 1; h < GT; ++h)
			if (lane == h)
				m = mw[h], l = lw[h];
		wml[wave][lane][0] = m;
		wml[wave][lane][1] = l;
	}
#pragma unroll
	for (int k = 0; k < GT * 16; ++k)
		acc[k] = attn_fold_row<LPK, false>(acc[k]);
#pragma unroll
	for (int k = 0; k < GT * 4; ++k) {
		const float v4[4] = {acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
		const float s = sum4_rows(v4);
		const int idx = 4 * k + (lane >> 4), h = idx >> 4, e = idx & 15;
		if (h < Gh && (lane & 15) < LPK)
			wsum[wave][h][(lane & 15) * 16 + e] = s;
	}
	__syncthreads();

	// ---- combine the waves (fixed order): o = sum_w e^(m_w - M) o_w, L likewise
	for (int i = tid; i < Gh * D; i += ATTN_THREADS) {
		const int h = i / D, d = i % D;
		float M = wml[0][h][0];
#pragma unroll
		for (int w = 1; w < ATTN_WAVES; ++w)
			M = fmaxf(M, wml[w][h][0]);
		float o = 0.0f, L = 0.0f;
#pragma unroll
		for (int w = 0; w < ATTN_WAVES; ++w) {
			const float c = expf(wml[w][h][0] - M); // 0 for a wave without valid rows
			o = fmaf(wsum[w][h][d], c, o);
			L = fmaf(wml[w][h][1], c, L);
		}
		if (final_out) {
			out[(size_t)(hb + h) * D + d] = o / L;
		} else { // this workgroup's partial (o[D], M, L per head) as tagged granules
			const size_t pp = ((size_t)(hb + h) * nsplit + s_part) * (D + 2);
			attn_out<true>((float *)part, pp + d, o, ptag);
			if (d == 0) {
				attn_out<true>((float *)part, pp + D, M, ptag);
				attn_out<true>((float *)part, pp + D + 1, L, ptag);
			}
		}
	}
}

// One attention workgroup, unit u of kv head g's S + G - 1 units: attn_decode_body's head and split
// units and its two modes, over the shadow.
template <int D, int GT>
__device__ __forceinline__ void attn_q8_body(int g, int u, int S, int head_max, const float *q, const Q8Caches &cc,
                                             const StepState *step, int n_heads, int n_kv_heads, int max_seq_len,
                                             int nsplit, unsigned long long *part, unsigned ptag, float *out) {
	constexpr int CHUNK = attn_chunk<D>();
	constexpr int NK = Q8Geo<D>::NK;
	constexpr int QL = (GT * D + 255) / 256;
	const int G = n_heads / n_kv_heads;
	const int lane = threadIdx.x & 63;
	const bool hu = u < G;            // head unit (query head u)
	const int s = hu ? 0 : u - G + 1; // key split
	// speculative loads: q of the group's G heads, a head unit's chunk 0 (zeros past the cache)
	const int gq = G * D;
	float4_t qv[QL];
#pragma unroll
	for (int j = 0; j < QL; ++j)
		qv[j] = *(const float4_t *)(q + (size_t)g * gq + min((j * 64 + lane) * 4, gq - 4));
	u32x4_t kA[NK], vA[NK];
	float ksA[NK], vsA[NK];
	const KvRowsQ8<D> rows(cc.kq, cc.ks, cc.vq, cc.vs, n_kv_heads, max_seq_len, g);
	rows.load(0, hu, kA, vA, ksA, vsA);
	const int kv_len = step->kv_len, kv_sink = step->kv_sink, kv_pos = step->kv_pos;
	const int ns = (kv_len + CHUNK - 1) / CHUNK;
	if (ns <= head_max) { // head mode
		if (hu)
			attn_q8_core<D, 1, GT>(g, u, 1, 0, 1, ns, true, 0, qv, kA, vA, ksA, vsA, kv_len, kv_sink, kv_pos, cc, n_heads,
			                       n_kv_heads, max_seq_len, nsplit, part, ptag, out);
		return;
	}
	if (s * CHUNK >= kv_len)
		return;
	if (!hu)
		rows.load(s * CHUNK, true, kA, vA, ksA, vsA);
	if (hu) // key mode: split 0 by the head units, one query head each
		attn_q8_core<D, 1, GT>(g, u, 1, 0, S, ns, false, 0, qv, kA, vA, ksA, vsA, kv_len, kv_sink, kv_pos, cc, n_heads,
		                       n_kv_heads, max_seq_len, nsplit, part, ptag, out);
	else
		attn_q8_core<D, GT, GT>(g, 0, G, s, S, ns, false, s, qv, kA, vA, ksA, vsA, kv_len, kv_sink, kv_pos, cc, n_heads,
		                        n_kv_heads, max_seq_len, nsplit, part, ptag, out);
}

// Grid as attn_decode_kernel's: n_kv * (S + G - 1) attention workgroups (b = g + n_kv * u), then
// n_kv * G mergers. Unit 0 of each kv head ends by quantising row kv_pos of its head.
template <int D, int GT>
__global__ __launch_bounds__(ATTN_THREADS) void attn_decode_q8_kernel(
    const float *__restrict__ q, const uint16_t *__restrict__ kc, const uint16_t *__restrict__ vc,
    uint8_t *__restrict__ kq, float *__restrict__ ks, uint8_t *__restrict__ vq, float *__restrict__ vs,
    const StepState *__restrict__ step, int n_heads, int n_kv_heads, int max_seq_len, int nsplit, int S, int head_max,
    unsigned long long *__restrict__ part, int layer, int n_layers, unsigned *__restrict__ err,
    float *__restrict__ out) {
	const int b = blockIdx.x, units = n_kv_heads * (S + n_heads / n_kv_heads - 1);
	const unsigned ptag = attn_part_tag(step, layer, n_layers);
	if (b < units) {
		const int g = b % n_kv_heads, u = b / n_kv_heads;
		const Q8Caches cc{kc, vc, kq, vq, ks, vs};
		attn_q8_body<D, GT>(g, u, S, head_max, q, cc, step, n_heads, n_kv_heads, max_seq_len, nsplit, part, ptag, out);
		if (u == 0 && threadIdx.x < 64)
			kvq8_quant_row<D>(kc, vc, kq, ks, vq, vs, n_kv_heads, step->kv_pos, g);
	} else {
		attn_merge_body<D, false>((b - units) % n_kv_heads, (b - units) / n_kv_heads, S, head_max, step, n_heads,
		                          n_kv_heads, max_seq_len, nsplit, part, ptag, err, out, nullptr);
	}
}
