// batch.h — batched decode: up to ROWS_MAX_T independent sequences per pass over the weights.
//
// Row s of a step belongs to sequence s: it has its own KV cache set, its own StepState (token,
// pos, n_gen, epoch: the sequence's state AND the row state of the step), its own token buffer
// and its own split-KV partial buffer. The weight matrices are streamed once for all rows by the
// multi-row GEMV (gemv_rows.h), unchanged: a row of gemv_rows_kernel depends on neither T nor the
// other rows, so row s computes what a one-row forward of its token at its position computes,
// bit for bit. A step is
//   begin (1) -> per layer QKV, [q / k norm], attention, Wo, W1|W3, W2 -> norm + logits (1) -> commit (1)
// with the attention of all sequences as ONE launch (attn_decode_batch_kernel: 3 + 5 L launches,
// + L with the q / k norm) or as one launch per sequence of the decode kernel (3 + L (4 + n_seq)).
// No ring wrap and no sink rotation: pos < max_seq_len for every row (the host checks).
#pragma once

#include <type_traits>

#include "attention.h"
#include "device_common.h"
#include "gemv_rows.h"
#include "misc_kernels.h"
#include "sampler.h"

// Per-sequence device pointers, passed by value (kernel arguments).
struct BatchKV {
	uint16_t *k[ROWS_MAX_T], *v[ROWS_MAX_T]; // one layer's K and V cache of every sequence
};
struct BatchTok {
	int *p[ROWS_MAX_T]; // every sequence's token buffer
};
struct BatchPart {
	unsigned long long *p[ROWS_MAX_T]; // every sequence's split-KV partial buffer
};

// The host's (token, pos) of every sequence (kernel arguments: no host buffer to outlive the call).
__global__ void batch_set_kernel(StepState *seq, int n_seq, int t0, int t1, int t2, int t3, int p0, int p1, int p2,
                                 int p3, int reset_gen) {
	const int tok[ROWS_MAX_T] = {t0, t1, t2, t3}, pos[ROWS_MAX_T] = {p0, p1, p2, p3};
	for (int s = 0; s < n_seq; ++s) {
		seq[s].token = tok[s];
		seq[s].pos = pos[s];
		if (reset_gen)
			seq[s].n_gen = 0;
	}
}

// First launch of a step, one workgroup per sequence: rows_begin_kernel (spec.h) with the row's
// (token, pos) read from its own sequence state. kv_pos = pos, kv_len = pos + 1, the rope table
// of pos, a new epoch of the sequence's own counter (its partial buffer is its own, so the tags
// of two sequences never meet) and x[s] = embedding[token].
template <class WT>
__global__ __launch_bounds__(256) void batch_begin_kernel(StepState *seq, const void *__restrict__ emb, int dim,
                                                          float *__restrict__ x, const float *__restrict__ inv_freq,
                                                          int half) {
	const int s = blockIdx.x;
	StepState *r = seq + s;
	const int token = r->token, pos = r->pos;
	step_rope(r, pos, inv_freq, half);
	embed_row<WT>((const char *)emb + WT::row_off((size_t)token, dim), dim, x + (size_t)s * dim);
	if (threadIdx.x == 0) {
		r->kv_sink = 0;
		r->kv_pos = pos;
		r->kv_len = pos + 1;
		r->epoch = r->epoch + 1u;
		r->xbase = 0;
		r->xnext = 0;
	}
}

// RQKV / RQKVB / RQKVN (gemv_rows.h) over a batch: row t's epilogue is the base policy's finish
// with row t's StepState, q (or raw) row AND the K / V cache of sequence t. BP: PQKV, PQKVB or
// PQKVN; `stride`: floats between the q rows (PQKVN: the raw rows).
template <class WT, class BP>
struct BQKVT {
	static constexpr int R = 2;
	BP base; // step = the sequence states, q_out (raw) = row 0's
	int n, n_groups, stride;
	BatchKV kv;
	__device__ __forceinline__ const char *row(int g, int r) const { return base.row(g, r); }
	template <int T>
	__device__ __forceinline__ void finish(int g, const float (&acc)[R][T]) const {
#pragma unroll
		for (int t = 0; t < T; ++t) {
			BP b = base;
			b.step = base.step + t;
			b.kcache = kv.k[t];
			b.vcache = kv.v[t];
			if constexpr (std::is_same<BP, PQKVN<WT>>::value)
				b.raw = base.raw + (size_t)t * stride;
			else
				b.q_out = base.q_out + (size_t)t * stride;
			const float a[2] = {acc[0][t], acc[1][t]};
			b.finish(g, a, 0);
		}
	}
};
template <class WT>
using BQKV = BQKVT<WT, PQKV<WT>>;
template <class WT>
using BQKVB = BQKVT<WT, PQKVB<WT>>;
template <class WT>
using BQKVN = BQKVT<WT, PQKVN<WT>>;

// qk_norm_rope_kernel (qk_norm.h: the same statements in the same order, so the same bits) with
// row `blockIdx.y`'s K row written into that sequence's cache.
__global__ __launch_bounds__(YALM_WAVE) void batch_qk_norm_rope_kernel(
    const float *__restrict__ raw, int raw_stride, const float *__restrict__ gq, const float *__restrict__ gk,
    int n_heads, int n_kv_heads, int head_dim, float eps, const StepState *__restrict__ step, float *__restrict__ q_out,
    int q_stride, BatchKV kv) {
	const int h = (int)blockIdx.x;
	const int lane = threadIdx.x & 63, row = blockIdx.y;
	const StepState *s = step + row;
	uint16_t *kcache = row == 0 ? kv.k[0] : row == 1 ? kv.k[1] : row == 2 ? kv.k[2] : kv.k[3];
	const bool is_q = h < n_heads;
	const float *a = raw + (size_t)row * raw_stride + (size_t)h * head_dim; // k heads follow the q heads
	const float *g = is_q ? gq : gk;
	const int half = head_dim >> 1;
	float2_t v[2], w[2], cs[2];
	float ss = 0.0f;
#pragma unroll
	for (int u = 0; u < 2; ++u) {
		const int p = lane + 64 * u;
		if (p < half) {
			v[u] = *(const float2_t *)(a + 2 * p);
			w[u] = *(const float2_t *)(g + 2 * p);
			cs[u] = *(const float2_t *)(s->rope + 2 * p);
			ss += __builtin_fmaf(v[u][1], v[u][1], v[u][0] * v[u][0]);
		}
	}
	ss = wave_sum(ss);
	const float scale = 1.0f / sqrtf(ss / head_dim + eps);
#pragma unroll
	for (int u = 0; u < 2; ++u) {
		const int p = lane + 64 * u;
		if (p < half) {
			const float a0 = v[u][0] * scale * w[u][0], a1 = v[u][1] * scale * w[u][1];
			const float fcr = cs[u][0], fci = cs[u][1];
			const float r0 = a0 * fcr - a1 * fci, r1 = a0 * fci + a1 * fcr;
			if (is_q) {
				float2_t o;
				o[0] = r0, o[1] = r1;
				*(float2_t *)(q_out + (size_t)row * q_stride + (size_t)h * head_dim + 2 * p) = o;
			} else {
				const size_t o = ((size_t)s->kv_pos * n_kv_heads + (h - n_heads)) * head_dim + 2 * p;
				*(uint32_t *)(kcache + o) = (uint32_t)f2h(r0) | ((uint32_t)f2h(r1) << 16);
			}
		}
	}
}

// The decode attention of every sequence of a batch as ONE launch: attn_decode_kernel's grid
// (attention.h) once per sequence, sequence-major. Workgroup b belongs to sequence b / per_seq and
// is workgroup b % per_seq of that sequence's grid: its n_kv * (S + G - 1) head and split units,
// then its n_heads mergers. So every unit a merger waits for has a LOWER linear index than the
// merger, as in the one-sequence launch: a waiting workgroup only waits for workgroups dispatched
// before it, which wait for nobody (the kernel's forward-progress argument; the wait stays
// bounded and reports into the same error word). Each sequence has its own partial buffer: the
// sequences' launches are concurrent here, and two writers of one (head, split) granule would
// not be told apart by their tags in time. q, out: rows q_stride floats apart.
template <int D, int GT>
__global__ __launch_bounds__(ATTN_THREADS) void attn_decode_batch_kernel(
    const float *q, int q_stride, BatchKV kv, const StepState *steps, int per_seq, int n_heads, int n_kv_heads,
    int max_seq_len, int nsplit, int S, int head_max, BatchPart parts, int layer, int n_layers, unsigned *err,
    float *out) {
	const int s = (int)blockIdx.x / per_seq, b = (int)blockIdx.x - s * per_seq;
	const uint16_t *kc = s == 0 ? kv.k[0] : s == 1 ? kv.k[1] : s == 2 ? kv.k[2] : kv.k[3];
	const uint16_t *vc = s == 0 ? kv.v[0] : s == 1 ? kv.v[1] : s == 2 ? kv.v[2] : kv.v[3];
	unsigned long long *part = s == 0 ? parts.p[0] : s == 1 ? parts.p[1] : s == 2 ? parts.p[2] : parts.p[3];
	const StepState *step = steps + s;
	const float *qs = q + (size_t)s * q_stride;
	float *os = out + (size_t)s * q_stride;
	const int units = n_kv_heads * (S + n_heads / n_kv_heads - 1);
	const unsigned ptag = attn_part_tag(step, layer, n_layers);
	if (b < units)
		attn_decode_body<D, GT, false>(b % n_kv_heads, b / n_kv_heads, S, head_max, qs, kc, vc, step, n_heads, n_kv_heads,
		                               max_seq_len, nsplit, part, ptag, os, nullptr);
	else
		attn_merge_body<D, false>((b - units) % n_kv_heads, (b - units) / n_kv_heads, S, head_max, step, n_heads,
		                          n_kv_heads, max_seq_len, nsplit, part, ptag, err, os, nullptr);
}

// Last launch of a greedy step, one workgroup per sequence: the first-maximum argmax of row s
// (argmax_block, the rule of argmax_kernel) appended to sequence s's token buffer; the sequence
// continues at (that token, pos + 1). VEC: every row is 16-byte aligned (n % 4 == 0).
template <bool VEC>
__global__ __launch_bounds__(1024) void batch_commit_kernel(const float *__restrict__ logits, int n, StepState *seq,
                                                            BatchTok tok, int cap) {
	const int s = blockIdx.x;
	int *out = s == 0 ? tok.p[0] : s == 1 ? tok.p[1] : s == 2 ? tok.p[2] : tok.p[3];
	float b = 0.0f;
	int idx = 0;
	argmax_block<VEC>(logits + (size_t)s * n, n, b, idx);
	if (threadIdx.x == 0)
		argmax_commit(seq + s, idx, out, cap);
}

// The sampled twin: workgroup s draws row s's token by the sampling rule (sampler.h: smp_first_max
// + sample_row, as spec_sample_rows_kernel) with uniforms[s * u_stride + n_gen of sequence s]
// (the index clamped to [0, u_stride - 1]) and commits it like the greedy one.
template <bool VEC>
__global__ __launch_bounds__(SMP_THREADS) void batch_sample_kernel(const float *__restrict__ logits, int n,
                                                                   const SampleParams *__restrict__ prm,
                                                                   const float *__restrict__ uniforms, int u_stride,
                                                                   StepState *seq, BatchTok tok, int cap) {
	__shared__ SampleShared sh;
	const int s = blockIdx.x;
	int *out = s == 0 ? tok.p[0] : s == 1 ? tok.p[1] : s == 2 ? tok.p[2] : tok.p[3];
	StepState *st = seq + s;
	const float *__restrict__ row = logits + (size_t)s * n;
	const int gen = st->n_gen; // read by every thread before thread 0 commits
	const int ui = gen < 0 ? 0 : gen < u_stride ? gen : u_stride - 1;
	const float u = uniforms[(size_t)s * u_stride + ui];
	smp_first_max<VEC>(row, n, sh);
	const SampleParams p{prm->temperature, prm->top_k, prm->top_p};
	const SampleDraw r = sample_row<VEC>(row, n, p, u, sh);
	if (threadIdx.x == 0)
		argmax_commit(st, r.token, out, cap);
}
