// spec.h — speculative greedy and sampled decode: the per-row step states of a multi-row forward
// (gemv_rows.h), the n-gram drafter and the verify / accept launch. Everything is plain kernel
// work on one stream: no cross-workgroup hand-off, no spin, no wait inside a launch.
//
// A speculative step of T rows is: draft (1 launch) -> rows begin (1) -> per layer QKV, T
// attention launches, Wo, W1|W3, W2 -> norm + logits (1) -> verify (1). Row 0 holds the token
// greedy decode would feed; rows 1..T-1 hold drafted next tokens. The verify launch takes the
// first-maximum argmax of every row (argmax_block, the rule of argmax_kernel) and accepts the
// longest prefix of drafts that equal the argmax of the row before them, so the tokens are
// those of plain greedy decode by construction.
//
// The sampled step ends with two launches in the verify launch's place: T workgroups draw every
// row's token by the sampling rule with the uniform of the output index the row would fill
// (spec_sample_rows_kernel), then one accepts the drafts that equal the draw of the row before
// them (spec_accept_kernel). The drafter proposes one token, not a distribution, so there is
// nothing to resample, and the tokens are those of the plain sampled loop for the same uniforms.
#pragma once

#include "device_common.h"
#include "misc_kernels.h"
#include "sampler.h"

#define SPEC_MAX_ROWS 4
#define SPEC_MAX_NGRAM 4
#define SPEC_DRAFT_THREADS 1024

// Device-resident state of the speculative loop (one per decoder).
struct SpecState {
	int tok[SPEC_MAX_ROWS];   // the tokens of the step's rows (tok[0]: StepState::token)
	int draft[SPEC_MAX_ROWS]; // draft[k], k >= 1: the drafted token of row k, -1 = none (the row is fed token 0)
	int steps;                // speculative steps run since the loop began
	int accepted;             // drafts accepted since the loop began
	int drawn[SPEC_MAX_ROWS]; // the sampled loop: the token drawn from each row (spec_sample_rows_kernel)
	int none;                 // the draft-model loop: this step's drafts are none (spec_model_sync_kernel)
};

// yalm_forward_rows: the host's row tokens (kernel arguments: no host buffer to outlive the call).
__global__ void spec_set_tok_kernel(SpecState *sp, int t0, int t1, int t2, int t3) {
	sp->tok[0] = t0;
	sp->tok[1] = t1;
	sp->tok[2] = t2;
	sp->tok[3] = t3;
}

// First launch of a multi-row forward: row t gets its own StepState (token, pos + t, the window
// indices of an in-window position, the rope table of pos + t and a DISTINCT epoch, so the T
// attention launches of a layer tag their chunk partials apart) and x[t] = embedding[token t].
// from_step: row 0's token is st->token (the device loop); else tok[0] (yalm_forward_rows).
// Requires pos + T <= max_seq_len (the host checks): no ring wrap, no sink rotation.
template <class WT>
__global__ __launch_bounds__(256) void rows_begin_kernel(StepState *st, StepState *rows, const int *__restrict__ tok,
                                                         int T, int from_step, const void *__restrict__ emb, int dim,
                                                         float *__restrict__ x, const float *__restrict__ inv_freq,
                                                         int half) {
	const int pos = st->pos;
	const unsigned e0 = st->epoch;
	const int tok0 = from_step ? st->token : tok[0];
	__syncthreads(); // every thread has read the step before thread 0 advances its epoch
	for (int t = 0; t < T; ++t) {
		const int token = t == 0 ? tok0 : tok[t];
		StepState *r = rows + t;
		step_rope(r, pos + t, inv_freq, half);
		embed_row<WT>((const char *)emb + WT::row_off((size_t)token, dim), dim, x + (size_t)t * dim);
		if (threadIdx.x == 0) {
			r->token = token;
			r->pos = pos + t;
			r->kv_sink = 0;
			r->kv_pos = pos + t;
			r->kv_len = pos + t + 1;
			r->n_gen = 0;
			r->epoch = e0 + 1u + (unsigned)t;
			r->xbase = 0;
			r->xnext = 0;
		}
	}
	if (threadIdx.x == 0)
		st->epoch = e0 + (unsigned)T;
}

// The n-gram drafter. History H[0, m) = ctx[0, n_ctx) then gen[0, n_gen) (the tokens produced so
// far), H[m - 1] the token to feed next. For g = gmax down to gmin: the LARGEST i with
// i + g <= m - 1 and H[i, i + g) == H[m - g, m); the first g with such an i wins and the drafts
// are d_k = H[i + g + k - 1], k = 1..T-1, while that index is < m; later drafts, and all of them
// when nothing matches, are none (-1). In terms of e = i + g - 1, the index of the match's last
// token: L(e) = how many tokens ending at e equal the tokens ending at m - 1 (at most gmax); the
// largest e <= m - 2 with L(e) >= g is the match of g. One workgroup; integers only.
// stream != null (test / benchmark hook): d_k = stream[n_gen + k - 1] instead, none past its end.
__device__ __forceinline__ int spec_hist(const int *__restrict__ ctx, int n_ctx, const int *__restrict__ gen, int j) {
	return j < n_ctx ? ctx[j] : gen[j - n_ctx];
}

__device__ __forceinline__ void spec_draft_body(const int *__restrict__ ctx, int n_ctx, const int *__restrict__ gen,
                                                int n_gen, int T, int gmax, int gmin, const int *__restrict__ stream,
                                                int stream_len, int *__restrict__ draft) {
	__shared__ int best[SPEC_MAX_NGRAM + 1];
	if (stream) {
		if (threadIdx.x < (unsigned)T && threadIdx.x >= 1) {
			const int j = n_gen + (int)threadIdx.x - 1;
			draft[threadIdx.x] = j < stream_len ? stream[j] : -1;
		}
		return;
	}
	const int m = n_ctx + n_gen;
	if (threadIdx.x <= SPEC_MAX_NGRAM)
		best[threadIdx.x] = -1;
	__syncthreads();
	int tail[SPEC_MAX_NGRAM]; // H[m - 1 - j]
#pragma unroll
	for (int j = 0; j < SPEC_MAX_NGRAM; ++j)
		tail[j] = j < m ? spec_hist(ctx, n_ctx, gen, m - 1 - j) : -1;
	int be[SPEC_MAX_NGRAM + 1];
#pragma unroll
	for (int g = 0; g <= SPEC_MAX_NGRAM; ++g)
		be[g] = -1;
	for (int e = threadIdx.x; e <= m - 2; e += blockDim.x) { // ascending per thread: the last hit is its largest
		int L = 0;
#pragma unroll
		for (int j = 0; j < SPEC_MAX_NGRAM; ++j)
			if (L == j && j < gmax && e - j >= 0 && spec_hist(ctx, n_ctx, gen, e - j) == tail[j])
				L = j + 1;
#pragma unroll
		for (int g = 1; g <= SPEC_MAX_NGRAM; ++g)
			if (L >= g)
				be[g] = e;
	}
#pragma unroll
	for (int g = 1; g <= SPEC_MAX_NGRAM; ++g)
		if (be[g] >= 0)
			atomicMax(&best[g], be[g]); // LDS, integers: the order does not matter
	__syncthreads();
	if (threadIdx.x == 0) {
		int e = -1;
		for (int g = gmax; g >= gmin && e < 0; --g)
			e = best[g];
		for (int k = 1; k < T; ++k)
			draft[k] = e >= 0 && e + k < m ? spec_hist(ctx, n_ctx, gen, e + k) : -1;
	}
}

// The loop's drafter: fills sp->draft and sp->tok of rows 1..T-1 (none: token 0).
__global__ __launch_bounds__(SPEC_DRAFT_THREADS) void spec_draft_kernel(const StepState *st, SpecState *sp,
                                                                         const int *__restrict__ ctx, int n_ctx,
                                                                         const int *__restrict__ gen, int gen_cap, int T,
                                                                         int gmax, int gmin,
                                                                         const int *__restrict__ stream,
                                                                         int stream_len, int vocab) {
	const int n_gen = min(st->n_gen, gen_cap);
	spec_draft_body(ctx, n_ctx, gen, n_gen, T, gmax, gmin, stream, stream_len, sp->draft);
	__syncthreads();
	if (threadIdx.x >= 1 && threadIdx.x < (unsigned)T) {
		const int dk = sp->draft[threadIdx.x];
		const bool ok = dk >= 0 && dk < vocab; // a token the model does not have is no draft
		if (!ok)
			sp->draft[threadIdx.x] = -1;
		sp->tok[threadIdx.x] = ok ? dk : 0;
	}
}

// The draft-model drafter (yalm_generate_speculative_model): a second decoder on the same stream
// proposes the rows. A step is sync (1 launch) -> rows - 1 greedy forwards of the draft decoder
// from its own device state -> one KV-only forward of it -> gather (1) -> the rows forward and the
// verify (or draw + accept) launches as above.
//
// Sync: the draft decoder's step becomes the target's (token, pos) with nothing produced, so its
// greedy forwards write d_1 .. d_(T-1) to its token buffer [0, T - 1) and its KV rows pos ..
// pos + T - 2; the KV-only forward then feeds d_(T-1) at pos + T - 1, so a fully accepted step
// leaves no hole in the draft's cache. A token the draft does not have is fed as token 0 and the
// step's drafts are none (sp->none): the draft's embedding is never read out of range.
__global__ __launch_bounds__(64) void spec_model_sync_kernel(const StepState *st, SpecState *sp, StepState *dst,
                                                             int draft_vocab) {
	if (threadIdx.x == 0) {
		const int token = st->token;
		const bool ok = token >= 0 && token < draft_vocab;
		dst->token = ok ? token : 0;
		dst->pos = st->pos;
		dst->n_gen = 0;
		sp->none = ok ? 0 : 1;
	}
}

// Gather: sp->draft and sp->tok of rows 1..T-1 as spec_draft_kernel leaves them, d_k =
// dtok[k - 1] (the draft decoder's token buffer), none when sp->none is set or the target does
// not have the token. stream != null (test / benchmark hook): d_k = stream[n_gen + k - 1]
// instead, none past its end, whatever the draft decoder produced.
__global__ __launch_bounds__(64) void spec_model_gather_kernel(const StepState *st, SpecState *sp,
                                                               const int *__restrict__ dtok, int gen_cap, int T,
                                                               const int *__restrict__ stream, int stream_len,
                                                               int vocab) {
	const int k = threadIdx.x;
	if (k < 1 || k >= T)
		return;
	int dk;
	if (stream) {
		const int j = min(st->n_gen, gen_cap) + k - 1;
		dk = j < stream_len ? stream[j] : -1;
	} else {
		dk = sp->none ? -1 : dtok[k - 1];
	}
	const bool ok = dk >= 0 && dk < vocab;
	sp->draft[k] = ok ? dk : -1;
	sp->tok[k] = ok ? dk : 0;
}

// yalm_spec_draft: the drafter on a given history alone.
__global__ __launch_bounds__(SPEC_DRAFT_THREADS) void spec_draft_test_kernel(const int *__restrict__ hist, int m, int T,
                                                                              int gmax, int gmin,
                                                                              int *__restrict__ draft) {
	spec_draft_body(hist, m, hist, 0, T, gmax, gmin, nullptr, 0, draft);
}

// Accept, by one thread: with tk[t] the token chosen from row t (the argmax, or the draw),
// a = 1 + the longest prefix of drafts with draft[k] == tk[k - 1] (a none draft never matches);
// tk[0..a-1] are appended to the token buffer and the next step is (tk[a - 1], pos + a).
__device__ __forceinline__ void spec_accept_commit(const int *tk, int T, StepState *st, SpecState *sp,
                                                   int *__restrict__ tokens_out, int cap) {
	int a = 1;
	while (a < T && sp->draft[a] >= 0 && sp->draft[a] == tk[a - 1])
		++a;
	const int k = st->n_gen;
	for (int j = 0; j < a; ++j)
		if (k + j < cap)
			tokens_out[k + j] = tk[j];
	st->n_gen = k + a;
	st->token = tk[a - 1];
	st->pos = st->pos + a;
	sp->steps = sp->steps + 1;
	sp->accepted = sp->accepted + (a - 1);
}

// Verify and accept, one launch of one workgroup: am_t = the first-maximum argmax of row t's
// logits; a = 1 + the longest prefix of drafts with draft[k] == am[k - 1] (a none draft never
// matches); am[0..a-1] are appended to the token buffer and the next step is (am[a - 1], pos + a).
// The KV rows of rejected drafts are overwritten by later steps.
__global__ __launch_bounds__(1024) void spec_verify_kernel(const float *__restrict__ logits, int n, int T, StepState *st,
                                                           SpecState *sp, int *__restrict__ tokens_out, int cap) {
	__shared__ int am[SPEC_MAX_ROWS];
	for (int t = 0; t < T; ++t) {
		float b = 0.0f;
		int idx = 0;
		argmax_block(logits + (size_t)t * n, n, b, idx);
		if (threadIdx.x == 0)
			am[t] = idx;
		__syncthreads(); // argmax_block's LDS scratch is reused by the next row
	}
	if (threadIdx.x == 0)
		spec_accept_commit(am, T, st, sp, tokens_out, cap);
}

// The sampled step's draws (sampler.h, the rule of sample_kernel): workgroup t draws row t's
// token from logits + t * stride with uniforms[n_gen + t] (clamped to [0, u_cap - 1]) into
// sp->drawn[t]; n_gen is read, not written. Row t is thereby drawn with the uniform of the
// output index it would fill. One workgroup per row, each with its own SampleShared; nothing
// passes between them. VEC: every row is 16-byte aligned (stride % 4 == 0); else the rows are
// read element by element. kept_out (may be null): [t] = the kept-set size of row t.
template <bool VEC>
__global__ __launch_bounds__(SMP_THREADS) void spec_sample_rows_kernel(const float *__restrict__ logits, int n,
                                                                       int stride,
                                                                       const SampleParams *__restrict__ prm,
                                                                       const float *__restrict__ uniforms, int u_cap,
                                                                       const StepState *__restrict__ st, SpecState *sp,
                                                                       int *__restrict__ kept_out) {
	__shared__ SampleShared sh;
	const int t = blockIdx.x;
	const float *__restrict__ row = logits + (size_t)t * stride;
	const long long gi = (long long)st->n_gen + t;
	const int ui = gi < 0 ? 0 : gi < u_cap ? (int)gi : u_cap - 1;
	smp_first_max<VEC>(row, n, sh);
	const SampleParams p{prm->temperature, prm->top_k, prm->top_p};
	const SampleDraw r = sample_row<VEC>(row, n, p, uniforms[ui], sh);
	if (threadIdx.x == 0) {
		sp->drawn[t] = r.token;
		if (kept_out)
			kept_out[t] = (int)r.kept;
	}
}

// The launch after it: spec_verify_kernel's tail over the drawn tokens.
__global__ __launch_bounds__(64) void spec_accept_kernel(int T, StepState *st, SpecState *sp,
                                                         int *__restrict__ tokens_out, int cap) {
	if (threadIdx.x == 0)
		spec_accept_commit(sp->drawn, T, st, sp, tokens_out, cap);
}

// After a batch that overshot the requested count: the device continues at (token, pos) with
// n_gen tokens produced.
__global__ void spec_fix_kernel(StepState *st, int token, int pos, int n_gen) {
	st->token = token;
	st->pos = pos;
	st->n_gen = n_gen;
}
