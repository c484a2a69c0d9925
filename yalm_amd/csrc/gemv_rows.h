// gemv_rows.h — weight-streaming GEMV for T = 1..4 activation rows (the verify step of
// speculative greedy decode, spec.h): every weight matrix is streamed ONCE for all T rows, with
// f32 activations and f32 accumulation as in decode (gemv.h). The single-row kernels of gemv.h
// are not touched: this header only reuses their weight-type policies (WT::row_off, the 16-byte
// chunk loads, WT::unpack), stage_x's norm arithmetic and the epilogue arithmetic of PQKV.
//
//   * one wave64 owns a group of R = 2 weight rows and streams them with 16-byte non-temporal
//     loads (U = 4 chunks per row in flight); a lane's x fragment of a chunk is read from LDS once
//     per row t and serves both weight rows (T x 4 B of LDS per 2 weight elements: a lane that
//     re-read x per weight row would pay twice that, the limit q4 met in DESIGN.md §11),
//   * x is staged in LDS as T rows of at most `kseg` floats, T * kseg * 4 B <= ROWS_X_BYTES: a
//     row longer than that (W2 at Mistral dims: 4 x 14336 x 4 B = 229 KB against 160 KiB per CU)
//     is staged by K segments, the wave keeping its R x T accumulators in registers across them
//     (the host then gives every wave ONE group, so a segment is staged once per workgroup),
//   * each row's rmsnorm follows stage_x's statement order (infer.cpp:134-144); the scale comes
//     from the whole row in global memory, so it holds for a segmented row too,
//   * a chunk is consumed in pieces of at most 8 elements (fp8: two per 16-byte load), which
//     keeps the x fragment of 4 rows in 32 registers,
//   * epilogue policies over acc[R][T]: RStore (logits), RResidual (Wo, W2), RQKV (clip + RoPE +
//     KV write through PQKV::finish with row t's StepState), RGlu.
// Any n that is a multiple of WT::EPL and of 4 (a row shorter than one chunk included).
#pragma once

#include "device_common.h"
#include "gemv.h"

#define ROWS_MAX_T 4
#define ROWS_THREADS 512
#define ROWS_U 4
#define ROWS_X_BYTES (128 * 1024) // LDS for the x segment of all T rows (160 KiB per CU)

template <class WT>
struct RStore {
	static constexpr int R = 2;
	const char *W;
	int n, n_rows, n_groups;
	float *out;
	int ostride;
	__device__ __forceinline__ const char *row(int g, int r) const {
		return W + WT::row_off((size_t)min(g * R + r, n_rows - 1), n);
	}
	template <int T>
	__device__ __forceinline__ void finish(int g, const float (&acc)[R][T]) const {
#pragma unroll
		for (int r = 0; r < R; ++r)
			if (g * R + r < n_rows) {
#pragma unroll
				for (int t = 0; t < T; ++t)
					out[(size_t)t * ostride + g * R + r] = acc[r][t];
			}
	}
};

template <class WT>
struct RResidual {
	static constexpr int R = 2;
	const char *W;
	int n, n_rows, n_groups;
	float *out;
	int ostride;
	__device__ __forceinline__ const char *row(int g, int r) const {
		return W + WT::row_off((size_t)min(g * R + r, n_rows - 1), n);
	}
	template <int T>
	__device__ __forceinline__ void finish(int g, const float (&acc)[R][T]) const {
#pragma unroll
		for (int r = 0; r < R; ++r)
			if (g * R + r < n_rows) {
#pragma unroll
				for (int t = 0; t < T; ++t)
					out[(size_t)t * ostride + g * R + r] += acc[r][t];
			}
	}
};

// Virtual row space [wq | wk | wv], a wave owns the RoPE pair (2g, 2g + 1) as PQKV; row t's
// epilogue is PQKV::finish itself with row t's StepState (its rope table and kv_pos) and q row.
template <class WT>
struct RQKV {
	static constexpr int R = 2;
	PQKV<WT> base; // step = the T step states, q_out = row 0's q
	int n, n_groups, q_stride;
	__device__ __forceinline__ const char *row(int g, int r) const { return base.row(g, r); }
	template <int T>
	__device__ __forceinline__ void finish(int g, const float (&acc)[R][T]) const {
#pragma unroll
		for (int t = 0; t < T; ++t) {
			PQKV<WT> b = base;
			b.step = base.step + t;
			b.q_out = base.q_out + (size_t)t * q_stride;
			const float a[2] = {acc[0][t], acc[1][t]};
			b.finish(g, a, 0);
		}
	}
};

// RQKV over a biased model: row t's epilogue is PQKVB::finish (the bias, then PQKV::finish).
template <class WT>
struct RQKVB {
	static constexpr int R = 2;
	PQKVB<WT> base;
	int n, n_groups, q_stride;
	__device__ __forceinline__ const char *row(int g, int r) const { return base.row(g, r); }
	template <int T>
	__device__ __forceinline__ void finish(int g, const float (&acc)[R][T]) const {
#pragma unroll
		for (int t = 0; t < T; ++t) {
			PQKVB<WT> b = base;
			b.step = base.step + t;
			b.q_out = base.q_out + (size_t)t * q_stride;
			const float a[2] = {acc[0][t], acc[1][t]};
			b.finish(g, a, 0);
		}
	}
};

// RQKV ahead of the q / k norm: row t's epilogue is PQKVN::finish into row t of the raw buffer
// ([T][raw_stride]); one qk_norm_rope_kernel launch then serves all T rows (qk_norm.h).
template <class WT>
struct RQKVN {
	static constexpr int R = 2;
	PQKVN<WT> base;
	int n, n_groups, raw_stride;
	__device__ __forceinline__ const char *row(int g, int r) const { return base.row(g, r); }
	template <int T>
	__device__ __forceinline__ void finish(int g, const float (&acc)[R][T]) const {
#pragma unroll
		for (int t = 0; t < T; ++t) {
			PQKVN<WT> b = base;
			b.step = base.step + t;
			b.raw = base.raw + (size_t)t * raw_stride;
			const float a[2] = {acc[0][t], acc[1][t]};
			b.finish(g, a, 0);
		}
	}
};

template <class WT, int ACT>
struct RGlu {
	static constexpr int R = 2;
	const char *w1, *w3;
	int n, n_groups;
	float *out;
	int ostride;
	__device__ __forceinline__ const char *row(int g, int r) const {
		return (r == 0 ? w1 : w3) + WT::row_off((size_t)g, n);
	}
	template <int T>
	__device__ __forceinline__ void finish(int g, const float (&acc)[R][T]) const {
#pragma unroll
		for (int t = 0; t < T; ++t)
			out[(size_t)t * ostride + g] = act_fn<ACT>(acc[0][t]) * acc[1][t];
	}
};

// acc[r][t] += w[r] . x_t over one 16-byte weight piece per row; xs_lane: row 0's x of the
// chunk at this lane's elements, rows kseg floats apart
template <class WT, int R, int T>
__device__ __forceinline__ void fma_rows(float (&acc)[R][T], const u32x4_t (&w)[R], const float *xs_lane, int kseg) {
	constexpr int EPL = WT::EPL;
	constexpr int SUB = EPL < 8 ? EPL : 8;
#pragma unroll
	for (int h = 0; h < EPL; h += SUB) {
		float xv[T][SUB];
#pragma unroll
		for (int t = 0; t < T; ++t)
#pragma unroll
			for (int e = 0; e < SUB; e += 4) {
				const float4_t v = *(const float4_t *)(xs_lane + (size_t)t * kseg + h + e);
				xv[t][e] = v[0];
				xv[t][e + 1] = v[1];
				xv[t][e + 2] = v[2];
				xv[t][e + 3] = v[3];
			}
#pragma unroll
		for (int r = 0; r < R; ++r) {
			float wf[EPL]; // the widening of the piece; the values outside [h, h + SUB) are dead code here
			WT::unpack(w[r], wf);
#pragma unroll
			for (int t = 0; t < T; ++t)
#pragma unroll
				for (int e = 0; e < SUB; ++e)
					acc[r][t] = fmaf(wf[h + e], xv[t][e], acc[r][t]);
		}
	}
}

// x: T rows, xstride floats apart. kseg: floats of one staged segment per row, a multiple of
// 64 * WT::EPL. Wave w of workgroup b owns groups (b * waves + w) * gpw .. + gpw - 1.
// LDS: T * kseg floats of x, then T * 16 floats of norm scratch.
template <class WT, class P, int T, bool NORM>
__global__ __launch_bounds__(ROWS_THREADS) void gemv_rows_kernel(P p, const float *__restrict__ x, int xstride,
                                                                 const float *__restrict__ normw, float eps, int gpw,
                                                                 int kseg) {
	extern __shared__ __attribute__((aligned(16))) float xs[];
	constexpr int R = P::R;
	constexpr int EPL = WT::EPL;
	constexpr int CH = YALM_WAVE * EPL;
	constexpr int U = ROWS_U;
	const int n = p.n;
	const int tid = threadIdx.x, nthreads = blockDim.x;
	const int lane = tid & 63, wave = tid >> 6, waves = nthreads >> 6;
	const int nseg = (n + kseg - 1) / kseg;

	float scale[T];
#pragma unroll
	for (int t = 0; t < T; ++t)
		scale[t] = 1.0f;
	if constexpr (NORM) { // stage_x's statement order, per row
		float *red = xs + (size_t)T * kseg;
#pragma unroll
		for (int t = 0; t < T; ++t) {
			float ss = 0.0f;
			for (int i = tid * 4; i < n; i += nthreads * 4) {
				const float4_t v = *(const float4_t *)(x + (size_t)t * xstride + i);
				ss = sumsq4(ss, v);
			}
			ss = wave_sum(ss);
			if (lane == 0)
				red[t * 16 + wave] = ss;
		}
		__syncthreads();
#pragma unroll
		for (int t = 0; t < T; ++t) {
			float tot = 0.0f;
			for (int w = 0; w < waves; ++w)
				tot += red[t * 16 + w];
			const float rms = sqrtf(tot / n + eps);
			scale[t] = 1.0f / rms;
		}
	}

	const int gbase = (blockIdx.x * waves + wave) * gpw;
	for (int gi = 0; gi < gpw; ++gi) { // (every wave runs every iteration: the staging barriers are inside)
		const int g = gbase + gi;
		const bool valid = g < p.n_groups;
		const char *rp[R];
#pragma unroll
		for (int r = 0; r < R; ++r)
			rp[r] = p.row(valid ? g : p.n_groups - 1, r) + (size_t)lane * 16;
		[[maybe_unused]] float rs[R]; // e4m3: each row's scale, requested ahead of the row's weights
		if constexpr (WT::ROW_SCALE) {
#pragma unroll
			for (int r = 0; r < R; ++r)
				rs[r] = WT::row_scale(rp[r] - (size_t)lane * 16, n);
		}
		float acc[R][T];
#pragma unroll
		for (int r = 0; r < R; ++r)
#pragma unroll
			for (int t = 0; t < T; ++t)
				acc[r][t] = 0.0f;
		for (int s = 0; s < nseg; ++s) {
			const int k0 = s * kseg, kl = min(kseg, n - k0);
			if (nseg > 1 || gi == 0) { // one segment: staged once for all the wave's groups
				__syncthreads();       // every wave is done with the previous segment
#pragma unroll
				for (int t = 0; t < T; ++t)
					for (int i = tid * 4; i < kl; i += nthreads * 4) {
						float4_t v = *(const float4_t *)(x + (size_t)t * xstride + k0 + i);
						if constexpr (NORM) {
							const float4_t w = *(const float4_t *)(normw + k0 + i);
							v[0] = v[0] * scale[t] * w[0];
							v[1] = v[1] * scale[t] * w[1];
							v[2] = v[2] * scale[t] * w[2];
							v[3] = v[3] * scale[t] * w[3];
						}
						*(float4_t *)(xs + (size_t)t * kseg + i) = v;
					}
				__syncthreads();
			}
			if (!valid)
				continue;
			const int nfull = kl / CH, rem = kl - nfull * CH;
			const size_t seg_off = (size_t)(k0 / CH) * WT_CHUNK_BYTES;
			int c = 0;
			for (; c + U <= nfull; c += U) {
				u32x4_t w[U][R];
#pragma unroll
				for (int u = 0; u < U; ++u)
#pragma unroll
					for (int r = 0; r < R; ++r)
						w[u][r] = load_nt16(rp[r] + seg_off + (size_t)(c + u) * WT_CHUNK_BYTES);
#pragma unroll
				for (int u = 0; u < U; ++u)
					fma_rows<WT, R, T>(acc, w[u], xs + (c + u) * CH + lane * EPL, kseg);
			}
			for (; c < nfull; ++c) {
				u32x4_t w[R];
#pragma unroll
				for (int r = 0; r < R; ++r)
					w[r] = load_nt16(rp[r] + seg_off + (size_t)c * WT_CHUNK_BYTES);
				fma_rows<WT, R, T>(acc, w, xs + c * CH + lane * EPL, kseg);
			}
			if (rem > 0 && lane * EPL < rem) { // the ragged end of the row (only the last segment has one)
				u32x4_t w[R];
#pragma unroll
				for (int r = 0; r < R; ++r)
					w[r] = load_nt16(rp[r] + seg_off + (size_t)nfull * WT_CHUNK_BYTES);
				fma_rows<WT, R, T>(acc, w, xs + nfull * CH + lane * EPL, kseg);
			}
		}
		if (valid) {
#pragma unroll
			for (int r = 0; r < R; ++r)
#pragma unroll
				for (int t = 0; t < T; ++t)
					acc[r][t] = wave_sum(acc[r][t]);
			if constexpr (WT::ROW_SCALE) {
#pragma unroll
				for (int r = 0; r < R; ++r)
#pragma unroll
					for (int t = 0; t < T; ++t)
						acc[r][t] *= rs[r];
			}
			if (lane == 0)
				p.finish(g, acc);
		}
	}
}
