// qk_norm.h — the per-head RMSNorm on q and k ahead of RoPE (Qwen3), as one small launch
// between the QKV GEMV (PQKVN, gemv.h: clipped raw f32 q | k) and attention.
//
// One wave64 per head, n_heads + n_kv_heads waves per row; blockIdx.y is the row (the multi-row
// verify step: row t's raw values, StepState and q row; decode is one row). A lane holds whole
// RoPE pairs (2 p, 2 p + 1) of the head, p = lane and lane + 64: head_dim <= 256 (the largest a
// decoder takes: StepState::rope holds 128 pairs), any even
// head_dim (16: lanes 0..7, 64: lanes 0..31, 128: all 64 lanes, one pair each).
//   ss = sum a[i]^2 (per lane a0 a0, then fma(a1, a1, .), pair by pair; the DPP wave_sum)
//   scale = 1 / sqrtf(ss / head_dim + eps);  a'[i] = a[i] * scale * g[i]       (stage_x's order)
//   RoPE from step->rope, then q_out (f32) or the K cache row step->kv_pos (f16), as PQKV::finish.
// The sum's order is fixed by the lane layout, so the same input gives the same bits.
#pragma once

#include "device_common.h"

template <int WPB>
__global__ __launch_bounds__(WPB * YALM_WAVE) void qk_norm_rope_kernel(
    const float *__restrict__ raw, int raw_stride, const float *__restrict__ gq, const float *__restrict__ gk,
    int n_heads, int n_kv_heads, int head_dim, float eps, const StepState *__restrict__ step, float *__restrict__ q_out,
    int q_stride, uint16_t *__restrict__ kcache) {
	const int h = (int)blockIdx.x * WPB + (int)(threadIdx.x >> 6);
	if (h >= n_heads + n_kv_heads)
		return;
	const int lane = threadIdx.x & 63, row = blockIdx.y;
	const StepState *s = step + row;
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
