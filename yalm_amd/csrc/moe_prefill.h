// moe_prefill.h — the FFN half of the batched prefill for mixture-of-experts (Mixtral)
// models: T prompt rows routed together, grouped by expert on the device and run through the
// 256-row MFMA tile kernels of prefill_gemm.h once per expert group (the reference runs one
// position per forward, infer.cpp:347-384).
//
// Per layer, after the FFN row norm (Xn = f16(rmsnorm(X) * rms_ffn), prefill.h):
//   moe_router_rows_kernel  one workgroup per row: logits = rmsnorm(X[t]) . moegate^T in f32 from
//                           the f32 residual stream (stage_x's arithmetic: the decode router's
//                           code on row t; the gate of an fp8 model as its exact f16 upcast, like
//                           the expert tensors, so its prefill is the f16 twin's bit for bit --
//                           an fp8 and an f16 row dot sum in different lane order), then moe_gate_device
//                           -> experts[t][k], weights[t][k] (kept per layer for read-back)
//   moe_group_kernel        one workgroup: per-expert counts, exclusive offsets, a stable counting
//                           sort of the T K (row, k) entries by expert (rows ascending inside an
//                           expert, so every run gives the same order), the inverse map
//                           slot(t, k), and the table of 256-row M tiles {expert, first slot,
//                           rows}; their number stays on the device
//   W1 | W3 + GLU           gemm16_kernel / gemm8p_kernel with RowGroups: A rows gathered from Xn
//                           through the slot list, B rows of the tile's expert, E16Glu -> H[slot]
//   W2                      A = H in slot order, B = W2 of the tile's expert, E16StoreScaled ->
//                           Y[slot][dim] f32 (x 2^hexp, the range guard's scale)
//   moe_combine_kernel      X[t] += sum_k weights[t][k] * Y[slot(t, k)], k ascending (the
//                           reference's selection order, infer.cpp:355-384); the expert weight is
//                           applied here in f32, and no float atomics anywhere: two prefills of the
//                           same input give the same bits
// The tile launches are sized for the host-side bound ceil(T K / 256) + min(E, T K) tiles.
#pragma once

#include "moe.h"
#include "prefill_gemm.h"

namespace pf {

// Row t of X through the decode router (moe.h moe_router_kernel, same block size, same
// arithmetic): LDS n floats + 64 (norm scratch) + E logits.
template <class WT, bool NORM>
__global__ __launch_bounds__(MOE_ROUTER_THREADS) void moe_router_rows_kernel(const char *__restrict__ gate,
                                                                             const float *__restrict__ X,
                                                                             const float *__restrict__ normw, float eps,
                                                                             int n, int E, int K, int *__restrict__ experts,
                                                                             float *__restrict__ weights) {
	extern __shared__ __attribute__((aligned(16))) float xs[];
	constexpr int EPL = WT::EPL;
	const size_t t = blockIdx.x;
	float *lg = xs + ((n + 3) & ~3) + 64;
	stage_x<NORM>(xs, X + t * n, normw, n, eps);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
	for (int e = wave; e < E; e += waves) {
		const char *row = gate + (size_t)e * n * WT::BYTES;
		float acc[1] = {0.0f};
		for (int i = lane * EPL; i < n; i += YALM_WAVE * EPL) {
			const u32x4_t w[1] = {load16(row + (size_t)i * WT::BYTES)};
			fma_chunk<WT, 1>(acc, w, xs + i);
		}
		const float s = wave_sum(acc[0]);
		if (lane == 0)
			lg[e] = s;
	}
	__syncthreads();
	if (threadIdx.x == 0)
		moe_gate_device(lg, E, K, experts + t * K, weights + t * K);
}

// The grouping tables of one layer's routing (all device memory, rewritten per layer).
struct MoeGroupTabs {
	int *slot_row; // [T K] slot -> prompt row t (the A-row gather list)
	int *slot_of;  // [T K] (t, k) -> slot
	int *tiles;    // [bound][4] {expert, first slot, rows, 0}
	int *ntiles;   // [1]
	int *counts;   // [E + 1] exclusive offsets (counts[E] = T K)
};

constexpr int MOE_GROUP_THREADS = 1024;
constexpr int MOE_GROUP_MAX = 128 * 1024; // entries (one LDS byte each)

// One workgroup. n = T K entries in (row, k) order, expert ids clamped into [0, E) (as
// MoeSel::prepare: an index outside the stack is never dereferenced). LDS: n bytes (the
// ids) + 2 x 64 ints. Wave w counts, then places, experts w, w + 16, ...: a ballot per 64
// entries, the entry's rank = the expert's running count + the set bits below its lane, so
// the order inside an expert is the entry order (rows ascending) whatever the timing.
__global__ __launch_bounds__(MOE_GROUP_THREADS) void moe_group_kernel(const int *__restrict__ experts, int n, int K,
                                                                      int E, int tile_bound, MoeGroupTabs g) {
	extern __shared__ __attribute__((aligned(16))) unsigned char ids[];
	int *cnt = (int *)(ids + ((n + 15) & ~15)), *off = cnt + MOE_MAX_EXPERTS;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
	for (int i = threadIdx.x; i < n; i += blockDim.x) {
		const int v = experts[i];
		ids[i] = (unsigned char)(v < 0 ? 0 : (v >= E ? E - 1 : v));
	}
	__syncthreads();
	for (int e = wave; e < E; e += waves) {
		int c = 0;
		for (int i0 = 0; i0 < n; i0 += 64) {
			const int i = i0 + lane;
			c += __popcll(__ballot(i < n && ids[i] == e));
		}
		if (lane == 0)
			cnt[e] = c;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		int o = 0, nt = 0;
		for (int e = 0; e < E; ++e) {
			off[e] = o;
			g.counts[e] = o;
			for (int r = 0; r < cnt[e] && nt < tile_bound; r += G_BM) {
				int *tt = g.tiles + 4 * nt++;
				tt[0] = e;
				tt[1] = o + r;
				tt[2] = min(G_BM, cnt[e] - r);
				tt[3] = 0;
			}
			o += cnt[e];
		}
		g.counts[E] = o;
		*g.ntiles = nt;
	}
	__syncthreads();
	for (int e = wave; e < E; e += waves) {
		int base = off[e];
		for (int i0 = 0; i0 < n; i0 += 64) {
			const int i = i0 + lane;
			const bool mine = i < n && ids[i] == e;
			const unsigned long long m = __ballot(mine);
			if (mine) {
				const int s = base + __popcll(m & ((1ull << lane) - 1ull));
				g.slot_of[i] = s;
				g.slot_row[s] = i / K;
			}
			base += __popcll(m);
		}
	}
}

// C rows "slot" as f32 with an exact power-of-two scale (the W2 product of an H stored as
// f16(h * 2^-e), E16Glu::hscale)
struct E16StoreScaled {
	static constexpr bool NEEDS_LDS = false;
	float *red = nullptr;
	float *c;
	int ldc, M;
	float scale = 1.0f;
	template <int FI, int FJ>
	__device__ __forceinline__ void apply(f32x4_t (&acc)[FI][FJ], int m0, int n0, int lane, int, int) const {
#pragma unroll
		for (int i = 0; i < FI; ++i)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int m = m0 + 16 * i + crow16(r, lane);
				if (m >= M)
					continue;
#pragma unroll
				for (int j = 0; j < FJ; ++j)
					c[(size_t)m * ldc + n0 + 16 * j + (lane & 15)] = acc[i][j][r] * scale;
			}
	}
};

// out[t] (+)= sum_k weights[t][k] * Y[slot_of[t K + k]], k ascending; RESID: out is the residual
// stream and is added to, else it is overwritten. One workgroup per row, float4 columns.
// weights null: the plain sum (the grouped-GEMM test hook's scatter back to row order, K = 1).
template <bool RESID>
__global__ __launch_bounds__(256) void moe_combine_kernel(float *__restrict__ out, const float *__restrict__ Y,
                                                          const int *__restrict__ slot_of,
                                                          const float *__restrict__ weights, int K, int dim) {
	const size_t t = blockIdx.x;
	for (int c = threadIdx.x * 4; c < dim; c += blockDim.x * 4) {
		float4_t a = {0.f, 0.f, 0.f, 0.f};
		if constexpr (RESID)
			a = *(const float4_t *)(out + t * dim + c);
		for (int k = 0; k < K; ++k) {
			const float w = weights ? weights[t * K + k] : 1.0f;
			const float4_t y = *(const float4_t *)(Y + (size_t)slot_of[t * K + k] * dim + c);
			a[0] += w * y[0];
			a[1] += w * y[1];
			a[2] += w * y[2];
			a[3] += w * y[3];
		}
		*(float4_t *)(out + t * dim + c) = a;
	}
}

// f32 rows -> f16 (the FFN-rows test hook's A operand; SPLIT: [hi | lo])
template <bool SPLIT>
__global__ __launch_bounds__(256) void moe_rows_f16_kernel(const float *__restrict__ x, int dim, uint16_t *__restrict__ xn) {
	const size_t t = blockIdx.x;
	for (int c = threadIdx.x; c < dim; c += blockDim.x) {
		const float v = x[t * dim + c];
		const uint16_t hb = f2h_bits(v);
		xn[t * (SPLIT ? 2 : 1) * dim + c] = hb;
		if constexpr (SPLIT)
			xn[t * 2 * dim + dim + c] = f2h_bits(v - h2f(hb));
	}
}

} // namespace pf
