// moe.h — mixture-of-experts (Mixtral) decode on gfx950: the router and the GEMV policies
// that stream only the selected experts' rows (reference CPU forward infer.cpp:100-132,
// 347-384; the reference's GPU path asserts on MoE, infer.cu:865-867).
//
// Per layer, after the attention half:
//   moe_router_kernel   logits = rmsnorm(x, rms_ffn) . moegate^T (one wave per expert row),
//                       then one lane runs the reference's top-k (moe_gate) and writes the K
//                       expert indices and softmax weights into the layer's slot in device
//                       memory -- no host round trip, so the launch sits in the per-token graph
//   PMoeGlu             W1 | W3 + GLU over the virtual row space K x hidden_dim: the launch reads the
//                       expert indices from the slot once (prepare) and row() addresses the stacked
//                       (E, hidden, dim) tensors; the epilogue folds the expert weight in:
//                       hb[k * hidden + i] = weight_k * act(a) * b
//   PMoeW2              x[row] += sum_k W2[e_k][row] . hb_k as ONE GEMV of row length K x hidden:
//                       chunk() switches expert matrix at each hidden_dim boundary
//   PMoeW2One           the same sum as one launch per selected expert (x[row] += W2[e_k][row] . hb_k),
//                       for row lengths past the LDS, more than MOE_SEL_REGS selected experts and
//                       the generic (ragged) GEMV kernel
// The dense policies (PGlu, PResidual) and their instantiations are untouched.
#pragma once

#include <float.h>

#include "device_common.h"
#include "gemv.h"

#define MOE_MAX_EXPERTS 64 // the reference's selection mask is a uint64_t (infer.cpp:113)
#define MOE_ROUTER_THREADS 512

#define MOE_SEL_REGS 8 // selected experts one launch addresses (a launch per 8 beyond that)

// The selected expert indices of one launch, in registers (the GEMV kernels' prepare hook, gemv.h):
// 8 indices < 64 packed a byte each into one 64-bit value -- an int[8] member was kept in scratch
// memory and indexed there by the compiler (36 bytes of private segment, a scratch load per row).
struct MoeRegs {
	unsigned long long packed;
	__device__ __forceinline__ int expert(int k) const { // k < count
		return (int)((packed >> (8 * k)) & 0xffull);
	}
};

// (Part of) the routing slot of one layer, written by the router: `count` <= MOE_SEL_REGS expert
// indices and weights. prepare() reads the indices ONCE, ahead of the weight stream: read per row
// from memory (first version) every weight address depended on a load in the stream, and the
// expert GLU ran at half the dense kernel's rate.
struct MoeSel {
	const int *experts;
	const float *weights;
	int n_experts, count;
	__device__ __forceinline__ MoeRegs prepare() const {
		MoeRegs r{0ull};
#pragma unroll
		for (int j = 0; j < MOE_SEL_REGS; ++j) {
			// an index outside the stack must never be dereferenced, whatever the router saw
			const int v = experts[j < count ? j : 0];
			const int e = v < 0 ? 0 : (v >= n_experts ? n_experts - 1 : v);
			r.packed |= (unsigned long long)e << (8 * j);
		}
		return r;
	}
};

// infer.cpp:100-132 (moe_gate), statement for statement, by one thread.
__device__ __forceinline__ void moe_gate_device(const float *lg, int E, int K, int *experts, float *weights) {
	float max_val = -FLT_MAX;
	for (int j = 0; j < E; ++j)
		if (lg[j] > max_val)
			max_val = lg[j];
	unsigned long long mask = 0;
	float wsum = 0.0f;
	float ex[MOE_MAX_EXPERTS];
	int sel[MOE_MAX_EXPERTS];
	for (int k = 0; k < K; ++k) {
		int best = -1;
		for (int j = 0; j < E; ++j)
			if ((mask & (1ull << j)) == 0 && (best == -1 || lg[j] > lg[best]))
				best = j;
		best = best < 0 ? 0 : (best >= E ? E - 1 : best); // K <= E: never taken; keeps the index in range
		sel[k] = best;
		ex[k] = expf(lg[best] - max_val);
		wsum += ex[k];
		mask |= 1ull << best;
	}
	for (int k = 0; k < K; ++k) {
		experts[k] = sel[k];
		weights[k] = ex[k] / wsum;
	}
}

// One workgroup: x (optionally rmsnorm'ed, as the GLU GEMV stages it) into LDS, one wave per
// expert row of moegate (E, n), then thread 0 selects. LDS: n floats + 64 (norm scratch) + E logits.
template <class WT, bool NORM>
__global__ __launch_bounds__(MOE_ROUTER_THREADS) void moe_router_kernel(const char *__restrict__ gate,
                                                                        const float *__restrict__ x,
                                                                        const float *__restrict__ normw, float eps, int n,
                                                                        int E, int K, int *__restrict__ experts,
                                                                        float *__restrict__ weights) {
	extern __shared__ __attribute__((aligned(16))) float xs[];
	constexpr int EPL = WT::EPL;
	float *lg = xs + ((n + 3) & ~3) + 64;
	stage_x<NORM>(xs, x, normw, n, eps);
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
		moe_gate_device(lg, E, K, experts, weights);
}

// Virtual group g = k * hidden + i: rows i of W1 and W3 of the k-th selected expert of this launch
// (k < sel.count <= MOE_SEL_REGS).
template <class WT, int ACT>
struct PMoeGlu {
	static constexpr int R = 2;
	static constexpr bool ROWS_MODE = true;
	static constexpr bool LOCAL_X = true; // the expert GLU never consumes a tensor-parallel exchange
	const char *w1, *w3; // stacked (E, hidden, n)
	int n;
	float *out; // [K * hidden]
	int n_groups; // sel.count * hidden
	int hidden;
	MoeSel sel;
	static constexpr bool PREPARE = true;
	using Prep = MoeRegs;
	__device__ __forceinline__ Prep prepare() const { return sel.prepare(); }
	__device__ __forceinline__ void prologue() const {}
	__device__ __forceinline__ void split(int g, int &k, int &i) const {
		k = 0;
		while (g >= hidden) { // count - 1 compares at most (1 for Mixtral)
			g -= hidden;
			++k;
		}
		i = g;
	}
	__device__ __forceinline__ const char *row(int g, int r, const Prep &pr) const {
		int k, i;
		split(g, k, i);
		return (r == 0 ? w1 : w3) + ((size_t)pr.expert(k) * hidden + i) * n * WT::BYTES;
	}
	__device__ __forceinline__ void finish(int g, const float *acc, int lane) const {
		if (lane != 0)
			return;
		int k, i;
		split(g, k, i);
		out[g] = sel.weights[k] * (act_fn<ACT>(acc[0]) * acc[1]);
	}
	__device__ __forceinline__ void finish_all(int g, const float *acc) const { finish(g, acc, 0); }
};

// out[g] += W2cat[g] . hb, W2cat[g] = [W2[e_0][g] | W2[e_1][g] | ...] (n = K * hidden): the 64-lane
// chunk c lies inside one expert's row because hidden is a multiple of the chunk (the launcher checks).
template <class WT>
struct PMoeW2 {
	static constexpr int R = 1;
	static constexpr bool CHUNKED = true;
	static constexpr bool ROWS_MODE = true;
	const char *W; // stacked (E, dim, hidden)
	int n;         // K * hidden
	float *out;
	int n_groups; // dim
	int hidden;
	MoeSel sel;
	static constexpr bool PREPARE = true;
	using Prep = MoeRegs;
	__device__ __forceinline__ Prep prepare() const { return sel.prepare(); }
	__device__ __forceinline__ void prologue() const {}
	__device__ __forceinline__ const char *chunk(int g, int, int c, const Prep &pr) const {
		int off = c * (YALM_WAVE * WT::EPL), k = 0;
		while (off >= hidden) {
			off -= hidden;
			++k;
		}
		return W + (((size_t)pr.expert(k) * n_groups + g) * hidden + off) * WT::BYTES;
	}
	__device__ __forceinline__ void finish_all(int g, const float *acc) const { out[g] += acc[0]; }
	static constexpr bool PRE = true; // as PResidual: the residual row is read ahead of the weight stream
	__device__ __forceinline__ float pre(int g, int) const { return out[g]; }
	__device__ __forceinline__ void finish_pre(int g, const float *acc, const float *xr) const {
		out[g] = xr[0] + acc[0];
	}
};

// out[g] += W2[e_k][g] . hb_k for one selected expert k (hb_k already carries weight_k).
template <class WT>
struct PMoeW2One {
	static constexpr int R = 1;
	static constexpr bool ROWS_MODE = true;
	const char *W; // stacked (E, dim, n)
	int n;         // hidden
	float *out;
	int n_groups; // dim
	MoeSel sel; // the one expert: count 1
	static constexpr bool PREPARE = true;
	using Prep = MoeRegs;
	__device__ __forceinline__ Prep prepare() const { return sel.prepare(); }
	__device__ __forceinline__ void prologue() const {}
	__device__ __forceinline__ const char *row(int g, int, const Prep &pr) const {
		return W + ((size_t)pr.expert(0) * n_groups + g) * n * WT::BYTES;
	}
	__device__ __forceinline__ void finish(int g, const float *acc, int lane) const {
		if (lane == 0)
			out[g] += acc[0];
	}
	__device__ __forceinline__ void finish_all(int g, const float *acc) const { out[g] += acc[0]; }
	static constexpr bool PRE = true;
	__device__ __forceinline__ float pre(int g, int) const { return out[g]; }
	__device__ __forceinline__ void finish_pre(int g, const float *acc, const float *xr) const {
		out[g] = xr[0] + acc[0];
	}
};
