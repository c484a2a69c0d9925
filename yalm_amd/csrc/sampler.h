// sampler.h — temperature / top-k / top-p sampling on the device: one launch of one
// workgroup in the place of argmax_kernel, so a sampled decode step has the greedy step's
// launch count and only the token leaves the device.
//
// The rule is in integers, so it is independent of the reduction order and checkable exactly
// (tests/sampling_ref.py restates it in numpy):
//   m    = the first-maximum of the logits (argmax_block);
//   w_i  = expf((l_i - m) / T) (sampler.cpp:50, the division in f32), q_i = (uint64) ldexpf(w_i, 40),
//          0 when w_i is not a finite positive number;
//   order: logit descending as order-preserving 32-bit keys, index ascending among equal keys;
//   top-k keeps the first min(top_k, n) of that order (q sum S_k); top-p then the shortest prefix
//          of those whose q sum reaches need = min(S_k, max(1, ceil((double)top_p * (double)S_k)));
//          the kept set is always {i : key_i > K or (key_i == K and i <= istar)};
//   draw:  S = the kept q sum, t = min(S, max(1, ceil((double)u * (double)S))), the token is the
//          first kept i, ascending, whose inclusive kept prefix sum reaches t (sampler.cpp:53-57);
//   S == 0 (m not finite, all -inf): the first-maximum argmax.
// Every sum is a uint64 sum (below 2^57 for n <= 2^17): LDS integer atomics and any reduction
// tree give the same bits. No float atomics.
//
// Passes (each thread owns elements [4t, 4t + 4) of every 4096-element span, float4 loads, the
// logits are L2-resident): the maximum; K by a radix select over the keys, 12 + 10 + 10 bits, with
// count (top-k) or count and q (top-p) histograms in LDS, the crossing bin found by a block scan
// from the top bin down; istar by an index-order count scan over the elements equal to K, only
// when the cut falls inside a plateau of equal logits (equal keys have equal q, so the number of
// them to keep is one division); the token by per-span sums of the kept q and a block scan of the
// span the draw lands in. A select's second pass also copies the elements at or above the first
// digit's crossing bin to a list in LDS; when they fit (1024), its third pass and the top-p select
// after a top-k select read the list in the place of the logits. top_k == 0 and top_p == 1 skip the
// selects: two passes after the maximum.
#pragma once

#include <float.h>
#include <limits.h>

#include "device_common.h"
#include "misc_kernels.h"

// layout of yalm_sampling (include/yalm_hip.h), read from device memory so the step stays static
struct SampleParams {
	float temperature;
	int top_k;
	float top_p;
};

constexpr int SMP_THREADS = 1024;
constexpr int SMP_SPAN = 4 * SMP_THREADS;
constexpr int SMP_MAX_N = 131072;
constexpr int SMP_MAX_SPANS = SMP_MAX_N / SMP_SPAN;
constexpr int SMP_BINS = 4096;
constexpr int SMP_CAND = 1024; // candidate list: the elements at or above the first digit's crossing bin

struct SampleShared {
	unsigned long long hw[SMP_BINS]; // q per key digit
	unsigned hc[SMP_BINS];           // elements per key digit
	unsigned long long span[SMP_MAX_SPANS];
	unsigned long long wtot[SMP_THREADS / 64];
	// results of a block step, written by the one thread that found them
	unsigned long long res_wa, res_wt;
	unsigned res_ca, res_ct;
	int res_bin, res_idx;
	int ncand; // elements offered to the list; it is complete when ncand <= SMP_CAND
	int cand_i[SMP_CAND];
	float cand_l[SMP_CAND];
	float m;
	int amax;
};

// logit -> key: larger logit, larger key; -0 as +0; NaN below everything
__device__ __forceinline__ unsigned smp_key(float l) {
	if (l != l)
		return 0u;
	const unsigned u = __float_as_uint(l + 0.0f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long smp_q(float l, float m, float T) {
	const float w = expf((l - m) / T);
	return (w > 0.0f && w <= FLT_MAX) ? (unsigned long long)ldexpf(w, 40) : 0ull;
}

// f(i, l) for every element this thread owns, ascending; after the thread's 4 elements of span s, g(s).
// Both are called by every thread for every span (g may hold wave-wide operations).
// VEC: logits is 16-byte aligned (float4 loads); else the same elements one by one.
template <bool VEC, class F, class G>
__device__ __forceinline__ void smp_for_each(const float *__restrict__ logits, int n, F f, G g) {
	constexpr int B = 4; // spans in flight
	const int nsp = (n + SMP_SPAN - 1) / SMP_SPAN;
	for (int s0 = 0; s0 < nsp; s0 += B) {
		float v[B][4];
#pragma unroll
		for (int k = 0; k < B; ++k) {
			const int i0 = (s0 + k) * SMP_SPAN + 4 * (int)threadIdx.x;
			if (VEC && i0 + 3 < n) {
				const float4_t x = *(const float4_t *)(logits + i0);
#pragma unroll
				for (int e = 0; e < 4; ++e)
					v[k][e] = x[e];
			} else {
#pragma unroll
				for (int e = 0; e < 4; ++e)
					v[k][e] = i0 + e < n ? logits[i0 + e] : 0.0f;
			}
		}
#pragma unroll
		for (int k = 0; k < B; ++k) {
			if (s0 + k >= nsp)
				break;
			const int i0 = (s0 + k) * SMP_SPAN + 4 * (int)threadIdx.x;
#pragma unroll
			for (int e = 0; e < 4; ++e)
				if (i0 + e < n)
					f(i0 + e, v[k][e]);
			g(s0 + k);
		}
	}
}

// Inclusive scan of v over the workgroup in thread order; total = the sum. Called by all threads.
__device__ __forceinline__ unsigned long long smp_block_scan(unsigned long long v, SampleShared &sh,
                                                             unsigned long long &total) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned long long x = v;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const unsigned long long y = __shfl_up(x, off, 64);
		if (lane >= off)
			x += y;
	}
	__syncthreads(); // the previous scan's wave totals have been read
	if (lane == 63)
		sh.wtot[wave] = x;
	__syncthreads();
	unsigned long long pre = 0, tot = 0;
#pragma unroll
	for (int w = 0; w < SMP_THREADS / 64; ++w) {
		const unsigned long long t = sh.wtot[w];
		if (w < wave)
			pre += t;
		tot += t;
	}
	total = tot;
	return x + pre;
}

__device__ __forceinline__ unsigned long long smp_frac_target(double frac, unsigned long long S) {
	const unsigned long long c = (unsigned long long)ceil(frac * (double)S);
	const unsigned long long lo = c > 1ull ? c : 1ull;
	return lo < S ? lo : S;
}

// The histogram bin, walking from bin nb - 1 down, in which the running count (BY_W: q sum)
// reaches target (BY_W and frac >= 0: the target is smp_frac_target(frac, all q), returned in
// target with all q in total_w). Leaves the bin, the count and q above it and its own count and
// q in sh.res_*. false when there is nothing to reach (BY_W: the q sum is 0). Called by all threads.
template <bool BY_W>
__device__ __forceinline__ bool smp_crossing(SampleShared &sh, int nb, unsigned long long &target, double frac,
                                             unsigned long long &total_w) {
	const int per = nb / SMP_THREADS > 0 ? nb / SMP_THREADS : 1; // 4 or 1 bins per thread, descending
	unsigned long long mw = 0, mc = 0;
	for (int j = 0; j < per; ++j) {
		const int b = nb - 1 - ((int)threadIdx.x * per + j);
		if (b >= 0) {
			mc += sh.hc[b];
			if (BY_W)
				mw += sh.hw[b];
		}
	}
	unsigned long long tot_c = 0, tot_w = 0;
	const unsigned long long inc_c = smp_block_scan(mc, sh, tot_c);
	const unsigned long long inc_w = BY_W ? smp_block_scan(mw, sh, tot_w) : 0ull;
	total_w = tot_w;
	if (BY_W && frac >= 0.0)
		target = smp_frac_target(frac, tot_w);
	const unsigned long long tot = BY_W ? tot_w : tot_c;
	if (tot == 0 || target == 0 || target > tot)
		return false;
	const unsigned long long inc = BY_W ? inc_w : inc_c, mine = BY_W ? mw : mc;
	if (inc - mine < target && target <= inc) { // exactly one thread
		unsigned long long cw = inc_w - mw, cc = inc_c - mc;
		for (int j = 0; j < per; ++j) {
			const int b = nb - 1 - ((int)threadIdx.x * per + j);
			const unsigned long long bc = sh.hc[b], bw = BY_W ? sh.hw[b] : 0ull;
			if ((BY_W ? cw + bw : cc + bc) >= target) {
				sh.res_bin = b;
				sh.res_ca = (unsigned)cc;
				sh.res_wa = cw;
				sh.res_ct = (unsigned)bc;
				sh.res_wt = bw;
				break;
			}
			cw += bw;
			cc += bc;
		}
	}
	__syncthreads();
	return true;
}

// Radix select over the keys of the elements in_set(i, key): the key K at which the running
// count (BY_W: q sum), in descending key order, reaches target (BY_W: smp_frac_target(frac, the
// set's q sum), returned in target, the sum in set_w). ca / wa: the count and q of the set's keys
// above K, ct / wt: of its elements equal to K. The second pass also copies the set's elements
// at or above the first digit's crossing bin -- everything a later step can keep -- to the
// candidate list in LDS (any order: histograms do not care); when they fit, the third pass
// reads the list, and a later select whose set lies inside it (from_list) reads nothing else.
// Called by all threads.
template <bool BY_W, bool VEC, class P>
__device__ __forceinline__ bool smp_select(const float *__restrict__ logits, int n, float m, float T, P in_set,
                                           bool from_list, unsigned long long &target, double frac,
                                           unsigned long long &set_w, SampleShared &sh, unsigned &K,
                                           unsigned long long &ca, unsigned long long &wa, unsigned long long &ct,
                                           unsigned long long &wt) {
	unsigned prefix = 0;
	ca = 0;
	wa = 0;
	int hi = 32; // the key bits above hi are fixed to prefix
	for (int level = 0; level < 3; ++level) {
		const int bits = level == 0 ? 12 : 10, nb = 1 << bits, shift = hi - bits;
		for (int b = threadIdx.x; b < nb; b += SMP_THREADS) {
			sh.hc[b] = 0u;
			sh.hw[b] = 0ull;
		}
		const bool collect = level == 1 && !from_list;
		if (collect && threadIdx.x == 0)
			sh.ncand = 0;
		__syncthreads();
		auto body = [&](int i, float l) {
			const unsigned key = smp_key(l);
			if (!in_set(i, key))
				return;
			if (collect && (key >> hi) >= prefix) {
				const int at = atomicAdd(&sh.ncand, 1);
				if (at < SMP_CAND) {
					sh.cand_i[at] = i;
					sh.cand_l[at] = l;
				}
			}
			if (level == 0 || (key >> hi) == prefix) {
				const unsigned dgt = (key >> shift) & (unsigned)(nb - 1);
				atomicAdd(&sh.hc[dgt], 1u);
				if (BY_W) {
					const unsigned long long q = smp_q(l, m, T);
					if (q)
						atomicAdd(&sh.hw[dgt], q);
				}
			}
		};
		if (from_list || (level == 2 && sh.ncand <= SMP_CAND)) {
			const int nc = sh.ncand;
			for (int j = threadIdx.x; j < nc; j += SMP_THREADS)
				body(sh.cand_i[j], sh.cand_l[j]);
		} else {
			smp_for_each<VEC>(logits, n, body, [](int) {});
		}
		__syncthreads();
		unsigned long long tw = 0;
		if (!smp_crossing<BY_W>(sh, nb, target, level == 0 ? frac : -1.0, tw))
			return false;
		if (level == 0)
			set_w = tw;
		prefix = (prefix << bits) | (unsigned)sh.res_bin;
		ca += sh.res_ca;
		wa += sh.res_wa;
		ct = sh.res_ct;
		wt = sh.res_wt;
		target -= BY_W ? sh.res_wa : (unsigned long long)sh.res_ca;
		hi = shift;
		__syncthreads(); // res_* read before the next level writes them
	}
	K = prefix;
	return true;
}

// Per-span sums of val(i, l) into sh.span; returns their total. Called by all threads.
template <bool VEC, class V>
__device__ __forceinline__ unsigned long long smp_span_sums(const float *__restrict__ logits, int n, V val,
                                                            SampleShared &sh) {
	if (threadIdx.x < SMP_MAX_SPANS)
		sh.span[threadIdx.x] = 0ull;
	__syncthreads();
	unsigned long long acc = 0;
	smp_for_each<VEC>(
	    logits, n, [&](int i, float l) { acc += val(i, l); },
	    [&](int s) {
		    if (__ballot(acc != 0ull)) {
#pragma unroll
			    for (int off = 32; off > 0; off >>= 1)
				    acc += __shfl_xor(acc, off, 64);
			    if ((threadIdx.x & 63) == 0)
				    atomicAdd(&sh.span[s], acc);
		    }
		    acc = 0;
	    });
	__syncthreads();
	unsigned long long tot = 0;
	for (int s = 0; s < SMP_MAX_SPANS; ++s)
		tot += sh.span[s];
	return tot;
}

// After smp_span_sums(val): the first index, ascending, whose inclusive prefix sum of val reaches
// target (1 <= target <= the total). Called by all threads.
template <class V>
__device__ __forceinline__ int smp_locate(const float *__restrict__ logits, int n, V val, unsigned long long target,
                                          SampleShared &sh) {
	int s = 0;
	unsigned long long before = 0;
	const int nsp = (n + SMP_SPAN - 1) / SMP_SPAN;
	while (s < nsp - 1 && before + sh.span[s] < target) {
		before += sh.span[s];
		++s;
	}
	const unsigned long long rem = target - before;
	const int i0 = s * SMP_SPAN + 4 * (int)threadIdx.x;
	unsigned long long v[4], sum = 0;
#pragma unroll
	for (int e = 0; e < 4; ++e) {
		v[e] = i0 + e < n ? val(i0 + e, logits[i0 + e]) : 0ull;
		sum += v[e];
	}
	unsigned long long tot = 0;
	const unsigned long long inc = smp_block_scan(sum, sh, tot);
	if (threadIdx.x == 0)
		sh.res_idx = -1;
	__syncthreads();
	if (inc - sum < rem && rem <= inc) {
		unsigned long long c = inc - sum;
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			c += v[e];
			if (c >= rem) {
				sh.res_idx = i0 + e;
				break;
			}
		}
	}
	__syncthreads();
	return sh.res_idx;
}

// The first-maximum of logits[0, n) into sh.m / sh.amax, visible to every thread on return.
template <bool VEC>
__device__ __forceinline__ void smp_first_max(const float *__restrict__ logits, int n, SampleShared &sh) {
	float b = 0.0f;
	int idx = 0;
	argmax_block<VEC>(logits, n, b, idx);
	if (threadIdx.x == 0) {
		sh.m = b;
		sh.amax = idx;
	}
	__syncthreads();
}

struct SampleDraw {
	int token;
	long long kept; // the kept-set size
};

// The rule's draw from logits[0, n), n <= SMP_MAX_N, with the uniform u, after smp_first_max on
// the same logits. sh is this workgroup's alone. VEC: logits is 16-byte aligned. Called by all
// threads; every thread gets the result.
template <bool VEC>
__device__ __forceinline__ SampleDraw sample_row(const float *__restrict__ logits, int n, const SampleParams prm,
                                                 float u, SampleShared &sh) {
	const float m = sh.m, T = prm.temperature, top_p = prm.top_p;
	const int amax = sh.amax, top_k = prm.top_k;
	// the kept set {key > K or (key == K and i <= istar)}; everything to begin with
	unsigned K = 0;
	int istar = INT_MAX;
	long long kept = n;
	bool empty = false, have_list = false;
	unsigned long long ca, wa, ct, wt, target, set_w = 0;
	if (top_k > 0 && top_k < n) {
		target = (unsigned long long)top_k;
		unsigned K1 = 0;
		smp_select<false, VEC>(
		    logits, n, m, T, [](int, unsigned) { return true; }, false, target, -1.0, set_w, sh, K1, ca, wa, ct, wt);
		const unsigned long long r = (unsigned long long)top_k - ca; // of the ct elements equal to K1
		if (r < ct) {
			auto tie = [&](int, float l) { return smp_key(l) == K1 ? 1ull : 0ull; };
			smp_span_sums<VEC>(logits, n, tie, sh);
			istar = smp_locate(logits, n, tie, r, sh);
		}
		K = K1;
		kept = top_k;
		have_list = sh.ncand <= SMP_CAND; // holds the whole top-k set
	}
	if (top_p < 1.0f) {
		const unsigned K1 = K;
		const int i1 = istar;
		unsigned K2 = 0;
		target = 0;
		const bool ok = smp_select<true, VEC>(
		    logits, n, m, T, [&](int i, unsigned key) { return key > K1 || (key == K1 && i <= i1); }, have_list,
		    target, (double)top_p, set_w, sh, K2, ca, wa, ct, wt);
		if (!ok) { // S_k == 0: need is 0, the empty prefix
			empty = true;
			kept = 0;
		} else {
			const unsigned long long qK = wt / ct, need = smp_frac_target((double)top_p, set_w);
			unsigned long long r = (need - wa + qK - 1) / qK;
			r = r < 1 ? 1 : r > ct ? ct : r;
			if (r < ct) {
				auto tie = [&](int, float l) { return smp_key(l) == K2 ? 1ull : 0ull; };
				smp_span_sums<VEC>(logits, n, tie, sh);
				istar = smp_locate(logits, n, tie, r, sh);
			} else if (K2 != K1) {
				istar = INT_MAX;
			}
			K = K2;
			kept = (long long)(ca + r);
		}
	}

	int token = amax;
	if (!empty) {
		auto val = [&](int i, float l) {
			const unsigned key = smp_key(l);
			return key > K || (key == K && i <= istar) ? smp_q(l, m, T) : 0ull;
		};
		const unsigned long long S = smp_span_sums<VEC>(logits, n, val, sh);
		if (S > 0) {
			const int idx = smp_locate(logits, n, val, smp_frac_target((double)u, S), sh);
			if (idx >= 0)
				token = idx;
		}
	}
	return SampleDraw{token, kept};
}

// One sampled token from logits[0, n), n <= SMP_MAX_N: the uniform is uniforms[st->n_gen]
// (clamped to u_cap - 1), the token is committed like the greedy one (argmax_commit).
// kept_out (may be null): [st->n_gen] = the kept-set size; weights_out (may be null): every q_i.
__global__ __launch_bounds__(SMP_THREADS) void sample_kernel(const float *__restrict__ logits, int n,
                                                             const SampleParams *__restrict__ prm,
                                                             const float *__restrict__ uniforms, int u_cap,
                                                             StepState *st, int *__restrict__ tokens_out, int cap,
                                                             int *__restrict__ kept_out,
                                                             unsigned long long *__restrict__ weights_out) {
	__shared__ SampleShared sh;
	const int gen = st->n_gen; // read by every thread before thread 0 commits
	smp_first_max<true>(logits, n, sh);
	const float m = sh.m, T = prm->temperature, top_p = prm->top_p;
	const int top_k = prm->top_k;
	const int ui = gen < 0 ? 0 : gen < u_cap ? gen : u_cap - 1;
	const float u = uniforms[ui];
	if (weights_out)
		smp_for_each<true>(
		    logits, n, [&](int i, float l) { weights_out[i] = smp_q(l, m, T); }, [](int) {});
	const SampleDraw r = sample_row<true>(logits, n, SampleParams{T, top_k, top_p}, u, sh);
	if (threadIdx.x == 0) {
		if (kept_out && gen >= 0 && gen < cap)
			kept_out[gen] = (int)r.kept;
		argmax_commit(st, r.token, tokens_out, cap);
	}
}
