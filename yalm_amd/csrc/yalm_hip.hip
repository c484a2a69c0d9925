// yalm_hip.hip — C ABI (include/yalm_hip.h) of the MI355X decode engine:
// device shim, decoder (graph-captured per-token forward) and the kernel-level
// test API. Replaces /root/reference/src/infer.cu:33-90 (shim), 699-888
// (_block_cuda), 890-1019 (test API), 1021-1164 (_forward_cuda + CudaGraph)
// and the device upload of model.cpp:185-211, 323-345, 380-394.
#include "../../include/yalm_hip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "attention.h"
#include "attn_wo.h"
#include "batch.h"
#include "decoder.h"
#include "device_common.h"
#include "gemv.h"
#include "gemv_rows.h"
#include "misc_kernels.h"
#include "moe.h"
#include "qk_norm.h"
#include "sampler.h"
#include "spec.h"

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

void set_err(const std::string &s) {
	g_err = s;
}

extern "C" const char *yalm_last_error(void) {
	return g_err.c_str();
}

// ------------------------------------------------------------------ shim
extern "C" int yalm_set_device(int device) {
	HIPCHK(hipSetDevice(device));
	return YALM_OK;
}

extern "C" void *yalm_upload(const void *host, size_t size) {
	void *dev = nullptr;
	if (hipMalloc(&dev, size ? size : 1) != hipSuccess) {
		set_err("hipMalloc failed in yalm_upload");
		return nullptr;
	}
	if (size && hipMemcpy(dev, host, size, hipMemcpyHostToDevice) != hipSuccess) {
		set_err("hipMemcpy H2D failed in yalm_upload");
		(void)hipFree(dev);
		return nullptr;
	}
	return dev;
}

extern "C" void *yalm_alloc(size_t size) {
	void *dev = nullptr;
	if (hipMalloc(&dev, size ? size : 1) != hipSuccess) {
		set_err("hipMalloc failed in yalm_alloc");
		return nullptr;
	}
	if (hipMemset(dev, 0, size ? size : 1) != hipSuccess) {
		set_err("hipMemset failed in yalm_alloc");
		(void)hipFree(dev);
		return nullptr;
	}
	return dev;
}

extern "C" int yalm_download(void *host, const void *device, size_t size) {
	HIPCHK(hipMemcpy(host, device, size, hipMemcpyDeviceToHost));
	return YALM_OK;
}

extern "C" int yalm_register_host(void *host, size_t size) {
	HIPCHK(hipHostRegister(host, size, hipHostRegisterDefault));
	return YALM_OK;
}

extern "C" int yalm_unregister_host(void *host) {
	HIPCHK(hipHostUnregister(host));
	return YALM_OK;
}

extern "C" int yalm_free(void *device) {
	HIPCHK(hipFree(device));
	return YALM_OK;
}

extern "C" int yalm_stream_create(yalm_stream *out) {
	ARGCHK(out, "null stream out");
	hipStream_t s;
	HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
	*out = reinterpret_cast<yalm_stream>(s);
	return YALM_OK;
}

// A stream restricted to CU block `part` of `n_parts` (hipExtStreamCreateWithCUMask):
// bits [part * ncu / n_parts, (part + 1) * ncu / n_parts). The driver spreads such a block
// evenly over the 8 XCDs (tools/cumask_probe.hip, profiles/r6a_cumask_probe.txt: 256 / N CUs
// on all 8 XCCs, disjoint between parts); an interleaved mask (bit i to part i mod N) was
// not honoured (every part ran on all 256 CUs). Used to run N tensor-parallel rank
// processes on ONE GPU as N disjoint sets of CUs (the multi-GPU rehearsal).
extern "C" int yalm_stream_create_cu_part(int part, int n_parts, yalm_stream *out) {
	ARGCHK(out && n_parts >= 1 && part >= 0 && part < n_parts, "yalm_stream_create_cu_part: bad argument");
	const int ncu = device_cu_count();
	ARGCHK(ncu % n_parts == 0 && ncu <= 32 * YALM_CU_MASK_WORDS, "yalm_stream_create_cu_part: CUs do not divide");
	uint32_t m[YALM_CU_MASK_WORDS] = {};
	for (int i = part * (ncu / n_parts); i < (part + 1) * (ncu / n_parts); ++i)
		m[i / 32] |= 1u << (i % 32);
	hipStream_t s;
	HIPCHK(hipExtStreamCreateWithCUMask(&s, (uint32_t)((ncu + 31) / 32), m));
	*out = reinterpret_cast<yalm_stream>(s);
	return YALM_OK;
}

// The CUs a stream may run on (all of them for an ordinary stream).
static int stream_cu_mask(hipStream_t s, uint32_t *m) {
	const int ncu = device_cu_count();
	for (int i = 0; i < YALM_CU_MASK_WORDS; ++i)
		m[i] = 0;
	if (!s || hipExtStreamGetCUMask(s, (uint32_t)((ncu + 31) / 32), m) != hipSuccess) {
		(void)hipGetLastError();
		for (int i = 0; i < ncu && i < 32 * YALM_CU_MASK_WORDS; ++i)
			m[i / 32] |= 1u << (i % 32);
	}
	return YALM_OK;
}

extern "C" int yalm_stream_destroy(yalm_stream s) {
	HIPCHK(hipStreamDestroy(reinterpret_cast<hipStream_t>(s)));
	return YALM_OK;
}

extern "C" int yalm_stream_sync(yalm_stream s) {
	HIPCHK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(s)));
	return YALM_OK;
}

// a weight format of this library (each entry point first refuses the formats it has no form for)
static bool dtype_ok(int dtype) {
	return dtype == YALM_F32 || dtype == YALM_F16 || dtype == YALM_F8E5M2 || dtype == YALM_Q4 || dtype == YALM_E4M3;
}

extern "C" int yalm_synth(void *device, size_t n, int dtype, uint64_t seed, float scale, float offset, yalm_stream s) {
	ARGCHK(dtype != YALM_Q4, "yalm_synth: q4 tensors need their row length (yalm_synth_q4)");
	ARGCHK(dtype != YALM_E4M3, "yalm_synth: e4m3 tensors need their row length (yalm_synth_e4m3)");
	ARGCHK(dtype_ok(dtype), "yalm_synth: bad dtype");
	hipStream_t st = reinterpret_cast<hipStream_t>(s);
	synth_kernel<<<4096, 256, 0, st>>>(device, n, dtype, seed, scale, offset);
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

extern "C" size_t yalm_row_bytes(int dtype, int n) {
	if (n <= 0)
		return 0;
	switch (dtype) {
	case YALM_F32:
		return (size_t)n * 4;
	case YALM_F16:
		return (size_t)n * 2;
	case YALM_F8E5M2:
		return (size_t)n;
	case YALM_Q4:
		return n % 32 ? 0 : q4_row_bytes(n);
	case YALM_E4M3:
		return n % 16 ? 0 : WE4M3::row_bytes(n);
	}
	return 0;
}

// The f16 with the low 3 mantissa bits zero nearest the f16 nearest v (bits + 4, low bits
// cleared: a carry moves into the exponent as it should); models.q4_restrict_scale.
static uint16_t q4_restricted_f16(float v) {
	const _Float16 h = (_Float16)v;
	uint16_t b;
	memcpy(&b, &h, 2);
	return (uint16_t)((b + 4u) & ~7u);
}

extern "C" int yalm_synth_q4(void *device, size_t rows, int n, uint64_t seed, float scale, yalm_stream s) {
	ARGCHK(device && rows > 0 && n > 0 && n % 32 == 0, "yalm_synth_q4: rows > 0 and a row length that is a multiple of 32 (q4)");
	hipStream_t st = reinterpret_cast<hipStream_t>(s);
	synth_q4_kernel<<<4096, 256, 0, st>>>((u32x4_t *)device, rows, n, seed, q4_restricted_f16(scale / 7.0f));
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

// Every row's scale: the power of two 2^k, -15 <= k <= 7, that puts 448 (the largest code) at or
// just above `scale`; models.synth_e4m3_scale.
static float e4m3_synth_scale(float scale) {
	int k = -15;
	while (k < 7 && ldexpf(448.0f, k) < scale)
		++k;
	return ldexpf(1.0f, k);
}

extern "C" int yalm_synth_e4m3(void *device, size_t rows, int n, uint64_t seed, float scale, yalm_stream s) {
	ARGCHK(device && rows > 0 && n > 0 && n % 16 == 0,
	       "yalm_synth_e4m3: rows > 0 and a row length that is a multiple of 16 (e4m3)");
	hipStream_t st = reinterpret_cast<hipStream_t>(s);
	synth_e4m3_kernel<<<4096, 256, 0, st>>>((u32x4_t *)device, rows, n, seed, e4m3_synth_scale(scale));
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

// ------------------------------------------------------------------ launch helpers
int device_cu_count() {
	static int n = 0;
	if (!n) {
		int dev = 0;
		if (hipGetDevice(&dev) != hipSuccess ||
		    hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
			n = 256;
	}
	return n;
}

// Row-block geometry (gemv_rb_kernel): `gpw` = workgroups per CU (default 1),
// threads 512 (8 waves), U = 8 loads in flight per wave. Whole-row mode (gemv.h ROWS) for the
// policies that declare ROWS_MODE when the rows divide evenly over the waves.

// One launch of gemv_rb_kernel; a consumer of an IPC exchange (tin.n > 0, always a
// normalising GEMV: QKV, W1|W3, logits) runs the TIN instantiation.
template <class WT, class P, bool NORM, int THREADS, int U, bool ROWS>
static int launch_rb_k(const P &p, const float *x, const float *normw, float eps, int nb, size_t lds, hipStream_t st,
                       const TpX &tin) {
	auto kern = gemv_rb_kernel<WT, P, U, NORM, THREADS, ROWS>;
	if constexpr (NORM && !gemv_local_x<P>::value && !WT::Q4 && !WT::ROW_SCALE) { // (q4, e4m3: no tensor-parallel form)
		if (tin.n > 0)
			kern = gemv_rb_kernel<WT, P, U, NORM, THREADS, ROWS, true>;
	} else if (tin.n > 0) {
		set_err("internal: an exchange consumer must be a normalising GEMV");
		return YALM_ERR_UNSUPPORTED;
	}
	if (lds > 65536)
		HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	hipLaunchKernelGGL(kern, dim3(nb), dim3(THREADS), lds, st, p, x, normw, eps, tin);
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

// The geometry of one single-row GEMV launch (launch_gemv: gemv_kernel when the row is no whole
// number of CH-element chunks, else gemv_rb_kernel) over n_groups groups of R rows of n elements.
// `def` is the kind's default {threads, U, workgroups per CU}, `want` what the caller overrides
// (0: the default), with want.cus CUs (0: this device's) and want.rows (-1: whole-row mode where
// rows_ok and the rows divide; 0: chunk order). Pure host arithmetic when want.cus > 0.
struct GemvPlan {
	bool generic, rows, xregs;
	int threads, U, nb;    // block, loads in flight, grid
	int ngl_min, ngl_max;  // groups of a workgroup, the fewest and the most
	size_t lds;            // dynamic LDS bytes
};
static GemvPlan gemv_plan(int CH, bool q4, int R, bool rows_ok, bool norm, int n, int n_groups, const GemvCfg &def,
                          const GemvCfg &want, bool tin) {
	GemvPlan g{};
	const size_t xl = q4 ? (size_t)xs_len<true>(n) : (size_t)xs_len<false>(n);
	if (n % CH != 0) { // ragged K: generic kernel (tests / unusual shapes), one group per wave
		constexpr int W = GEMV_THREADS / YALM_WAVE;
		g.generic = true;
		g.threads = GEMV_THREADS;
		g.U = 4;
		g.nb = (n_groups + W - 1) / W;
		g.ngl_max = std::min(n_groups, W);
		g.ngl_min = n_groups - (g.nb - 1) * W;
		g.lds = xl * sizeof(float) + 64 * sizeof(float);
		return g;
	}
	const int threads = want.threads ? want.threads : def.threads;
	const int U = want.U ? want.U : def.U;
	const int wpc = want.gpw ? want.gpw : def.gpw;
	g.threads = threads == 256 || threads == 1024 ? threads : 512;
	g.U = U == 2 || U == 8 ? U : 4;
	const int W = g.threads / YALM_WAVE;
	const int cus = want.cus > 0 ? want.cus : device_cu_count();
	// an exchange consumer stages x from the exchange once per CU: one workgroup per CU
	g.nb = std::max(1, std::min(n_groups, cus * (tin ? 1 : std::max(1, wpc))));
	const int ngl = (n_groups + g.nb - 1) / g.nb;
	g.ngl_max = ngl;
	g.ngl_min = n_groups / g.nb;
	g.lds = (xl + 64 + (size_t)ngl * R * W) * sizeof(float);
	// every workgroup the same number of rows and a whole number of rows, at least 2,
	// per wave (profiles/r3_gemv_rows.txt: W1|W3 fp16 39.4-40.0 -> 36.9 us, fp8 W2 13.4 ->
	// 12.7-13.0; fp16 W2 with ONE 28-KB row per wave went 20.3 -> 21.3, so it keeps the
	// chunk order); YALM_GEMV_ROWS=0 keeps the chunk order everywhere (A/B)
	const bool rows_on = want.rows != 0 && (!ab_env("YALM_GEMV_ROWS") || atoi(ab_env("YALM_GEMV_ROWS")) != 0);
	g.rows = rows_ok && rows_on && n_groups % g.nb == 0 && (ngl * R) % W == 0 && ngl * R >= 2 * W;
	const int xpre = g.threads == 256    ? (norm ? xpre_n<true, 256>() : xpre_n<false, 256>())
	                 : g.threads == 1024 ? (norm ? xpre_n<true, 1024>() : xpre_n<false, 1024>())
	                                     : (norm ? xpre_n<true, 512>() : xpre_n<false, 512>());
	g.xregs = !tin && n <= 4 * xpre * g.threads; // (the kernel's own test)
	return g;
}

template <class WT, class P, bool NORM, int THREADS, int U>
static int launch_rb_t(const P &p, const float *x, const float *normw, float eps, const GemvPlan &g, hipStream_t st,
                       const TpX &tin) {
	if constexpr (gemv_rows_mode<P>::value) {
		if (g.rows)
			return launch_rb_k<WT, P, NORM, THREADS, U, true>(p, x, normw, eps, g.nb, g.lds, st, tin);
	}
	return launch_rb_k<WT, P, NORM, THREADS, U, false>(p, x, normw, eps, g.nb, g.lds, st, tin);
}

// Per-kind, per-weight-type defaults from tools/sweep_gemv.py on MI355X
// (profiles/r1_sweep_rb*.txt): {threads, U, workgroups per CU}.
// fp8 (E5M2, e4m3) and q4: more ALU per byte than f16 / f32
template <class WT>
constexpr bool wt_narrow() {
	if constexpr (WT::Q4 || WT::ROW_SCALE)
		return true;
	else
		return WT::BYTES == 1;
}
template <class WT>
static GemvCfg default_rb_cfg(int kind) {
	if constexpr (WT::Q4) { // tools/sweep_gemv.py --dtype q4 (profiles/q4_sweep.txt): the unpack is the work
		switch (kind) {
		case GK_QKV: // 7.96 us vs 8.67 for fp8's {512, 4, 1}
			return GemvCfg{512, 2, 1};
		case GK_WO: // 5.80 vs 6.76 for {512, 2, 2}
			return GemvCfg{512, 4, 1};
		case GK_GLU: // 17.33 vs 20.31 for {512, 4, 1}
			return GemvCfg{512, 2, 2};
		case GK_W2: // 11.33 vs 11.63 for {512, 4, 1}
			return GemvCfg{512, 2, 1};
		default: // logits: 20.63 vs 22.44 for {512, 2, 2}
			return GemvCfg{512, 4, 3};
		}
	}
	if constexpr (wt_narrow<WT>()) { // fp8 (e4m3 takes E5M2's: the same chunk): more ALU per byte -> fewer loads in flight per lane
		switch (kind) {
		case GK_W2:
			return GemvCfg{512, 4, 1};
		case GK_GLU: // round 3, whole-row mode (14 rows per wave): 20.5 us vs 21.4-21.6 for {512, 2, 2}
			return GemvCfg{512, 4, 1};
		case GK_QKV: // round 3, whole-row mode (3 rows per wave): 7.6 us vs 8.0-8.4 for {512, 2, 2}
			return GemvCfg{512, 4, 1};
		default:
			return GemvCfg{512, 2, 2};
		}
	}
	switch (kind) {
	case GK_QKV: // one workgroup per CU: 24 rows each = 3 whole rows per wave (ROWS mode),
	             // 10.6-10.7 vs 11.2-11.4 us for {512, 2, 2} (profiles/r3_gemv_rows.txt)
		return GemvCfg{512, 4, 1};
	case GK_WO:
		return GemvCfg{1024, 2, 2};
	case GK_W2:
		return GemvCfg{1024, 2, 1};
	case GK_CLS:
		return GemvCfg{512, 4, 4};
	default:
		return GemvCfg{512, 4, 1};
	}
}

// the plan of launch_gemv<WT, P, NORM>
template <class WT, class P>
static GemvPlan gemv_plan_of(bool norm, int n, int n_groups, int kind, const GemvCfg &want, bool tin) {
	return gemv_plan(YALM_WAVE * WT::EPL, WT::Q4, P::R, gemv_rows_mode<P>::value, norm, n, n_groups, default_rb_cfg<WT>(kind),
	                 want, tin);
}

template <class WT, class P, bool NORM, int THREADS>
static int launch_rb_u(const P &p, const float *x, const float *normw, float eps, const GemvPlan &g, hipStream_t st,
                       const TpX &tin) {
	switch (g.U) {
	case 2:
		return launch_rb_t<WT, P, NORM, THREADS, 2>(p, x, normw, eps, g, st, tin);
	case 8:
		return launch_rb_t<WT, P, NORM, THREADS, 8>(p, x, normw, eps, g, st, tin);
	default:
		return launch_rb_t<WT, P, NORM, THREADS, 4>(p, x, normw, eps, g, st, tin);
	}
}

template <class WT, class P, bool NORM>
static int launch_rb_g(const P &p, const float *x, const float *normw, float eps, const GemvPlan &g, hipStream_t st,
                       const TpX &tin) {
	if (g.generic) {
		set_err("internal: the row-block GEMV needs rows of whole chunks");
		return YALM_ERR_UNSUPPORTED;
	}
	if (g.threads == 256)
		return launch_rb_u<WT, P, NORM, 256>(p, x, normw, eps, g, st, tin);
	if (g.threads == 1024)
		return launch_rb_u<WT, P, NORM, 1024>(p, x, normw, eps, g, st, tin);
	return launch_rb_u<WT, P, NORM, 512>(p, x, normw, eps, g, st, tin);
}

template <class WT, class P, bool NORM>
static int launch_rb(const P &p, const float *x, const float *normw, float eps, int kind, GemvCfg want,
                     hipStream_t st, const TpX &tin) {
	return launch_rb_g<WT, P, NORM>(p, x, normw, eps, gemv_plan_of<WT, P>(NORM, p.n, p.n_groups, kind, want, tin.n > 0),
	                                st, tin);
}

// tin: the exchange this launch consumes (tensor parallelism over IPC), default none
template <class WT, class P, bool NORM>
static int launch_gemv(const P &p, const float *x, const float *normw, float eps, int kind, GemvCfg want,
                       hipStream_t st, const TpX &tin = TpX{}) {
	const GemvPlan g = gemv_plan_of<WT, P>(NORM, p.n, p.n_groups, kind, want, tin.n > 0);
	if (g.generic) {
		if (tin.n > 0) {
			set_err("tensor parallel: dim must be a multiple of 64 x elements per 16 bytes");
			return YALM_ERR_UNSUPPORTED;
		}
		auto kern = gemv_kernel<WT, P, 4, NORM>;
		if (g.lds > 65536)
			HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
		hipLaunchKernelGGL(kern, dim3(g.nb), dim3(GEMV_THREADS), g.lds, st, p, x, normw, eps, 1);
		HIPCHK(hipGetLastError());
		return YALM_OK;
	}
	return launch_rb_g<WT, P, NORM>(p, x, normw, eps, g, st, tin);
}

// The decoder's weight-streaming GEMVs: gemv_rb_kernel with the geometry set
// through yalm_set_gemv_config (or the per-kind default).
template <class WT, class P, bool NORM>
static int launch_gemv_d(yalm_decoder_s *d, const P &p, const float *x, const float *normw, float eps, int kind,
                         const TpX &tin = TpX{}) {
	return launch_gemv<WT, P, NORM>(p, x, normw, eps, kind, d->gemv[kind], d->stream, tin);
}

// ---- the policies, filled: the forward, the timing hook and the host-pointer test entry points
// all build theirs here. `rows` weight rows of n elements each.
template <class WT, int R>
static PStore<WT, R> make_store(const void *W, int n, float *out, int rows) {
	return {(const char *)W, n, out, rows / R};
}
template <class WT>
static PResidual<WT, 1> make_residual(const void *W, int n, float *out, int rows) {
	return {(const char *)W, n, out, rows};
}
template <class WT>
static PAddTo<WT, 1> make_addto(const void *W, int n, float *out, const float *base, int rows) {
	return {(const char *)W, n, out, base, rows};
}
template <class WT>
static PPush<WT, 1> make_push(const void *W, int n, const float *base, const TpX &t, int rows) {
	return {(const char *)W, n, base, t, 0, rows};
}
template <class WT>
static PQKV<WT> make_pqkv(const void *wq, const void *wk, const void *wv, int n, int n_heads, int n_kv_heads,
                          int head_dim, float qkv_clip, const float *inv_freq, const StepState *step, float *q_out,
                          uint16_t *kcache, uint16_t *vcache) {
	const int q_dim = n_heads * head_dim, kv_dim = n_kv_heads * head_dim;
	return {(const char *)wq, (const char *)wk, (const char *)wv, n, q_dim, kv_dim, head_dim, (q_dim + 2 * kv_dim) / 2,
	        qkv_clip, inv_freq, step, q_out, kcache, vcache};
}
// W1 | W3 + GLU: the one place that maps `act` to PGlu's template argument
template <class WT, bool NORM>
static int launch_glu(const void *w1, const void *w3, int n, float *out, int hidden, int act, const float *x,
                      const float *normw, float eps, int kind, const GemvCfg &want, hipStream_t st,
                      const TpX &tin = TpX{}) {
	if (act == YALM_SILU)
		return launch_gemv<WT, PGlu<WT, 1>, NORM>({(const char *)w1, (const char *)w3, n, out, hidden}, x, normw, eps, kind,
		                                          want, st, tin);
	return launch_gemv<WT, PGlu<WT, 0>, NORM>({(const char *)w1, (const char *)w3, n, out, hidden}, x, normw, eps, kind,
	                                          want, st, tin);
}

// ---- mixture of experts (moe.h): router, the selected experts' W1 | W3 + GLU, their W2
struct MoeArgs {
	const void *gate, *w1, *w2, *w3; // moegate (E, dim); stacked (E, hidden, dim) / (E, dim, hidden)
	int E, K, hidden, dim, act;
	int *experts;   // the layer's routing slot [K]
	float *weights; // [K]
	float *hb;      // [K * hidden]
};

#define MOE_LDS_BYTES (160 * 1024) // LDS of one gfx950 CU

// W2 of all K selected experts as ONE launch of row length K * hidden: every 64-lane chunk must
// lie inside one expert's row, the launch addresses at most MOE_SEL_REGS experts, and hb plus the partial slots (at most 16 waves) must fit the LDS.
template <class WT>
static bool moe_w2_one_launch(const MoeArgs &a) {
	constexpr int CH = YALM_WAVE * WT::EPL;
	if (a.hidden % CH != 0 || a.K > MOE_SEL_REGS)
		return false;
	const int ncu = device_cu_count();
	const size_t ngl = a.dim <= ncu ? 1 : (a.dim + ncu - 1) / ncu;
	return ((size_t)a.K * a.hidden + 64 + ngl * 16) * sizeof(float) <= MOE_LDS_BYTES;
}

template <class WT, bool NORM>
static int launch_moe_router(const MoeArgs &a, const float *x, const float *normw, float eps, hipStream_t st) {
	const size_t lds = ((size_t)((a.dim + 3) & ~3) + 64 + MOE_MAX_EXPERTS) * sizeof(float);
	auto kern = moe_router_kernel<WT, NORM>;
	if (lds > 65536)
		HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	hipLaunchKernelGGL(kern, dim3(1), dim3(MOE_ROUTER_THREADS), lds, st, (const char *)a.gate, x, normw, eps, a.dim, a.E,
	                   a.K, a.experts, a.weights);
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

template <class WT, bool NORM, int ACT>
static int launch_moe_glu_act(const MoeArgs &a, const float *x, const float *normw, float eps, GemvCfg cfg,
                              hipStream_t st) {
	for (int k0 = 0; k0 < a.K; k0 += MOE_SEL_REGS) { // one launch per MOE_SEL_REGS selected experts
		const int cnt = std::min(MOE_SEL_REGS, a.K - k0);
		PMoeGlu<WT, ACT> p;
		p.w1 = (const char *)a.w1;
		p.w3 = (const char *)a.w3;
		p.n = a.dim;
		p.out = a.hb + (size_t)k0 * a.hidden;
		p.n_groups = cnt * a.hidden;
		p.hidden = a.hidden;
		p.sel = MoeSel{a.experts + k0, a.weights + k0, a.E, cnt};
		TRY((launch_gemv<WT, PMoeGlu<WT, ACT>, NORM>(p, x, normw, eps, GK_GLU, cfg, st)));
	}
	return YALM_OK;
}
template <class WT, bool NORM>
static int launch_moe_glu(const MoeArgs &a, const float *x, const float *normw, float eps, GemvCfg cfg, hipStream_t st) {
	return a.act == YALM_SILU ? launch_moe_glu_act<WT, NORM, 1>(a, x, normw, eps, cfg, st)
	                          : launch_moe_glu_act<WT, NORM, 0>(a, x, normw, eps, cfg, st);
}

// out[row] += sum_k W2[e_k][row] . hb_k
template <class WT>
static int launch_moe_w2(const MoeArgs &a, float *out, GemvCfg cfg, hipStream_t st) {
	if (moe_w2_one_launch<WT>(a)) {
		PMoeW2<WT> p;
		p.W = (const char *)a.w2;
		p.n = a.K * a.hidden;
		p.out = out;
		p.n_groups = a.dim;
		p.hidden = a.hidden;
		p.sel = MoeSel{a.experts, a.weights, a.E, a.K};
		return launch_rb<WT, PMoeW2<WT>, false>(p, a.hb, nullptr, 0.f, GK_W2, cfg, st, TpX{});
	}
	for (int k = 0; k < a.K; ++k) { // one launch per selected expert, in selection order
		PMoeW2One<WT> p;
		p.W = (const char *)a.w2;
		p.n = a.hidden;
		p.out = out;
		p.n_groups = a.dim;
		p.sel = MoeSel{a.experts + k, a.weights + k, a.E, 1};
		TRY((launch_gemv<WT, PMoeW2One<WT>, false>(p, a.hb + (size_t)k * a.hidden, nullptr, 0.f, GK_W2, cfg, st)));
	}
	return YALM_OK;
}

static int validate_moe(int n_experts, int n_active) {
	ARGCHK(n_experts >= 1 && n_experts <= MOE_MAX_EXPERTS && n_active >= 1 && n_active <= n_experts,
	       "mixture of experts: need 1 <= n_experts_active <= n_experts <= 64");
	return YALM_OK;
}

static bool attn_supported(int head_dim, int G) {
	return (head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128 || head_dim == 256) && G >= 1 &&
	       G <= 8;
}

// head mode up to this many 64-key chunks (attention.h attn_decode_body; A/B build:
// YALM_ATTN_HEADMAX). At least 1 (one chunk is key split 0 alone: the same work with a
// merger hop more), and every context with one key split (S = 1): key mode needs two.
// (A kernel-side `ns == 1 ||` cost the attention 44 VGPRs: 192 -> 236.)
static int attn_head_max(int S, int nchunks) {
	static const int h = ab_env("YALM_ATTN_HEADMAX") ? atoi(ab_env("YALM_ATTN_HEADMAX")) : ATTN_HEAD_MAX;
	return S <= 1 ? nchunks : std::max(1, h);
}

template <int D>
static void launch_attn_D(int G, const float *q, const uint16_t *kc, const uint16_t *vc, const StepState *step,
                          int n_heads, int n_kv, int max_seq_len, int nsplit, unsigned long long *part, int layer,
                          int n_layers, unsigned *err, float *att, float *out, hipStream_t st) {
	// S key-chunk splits per kv head, each workgroup looping over chunks s, s + S, ...: a grid
	// sized for max_seq_len would issue the speculative first-chunk loads of every idle
	// workgroup (15.6 MB of dead KV reads per layer at max_seq_len 4096, kv_len ~150).
	static const int splits = ab_env("YALM_ATTN_SPLITS") ? std::max(1, std::min(ATTN_MAX_SPLITS, atoi(ab_env("YALM_ATTN_SPLITS")))) : ATTN_SPLITS;
	const int nchunks = (max_seq_len + attn_chunk<D>() - 1) / attn_chunk<D>();
	const int S = std::min(nchunks, splits);
	const int grid = n_kv * (S + G - 1) + n_heads; // head + split units, then one merger per query head
	const int hmax = attn_head_max(S, nchunks);
#define YALM_ATTN(GT)                                                                                                  \
	attn_decode_kernel<D, GT><<<grid, ATTN_THREADS, 0, st>>>(q, kc, vc, step, n_heads, n_kv, max_seq_len, nsplit, S, \
	                                                         hmax, part, layer, n_layers, err, out, att)
	if (G <= 1)
		YALM_ATTN(1);
	else if (G <= 2)
		YALM_ATTN(2);
	else if (G <= 4)
		YALM_ATTN(4);
	else
		YALM_ATTN(8);
#undef YALM_ATTN
}

// partial-buffer stride: chunks per kv head (the chunk is 64 keys for every head_dim)
static int attn_nsplit(int max_seq_len) {
	return (max_seq_len + attn_chunk<128>() - 1) / attn_chunk<128>();
}

// part: (n_heads, nsplit, head_dim + 2) granules (zeroed once; tags never repeat);
// err: error word (bit 2: a merger gave up waiting).
static int launch_attn(int head_dim, int n_heads, int n_kv, const float *q, const uint16_t *kc, const uint16_t *vc,
                       const StepState *step, int max_seq_len, unsigned long long *part, int layer, int n_layers,
                       unsigned *err, float *att,
                       float *out, hipStream_t st) {
	const int G = n_heads / n_kv;
	const int nsplit = attn_nsplit(max_seq_len);
	switch (head_dim) {
	case 16:
		launch_attn_D<16>(G, q, kc, vc, step, n_heads, n_kv, max_seq_len, nsplit, part, layer, n_layers, err, att,
		                   out, st);
		break;
	case 32:
		launch_attn_D<32>(G, q, kc, vc, step, n_heads, n_kv, max_seq_len, nsplit, part, layer, n_layers, err, att,
		                   out, st);
		break;
	case 64:
		launch_attn_D<64>(G, q, kc, vc, step, n_heads, n_kv, max_seq_len, nsplit, part, layer, n_layers, err, att,
		                   out, st);
		break;
	case 128:
		launch_attn_D<128>(G, q, kc, vc, step, n_heads, n_kv, max_seq_len, nsplit, part, layer, n_layers, err, att,
		                   out, st);
		break;
	case 256:
		launch_attn_D<256>(G, q, kc, vc, step, n_heads, n_kv, max_seq_len, nsplit, part, layer, n_layers, err, att,
		                   out, st);
		break;
	default:
		set_err("unsupported head_dim");
		return YALM_ERR_UNSUPPORTED;
	}
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

// ---- attention + Wo in one launch (attn_wo.h)
template <class WT, int GT, int KB>
static const void *attn_wo_fn() {
	return (const void *)attn_wo_kernel<WT, GT, KB>;
}
template <class WT, int KB>
static const void *attn_wo_fn_g(int G) {
	return G <= 1 ? attn_wo_fn<WT, 1, KB>() : G <= 2 ? attn_wo_fn<WT, 2, KB>() : G <= 4 ? attn_wo_fn<WT, 4, KB>()
	                                                                         : attn_wo_fn<WT, 8, KB>();
}
template <class WT>
static const void *attn_wo_fn_kb(int G, int KB) {
	return KB == 1 ? attn_wo_fn_g<WT, 1>(G) : KB == 2 ? attn_wo_fn_g<WT, 2>(G) : KB == 4 ? attn_wo_fn_g<WT, 4>(G)
	                                                                            : attn_wo_fn_g<WT, 8>(G);
}
static const void *attn_wo_pick(int dtype, int G, int KB) {
	if (dtype == YALM_E4M3) // one GPU only: rows of 4 or 8 KiB of codes
		return KB == 4 ? attn_wo_fn_g<WE4M3, 4>(G) : attn_wo_fn_g<WE4M3, 8>(G);
	return dtype == YALM_F16 ? attn_wo_fn_kb<WF16>(G, KB) : attn_wo_fn_kb<WF8>(G, KB);
}
// The fused launch's plan for a (per-rank) config: 1 with the key splits S and the grid,
// or 0 = separate attention and Wo launches. Fused needs head_dim 128, G <= 8, fp16 / fp8
// Wo rows of 1, 2, 4 or 8 KiB (one GPU: 4 / 8; a tensor-parallel rank's Wo slice: 1 / 2 too)
// or e4m3 Wo rows of 4 or 8 KiB of codes (the format has no tensor-parallel form),
// and the whole grid (attention, one merger per query head, Wo)
// within the co-resident workgroup slots: a workgroup past them is dispatched only when
// an earlier one exits, and at short contexts every attention workgroup without keys
// still holds its slot for the kv_len load (S 32 at Mistral: 256 + 32 + 256 = 544 > 512
// slots put the last 32 Wo slices ~2 us late, fused launch 8.9 -> 11.2 us at kv 17). When
// fewer than 2 key splits fit (dim 8192 has 512 Wo workgroups) the fused launch
// would run every context in head mode -- one workgroup per query head over all the
// chunks -- so the separate launches (standalone attention at ATTN_SPLITS) are kept.
// Pure host arithmetic (tests/test_abi.py calls it without a GPU).
extern "C" int yalm_attn_wo_plan(const yalm_config *cp, int slots, int *splits, int *grid) {
	if (!cp || slots <= 0)
		return 0;
	const yalm_config &c = *cp;
	if (c.head_dim != 128 || c.n_kv_heads <= 0 || c.n_heads % c.n_kv_heads)
		return 0;
	const int G = c.n_heads / c.n_kv_heads;
	if (G < 1 || G > 8 ||
	    (c.weight_dtype != YALM_F16 && c.weight_dtype != YALM_F8E5M2 && c.weight_dtype != YALM_E4M3))
		return 0;
	const int rb = c.n_heads * c.head_dim * (c.weight_dtype == YALM_F16 ? 2 : 1);
	if ((rb != 1024 && rb != 2048 && rb != 4096 && rb != 8192) || c.dim < AWO_RPW)
		return 0;
	if (c.weight_dtype == YALM_E4M3 && rb < 4096)
		return 0;
	const int nchunks = (c.max_seq_len + attn_chunk<128>() - 1) / attn_chunk<128>();
	const int n_wo = (c.dim + AWO_RPW - 1) / AWO_RPW;
	const int fit = (slots - c.n_heads - n_wo) / c.n_kv_heads - (G - 1); // key splits: S + G - 1 units per kv head
	const char *senv = ab_env("YALM_AWO_SPLITS");
	const int S = std::max(1, std::min(nchunks, senv ? std::max(1, std::min(ATTN_MAX_SPLITS, atoi(senv)))
	                                                 : std::min(ATTN_SPLITS, fit)));
	if (!senv && fit < 2 && nchunks > ATTN_HEAD_MAX)
		return 0;
	if (splits)
		*splits = S;
	if (grid)
		*grid = c.n_kv_heads * (S + G - 1) + c.n_heads + n_wo;
	return 1;
}

// Decoders whose plan (yalm_attn_wo_plan, on the per-rank config) fuses: one GPU, and
// (round 5) every tensor-parallel rank too -- the Wo workgroups then write the rank's
// partial for the all-reduce (RCCL) or push it to the exchange (IPC, tp_exchange.h).
static int attn_wo_init(yalm_decoder_s *d) {
	const yalm_config &c = d->c;
	if (c.head_dim != 128)
		return YALM_OK;
	const int G = c.n_heads / c.n_kv_heads;
	const int rb = c.n_heads * c.head_dim * (c.weight_dtype == YALM_F16 ? 2 : 1);
	if (!yalm_attn_wo_plan(&c, 1 << 30, nullptr, nullptr))
		return YALM_OK;
	int occ = 0; // the Wo workgroups spin, but only on attention workgroups dispatched before them
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, attn_wo_pick(c.weight_dtype, G, rb / 1024), ATTN_THREADS,
	                                                 0) != hipSuccess ||
	    occ < 1)
		return YALM_OK;
	if (!yalm_attn_wo_plan(&c, occ * device_cu_count(), &d->awo_S, &d->awo_nb))
		return YALM_OK;
	d->awo_slots = occ * device_cu_count();
	// per layer: the attention output as {value, epoch} granules (zero tags never match:
	// the epoch is >= 1 from the first forward / yalm_block on)
	const size_t gran = (size_t)c.n_layers * c.n_heads * c.head_dim;
	TRY(dalloc(d, (void **)&d->awo_gran, sizeof(unsigned long long) * gran));
	const char *denv = ab_env("YALM_ATTN_WO_DELAY");
	// default 0.2 us (fp16) / 0.5 us (fp8): the attention workgroups' K/V loads reach HBM
	// ahead of the Wo stream. fp16 (33.5 MB, slice lands ~5.4 us, after the heads):
	// profiles/r2_sweep_awo_delay.txt 10.6 -> 10.1 us at kv_len 17. fp8 (16.8 MB, slice lands
	// ~3.1 us, before the heads): 0.5 us gives 9.4 -> 8.4 us at kv 17, 11.3 -> 10.3 at kv 151,
	// 579 -> 586 tok/s (profiles/r3_ab_awo_delay.txt); fp16 at 0.5 us is within noise
	const bool fp8 = c.weight_dtype == YALM_F8E5M2 || c.weight_dtype == YALM_E4M3; // (e4m3: the same slice bytes)
	d->awo_delay = denv ? std::max(0, atoi(denv)) : (fp8 ? 50 : 20);
	d->awo_delay_short = denv ? -1 : (fp8 ? 0 : -1);
	// Removed in round 4 (measured losers, round 3, profiles/r3_ab_awo*.txt): the combined
	// first gather attempt (YALM_AWO_SPEC), per-XCD copies of the head outputs
	// (YALM_AWO_REPL) and a sliding window on the Wo slice loads (YALM_ATTN_WO_WIN)
	const char *tenv = ab_env("YALM_ATTN_WO_TRACE");
	if (tenv && atoi(tenv) != 0)
		TRY(dalloc(d, (void **)&d->awo_trace, sizeof(unsigned long long) * AWO_TRACE_N * d->awo_nb));
	d->attn_wo = d->attn_wo_ok = true;
	return YALM_OK;
}

// After a sync: report (once) a bounded spin that gave up -- the fused attention + Wo
// launch waiting for its heads, or an IPC exchange waiting for a peer.
int awo_check(yalm_decoder_s *d) {
	if (d->awo_err) {
		unsigned e = 0;
		HIPCHK(hipMemcpy(&e, d->awo_err, sizeof(e), hipMemcpyDeviceToHost));
		if (e) { // cleared so that later calls report only their own failures
			HIPCHK(hipMemset(d->awo_err, 0, sizeof(e)));
			// bit 1: a Wo workgroup of the fused launch gave up waiting for its head granules;
			// bit 2: a split-KV merger (fused or standalone attention) gave up waiting for a chunk
			std::string m = "bounded in-launch wait gave up (results invalid):";
			if (e & 1u)
				m += " the fused attention + Wo launch's Wo gather timed out waiting for the attention heads"
				     " (yalm_decoder_set_launch YALM_LAUNCH_SEPARATE_ATTN_WO selects separate launches);";
			if (e & 2u)
				m += " the split-KV attention merger timed out waiting for a key-chunk partial;";
			if (e & ~3u)
				m += " unknown error bits " + std::to_string(e & ~3u) + ";";
			set_err(m);
			return YALM_ERR_HIP;
		}
	}
	if (d->ipc) { // tp_exchange.h: a consumer's bounded wait for a peer's exchange gave up
		unsigned *flag = (unsigned *)((unsigned long long *)d->ipc_own + 2 * (size_t)d->tp_size * d->ipc_S); // TpX::err
		unsigned e = 0;
		HIPCHK(hipMemcpy(&e, flag, sizeof(e), hipMemcpyDeviceToHost));
		if (e) {
			HIPCHK(hipMemset(flag, 0, sizeof(e)));
			set_err("tensor-parallel IPC exchange gave up waiting for a peer rank (results invalid)");
			return YALM_ERR_HIP;
		}
	}
	return YALM_OK;
}

// The exchange descriptor of a launch taking part in exchange `ex` of the current launch
// sequence (tp_exchange.h: g = StepState.xbase + ex).
static TpX tpx_ex(const yalm_decoder_s *d, int ex) {
	TpX t = d->tpx;
	t.ex = ex;
	return t;
}

// weight types with a fused attention + Wo kernel (attn_wo.h): f16, fp8 and e4m3
template <class WT>
constexpr bool wt_fused_wo() {
	if constexpr (WT::Q4)
		return false;
	else if constexpr (WT::ROW_SCALE)
		return true;
	else
		return WT::BYTES == 2 || WT::BYTES == 1;
}
// formats that exist on one GPU and in dense models only (q4, e4m3)
template <class WT>
constexpr bool wt_dense_one_gpu() {
	return WT::Q4 || WT::ROW_SCALE;
}
template <class WT, int GT, int KB>
static void launch_attn_wo_k(yalm_decoder_s *d, const yalm_block_weights &w, const AttnWoArgs &p) {
	attn_wo_kernel<WT, GT, KB><<<d->awo_nb, ATTN_THREADS, 0, d->stream>>>(d->q, w.key_cache, w.value_cache, d->step, p);
}
template <class WT, int KB>
static void launch_attn_wo_g(yalm_decoder_s *d, const yalm_block_weights &w, const AttnWoArgs &p, int G) {
	if (G <= 1)
		launch_attn_wo_k<WT, 1, KB>(d, w, p);
	else if (G <= 2)
		launch_attn_wo_k<WT, 2, KB>(d, w, p);
	else if (G <= 4)
		launch_attn_wo_k<WT, 4, KB>(d, w, p);
	else
		launch_attn_wo_k<WT, 8, KB>(d, w, p);
}
// The fused attention + Wo launch of one layer. One GPU: x += Wo attn(q). Tensor parallel:
// the rank's partial (+ x on rank 0) -- into xs, then the RCCL all-reduce into x; or pushed
// to the IPC exchange `ex` (consumed by the GLU GEMV's x staging, tp_exchange.h).
template <class WT>
static int launch_attn_wo(yalm_decoder_s *d, int layer, int ex) {
	const yalm_config &c = d->c;
	const yalm_block_weights &w = d->b[layer];
	AttnWoArgs p;
	p.n_heads = c.n_heads;
	p.n_kv = c.n_kv_heads;
	p.max_seq_len = c.max_seq_len;
	p.nsplit = attn_nsplit(c.max_seq_len);
	p.S = d->awo_S;
	p.head_max = attn_head_max(d->awo_S, (c.max_seq_len + attn_chunk<128>() - 1) / attn_chunk<128>());
	p.q_dim = c.n_heads * c.head_dim;
	p.dim = c.dim;
	p.part = d->part;
	p.layer = layer;
	p.n_layers = c.n_layers;
	p.gran = d->awo_gran + (size_t)layer * p.q_dim;
	p.wo = (const char *)w.wo;
	p.x = d->x;
	p.out = d->comm ? d->xs : d->x;
	p.add_base = d->tp_rank == 0;
	p.push = d->ipc ? tpx_ex(d, ex) : TpX{};
	p.err = d->awo_err;
	p.trace = d->awo_trace;
	p.delay = d->awo_delay_short >= 0 && d->awo_kv_hint >= 0 && d->awo_kv_hint <= AWO_SHORT_KV ? d->awo_delay_short
	                                                                                         : d->awo_delay;
	const int G = c.n_heads / c.n_kv_heads;
	if constexpr (WT::ROW_SCALE) { // one GPU only: rows of 4 or 8 KiB of codes (attn_wo_plan)
		if (p.q_dim == 4096)
			launch_attn_wo_g<WT, 4>(d, w, p, G);
		else
			launch_attn_wo_g<WT, 8>(d, w, p, G);
	} else if constexpr (wt_fused_wo<WT>()) {
		switch (p.q_dim * WT::BYTES) {
		case 1024:
			launch_attn_wo_g<WT, 1>(d, w, p, G);
			break;
		case 2048:
			launch_attn_wo_g<WT, 2>(d, w, p, G);
			break;
		case 4096:
			launch_attn_wo_g<WT, 4>(d, w, p, G);
			break;
		default:
			launch_attn_wo_g<WT, 8>(d, w, p, G);
		}
	}
	HIPCHK(hipGetLastError());
	if (d->comm && ncclAllReduce(d->xs, d->x, c.dim, ncclFloat, ncclSum, (ncclComm_t)d->comm, d->stream) != ncclSuccess) {
		set_err("ncclAllReduce failed");
		return YALM_ERR_HIP;
	}
	return YALM_OK;
}

// One tensor-parallel exchange of x alone, as launches of their own: timing hook for the
// communication cost (yalm_time_kernel id 6). RCCL: one all-reduce. IPC: x pushed to every
// rank, then the consumer side (wait for every rank + sum) -- in the forward the push is the
// producer GEMV's epilogue and the sum runs inside the next GEMV's x staging.
static int enqueue_exchange(yalm_decoder_s *d) {
	if (d->ipc) {
		tpx_push_kernel<<<1, 1024, 0, d->stream>>>(tpx_ex(d, 0), d->c.dim, d->x);
		tpx_collect_kernel<<<TPX_COLLECT_WG, 256, 0, d->stream>>>(tpx_ex(d, 0), d->c.dim, 0, d->xs);
		HIPCHK(hipGetLastError());
		return YALM_OK;
	}
	if (!d->comm) {
		set_err("kernel 6 (tensor-parallel exchange) needs a tensor-parallel decoder");
		return YALM_ERR_ARG;
	}
	if (ncclAllReduce(d->x, d->xs, d->c.dim, ncclFloat, ncclSum, (ncclComm_t)d->comm, d->stream) != ncclSuccess) {
		set_err("ncclAllReduce failed");
		return YALM_ERR_HIP;
	}
	return YALM_OK;
}

// x += W v (fused_matmul_add_residuals). Under tensor parallelism W holds this
// rank's input columns: rank 0's partial carries x. RCCL: rank 0 writes xs = x + W v, the
// others xs = W v, and one all-reduce (sum, captured in the graph) lands the sum in x on
// every rank (identical bits). IPC: the partial is pushed to every rank's exchange slot
// (PPush, exchange `ex`, tp_exchange.h); the next GEMV sums the slots while its weights
// stream in. ex < 0 under IPC: a result nothing reads (the last W2 of a hydration forward)
// stays local -- an exchange nobody consumes would break the slot-reuse order. ex == EX_LOCAL
// (the timing hook): this rank's own x += W v under either transport, no exchange, no all-reduce.
enum { EX_LOCAL = -2 };
template <class WT>
static int enqueue_residual_gemv(yalm_decoder_s *d, const void *W, int n, const float *v, int kind, int ex) {
	const int dim = d->c.dim;
	if constexpr (!wt_dense_one_gpu<WT>()) { // (q4 and e4m3 run on one GPU only: yalm_decoder_create_tp / _tp_ipc refuse them)
		if (d->ipc && ex >= 0)
			return launch_gemv_d<WT, PPush<WT, 1>, false>(
			    d, make_push<WT>(W, n, d->tp_rank == 0 ? d->x : nullptr, tpx_ex(d, ex), dim), v, nullptr, 0.f, kind);
		if (d->comm && ex != EX_LOCAL) {
			if (d->tp_rank == 0)
				TRY((launch_gemv_d<WT, PAddTo<WT, 1>, false>(d, make_addto<WT>(W, n, d->xs, d->x, dim), v, nullptr, 0.f, kind)));
			else
				TRY((launch_gemv_d<WT, PStore<WT, 1>, false>(d, make_store<WT, 1>(W, n, d->xs, dim), v, nullptr, 0.f, kind)));
			if (ncclAllReduce(d->xs, d->x, dim, ncclFloat, ncclSum, (ncclComm_t)d->comm, d->stream) != ncclSuccess) {
				set_err("ncclAllReduce failed");
				return YALM_ERR_HIP;
			}
			return YALM_OK;
		}
	}
	// one GPU, the unread IPC case above, or the timing hook
	return launch_gemv_d<WT, PResidual<WT, 1>, false>(d, make_residual<WT>(W, n, d->x, dim), v, nullptr, 0.f, kind);
}

// The exchange descriptor for a consumer launch (tp_exchange.h). Up to TPX_STAGE_MAX_RANKS
// ranks every consumer workgroup sums the ranks' granules itself; past that a collect launch
// sums x once and the consumer stages it as on one GPU (the collect form). When this rank
// shares its GPU with a peer (tests: several rank processes on one device), a 1-wave gate
// launch waits for the exchange first: a consumer whose 256 workgroups spin could otherwise
// hold every CU a peer's producer needs (a deadlock the bounded wait only reports). One GPU
// per rank (the real configuration) needs no gate: the consumer waits inside its own launch.
static TpX tpx_consume(yalm_decoder_s *d, int ex, int n) {
	if (!d->ipc || ex < 0) // a local x: one GPU, RCCL (x all-reduced in place), the timing hook
		return TpX{};
	if (d->tpx_collect) { // many ranks: x summed once by a collect launch, the consumer stages it as on one GPU
		tpx_collect_kernel<<<TPX_COLLECT_WG, 256, 0, d->stream>>>(tpx_ex(d, ex), n, 0, d->x);
		return TpX{};
	}
	if (d->tpx_gate)
		tpx_gate_kernel<<<1, 64, 0, d->stream>>>(tpx_ex(d, ex), n);
	return tpx_ex(d, ex);
}

static MoeArgs moe_layer_args(const yalm_decoder_s *d, int l) {
	const yalm_block_weights &w = d->b[l];
	return MoeArgs{d->moegate[l], w.w1, w.w2, w.w3, d->moe_E, d->moe_K, d->c.hidden_dim, d->c.dim, d->c.act,
	               d->moe_sel + (size_t)l * d->moe_K, d->moe_wts + (size_t)l * d->moe_K, d->hb};
}

// ---- the launches of a layer, one function each: enqueue_layer_t calls them in order with the
// layer's exchanges, the timing hook (enqueue_one_t) one of them with none. Beside each, the policy
// name yalm_kernel_name reports for it, chosen by the same condition as the launch.

// The QKV policy a decoder's layers run: q / k normed (yalm_decoder_set_qk_norm) and biased
// (yalm_decoder_set_qkv_bias) models are never tensor parallel, and no form runs both.
enum QkvForm { QKV_PLAIN, QKV_BIAS, QKV_NORM };
static QkvForm qkv_form(const yalm_decoder_s *d) {
	return !d->gq.empty() ? QKV_NORM : !d->bq.empty() ? QKV_BIAS : QKV_PLAIN;
}
static const char *qkv_policy_name(const yalm_decoder_s *d) {
	static const char *const names[] = {", PQKV<", ", PQKVB<", ", PQKVN<"};
	return names[qkv_form(d)];
}
static bool moe_ffn(const yalm_decoder_s *d) {
	return d->moe_E > 0;
}
static const char *glu_policy_name(const yalm_decoder_s *d) {
	return moe_ffn(d) ? ", PMoeGlu<" : ", PGlu<";
}
static const char *w2_policy_name(const yalm_decoder_s *d) {
	return moe_ffn(d) ? ", PMoeW2" : ", PResidual<";
}
static const char *const WO_POLICY_NAME = ", PResidual<", *const CLS_POLICY_NAME = ", PStore<";
// the router launch's kernel (moe_router_kernel<WT, NORM>) ahead of the weight type; none on a dense decoder
static const char *router_kernel_name(const yalm_decoder_s *d) {
	return moe_ffn(d) ? "moe_router_kernel<" : "";
}

// The QKV policy of layer l's weights on the decoder's single-row state (the multi-row verify
// step points step / q_out at its row states).
template <class WT>
static PQKV<WT> make_pqkv(const yalm_decoder_s *d, int l) {
	const yalm_config &c = d->c;
	const yalm_block_weights &w = d->b[l];
	return make_pqkv<WT>(w.wq, w.wk, w.wv, c.dim, c.n_heads, c.n_kv_heads, c.head_dim, c.qkv_clip, d->inv_freq, d->step,
	                     d->q, w.key_cache, w.value_cache);
}
// ... with layer l's q / k / v bias (yalm_decoder_set_qkv_bias)
template <class WT>
static PQKVB<WT> make_pqkvb(const yalm_decoder_s *d, int l) {
	return {make_pqkv<WT>(d, l), d->bq[l], d->bk[l], d->bv[l]};
}
// ... ahead of layer l's q / k norm (yalm_decoder_set_qk_norm): q and k raw into qk_raw
template <class WT>
static PQKVN<WT> make_pqkvn(const yalm_decoder_s *d, int l) {
	return {make_pqkv<WT>(d, l), d->qk_raw};
}

// QKV GEMV of layer l; consume_ex >= 0 (IPC tensor parallelism): its x is that exchange.
template <class WT>
static int enqueue_qkv(yalm_decoder_s *d, int l, int consume_ex) {
	const yalm_config &c = d->c;
	const float *nw = d->b[l].rms_att;
	const TpX tin = tpx_consume(d, consume_ex, c.dim);
	switch (qkv_form(d)) {
	case QKV_NORM:
		return launch_gemv_d<WT, PQKVN<WT>, true>(d, make_pqkvn<WT>(d, l), d->x, nw, c.norm_eps, GK_QKV, tin);
	case QKV_BIAS:
		return launch_gemv_d<WT, PQKVB<WT>, true>(d, make_pqkvb<WT>(d, l), d->x, nw, c.norm_eps, GK_QKV, tin);
	default:
		return launch_gemv_d<WT, PQKV<WT>, true>(d, make_pqkv<WT>(d, l), d->x, nw, c.norm_eps, GK_QKV, tin);
	}
}

// The q / k norm launch of layer l over `rows` rows (qk_norm.h): raw rows of qk_raw, the step
// states step[0 .. rows), q rows of q_dim at q_out. One wave per workgroup, n_heads + n_kv_heads
// workgroups per row: four waves per workgroup over a quarter as many CUs measured the same at
// the Qwen3-8B shape (profiles/qknorm_bench.txt: no difference outside the repeat spread).
static int launch_qk_norm(yalm_decoder_s *d, int l, int rows, const StepState *step, float *q_out) {
	const yalm_config &c = d->c;
	const int q_dim = c.n_heads * c.head_dim, kv_dim = c.n_kv_heads * c.head_dim, heads = c.n_heads + c.n_kv_heads;
	qk_norm_rope_kernel<1><<<dim3(heads, rows), YALM_WAVE, 0, d->stream>>>(
	    d->qk_raw, q_dim + kv_dim, d->gq[l], d->gk[l], c.n_heads, c.n_kv_heads, c.head_dim, c.norm_eps, step, q_out,
	    q_dim, d->b[l].key_cache);
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

// Attention of layer l for one row: its step state and q, its output row.
static int enqueue_attn(yalm_decoder_s *d, int l, const float *q, const StepState *step, float *out) {
	const yalm_config &c = d->c;
	return launch_attn(c.head_dim, c.n_heads, c.n_kv_heads, q, d->b[l].key_cache, d->b[l].value_cache, step,
	                   c.max_seq_len, d->part, l, c.n_layers, d->awo_err, nullptr, out, d->stream);
}

// x += Wo xb2; ex: the exchange its partial is (enqueue_residual_gemv).
template <class WT>
static int enqueue_wo(yalm_decoder_s *d, int l, int ex) {
	return enqueue_residual_gemv<WT>(d, d->b[l].wo, d->c.n_heads * d->c.head_dim, d->xb2, GK_WO, ex);
}

// Router of layer l's experts (never tensor parallel; no q4 or e4m3 experts: yalm_decoder_create_moe refuses).
template <class WT>
static int enqueue_router(yalm_decoder_s *d, int l) {
	if constexpr (!wt_dense_one_gpu<WT>()) {
		if (moe_ffn(d))
			return launch_moe_router<WT, true>(moe_layer_args(d, l), d->x, d->b[l].rms_ffn, d->c.norm_eps, d->stream);
	}
	set_err("internal: the expert router needs a mixture-of-experts decoder");
	return YALM_ERR_ARG;
}

// hb = act(W1 xn) * (W3 xn), xn the normed x: the selected experts' on layer l's last routing, or
// the dense GLU, which consumes exchange consume_ex (the Wo partial) under IPC tensor parallelism.
template <class WT>
static int enqueue_glu(yalm_decoder_s *d, int l, int consume_ex) {
	const yalm_config &c = d->c;
	const yalm_block_weights &w = d->b[l];
	if constexpr (!wt_dense_one_gpu<WT>()) {
		if (moe_ffn(d))
			return launch_moe_glu<WT, true>(moe_layer_args(d, l), d->x, w.rms_ffn, c.norm_eps, d->gemv[GK_GLU], d->stream);
	}
	return launch_glu<WT, true>(w.w1, w.w3, c.dim, d->hb, c.hidden_dim, c.act, d->x, w.rms_ffn, c.norm_eps, GK_GLU,
	                            d->gemv[GK_GLU], d->stream, tpx_consume(d, consume_ex, c.dim));
}

// x += W2 hb (the selected experts' W2 on their hb rows); ex: the exchange its partial is.
template <class WT>
static int enqueue_w2(yalm_decoder_s *d, int l, int ex) {
	if constexpr (!wt_dense_one_gpu<WT>()) {
		if (moe_ffn(d))
			return launch_moe_w2<WT>(moe_layer_args(d, l), d->x, d->gemv[GK_W2], d->stream);
	}
	return enqueue_residual_gemv<WT>(d, d->b[l].w2, d->c.hidden_dim, d->hb, GK_W2, ex);
}

// One layer. IPC tensor parallelism (tp_exchange.h): the Wo partial is exchange ex0 (the GLU
// consumes it), the W2 partial exchange ex0 + 1 (push_w2; the next QKV or the logits GEMV
// consumes it); x_exchanged: the layer's input x is exchange ex0 - 1 (the QKV GEMV consumes
// it), not a local x (the embedding of layer 0, or the x yalm_block / yalm_set_x left).
template <class WT>
static int enqueue_layer_t(yalm_decoder_s *d, int l, int ex0, bool x_exchanged, bool push_w2) {
	TRY(enqueue_qkv<WT>(d, l, x_exchanged ? ex0 - 1 : -1));
	if (qkv_form(d) == QKV_NORM)
		TRY(launch_qk_norm(d, l, 1, d->step, d->q));
	if (d->attn_wo && wt_fused_wo<WT>()) {
		TRY(launch_attn_wo<WT>(d, l, ex0));
	} else {
		TRY(enqueue_attn(d, l, d->q, d->step, d->xb2));
		TRY(enqueue_wo<WT>(d, l, ex0));
	}
	if (moe_ffn(d))
		TRY(enqueue_router<WT>(d, l));
	TRY(enqueue_glu<WT>(d, l, ex0));
	return enqueue_w2<WT>(d, l, push_w2 ? ex0 + 1 : -1);
}

// Final norm + classifier rows of this rank. IPC tensor parallelism: consume_ex >= 0 = the
// GEMV consumes that exchange (the last layer's W2); push_ex >= 0 (OUTPUT_LOGITS) = it also
// produces that exchange, the logits gather: this rank's vocabulary rows pushed to every rank.
template <class WT>
static int enqueue_logits_t(yalm_decoder_s *d, int consume_ex, int push_ex) {
	const yalm_config &c = d->c;
	const TpX tin = tpx_consume(d, consume_ex, c.dim);
	if constexpr (!wt_dense_one_gpu<WT>()) {
		if (push_ex >= 0)
			return launch_gemv_d<WT, PPush<WT, 1>, true>(
			    d, make_push<WT>(d->wcls, c.dim, nullptr, tpx_ex(d, push_ex), c.vocab_size), d->x, d->rms_final, c.norm_eps,
			    GK_CLS, tin);
	}
	if (c.vocab_size % 2 == 0)
		return launch_gemv_d<WT, PStore<WT, 2>, true>(d, make_store<WT, 2>(d->wcls, c.dim, d->logits_local, c.vocab_size),
		                                              d->x, d->rms_final, c.norm_eps, GK_CLS, tin);
	return launch_gemv_d<WT, PStore<WT, 1>, true>(d, make_store<WT, 1>(d->wcls, c.dim, d->logits_local, c.vocab_size),
	                                              d->x, d->rms_final, c.norm_eps, GK_CLS, tin);
}

template <class WT>
static int enqueue_begin_t(yalm_decoder_s *d, int n_ex) {
	step_begin_kernel<WT><<<1, 256, 0, d->stream>>>(d->step, d->emb, d->c.dim, d->x, d->c.max_seq_len, n_ex,
	                                                 d->inv_freq, d->c.head_dim / 2);
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

#define DISPATCH_WT(dtype, FN, ...)                                                                                    \
	((dtype) == YALM_F32   ? FN<WF32>(__VA_ARGS__)                                                                     \
	 : (dtype) == YALM_F16 ? FN<WF16>(__VA_ARGS__)                                                                     \
	 : (dtype) == YALM_Q4  ? FN<WQ4>(__VA_ARGS__)                                                                      \
	 : (dtype) == YALM_E4M3 ? FN<WE4M3>(__VA_ARGS__)                                                                   \
	                       : FN<WF8>(__VA_ARGS__))
// the formats with a multi-row form (gemv_rows.h): all but q4
#define DISPATCH_WT_ROWS(dtype, FN, ...)                                                                               \
	((dtype) == YALM_F32    ? FN<WF32>(__VA_ARGS__)                                                                    \
	 : (dtype) == YALM_F16  ? FN<WF16>(__VA_ARGS__)                                                                    \
	 : (dtype) == YALM_E4M3 ? FN<WE4M3>(__VA_ARGS__)                                                                   \
	                        : FN<WF8>(__VA_ARGS__))
// the element-typed formats alone (the expert kernels)
#define DISPATCH_WT_EL(dtype, FN, ...)                                                                                 \
	((dtype) == YALM_F32   ? FN<WF32>(__VA_ARGS__)                                                                     \
	 : (dtype) == YALM_F16 ? FN<WF16>(__VA_ARGS__)                                                                     \
	                       : FN<WF8>(__VA_ARGS__))

// IPC tensor parallelism (tp_exchange.h): layer l's Wo and W2 partials are exchanges 2 l and
// 2 l + 1, the logits gather / argmax pairs exchange 2 L. Every exchange of the sequence is
// consumed (the slot-reuse order relies on it), so a hydration forward keeps its last W2
// local: 2 L - 1 exchanges, 2 L + 1 with an output.
static int enqueue_forward(yalm_decoder_s *d, int which) {
	const int L = d->c.n_layers;
	const bool hyd = which == GRAPH_HYDRATE;
	TRY(DISPATCH_WT(d->c.weight_dtype, enqueue_begin_t, d, d->ipc ? (hyd ? 2 * L - 1 : 2 * L + 1) : 0));
	for (int l = 0; l < L; ++l)
		TRY(DISPATCH_WT(d->c.weight_dtype, enqueue_layer_t, d, l, 2 * l, l > 0, !(hyd && l == L - 1)));
	if (hyd)
		return YALM_OK;
	TRY(DISPATCH_WT(d->c.weight_dtype, enqueue_logits_t, d, d->ipc ? 2 * L - 1 : -1,
	                d->ipc && which == GRAPH_LOGITS ? 2 * L : -1));
	if (d->ipc) { // tp_exchange.h: no exchange launches
		if (which == GRAPH_LOGITS) { // every rank's vocabulary slice, side by side
			tpx_collect_kernel<<<TPX_COLLECT_WG, 256, 0, d->stream>>>(tpx_ex(d, 2 * L), d->c.vocab_size, 1, d->logits);
			HIPCHK(hipGetLastError());
			HIPCHK(hipMemcpyAsync(d->logits_pinned, d->logits, sizeof(float) * d->vocab_full, hipMemcpyDeviceToHost,
			                      d->stream));
		} else { // local first max, pushed; every rank's pair gathered and picked in the same launch
			argmax_tp_kernel<<<1, 1024, 0, d->stream>>>(d->logits_local, d->c.vocab_size, d->step, d->tokens,
			                                            d->tokens_cap, tpx_ex(d, 2 * L));
			HIPCHK(hipGetLastError());
		}
		return YALM_OK;
	}
	if (which == GRAPH_LOGITS) {
		if (d->comm && ncclAllGather(d->logits_local, d->logits, d->c.vocab_size, ncclFloat, (ncclComm_t)d->comm,
		                             d->stream) != ncclSuccess) {
			set_err("ncclAllGather (logits) failed");
			return YALM_ERR_HIP;
		}
		HIPCHK(hipMemcpyAsync(d->logits_pinned, d->logits, sizeof(float) * d->vocab_full, hipMemcpyDeviceToHost,
		                      d->stream));
	} else if (which == GRAPH_SAMPLED) { // one GPU only (yalm_generate_sampled checks): the whole vocabulary is here
		sample_kernel<<<1, SMP_THREADS, 0, d->stream>>>(d->logits, d->c.vocab_size, d->smp_params, d->smp_u,
		                                                d->tokens_cap, d->step, d->tokens, d->tokens_cap, nullptr,
		                                                nullptr);
		HIPCHK(hipGetLastError());
	} else if (!d->comm) {
		argmax_kernel<<<1, 1024, 0, d->stream>>>(d->logits, d->c.vocab_size, d->step, d->tokens, d->tokens_cap);
		HIPCHK(hipGetLastError());
	} else { // sharded vocabulary: local first-max, gather (value, index) pairs, pick (identical on all ranks)
		argmax_kernel<<<1, 1024, 0, d->stream>>>(d->logits_local, d->c.vocab_size, d->step, d->tokens,
		                                         d->tokens_cap, d->amax, d->tp_rank * d->c.vocab_size);
		HIPCHK(hipGetLastError());
		if (ncclAllGather(d->amax, d->amax_all, 2, ncclFloat, (ncclComm_t)d->comm, d->stream) != ncclSuccess) {
			set_err("ncclAllGather (argmax) failed");
			return YALM_ERR_HIP;
		}
		argmax_pick_kernel<<<1, 1, 0, d->stream>>>(d->amax_all, d->tp_size, d->step, d->tokens, d->tokens_cap);
		HIPCHK(hipGetLastError());
	}
	return YALM_OK;
}

static int ensure_graph(yalm_decoder_s *d, int which) {
	if (d->exec[which] || d->eager)
		return YALM_OK;
	HIPCHK(hipStreamBeginCapture(d->stream, hipStreamCaptureModeRelaxed));
	int r = enqueue_forward(d, which);
	hipGraph_t g = nullptr;
	hipError_t e = hipStreamEndCapture(d->stream, &g);
	if (r != YALM_OK)
		return r;
	HIPCHK(e);
	d->graph[which] = g;
	HIPCHK(hipGraphInstantiate(&d->exec[which], g, nullptr, nullptr, 0));
	return YALM_OK;
}

static void drop_graphs(yalm_decoder_s *d) {
	for (int i = 0; i < N_GRAPHS; ++i) {
		if (d->exec[i])
			(void)hipGraphExecDestroy(d->exec[i]);
		if (d->graph[i])
			(void)hipGraphDestroy(d->graph[i]);
		d->exec[i] = nullptr;
		d->graph[i] = nullptr;
	}
}

static int validate_config(const yalm_config *c) {
	ARGCHK(c->dim > 0 && c->hidden_dim > 0 && c->n_layers > 0 && c->n_heads > 0 && c->n_kv_heads > 0 &&
	           c->vocab_size > 0 && c->max_seq_len > 2,
	       "config: non-positive dimension");
	ARGCHK(c->n_heads % c->n_kv_heads == 0, "config: n_heads % n_kv_heads != 0");
	ARGCHK(dtype_ok(c->weight_dtype), "config: weight_dtype must be F32, F16, F8E5M2, Q4 or E4M3");
	ARGCHK(c->dim % 16 == 0 && c->hidden_dim % 16 == 0 && (c->n_heads * c->head_dim) % 16 == 0,
	       "config: dim, hidden_dim and n_heads*head_dim must be multiples of 16 (infer.cpp:66)");
	ARGCHK(c->weight_dtype != YALM_Q4 ||
	           (c->dim % 32 == 0 && c->hidden_dim % 32 == 0 && (c->n_heads * c->head_dim) % 32 == 0),
	       "config: q4 needs dim, hidden_dim and n_heads*head_dim multiples of 32 (its scale group)");
	ARGCHK(c->rotary_dim <= c->head_dim && c->rotary_dim % 2 == 0, "config: bad rotary_dim");
	if (!attn_supported(c->head_dim, c->n_heads / c->n_kv_heads)) {
		set_err("config: attention kernel needs head_dim in {16,32,64,128,256} and n_heads/n_kv_heads <= 8");
		return YALM_ERR_UNSUPPORTED;
	}
	return YALM_OK;
}

// The RoPE frequency table (head_dim / 2). The plain table is create_decoder's powf form (see
// there); rs.type 1 (Llama-3.1 / 3.2 "llama3") rescales each pair frequency f by its wavelength
// w = 2 pi / f against the original context `orig`: w < orig / high keeps f, w > orig / low
// gives f / factor, between them s = (orig / w - low) / (high - low) blends
// (1 - s) f / factor + s f. In double from the f32 f, rounded once to f32.
static std::vector<float> rope_inv_freq(const yalm_config &c, const yalm_rope_scaling &rs) {
	std::vector<float> inv(c.head_dim / 2);
	const float rinv = 1.0f / (float)c.rotary_dim;
	for (int j = 0; j < c.head_dim; j += 2)
		inv[j / 2] = j >= c.rotary_dim ? 0.f : powf(c.rope_theta, -((float)j * rinv));
	if (rs.type == 1) {
		const double orig = (double)rs.original_max_position, lo = (double)rs.low_freq_factor,
		             hi = (double)rs.high_freq_factor, factor = (double)rs.factor;
		for (float &fv : inv) {
			const double f = (double)fv;
			if (f == 0.0)
				continue;
			const double w = 2.0 * M_PI / f;
			if (w < orig / hi)
				continue;
			if (w > orig / lo) {
				fv = (float)(f / factor);
			} else {
				const double s = (orig / w - lo) / (hi - lo);
				fv = (float)((1.0 - s) * f / factor + s * f);
			}
		}
	}
	return inv;
}

extern "C" int yalm_decoder_set_rope_scaling(yalm_decoder d, const yalm_rope_scaling *s) {
	ARGCHK(d && s, "yalm_decoder_set_rope_scaling: null argument");
	ARGCHK(s->type == 0 || s->type == 1, "yalm_decoder_set_rope_scaling: unknown type (0 none, 1 llama3)");
	ARGCHK(s->type == 0 || (s->factor >= 1.0f && s->high_freq_factor > s->low_freq_factor &&
	                        s->low_freq_factor > 0.0f && s->original_max_position > 0),
	       "yalm_decoder_set_rope_scaling: need factor >= 1, high_freq_factor > low_freq_factor > 0 and "
	       "original_max_position > 0");
	yalm_rope_scaling rs{};
	if (s->type)
		rs = *s;
	const std::vector<float> inv = rope_inv_freq(d->c, rs);
	HIPCHK(hipStreamSynchronize(d->stream)); // no forward in flight reads the old table
	HIPCHK(hipMemcpy(d->inv_freq, inv.data(), sizeof(float) * inv.size(), hipMemcpyHostToDevice));
	d->rope_scaling = rs;
	return YALM_OK;
}

extern "C" int yalm_decoder_get_inv_freq(yalm_decoder d, float *host) {
	ARGCHK(d && host, "yalm_decoder_get_inv_freq: null argument");
	HIPCHK(hipStreamSynchronize(d->stream));
	HIPCHK(hipMemcpy(host, d->inv_freq, sizeof(float) * (d->c.head_dim / 2), hipMemcpyDeviceToHost));
	return YALM_OK;
}

extern "C" int yalm_decoder_set_qkv_bias(yalm_decoder d, const float *const *bq, const float *const *bk,
                                         const float *const *bv) {
	ARGCHK(d, "yalm_decoder_set_qkv_bias: null decoder");
	if (d->tp_size > 1 || d->comm || d->ipc || d->moe_E > 0) {
		set_err("yalm_decoder_set_qkv_bias: a q / k / v bias runs on dense one-GPU decoders only (no tensor-parallel or "
		        "mixture-of-experts form)");
		return YALM_ERR_UNSUPPORTED;
	}
	const bool none = !bq && !bk && !bv;
	ARGCHK(none || (bq && bk && bv), "yalm_decoder_set_qkv_bias: bias arrays for q, k and v, or all three NULL");
	if (!none && !d->gq.empty()) {
		set_err("yalm_decoder_set_qkv_bias: the decoder has a q / k norm (yalm_decoder_set_qk_norm); no form runs a "
		        "bias together with the q / k norm");
		return YALM_ERR_UNSUPPORTED;
	}
	const int L = d->c.n_layers;
	if (!none)
		for (int l = 0; l < L; ++l) // (the epilogue reads a RoPE pair's two values as one 8-byte load)
			ARGCHK(bq[l] && bk[l] && bv[l] && (uintptr_t)bq[l] % 8 == 0 && (uintptr_t)bk[l] % 8 == 0 &&
			           (uintptr_t)bv[l] % 8 == 0,
			       "yalm_decoder_set_qkv_bias: a layer's bias pointer is null or not 8-byte aligned");
	HIPCHK(hipStreamSynchronize(d->stream));
	drop_graphs(d); // captured graphs bake the QKV launches without (or with the old) bias pointers
	if (none) {
		d->bq.clear(), d->bk.clear(), d->bv.clear();
	} else {
		d->bq.assign(bq, bq + L), d->bk.assign(bk, bk + L), d->bv.assign(bv, bv + L);
	}
	return YALM_OK;
}

extern "C" int yalm_decoder_set_qk_norm(yalm_decoder d, const float *const *gq, const float *const *gk) {
	ARGCHK(d, "yalm_decoder_set_qk_norm: null decoder");
	const char *why = nullptr;
	if (d->tp_size > 1 || d->comm || d->ipc)
		why = "a tensor-parallel decoder";
	else if (d->moe_E > 0)
		why = "a mixture-of-experts decoder";
	else if (!d->bq.empty())
		why = "a decoder that has a q / k / v bias (yalm_decoder_set_qkv_bias)";
	if (why) {
		set_err(std::string("yalm_decoder_set_qk_norm: the q / k norm runs on dense one-GPU decoders without a bias, not on ") +
		        why);
		return YALM_ERR_UNSUPPORTED;
	}
	const bool none = !gq && !gk;
	ARGCHK(none || (gq && gk), "yalm_decoder_set_qk_norm: q / k norm arrays for q and k, or both NULL");
	const int L = d->c.n_layers;
	if (!none)
		for (int l = 0; l < L; ++l) // (the kernel reads a RoPE pair's two weights as one 8-byte load)
			ARGCHK(gq[l] && gk[l] && (uintptr_t)gq[l] % 8 == 0 && (uintptr_t)gk[l] % 8 == 0,
			       "yalm_decoder_set_qk_norm: a layer's q / k norm pointer is null or not 8-byte aligned");
	HIPCHK(hipStreamSynchronize(d->stream));
	drop_graphs(d); // captured graphs bake the launch sequence without (or with the old) norm
	if (none) {
		d->gq.clear(), d->gk.clear();
		return YALM_OK;
	}
	if (!d->qk_raw)
		TRY(dalloc(d, (void **)&d->qk_raw,
		           sizeof(float) * ROWS_MAX_T * (size_t)(d->c.n_heads + d->c.n_kv_heads) * d->c.head_dim));
	d->gq.assign(gq, gq + L), d->gk.assign(gk, gk + L);
	return YALM_OK;
}

static void destroy_decoder(yalm_decoder_s *d) {
	drop_graphs(d);
	if (d->comm)
		(void)ncclCommDestroy((ncclComm_t)d->comm);
	for (void *p : d->ipc_opened)
		(void)hipIpcCloseMemHandle(p);
	if (d->ipc_own)
		(void)hipFree(d->ipc_own);
	for (void *p : d->dev_allocs)
		(void)hipFree(p);
	if (d->logits_pinned)
		(void)hipHostFree(d->logits_pinned);
	if (d->rlogits_pinned)
		(void)hipHostFree(d->rlogits_pinned);
	if (d->own_stream && d->stream)
		(void)hipStreamDestroy(d->stream);
	delete d;
}

int dalloc(yalm_decoder_s *d, void **p, size_t bytes) {
	HIPCHK(hipMalloc(p, bytes ? bytes : 4));
	d->dev_allocs.push_back(*p);
	HIPCHK(hipMemset(*p, 0, bytes ? bytes : 4));
	return YALM_OK;
}

// One forward of graph `which`: a graph replay, or the same kernels launched
// eagerly when d->eager.
static int replay(yalm_decoder_s *d, int which) {
	if (d->eager || ((which == GRAPH_GREEDY || which == GRAPH_SAMPLED) && d->greedy_eager))
		return enqueue_forward(d, which);
	HIPCHK(hipGraphLaunch(d->exec[which], d->stream));
	if (d->graph_sync)
		HIPCHK(hipStreamSynchronize(d->stream));
	return YALM_OK;
}

// comm: an initialised ncclComm_t (tensor parallelism) or null. config holds
// the local (per-rank) dims; vocab_full the unsharded vocabulary.
static int create_decoder(const yalm_config *config, const yalm_model_weights *weights, yalm_stream s,
                          yalm_decoder *out, void *comm, int tp_rank, int tp_size, int vocab_full,
                          const yalm_moe_config *moe = nullptr, const void *const *moegate = nullptr) {
	ARGCHK(config && weights && out && weights->blocks, "yalm_decoder_create: null argument");
	TRY(validate_config(config));
	if (moe)
		TRY(validate_moe(moe->n_experts, moe->n_experts_active));
	yalm_decoder_s *d = new yalm_decoder_s();
	d->c = *config;
	if (moe) {
		d->moe_E = moe->n_experts;
		d->moe_K = moe->n_experts_active;
		d->moegate.assign(moegate, moegate + config->n_layers);
	}
	d->comm = comm;
	d->tp_rank = tp_rank;
	d->tp_size = tp_size;
	d->vocab_full = vocab_full;
	d->emb = weights->token_embedding;
	d->rms_final = weights->rms_final;
	d->wcls = weights->wcls;
	d->b.assign(weights->blocks, weights->blocks + config->n_layers);
	int r = YALM_OK;
	auto fail = [&](int code) {
		destroy_decoder(d);
		return code;
	};
	if (s) {
		d->stream = reinterpret_cast<hipStream_t>(s);
	} else {
		if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
			set_err("hipStreamCreate failed");
			return fail(YALM_ERR_HIP);
		}
		d->own_stream = true;
	}
	const yalm_config &c = d->c;
	const int q_dim = c.n_heads * c.head_dim, kv_dim = c.n_kv_heads * c.head_dim;
	const int nsplit = attn_nsplit(c.max_seq_len);
	d->tokens_cap = 1 << 16;
	d->pf_forms = pf_forms_default();
	{
		const char *g = ab_env("YALM_GREEDY_GRAPH");
		d->greedy_eager = !(g && atoi(g) != 0);
	}
	// geometry overrides for A/B runs without a rebuild (same meaning as yalm_set_gemv_config):
	// YALM_GEMV_CFG="kind:threads:unroll:gpw[,kind:threads:unroll:gpw...]", kind 0..4
	if (const char *g = ab_env("YALM_GEMV_CFG")) {
		int k, t, u, w, n = 0;
		for (const char *p = g; sscanf(p, "%d:%d:%d:%d%n", &k, &t, &u, &w, &n) == 4; p += n + (p[n] == ',')) {
			if (k >= 0 && k < GK_N && (t == 0 || t == 256 || t == 512 || t == 1024) &&
			    (u == 0 || u == 2 || u == 4 || u == 8) && w >= 0)
				d->gemv[k] = GemvCfg{t, u, w};
			if (!p[n])
				break;
		}
	}
	if ((r = dalloc(d, (void **)&d->step, sizeof(StepState))) || (r = dalloc(d, (void **)&d->x, sizeof(float) * c.dim)) ||
	    (r = dalloc(d, (void **)&d->q, sizeof(float) * q_dim)) ||
	    (r = dalloc(d, (void **)&d->xb2, sizeof(float) * q_dim)) ||
	    (r = dalloc(d, (void **)&d->hb, sizeof(float) * c.hidden_dim * std::max(1, d->moe_K))) ||
	    (r = dalloc(d, (void **)&d->moe_sel, sizeof(int) * (size_t)c.n_layers * d->moe_K)) ||
	    (r = dalloc(d, (void **)&d->moe_wts, sizeof(float) * (size_t)c.n_layers * d->moe_K)) ||
	    (r = dalloc(d, (void **)&d->part, sizeof(unsigned long long) * (size_t)c.n_heads * nsplit * (c.head_dim + 2))) ||
	    (r = dalloc(d, (void **)&d->awo_err, sizeof(unsigned) * AWO_REPL_STRIDE)) ||
	    (r = dalloc(d, (void **)&d->logits, sizeof(float) * vocab_full)) ||
	    (r = dalloc(d, (void **)&d->xs, sizeof(float) * c.dim)) ||
	    (r = dalloc(d, (void **)&d->amax, sizeof(float) * 2)) ||
	    (r = dalloc(d, (void **)&d->amax_all, sizeof(float) * 2 * tp_size)) ||
	    (r = dalloc(d, (void **)&d->inv_freq, sizeof(float) * c.head_dim / 2)) ||
	    (r = dalloc(d, (void **)&d->tokens, sizeof(int) * d->tokens_cap)) ||
	    (r = dalloc(d, (void **)&d->smp_params, sizeof(SampleParams))) ||
	    (r = dalloc(d, (void **)&d->smp_u, sizeof(float) * d->tokens_cap)) ||
	    (r = dalloc(d, (void **)&d->smp_step, sizeof(StepState))))
		return fail(r);
	// RoPE frequencies on the host, bit for bit as the reference's compiled rope computes
	// them. infer.cpp:203 reads 1/powf(theta, j/rotary_dim), but under its -ffast-math
	// (Makefile:36-39) gcc emits r = 1.0f / rotary_dim; powf(theta, -(j * r)) (one scalar
	// glibc powf call; the division folded into the exponent): a freq one ulp away moves
	// the angle pos * freq by pos ulps, 2e-4 rad at pos 4095 -- tests/test_gpu_ref_glue.py
	// measured 60 f16 ulps on a K row against the reference's own rope before this form.
	const std::vector<float> inv = rope_inv_freq(c, d->rope_scaling);
	if (hipMemcpy(d->inv_freq, inv.data(), sizeof(float) * inv.size(), hipMemcpyHostToDevice) != hipSuccess) {
		set_err("inv_freq upload failed");
		return fail(YALM_ERR_HIP);
	}
	// the sampling parameters before any yalm_generate_sampled (yalm_time_kernel id 10): T = 1, no truncation
	const SampleParams smp0{1.0f, 0, 1.0f};
	if (hipMemcpy(d->smp_params, &smp0, sizeof(smp0), hipMemcpyHostToDevice) != hipSuccess) {
		set_err("sampling parameter upload failed");
		return fail(YALM_ERR_HIP);
	}
	for (auto &bw : d->b) {
		const size_t kvb = sizeof(uint16_t) * (size_t)c.max_seq_len * kv_dim;
		if (!bw.key_cache && (r = dalloc(d, (void **)&bw.key_cache, kvb)))
			return fail(r);
		if (!bw.value_cache && (r = dalloc(d, (void **)&bw.value_cache, kvb)))
			return fail(r);
	}
	d->logits_local = d->logits;
	if (tp_size > 1 && (r = dalloc(d, (void **)&d->logits_local, sizeof(float) * c.vocab_size)))
		return fail(r);
	if (hipHostMalloc((void **)&d->logits_pinned, sizeof(float) * vocab_full, hipHostMallocDefault) != hipSuccess) {
		set_err("hipHostMalloc failed");
		return fail(YALM_ERR_HIP);
	}
	if ((r = attn_wo_init(d)))
		return fail(r);
	if (hipDeviceSynchronize() != hipSuccess) {
		set_err("hipDeviceSynchronize failed after decoder allocation");
		return fail(YALM_ERR_HIP);
	}
	*out = d;
	return YALM_OK;
}

extern "C" int yalm_decoder_create(const yalm_config *config, const yalm_model_weights *weights, yalm_stream s,
                                   yalm_decoder *out) {
	ARGCHK(config, "yalm_decoder_create: null config");
	return create_decoder(config, weights, s, out, nullptr, 0, 1, config->vocab_size);
}

// Mixture of experts on one GPU (moe.h): blocks[l].w1 / w2 / w3 are the stacked expert tensors.
extern "C" int yalm_decoder_create_moe(const yalm_config *config, const yalm_moe_config *moe,
                                       const yalm_model_weights *weights, const void *const *moegate, yalm_stream s,
                                       yalm_decoder *out) {
	ARGCHK(config && moe && moegate, "yalm_decoder_create_moe: null argument");
	if (config->weight_dtype == YALM_E4M3) {
		set_err("yalm_decoder_create_moe: e4m3 weights have no mixture-of-experts form (the expert kernels take "
		        "no row scale)");
		return YALM_ERR_UNSUPPORTED;
	}
	if (config->weight_dtype == YALM_Q4) {
		set_err("yalm_decoder_create_moe: q4 weights have no mixture-of-experts form (the expert kernels address "
		        "their own chunks)");
		return YALM_ERR_UNSUPPORTED;
	}
	for (int l = 0; l < config->n_layers; ++l)
		ARGCHK(moegate[l], "yalm_decoder_create_moe: null moegate pointer");
	return create_decoder(config, weights, s, out, nullptr, 0, 1, config->vocab_size, moe, moegate);
}

extern "C" int yalm_moe_routing(yalm_decoder d, int *experts, float *weights) {
	ARGCHK(d && d->moe_E > 0, "yalm_moe_routing: not a mixture-of-experts decoder");
	HIPCHK(hipStreamSynchronize(d->stream));
	const size_t n = (size_t)d->c.n_layers * d->moe_K;
	if (experts)
		HIPCHK(hipMemcpy(experts, d->moe_sel, sizeof(int) * n, hipMemcpyDeviceToHost));
	if (weights)
		HIPCHK(hipMemcpy(weights, d->moe_wts, sizeof(float) * n, hipMemcpyDeviceToHost));
	return YALM_OK;
}

// ------------------------------------------------------------------ tensor parallelism
static int tp_local_config(const yalm_config &f, int tp_size, yalm_config &lc) {
	ARGCHK(f.n_kv_heads % tp_size == 0 && f.n_heads % tp_size == 0 && f.hidden_dim % tp_size == 0 &&
	           f.vocab_size % tp_size == 0,
	       "tensor parallel: n_heads, n_kv_heads, hidden_dim and vocab_size must divide by tp_size");
	lc = f;
	lc.n_heads = f.n_heads / tp_size;
	lc.n_kv_heads = f.n_kv_heads / tp_size;
	lc.hidden_dim = f.hidden_dim / tp_size;
	lc.vocab_size = f.vocab_size / tp_size;
	return YALM_OK;
}

// {value, tag} granules per (parity, source rank) slot of the IPC exchange: x, or a rank's
// vocabulary rows (tp_exchange.h)
static int ipc_slot_floats(const yalm_config &f, int tp_size) {
	const int need = std::max(f.dim, f.vocab_size / tp_size + 2);
	return (need + 63) / 64 * 64;
}
static size_t ipc_buf_bytes(const yalm_config &f, int tp_size) {
	return 2 * (size_t)tp_size * ipc_slot_floats(f, tp_size) * sizeof(unsigned long long) + TPX_CTRL_WORDS * sizeof(float);
}

extern "C" int yalm_tp_unique_id(void *id_out) {
	ARGCHK(id_out, "null id");
	ncclUniqueId id;
	if (ncclGetUniqueId(&id) != ncclSuccess) {
		set_err("ncclGetUniqueId failed");
		return YALM_ERR_HIP;
	}
	memcpy(id_out, &id, sizeof(id));
	return YALM_OK;
}

extern "C" int yalm_decoder_create_tp(const yalm_config *config, const yalm_model_weights *weights, int tp_rank,
                                      int tp_size, const void *unique_id, yalm_stream s, yalm_decoder *out) {
	ARGCHK(config && weights && unique_id && out, "yalm_decoder_create_tp: null argument");
	ARGCHK(tp_size >= 1 && tp_rank >= 0 && tp_rank < tp_size, "yalm_decoder_create_tp: bad rank / size");
	if (config->weight_dtype == YALM_E4M3) {
		set_err("yalm_decoder_create_tp: e4m3 weights have no tensor-parallel form (a column shard of a row has "
		        "no scale of its own)");
		return YALM_ERR_UNSUPPORTED;
	}
	if (config->weight_dtype == YALM_Q4) {
		set_err("yalm_decoder_create_tp: q4 weights have no tensor-parallel form (a column shard of a q4 row is "
		        "two strided pieces)");
		return YALM_ERR_UNSUPPORTED;
	}
	const yalm_config &f = *config;
	yalm_config lc;
	TRY(tp_local_config(f, tp_size, lc));
	ncclUniqueId id;
	memcpy(&id, unique_id, sizeof(id));
	ncclComm_t comm = nullptr;
	if (ncclCommInitRank(&comm, tp_size, id, tp_rank) != ncclSuccess) {
		set_err("ncclCommInitRank failed");
		return YALM_ERR_HIP;
	}
	const int r = create_decoder(&lc, weights, s, out, comm, tp_rank, tp_size, f.vocab_size);
	if (r != YALM_OK)
		(void)ncclCommDestroy(comm);
	return r;
}

// The rank record every rank shares (YALM_TP_HANDLE_BYTES): the IPC handle of its exchange
// buffer, then WHERE the rank runs -- its GPU's UUID and the CU mask of its decoder stream.
// Two ranks contend for compute only when both match (same GPU, overlapping CUs): ADVICE r5
// (medium) -- the round-5 test compared hipPointerGetAttributes(peer mapping).device with the
// current device, which an IPC-imported mapping need not report as the exporter's.
struct TpRankRecord {
	unsigned char ipc[64];
	unsigned char uuid[16];
	uint32_t cu_mask[YALM_CU_MASK_WORDS];
	unsigned char reserved[YALM_TP_HANDLE_BYTES - 64 - 16 - 4 * YALM_CU_MASK_WORDS];
};
static_assert(sizeof(TpRankRecord) == YALM_TP_HANDLE_BYTES, "rank record size");
static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");

extern "C" int yalm_tp_ipc_alloc(const yalm_config *config, int tp_size, yalm_stream s, void **buf,
                                 void *handle_out) {
	ARGCHK(config && buf && handle_out && tp_size >= 1 && tp_size <= 8, "yalm_tp_ipc_alloc: bad argument (1..8 ranks)");
	const size_t bytes = ipc_buf_bytes(*config, tp_size);
	// uncached (tp_exchange.h): peers push into it, so no reader's L2 may hold a stale line
	HIPCHK(hipExtMallocWithFlags(buf, bytes, hipDeviceMallocUncached));
	HIPCHK(hipMemset(*buf, 0, bytes));
	TpRankRecord rec;
	memset(&rec, 0, sizeof(rec));
	hipIpcMemHandle_t h;
	HIPCHK(hipIpcGetMemHandle(&h, *buf));
	memcpy(rec.ipc, &h, sizeof(h));
	int dev = 0;
	HIPCHK(hipGetDevice(&dev));
	hipUUID u;
	HIPCHK(hipDeviceGetUuid(&u, dev));
	memcpy(rec.uuid, &u, sizeof(rec.uuid));
	TRY(stream_cu_mask(reinterpret_cast<hipStream_t>(s), rec.cu_mask));
	memcpy(handle_out, &rec, sizeof(rec));
	HIPCHK(hipDeviceSynchronize());
	return YALM_OK;
}

extern "C" int yalm_decoder_create_tp_ipc(const yalm_config *config, const yalm_model_weights *weights, int tp_rank,
                                          int tp_size, void *own_buf, const void *handles, yalm_stream s,
                                          yalm_decoder *out) {
	ARGCHK(config && weights && own_buf && handles && out, "yalm_decoder_create_tp_ipc: null argument");
	ARGCHK(tp_size >= 1 && tp_size <= 8 && tp_rank >= 0 && tp_rank < tp_size, "bad rank / size (1..8 ranks)");
	if (config->weight_dtype == YALM_E4M3) {
		set_err("yalm_decoder_create_tp_ipc: e4m3 weights have no tensor-parallel form (a column shard of a row "
		        "has no scale of its own)");
		return YALM_ERR_UNSUPPORTED;
	}
	if (config->weight_dtype == YALM_Q4) {
		set_err("yalm_decoder_create_tp_ipc: q4 weights have no tensor-parallel form (a column shard of a q4 row is "
		        "two strided pieces)");
		return YALM_ERR_UNSUPPORTED;
	}
	yalm_config lc;
	TRY(tp_local_config(*config, tp_size, lc));
	ARGCHK(config->dim % (64 * (config->weight_dtype == YALM_F32 ? 4 : config->weight_dtype == YALM_F16 ? 8 : 16)) == 0,
	       "tensor parallel (IPC): dim must be a multiple of 64 x the elements of a 16-byte load");
	std::vector<TpRankRecord> recs(tp_size);
	memcpy(recs.data(), handles, sizeof(TpRankRecord) * tp_size);
	{ // this rank's record must describe the stream it decodes on
		uint32_t m[YALM_CU_MASK_WORDS];
		TRY(stream_cu_mask(reinterpret_cast<hipStream_t>(s), m));
		ARGCHK(!memcmp(m, recs[tp_rank].cu_mask, sizeof(m)),
		       "yalm_decoder_create_tp_ipc: this rank's record was made for another stream (CU mask differs)");
	}
	std::vector<float *> bases(tp_size);
	std::vector<void *> opened;
	for (int p = 0; p < tp_size; ++p) {
		if (p == tp_rank) {
			bases[p] = (float *)own_buf;
			continue;
		}
		hipIpcMemHandle_t h;
		memcpy(&h, recs[p].ipc, sizeof(h));
		void *ptr = nullptr;
		if (hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
			for (void *q : opened)
				(void)hipIpcCloseMemHandle(q);
			set_err("hipIpcOpenMemHandle failed");
			return YALM_ERR_HIP;
		}
		opened.push_back(ptr);
		bases[p] = (float *)ptr;
	}
	const int r = create_decoder(&lc, weights, s, out, nullptr, tp_rank, tp_size, config->vocab_size);
	if (r != YALM_OK) {
		for (void *q : opened)
			(void)hipIpcCloseMemHandle(q);
		return r;
	}
	yalm_decoder_s *d = *out;
	d->ipc = true;
	d->ipc_S = ipc_slot_floats(*config, tp_size);
	d->ipc_own = (float *)own_buf;
	d->ipc_opened = opened;
	void *dev_bases = nullptr;
	if (dalloc(d, &dev_bases, sizeof(float *) * tp_size) != YALM_OK ||
	    hipMemcpy(dev_bases, bases.data(), sizeof(float *) * tp_size, hipMemcpyHostToDevice) != hipSuccess) {
		destroy_decoder(d);
		*out = nullptr;
		set_err("IPC pointer table upload failed");
		return YALM_ERR_HIP;
	}
	d->ipc_bufs = (float **)dev_bases;
	// Ranks whose kernels can hold each other's CUs: the same GPU (UUID) with overlapping CU
	// masks (several rank processes on one GPU without yalm_stream_create_cu_part). One GPU
	// per rank -- or disjoint CU masks on one GPU, the rehearsal of that -- needs no gate.
	for (int p = 0; p < tp_size; ++p) {
		if (p == tp_rank || memcmp(recs[p].uuid, recs[tp_rank].uuid, sizeof(recs[p].uuid)))
			continue;
		for (int i = 0; i < YALM_CU_MASK_WORDS; ++i)
			if (recs[p].cu_mask[i] & recs[tp_rank].cu_mask[i])
				d->tpx_gate = true;
	}
	// The fused attention + Wo launch's Wo workgroups spin on attention workgroups of the
	// same launch; a workgroup only ever waits on lower-index ones, and each XCD dispatches
	// its workgroups in index order, so by induction on the index every workgroup is
	// dispatched and finishes whatever fits at once (on a CU-masked rehearsal stream the
	// production grid runs in several rounds: correct, just slower). Ranks whose grids SHARE
	// CUs break that: a workgroup dispatched on a full XCD can trail another rank's Wo
	// workgroups spinning there (measured: TP8 at Mistral dims, 8 unmasked processes on one
	// MI355X, the Wo gather timed out). Those ranks keep the separate attention and Wo launches.
	if (d->tpx_gate && d->attn_wo && d->awo_nb * tp_size > d->awo_slots)
		d->attn_wo = d->attn_wo_ok = false;
	d->tpx_collect = tp_size > TPX_STAGE_MAX_RANKS;
	d->tpx.bufs = d->ipc_bufs;
	d->tpx.rank = tp_rank;
	d->tpx.n = tp_size;
	d->tpx.S = d->ipc_S;
	d->tpx.xw = d->x;
	d->tpx.step = d->step;
	d->tpx.ex = 0;
	return YALM_OK;
}

extern "C" int yalm_copy_2d(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t width,
                            size_t height) {
	ARGCHK(dst && src && width <= dst_pitch && width <= src_pitch, "yalm_copy_2d: bad argument");
	HIPCHK(hipMemcpy2D(dst, dst_pitch, src, src_pitch, width, height, hipMemcpyDeviceToDevice));
	return YALM_OK;
}

extern "C" int yalm_decoder_destroy(yalm_decoder d) {
	if (!d)
		return YALM_OK;
	(void)hipStreamSynchronize(d->stream);
	destroy_decoder(d);
	return YALM_OK;
}

extern "C" int yalm_forward(yalm_decoder d, int token, int pos, int mode, float *logits_host) {
	ARGCHK(d, "null decoder");
	ARGCHK(token >= 0 && token < d->vocab_full, "token out of range");
	ARGCHK(pos >= 0, "negative pos");
	const int which = mode == YALM_HYDRATE_KV_CACHE ? GRAPH_HYDRATE : GRAPH_LOGITS;
	TRY(ensure_graph(d, which));
	set_step_kernel<<<1, 1, 0, d->stream>>>(d->step, token, pos, 0);
	HIPCHK(hipGetLastError());
	TRY(replay(d, which));
	d->host_pos = pos; // OUTPUT / HYDRATE forwards do not advance the device position
	if (which == GRAPH_LOGITS) {
		HIPCHK(hipStreamSynchronize(d->stream));
		TRY(awo_check(d));
		if (logits_host)
			memcpy(logits_host, d->logits_pinned, sizeof(float) * d->vocab_full);
	}
	return YALM_OK;
}

// n greedy forwards from position pos0 (-1: unknown); the eager path passes each forward's
// kv_len to the attention + Wo launch (awo_kv_hint), graph replays cannot
static int replay_greedy(yalm_decoder_s *d, int n, long long pos0, int which = GRAPH_GREEDY) {
	if (!d->greedy_eager)
		TRY(ensure_graph(d, which));
	int r = YALM_OK;
	for (int i = 0; i < n && r == YALM_OK; ++i) {
		d->awo_kv_hint = pos0 >= 0 ? std::min<long long>(pos0 + i + 1, d->c.max_seq_len) : -1;
		r = replay(d, which);
	}
	d->awo_kv_hint = -1;
	return r;
}

extern "C" int yalm_enqueue_greedy(yalm_decoder d, int n_steps) {
	ARGCHK(d, "null decoder");
	ARGCHK(n_steps >= 0, "bad n_steps");
	TRY(replay_greedy(d, n_steps, d->host_pos)); // each forward advances the device position by one
	if (d->host_pos >= 0)
		d->host_pos += n_steps;
	return YALM_OK;
}

extern "C" int yalm_generate_greedy(yalm_decoder d, int token, int pos, int n_steps, int *out_tokens) {
	ARGCHK(d && out_tokens, "null argument");
	ARGCHK(token >= 0 && token < d->vocab_full && pos >= 0 && n_steps >= 0, "bad token/pos/n_steps");
	int done = 0;
	bool first = true;
	while (done < n_steps) {
		const int batch = std::min(n_steps - done, d->tokens_cap);
		if (first)
			set_step_kernel<<<1, 1, 0, d->stream>>>(d->step, token, pos, 1);
		else
			set_step_kernel<<<1, 1, 0, d->stream>>>(d->step, out_tokens[done - 1], pos + done, 1);
		HIPCHK(hipGetLastError());
		first = false;
		TRY(replay_greedy(d, batch, (long long)pos + done));
		d->host_pos = (long long)pos + done + batch;
		HIPCHK(hipMemcpyAsync(out_tokens + done, d->tokens, sizeof(int) * batch, hipMemcpyDeviceToHost, d->stream));
		HIPCHK(hipStreamSynchronize(d->stream));
		TRY(awo_check(d));
		done += batch;
	}
	return YALM_OK;
}

static int validate_sampling(const yalm_sampling *s, const float *uniforms, int n_u) {
	ARGCHK(s && uniforms, "sampling: null argument");
	ARGCHK(s->temperature > 0.0f && std::isfinite(s->temperature), "sampling: temperature must be finite and > 0");
	ARGCHK(s->top_k >= 0, "sampling: top_k must be >= 0 (0 = off)");
	ARGCHK(s->top_p > 0.0f && s->top_p <= 1.0f, "sampling: top_p must be in (0, 1] (1 = off)");
	for (int i = 0; i < n_u; ++i)
		ARGCHK(uniforms[i] >= 0.0f && uniforms[i] <= 1.0f, "sampling: every uniform must be in [0, 1]");
	return YALM_OK;
}

extern "C" int yalm_generate_sampled(yalm_decoder d, int token, int pos, int n_steps, const yalm_sampling *s,
                                     const float *uniforms, int *out_tokens) {
	ARGCHK(d && out_tokens, "null argument");
	ARGCHK(token >= 0 && token < d->vocab_full && pos >= 0 && n_steps >= 0, "bad token/pos/n_steps");
	ARGCHK(n_steps <= d->tokens_cap, "yalm_generate_sampled: n_steps exceeds the token buffer (65536)");
	TRY(validate_sampling(s, uniforms, n_steps));
	if (d->tp_size > 1 || d->comm || d->ipc) {
		set_err("yalm_generate_sampled: tensor-parallel decoders shard the vocabulary; device sampling runs on one GPU");
		return YALM_ERR_UNSUPPORTED;
	}
	ARGCHK(d->c.vocab_size <= SMP_MAX_N, "yalm_generate_sampled: vocabulary above 131072");
	if (n_steps == 0)
		return YALM_OK;
	static_assert(sizeof(yalm_sampling) == sizeof(SampleParams), "yalm_sampling layout");
	HIPCHK(hipMemcpyAsync(d->smp_params, s, sizeof(SampleParams), hipMemcpyHostToDevice, d->stream));
	HIPCHK(hipMemcpyAsync(d->smp_u, uniforms, sizeof(float) * n_steps, hipMemcpyHostToDevice, d->stream));
	set_step_kernel<<<1, 1, 0, d->stream>>>(d->step, token, pos, 1);
	HIPCHK(hipGetLastError());
	TRY(replay_greedy(d, n_steps, pos, GRAPH_SAMPLED));
	d->host_pos = (long long)pos + n_steps;
	HIPCHK(hipMemcpyAsync(out_tokens, d->tokens, sizeof(int) * n_steps, hipMemcpyDeviceToHost, d->stream));
	HIPCHK(hipStreamSynchronize(d->stream));
	return awo_check(d);
}

// ------------------------------------------------------------------ multi-row forward, speculative greedy decode
// (gemv_rows.h, spec.h) Dense decoders on one GPU, f32 / f16 / fp8 (E5M2) / e4m3 weights.
static const char *const ROWS_Q4_WHY = ": q4 weights have no multi-row form (gemv_rows.h streams element-typed rows)";
static int rows_supported(const yalm_decoder_s *d, const char *who) {
	const char *why = nullptr;
	if (d->c.weight_dtype == YALM_Q4)
		why = ROWS_Q4_WHY;
	else if (d->moe_E > 0)
		why = ": mixture-of-experts decoders have no multi-row form (each row routes to its own experts)";
	else if (d->tp_size > 1 || d->comm || d->ipc)
		why = ": tensor-parallel decoders have no multi-row form (the exchanges carry one row)";
	if (!why)
		return YALM_OK;
	set_err(std::string(who) + why);
	return YALM_ERR_UNSUPPORTED;
}

static int rows_init(yalm_decoder_s *d) {
	if (d->rlogits_pinned)
		return YALM_OK;
	const yalm_config &c = d->c;
	const int q_dim = c.n_heads * c.head_dim;
	constexpr int T = ROWS_MAX_T;
	static_assert(ROWS_MAX_T == SPEC_MAX_ROWS, "rows of a step");
	TRY(dalloc(d, (void **)&d->rstep, sizeof(StepState) * T));
	TRY(dalloc(d, (void **)&d->rx, sizeof(float) * T * c.dim));
	TRY(dalloc(d, (void **)&d->rq, sizeof(float) * T * q_dim));
	TRY(dalloc(d, (void **)&d->rxb2, sizeof(float) * T * q_dim));
	TRY(dalloc(d, (void **)&d->rhb, sizeof(float) * T * c.hidden_dim));
	TRY(dalloc(d, (void **)&d->rlogits, sizeof(float) * T * c.vocab_size));
	TRY(dalloc(d, (void **)&d->spec, sizeof(SpecState)));
	TRY(dalloc(d, (void **)&d->spec_ctx, sizeof(int) * d->tokens_cap));
	d->spec_stream_cap = d->tokens_cap + 8;
	TRY(dalloc(d, (void **)&d->spec_stream, sizeof(int) * d->spec_stream_cap));
	HIPCHK(hipHostMalloc((void **)&d->rlogits_pinned, sizeof(float) * T * c.vocab_size, hipHostMallocDefault));
	return YALM_OK;
}

// The geometry of one gemv_rows_kernel launch over rows of n elements in chunks of CH, n_groups
// groups and T activation rows on `cus` CUs: x staged whole when T rows of it fit ROWS_X_BYTES
// (then a wave takes several groups, about one workgroup per CU), else by K segments with one
// group per wave. Pure host arithmetic.
struct RowsPlan {
	int kseg, nseg, gpw, blocks;
	size_t lds;
};
static RowsPlan rows_plan(int CH, int n, int n_groups, int T, int cus) {
	constexpr int W = ROWS_THREADS / YALM_WAVE;
	RowsPlan r;
	const int kcap = (int)(ROWS_X_BYTES / sizeof(float)) / T / CH * CH;
	r.kseg = std::min((n + CH - 1) / CH * CH, kcap);
	r.nseg = (n + r.kseg - 1) / r.kseg;
	r.gpw = r.nseg > 1 ? 1 : std::max(1, n_groups / (W * cus));
	r.blocks = (n_groups + W * r.gpw - 1) / (W * r.gpw);
	r.lds = ((size_t)T * r.kseg + (size_t)T * 16) * sizeof(float);
	return r;
}

extern "C" int yalm_rows_plan(int dtype, int n, int n_groups, int T, int cus, int *kseg, int *nseg, int *gpw,
                              int *blocks, size_t *lds) {
	if (dtype == YALM_Q4) {
		set_err(std::string("yalm_rows_plan") + ROWS_Q4_WHY);
		return YALM_ERR_UNSUPPORTED;
	}
	ARGCHK(dtype_ok(dtype), "yalm_rows_plan: bad dtype");
	ARGCHK(n > 0 && n_groups > 0 && cus >= 0 && T >= 1 && T <= ROWS_MAX_T, "yalm_rows_plan: bad argument");
	const int EPL = dtype == YALM_F32 ? WF32::EPL : dtype == YALM_F16 ? WF16::EPL : WF8::EPL; // (e4m3: WF8's)
	static_assert(WE4M3::EPL == WF8::EPL, "e4m3 plans as fp8");
	const RowsPlan r = rows_plan(YALM_WAVE * EPL, n, n_groups, T, cus ? cus : device_cu_count());
	if (kseg)
		*kseg = r.kseg;
	if (nseg)
		*nseg = r.nseg;
	if (gpw)
		*gpw = r.gpw;
	if (blocks)
		*blocks = r.blocks;
	if (lds)
		*lds = r.lds;
	return YALM_OK;
}

// One launch of gemv_rows_kernel at the geometry of rows_plan.
template <class WT, class P, bool NORM>
static int launch_rows(const P &p, const float *x, int xstride, const float *normw, float eps, int T, hipStream_t st) {
	const RowsPlan pl = rows_plan(YALM_WAVE * WT::EPL, p.n, p.n_groups, T, device_cu_count());
	const int kseg = pl.kseg, gpw = pl.gpw, blocks = pl.blocks;
	const size_t lds = pl.lds;
	auto kern = T == 1   ? gemv_rows_kernel<WT, P, 1, NORM>
	            : T == 2 ? gemv_rows_kernel<WT, P, 2, NORM>
	            : T == 3 ? gemv_rows_kernel<WT, P, 3, NORM>
	                     : gemv_rows_kernel<WT, P, 4, NORM>;
	if (lds > 65536)
		HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	hipLaunchKernelGGL(kern, dim3(blocks), dim3(ROWS_THREADS), lds, st, p, x, xstride, normw, eps, gpw, kseg);
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

// ---- the multi-row policies, filled (the rows forward and yalm_matmul_rows build theirs here): `rows`
// weight rows of n elements, the T outputs ostride floats apart
template <class WT>
static RStore<WT> make_rstore(const void *W, int n, int rows, float *out, int ostride) {
	return {(const char *)W, n, rows, (rows + 1) / 2, out, ostride};
}
template <class WT>
static RResidual<WT> make_rresidual(const void *W, int n, int rows, float *out, int ostride) {
	return {(const char *)W, n, rows, (rows + 1) / 2, out, ostride};
}
template <class WT, int ACT>
static RGlu<WT, ACT> make_rglu(const void *w1, const void *w3, int n, int hidden, float *out, int ostride) {
	return {(const char *)w1, (const char *)w3, n, hidden, out, ostride};
}
// a PQKV, PQKVB or PQKVN base as RQKV, RQKVB or RQKVN on the T row states: q rows (RQKVN: raw rows) `stride` apart
// (RQKVN gets q_out = rq as the others do: PQKVN's epilogue and the V path of PQKV's never read q_out)
template <class RP, class BP>
static RP make_rqkv(BP base, const StepState *rstep, float *rq, int stride) {
	base.step = rstep;
	base.q_out = rq;
	return {base, base.n, base.n_groups, stride};
}
template <class WT, bool NORM>
static int launch_rows_glu(const void *w1, const void *w3, int n, int hidden, float *out, int ostride, int act,
                           const float *x, int xstride, const float *normw, float eps, int T, hipStream_t st) {
	if (act == YALM_SILU)
		return launch_rows<WT, RGlu<WT, 1>, NORM>(make_rglu<WT, 1>(w1, w3, n, hidden, out, ostride), x, xstride, normw, eps,
		                                          T, st);
	return launch_rows<WT, RGlu<WT, 0>, NORM>(make_rglu<WT, 0>(w1, w3, n, hidden, out, ostride), x, xstride, normw, eps, T,
	                                          st);
}

// T rows through every layer: rows begin, then per layer QKV (+ clip, RoPE, KV write), one
// attention launch per row (the decode kernel with that row's step state, q and out), Wo, W1|W3,
// W2; then norm + logits into rlogits [T][vocab]. 2 + n_layers * (4 + T) launches, one more per
// layer with the q / k norm.
template <class WT>
static int enqueue_rows_forward_t(yalm_decoder_s *d, int T, int from_step) {
	if constexpr (WT::Q4) {
		return rows_supported(d, "multi-row forward");
	} else {
		const yalm_config &c = d->c;
		hipStream_t st = d->stream;
		const int q_dim = c.n_heads * c.head_dim;
		static_assert(offsetof(SpecState, tok) == 0, "SpecState begins with the row tokens");
		rows_begin_kernel<WT><<<1, 256, 0, st>>>(d->step, d->rstep, (const int *)d->spec, T, from_step, d->emb, c.dim,
		                                          d->rx, d->inv_freq, c.head_dim / 2);
		HIPCHK(hipGetLastError());
		for (int l = 0; l < c.n_layers; ++l) {
			const yalm_block_weights &w = d->b[l];
			switch (qkv_form(d)) {
			case QKV_NORM: // raw rows, then one norm launch for all T rows
				TRY((launch_rows<WT, RQKVN<WT>, true>(
				    make_rqkv<RQKVN<WT>>(make_pqkvn<WT>(d, l), d->rstep, d->rq, q_dim + c.n_kv_heads * c.head_dim), d->rx,
				    c.dim, w.rms_att, c.norm_eps, T, st)));
				TRY(launch_qk_norm(d, l, T, d->rstep, d->rq));
				break;
			case QKV_BIAS:
				TRY((launch_rows<WT, RQKVB<WT>, true>(make_rqkv<RQKVB<WT>>(make_pqkvb<WT>(d, l), d->rstep, d->rq, q_dim),
				                                      d->rx, c.dim, w.rms_att, c.norm_eps, T, st)));
				break;
			default:
				TRY((launch_rows<WT, RQKV<WT>, true>(make_rqkv<RQKV<WT>>(make_pqkv<WT>(d, l), d->rstep, d->rq, q_dim), d->rx,
				                                     c.dim, w.rms_att, c.norm_eps, T, st)));
			}
			for (int t = 0; t < T; ++t)
				TRY(enqueue_attn(d, l, d->rq + (size_t)t * q_dim, d->rstep + t, d->rxb2 + (size_t)t * q_dim));
			TRY((launch_rows<WT, RResidual<WT>, false>(make_rresidual<WT>(w.wo, q_dim, c.dim, d->rx, c.dim), d->rxb2, q_dim,
			                                           nullptr, 0.f, T, st)));
			TRY((launch_rows_glu<WT, true>(w.w1, w.w3, c.dim, c.hidden_dim, d->rhb, c.hidden_dim, c.act, d->rx, c.dim,
			                               w.rms_ffn, c.norm_eps, T, st)));
			TRY((launch_rows<WT, RResidual<WT>, false>(make_rresidual<WT>(w.w2, c.hidden_dim, c.dim, d->rx, c.dim), d->rhb,
			                                           c.hidden_dim, nullptr, 0.f, T, st)));
		}
		return launch_rows<WT, RStore<WT>, true>(make_rstore<WT>(d->wcls, c.dim, c.vocab_size, d->rlogits, c.vocab_size),
		                                         d->rx, c.dim, d->rms_final, c.norm_eps, T, st);
	}
}

static int enqueue_rows_forward(yalm_decoder_s *d, int T, int from_step) {
	return DISPATCH_WT(d->c.weight_dtype, enqueue_rows_forward_t, d, T, from_step);
}

extern "C" int yalm_forward_rows(yalm_decoder d, const int *tokens, int T, int pos, float *logits_host) {
	ARGCHK(d && tokens, "yalm_forward_rows: null argument");
	TRY(rows_supported(d, "yalm_forward_rows"));
	ARGCHK(T >= 1 && T <= ROWS_MAX_T, "yalm_forward_rows: 1 <= T <= 4 rows");
	for (int t = 0; t < T; ++t)
		ARGCHK(tokens[t] >= 0 && tokens[t] < d->vocab_full, "yalm_forward_rows: token out of range");
	ARGCHK(pos >= 0 && (long long)pos + T <= d->c.max_seq_len,
	       "yalm_forward_rows: pos + T must not exceed max_seq_len (no ring wrap inside a multi-row step)");
	TRY(rows_init(d));
	int tk[ROWS_MAX_T] = {0, 0, 0, 0};
	for (int t = 0; t < T; ++t)
		tk[t] = tokens[t];
	spec_set_tok_kernel<<<1, 1, 0, d->stream>>>(d->spec, tk[0], tk[1], tk[2], tk[3]);
	set_step_kernel<<<1, 1, 0, d->stream>>>(d->step, tk[0], pos, 0);
	HIPCHK(hipGetLastError());
	TRY(enqueue_rows_forward(d, T, 0));
	d->host_pos = pos; // as an OUTPUT forward: the device position does not advance
	if (logits_host) {
		const size_t bytes = sizeof(float) * (size_t)T * d->c.vocab_size;
		HIPCHK(hipMemcpyAsync(d->rlogits_pinned, d->rlogits, bytes, hipMemcpyDeviceToHost, d->stream));
		HIPCHK(hipStreamSynchronize(d->stream));
		TRY(awo_check(d));
		memcpy(logits_host, d->rlogits_pinned, bytes);
	}
	return YALM_OK;
}

extern "C" int yalm_spec_draft(const int *history, int m, int rows, int ngram_max, int ngram_min, int *drafts_out) {
	ARGCHK(history && drafts_out, "yalm_spec_draft: null argument");
	ARGCHK(m >= 1 && m <= 2 * 65536, "yalm_spec_draft: history of 1..131072 tokens");
	ARGCHK(rows >= 2 && rows <= SPEC_MAX_ROWS, "yalm_spec_draft: rows must be 2..4");
	ARGCHK(ngram_min >= 1 && ngram_min <= ngram_max && ngram_max <= SPEC_MAX_NGRAM,
	       "yalm_spec_draft: need 1 <= ngram_min <= ngram_max <= 4");
	int *dh = nullptr, *dd = nullptr;
	HIPCHK(hipMalloc((void **)&dh, sizeof(int) * m));
	if (hipMalloc((void **)&dd, sizeof(int) * SPEC_MAX_ROWS) != hipSuccess) {
		(void)hipFree(dh);
		set_err("yalm_spec_draft: hipMalloc failed");
		return YALM_ERR_HIP;
	}
	int out[SPEC_MAX_ROWS] = {-1, -1, -1, -1};
	hipError_t e = hipMemcpy(dh, history, sizeof(int) * m, hipMemcpyHostToDevice);
	if (e == hipSuccess) {
		spec_draft_test_kernel<<<1, SPEC_DRAFT_THREADS>>>(dh, m, rows, ngram_max, ngram_min, dd);
		e = hipGetLastError();
	}
	if (e == hipSuccess)
		e = hipMemcpy(out, dd, sizeof(out), hipMemcpyDeviceToHost);
	(void)hipFree(dh);
	(void)hipFree(dd);
	if (e != hipSuccess) {
		set_err(std::string("yalm_spec_draft failed: ") + hipGetErrorString(e));
		return YALM_ERR_HIP;
	}
	for (int k = 1; k < rows; ++k)
		drafts_out[k - 1] = out[k];
	return YALM_OK;
}

// ---- the draft-model drafter (spec.h): a second decoder on the target's stream proposes the rows
static int model_drafts_check(const yalm_decoder_s *d, const yalm_decoder_s *draft, const std::string &who) {
	ARGCHK(draft != d, who + ": the draft decoder must not be the target decoder");
	const char *why = nullptr;
	if (draft->moe_E > 0)
		why = ": a mixture-of-experts draft decoder is not supported (the draft is a dense one-GPU decoder)";
	else if (draft->tp_size > 1 || draft->comm || draft->ipc)
		why = ": a tensor-parallel draft decoder is not supported (the draft is a dense one-GPU decoder)";
	if (why) {
		set_err(who + why);
		return YALM_ERR_UNSUPPORTED;
	}
	ARGCHK(draft->stream == d->stream,
	       who + ": the two decoders must share one stream (create the draft on yalm_decoder_get_stream of the target)");
	ARGCHK(draft->c.max_seq_len >= d->c.max_seq_len, who + ": the draft's max_seq_len is below the target's");
	return YALM_OK;
}

// Kernel launches of one greedy and of one KV-only forward of the draft decoder: the kernel
// nodes of its own graphs (what yalm_graph_kernels reports in modes 2 and 0; an eagerly
// launching decoder captures the sequence once to count it). Leaves the KV-only graph ready.
static int graph_kernel_count(hipGraph_t g, int *kernels, int *nodes) {
	size_t n = 0;
	HIPCHK(hipGraphGetNodes(g, nullptr, &n));
	std::vector<hipGraphNode_t> v(n);
	if (n)
		HIPCHK(hipGraphGetNodes(g, v.data(), &n));
	int k = 0;
	for (auto node : v) {
		hipGraphNodeType t;
		HIPCHK(hipGraphNodeGetType(node, &t));
		k += t == hipGraphNodeTypeKernel;
	}
	*kernels = k;
	if (nodes)
		*nodes = (int)n;
	return YALM_OK;
}

static int model_drafts_kernels(yalm_decoder_s *draft, int *greedy, int *hydrate) {
	const int which[2] = {GRAPH_GREEDY, GRAPH_HYDRATE};
	int *const out[2] = {greedy, hydrate};
	for (int i = 0; i < 2; ++i) {
		if (!draft->eager) {
			TRY(ensure_graph(draft, which[i]));
			TRY(graph_kernel_count(draft->graph[which[i]], out[i], nullptr));
			continue;
		}
		HIPCHK(hipStreamBeginCapture(draft->stream, hipStreamCaptureModeRelaxed));
		const int r = enqueue_forward(draft, which[i]);
		hipGraph_t g = nullptr;
		const hipError_t e = hipStreamEndCapture(draft->stream, &g);
		if (r != YALM_OK)
			return r;
		HIPCHK(e);
		const int rc = graph_kernel_count(g, out[i], nullptr);
		(void)hipGraphDestroy(g);
		TRY(rc);
	}
	return YALM_OK;
}

// One step's drafts: sync, rows - 1 greedy forwards of the draft from its device state (the
// path of yalm_enqueue_greedy, position unknown to the host), the KV-only forward of the last
// draft at the state they left, gather. No host synchronisation.
static int enqueue_model_drafts(yalm_decoder_s *d, yalm_decoder_s *draft, int rows, const int *stream, int stream_len) {
	hipStream_t st = d->stream;
	spec_model_sync_kernel<<<1, 64, 0, st>>>(d->step, d->spec, draft->step, draft->c.vocab_size);
	HIPCHK(hipGetLastError());
	TRY(replay_greedy(draft, rows - 1, -1));
	TRY(replay(draft, GRAPH_HYDRATE));
	spec_model_gather_kernel<<<1, 64, 0, st>>>(d->step, d->spec, draft->tokens, d->tokens_cap, rows, stream, stream_len,
	                                           d->c.vocab_size);
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

// The speculative loop, greedy (smp == nullptr: every row's argmax, spec_verify_kernel) or sampled
// (every row drawn with the uniform of its output index, spec_sample_rows_kernel, then
// spec_accept_kernel; the plain steps past the window are sample_kernel steps).
// The drafter is the loop's one hook: the n-gram launch (draft == nullptr), or a draft decoder's
// forwards between a sync and a gather launch (model_drafts_check / enqueue_model_drafts).
static int generate_speculative(yalm_decoder_s *d, const char *name, int token, int pos, int n_tokens,
                                const yalm_spec *cfg, const yalm_sampling *smp, const float *uniforms,
                                const int *context, int n_context, int *out_tokens, yalm_spec_stats *stats,
                                yalm_decoder_s *draft = nullptr) {
	const std::string who(name);
	ARGCHK(d && cfg && (out_tokens || n_tokens == 0), who + ": null argument");
	TRY(rows_supported(d, name));
	if (draft)
		TRY(model_drafts_check(d, draft, who));
	ARGCHK(token >= 0 && token < d->vocab_full && pos >= 0 && n_tokens >= 0, who + ": bad token/pos/n_tokens");
	ARGCHK(cfg->rows >= 2 && cfg->rows <= SPEC_MAX_ROWS, who + ": rows must be 2..4");
	ARGCHK(cfg->ngram_min >= 1 && cfg->ngram_min <= cfg->ngram_max && cfg->ngram_max <= SPEC_MAX_NGRAM,
	       who + ": need 1 <= ngram_min <= ngram_max <= 4");
	ARGCHK(n_tokens <= d->tokens_cap, who + ": n_tokens exceeds the token buffer (65536)");
	ARGCHK(n_context >= 0 && (n_context == 0 || context), who + ": bad context");
	ARGCHK(n_context == 0 || context[n_context - 1] == token, who + ": the context must end with the token to feed");
	ARGCHK(cfg->draft_stream_len >= 0 && (cfg->draft_stream || cfg->draft_stream_len == 0), who + ": bad draft_stream");
	if (smp) {
		TRY(validate_sampling(smp, uniforms, n_tokens));
		ARGCHK(d->c.vocab_size <= SMP_MAX_N, who + ": vocabulary above 131072");
	}
	const int rows = cfg->rows, L = d->c.n_layers, n = n_tokens;
	yalm_spec_stats s{};
	s.launches_per_step = (smp ? 5 : 4) + L * ((d->gq.empty() ? 4 : 5) + rows);
	if (draft) { // sync + gather in the n-gram launch's place, and the draft's forwards
		int kg = 0, kh = 0;
		TRY(model_drafts_kernels(draft, &kg, &kh));
		s.launches_per_step += 1 + (rows - 1) * kg + kh;
	}
	if (n == 0) {
		if (stats)
			*stats = s;
		return YALM_OK;
	}
	TRY(rows_init(d));
	hipStream_t st = d->stream;
	if (smp) {
		HIPCHK(hipMemcpyAsync(d->smp_params, smp, sizeof(SampleParams), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d->smp_u, uniforms, sizeof(float) * n, hipMemcpyHostToDevice, st));
	}
	int n_ctx = 1;
	if (n_context == 0) {
		HIPCHK(hipMemcpyAsync(d->spec_ctx, &token, sizeof(int), hipMemcpyHostToDevice, st));
	} else {
		n_ctx = std::min(n_context, d->tokens_cap);
		HIPCHK(hipMemcpyAsync(d->spec_ctx, context + (n_context - n_ctx), sizeof(int) * n_ctx, hipMemcpyHostToDevice, st));
	}
	const int *stream = nullptr;
	int stream_len = 0;
	if (cfg->draft_stream) {
		stream = d->spec_stream;
		stream_len = std::min(cfg->draft_stream_len, std::min(n + rows, d->spec_stream_cap));
		if (stream_len > 0)
			HIPCHK(hipMemcpyAsync(d->spec_stream, cfg->draft_stream, sizeof(int) * stream_len, hipMemcpyHostToDevice, st));
	}
	HIPCHK(hipMemsetAsync(d->spec, 0, sizeof(SpecState), st));
	set_step_kernel<<<1, 1, 0, st>>>(d->step, token, pos, 1);
	HIPCHK(hipGetLastError());
	const int V = d->c.vocab_size;
	int done = 0;
	while (done < n) {
		const long long p = (long long)pos + done;
		// every step of a batch must keep its rows inside the window whatever the steps before it accepted
		const int room = p + rows <= d->c.max_seq_len ? (int)((d->c.max_seq_len - p) / rows) : 0;
		if (room == 0) { // the window's end (and past it): the plain steps
			TRY(replay_greedy(d, n - done, p, smp ? GRAPH_SAMPLED : GRAPH_GREEDY));
			s.plain_steps = n - done;
			done = n;
			break;
		}
		const int batch = std::min(std::min((n - done + rows - 1) / rows, room), 64);
		for (int i = 0; i < batch; ++i) {
			if (draft) {
				TRY(enqueue_model_drafts(d, draft, rows, stream, stream_len));
			} else {
				spec_draft_kernel<<<1, SPEC_DRAFT_THREADS, 0, st>>>(d->step, d->spec, d->spec_ctx, n_ctx, d->tokens,
				                                                    d->tokens_cap, rows, cfg->ngram_max, cfg->ngram_min,
				                                                    stream, stream_len, V);
				HIPCHK(hipGetLastError());
			}
			TRY(enqueue_rows_forward(d, rows, 1));
			if (smp) { // rows past output index n - 1 read the clamped last uniform; their tokens are dropped below
				if (V % 4 == 0)
					spec_sample_rows_kernel<true><<<rows, SMP_THREADS, 0, st>>>(d->rlogits, V, V, d->smp_params, d->smp_u,
					                                                           n, d->step, d->spec, nullptr);
				else
					spec_sample_rows_kernel<false><<<rows, SMP_THREADS, 0, st>>>(d->rlogits, V, V, d->smp_params,
					                                                            d->smp_u, n, d->step, d->spec, nullptr);
				HIPCHK(hipGetLastError());
				spec_accept_kernel<<<1, 64, 0, st>>>(rows, d->step, d->spec, d->tokens, d->tokens_cap);
			} else {
				spec_verify_kernel<<<1, 1024, 0, st>>>(d->rlogits, V, rows, d->step, d->spec, d->tokens, d->tokens_cap);
			}
			HIPCHK(hipGetLastError());
		}
		int produced = 0; // the batch's one round trip
		HIPCHK(hipMemcpyAsync(&produced, &d->step->n_gen, sizeof(int), hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		TRY(awo_check(d));
		if (draft)
			TRY(awo_check(draft));
		if (produced <= done) {
			set_err(who + ": internal: a batch produced no token");
			return YALM_ERR_HIP;
		}
		done = produced;
	}
	HIPCHK(hipMemcpyAsync(out_tokens, d->tokens, sizeof(int) * n, hipMemcpyDeviceToHost, st));
	SpecState sp;
	HIPCHK(hipMemcpyAsync(&sp, d->spec, sizeof(sp), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	TRY(awo_check(d));
	if (done > n) { // the last step accepted past the request: those drafts are not delivered
		spec_fix_kernel<<<1, 1, 0, st>>>(d->step, out_tokens[n - 1], pos + n, n);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(st));
	}
	d->host_pos = (long long)pos + n;
	if (draft)
		draft->host_pos = -1; // its device (token, pos) is wherever the last step's forwards left it
	s.spec_steps = sp.steps;
	s.accepted_drafts = sp.accepted - std::max(0, done - n);
	if (stats)
		*stats = s;
	return YALM_OK;
}

extern "C" int yalm_generate_speculative(yalm_decoder d, int token, int pos, int n_tokens, const yalm_spec *cfg,
                                         const int *context, int n_context, int *out_tokens,
                                         yalm_spec_stats *stats) {
	return generate_speculative(d, "yalm_generate_speculative", token, pos, n_tokens, cfg, nullptr, nullptr, context,
	                            n_context, out_tokens, stats);
}

extern "C" int yalm_generate_speculative_sampled(yalm_decoder d, int token, int pos, int n_tokens, const yalm_spec *cfg,
                                                 const yalm_sampling *s, const float *uniforms, const int *context,
                                                 int n_context, int *out_tokens, yalm_spec_stats *stats) {
	ARGCHK(s && (uniforms || n_tokens == 0), "yalm_generate_speculative_sampled: null argument");
	return generate_speculative(d, "yalm_generate_speculative_sampled", token, pos, n_tokens, cfg, s, uniforms, context,
	                            n_context, out_tokens, stats);
}

extern "C" int yalm_generate_speculative_model(yalm_decoder d, yalm_decoder draft, int token, int pos, int n_tokens,
                                               const yalm_spec_model *cfg, const yalm_sampling *s, const float *uniforms,
                                               int *out_tokens, yalm_spec_stats *stats) {
	static const char *const who = "yalm_generate_speculative_model";
	ARGCHK(d && draft && cfg, std::string(who) + ": null argument");
	ARGCHK(!s || uniforms || n_tokens == 0, std::string(who) + ": null argument");
	const yalm_spec spec{cfg->rows, 1, 1, cfg->draft_stream, cfg->draft_stream_len}; // (the n-gram bounds are unused)
	return generate_speculative(d, who, token, pos, n_tokens, &spec, s, s ? uniforms : nullptr, nullptr, 0, out_tokens,
	                            stats, draft);
}

extern "C" int yalm_decoder_get_stream(yalm_decoder d, yalm_stream *out) {
	ARGCHK(d && out, "yalm_decoder_get_stream: null argument");
	*out = reinterpret_cast<yalm_stream>(d->stream);
	return YALM_OK;
}

// ------------------------------------------------------------------ batched decode (batch.h)
// Up to ROWS_MAX_T independent sequences per pass over the decoder's weights. The batch owns every
// per-sequence buffer; it uses the decoder's stream, weights, frequency table, error word and (the
// q / k norm form) raw QKV scratch, and nothing else of it: a decoder without a batch launches
// what it launched before.
#define BATCH_GUARD_BYTES YALM_BATCH_GUARD_BYTES
struct yalm_batch_s {
	yalm_decoder_s *d = nullptr;
	int n_seq = 0, flags = 0;
	StepState *seq = nullptr;              // [n_seq] sequence = row states
	float *x = nullptr, *q = nullptr, *xb2 = nullptr, *hb = nullptr, *logits = nullptr; // [n_seq][...]
	float *logits_pinned = nullptr;        // [n_seq][vocab] host
	std::vector<BatchKV> kv;               // [n_layers]
	BatchTok tok{};
	BatchPart part{};
	SampleParams *smp_params = nullptr;
	float *smp_u = nullptr;                // [n_seq][tokens_cap]
	std::vector<void *> allocs;
};

static void batch_free(yalm_batch_s *b) {
	for (void *p : b->allocs)
		(void)hipFree(p);
	if (b->logits_pinned)
		(void)hipHostFree(b->logits_pinned);
	delete b;
}

// a zeroed device allocation owned by the batch, with BATCH_GUARD_BYTES of 0xA5 on either side
// when guarded (the caches and token buffers: nothing may write there, the tests read them back)
static int batch_alloc(yalm_batch_s *b, void **p, size_t bytes, bool guarded = false) {
	const size_t g = guarded ? BATCH_GUARD_BYTES : 0, payload = (bytes + 255) & ~(size_t)255;
	char *base = nullptr;
	HIPCHK(hipMalloc((void **)&base, payload + 2 * g + 4));
	b->allocs.push_back(base);
	HIPCHK(hipMemset(base, 0, payload + 2 * g + 4));
	if (g) {
		HIPCHK(hipMemset(base, 0xA5, g));
		HIPCHK(hipMemset(base + g + bytes, 0xA5, g));
	}
	*p = base + g;
	return YALM_OK;
}

extern "C" int yalm_batch_create(yalm_decoder d, int n_seq, yalm_batch *out) {
	ARGCHK(d && out, "yalm_batch_create: null argument");
	TRY(rows_supported(d, "yalm_batch_create"));
	ARGCHK(n_seq >= 1 && n_seq <= ROWS_MAX_T, "yalm_batch_create: 1 <= n_seq <= 4 sequences");
	const yalm_config &c = d->c;
	const int q_dim = c.n_heads * c.head_dim, kv_dim = c.n_kv_heads * c.head_dim;
	yalm_batch_s *b = new yalm_batch_s();
	b->d = d;
	b->n_seq = n_seq;
	b->kv.resize(c.n_layers);
	auto build = [&]() -> int {
		const size_t N = (size_t)n_seq;
		TRY(batch_alloc(b, (void **)&b->seq, sizeof(StepState) * N));
		TRY(batch_alloc(b, (void **)&b->x, sizeof(float) * N * c.dim));
		TRY(batch_alloc(b, (void **)&b->q, sizeof(float) * N * q_dim));
		TRY(batch_alloc(b, (void **)&b->xb2, sizeof(float) * N * q_dim));
		TRY(batch_alloc(b, (void **)&b->hb, sizeof(float) * N * c.hidden_dim));
		TRY(batch_alloc(b, (void **)&b->logits, sizeof(float) * N * c.vocab_size));
		TRY(batch_alloc(b, (void **)&b->smp_params, sizeof(SampleParams)));
		TRY(batch_alloc(b, (void **)&b->smp_u, sizeof(float) * N * d->tokens_cap));
		const size_t kvb = sizeof(uint16_t) * (size_t)c.max_seq_len * kv_dim;
		const size_t pb = sizeof(unsigned long long) * (size_t)c.n_heads * attn_nsplit(c.max_seq_len) * (c.head_dim + 2);
		for (int s = 0; s < ROWS_MAX_T; ++s) { // rows past n_seq alias sequence 0's buffers: never used, never null
			if (s >= n_seq) {
				for (int l = 0; l < c.n_layers; ++l)
					b->kv[l].k[s] = b->kv[l].k[0], b->kv[l].v[s] = b->kv[l].v[0];
				b->tok.p[s] = b->tok.p[0];
				b->part.p[s] = b->part.p[0];
				continue;
			}
			for (int l = 0; l < c.n_layers; ++l) {
				TRY(batch_alloc(b, (void **)&b->kv[l].k[s], kvb, true));
				TRY(batch_alloc(b, (void **)&b->kv[l].v[s], kvb, true));
			}
			TRY(batch_alloc(b, (void **)&b->tok.p[s], sizeof(int) * d->tokens_cap, true));
			TRY(batch_alloc(b, (void **)&b->part.p[s], pb));
		}
		HIPCHK(hipHostMalloc((void **)&b->logits_pinned, sizeof(float) * N * c.vocab_size, hipHostMallocDefault));
		if (qkv_form(d) == QKV_NORM && !d->qk_raw)
			TRY(dalloc(d, (void **)&d->qk_raw, sizeof(float) * ROWS_MAX_T * (size_t)(q_dim + kv_dim)));
		return YALM_OK;
	};
	const int r = build();
	if (r != YALM_OK) {
		batch_free(b);
		return r;
	}
	*out = b;
	return YALM_OK;
}

extern "C" int yalm_batch_destroy(yalm_batch b) {
	if (!b)
		return YALM_OK;
	(void)hipStreamSynchronize(b->d->stream);
	batch_free(b);
	return YALM_OK;
}

extern "C" int yalm_batch_set_launch(yalm_batch b, int flags) {
	ARGCHK(b, "yalm_batch_set_launch: null batch");
	ARGCHK((flags & ~YALM_BATCH_ATTN_PER_SEQ) == 0, "yalm_batch_set_launch: unknown flag");
	b->flags = flags;
	return YALM_OK;
}

extern "C" int yalm_batch_buffers(yalm_batch b, int seq, int layer, uint16_t **kcache, uint16_t **vcache,
                                  int **tokens) {
	ARGCHK(b, "yalm_batch_buffers: null batch");
	ARGCHK(seq >= 0 && seq < b->n_seq && layer >= 0 && layer < b->d->c.n_layers, "yalm_batch_buffers: bad seq or layer");
	if (kcache)
		*kcache = b->kv[layer].k[seq];
	if (vcache)
		*vcache = b->kv[layer].v[seq];
	if (tokens)
		*tokens = b->tok.p[seq];
	return YALM_OK;
}

extern "C" int yalm_batch_load(yalm_batch b, int seq, int n_positions) {
	ARGCHK(b, "yalm_batch_load: null batch");
	const yalm_decoder_s *d = b->d;
	ARGCHK(seq >= -1 && seq < b->n_seq, "yalm_batch_load: seq must be -1 (every sequence) or 0 .. n_seq - 1");
	ARGCHK(n_positions >= 0 && n_positions <= d->c.max_seq_len, "yalm_batch_load: n_positions outside [0, max_seq_len]");
	const size_t bytes = sizeof(uint16_t) * (size_t)n_positions * d->c.n_kv_heads * d->c.head_dim;
	if (bytes == 0)
		return YALM_OK;
	for (int s = seq < 0 ? 0 : seq; s < (seq < 0 ? b->n_seq : seq + 1); ++s)
		for (int l = 0; l < d->c.n_layers; ++l) {
			HIPCHK(hipMemcpyAsync(b->kv[l].k[s], d->b[l].key_cache, bytes, hipMemcpyDeviceToDevice, d->stream));
			HIPCHK(hipMemcpyAsync(b->kv[l].v[s], d->b[l].value_cache, bytes, hipMemcpyDeviceToDevice, d->stream));
		}
	return YALM_OK;
}

// The attention of every sequence as one launch: launch_attn_D's choices of S, hmax and nsplit.
template <int D>
static void launch_attn_batch_D(const yalm_batch_s *b, int l) {
	const yalm_decoder_s *d = b->d;
	const yalm_config &c = d->c;
	const int G = c.n_heads / c.n_kv_heads, q_dim = c.n_heads * c.head_dim;
	static const int splits = ab_env("YALM_ATTN_SPLITS") ? std::max(1, std::min(ATTN_MAX_SPLITS, atoi(ab_env("YALM_ATTN_SPLITS")))) : ATTN_SPLITS;
	const int nchunks = (c.max_seq_len + attn_chunk<D>() - 1) / attn_chunk<D>();
	const int S = std::min(nchunks, splits);
	const int per_seq = c.n_kv_heads * (S + G - 1) + c.n_heads;
	const int hmax = attn_head_max(S, nchunks);
#define YALM_ATTN_B(GT)                                                                                                \
	attn_decode_batch_kernel<D, GT><<<per_seq * b->n_seq, ATTN_THREADS, 0, d->stream>>>(                              \
	    b->q, q_dim, b->kv[l], b->seq, per_seq, c.n_heads, c.n_kv_heads, c.max_seq_len, attn_nsplit(c.max_seq_len), S, \
	    hmax, b->part, l, c.n_layers, d->awo_err, b->xb2)
	if (G <= 1)
		YALM_ATTN_B(1);
	else if (G <= 2)
		YALM_ATTN_B(2);
	else if (G <= 4)
		YALM_ATTN_B(4);
	else
		YALM_ATTN_B(8);
#undef YALM_ATTN_B
}

static int enqueue_batch_attn(const yalm_batch_s *b, int l) {
	const yalm_decoder_s *d = b->d;
	const yalm_config &c = d->c;
	const int q_dim = c.n_heads * c.head_dim;
	if (b->flags & YALM_BATCH_ATTN_PER_SEQ) {
		for (int s = 0; s < b->n_seq; ++s)
			TRY(launch_attn(c.head_dim, c.n_heads, c.n_kv_heads, b->q + (size_t)s * q_dim, b->kv[l].k[s], b->kv[l].v[s],
			                b->seq + s, c.max_seq_len, b->part.p[s], l, c.n_layers, d->awo_err, nullptr,
			                b->xb2 + (size_t)s * q_dim, d->stream));
		return YALM_OK;
	}
	switch (c.head_dim) {
	case 16: launch_attn_batch_D<16>(b, l); break;
	case 32: launch_attn_batch_D<32>(b, l); break;
	case 64: launch_attn_batch_D<64>(b, l); break;
	case 128: launch_attn_batch_D<128>(b, l); break;
	case 256: launch_attn_batch_D<256>(b, l); break;
	default:
		set_err("unsupported head_dim");
		return YALM_ERR_UNSUPPORTED;
	}
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

// One batch step up to the logits: begin, then per layer QKV (+ the q / k norm launch), attention
// (one launch, or one per sequence), Wo, W1|W3, W2; then norm + logits into logits [n_seq][vocab].
template <class WT>
static int enqueue_batch_forward_t(yalm_batch_s *b) {
	yalm_decoder_s *d = b->d;
	if constexpr (WT::Q4) {
		return rows_supported(d, "batched forward");
	} else {
		const yalm_config &c = d->c;
		hipStream_t st = d->stream;
		const int T = b->n_seq, q_dim = c.n_heads * c.head_dim, kv_dim = c.n_kv_heads * c.head_dim;
		batch_begin_kernel<WT><<<T, 256, 0, st>>>(b->seq, d->emb, c.dim, b->x, d->inv_freq, c.head_dim / 2);
		HIPCHK(hipGetLastError());
		for (int l = 0; l < c.n_layers; ++l) {
			const yalm_block_weights &w = d->b[l];
			switch (qkv_form(d)) {
			case QKV_NORM: { // raw rows, then one norm launch for all rows, each K row into its sequence's cache
				PQKVN<WT> base = make_pqkvn<WT>(d, l);
				base.step = b->seq;
				TRY((launch_rows<WT, BQKVN<WT>, true>({base, base.n, base.n_groups, q_dim + kv_dim, b->kv[l]}, b->x, c.dim,
				                                      w.rms_att, c.norm_eps, T, st)));
				batch_qk_norm_rope_kernel<<<dim3(c.n_heads + c.n_kv_heads, T), YALM_WAVE, 0, st>>>(
				    d->qk_raw, q_dim + kv_dim, d->gq[l], d->gk[l], c.n_heads, c.n_kv_heads, c.head_dim, c.norm_eps, b->seq,
				    b->q, q_dim, b->kv[l]);
				HIPCHK(hipGetLastError());
				break;
			}
			case QKV_BIAS: {
				PQKVB<WT> base = make_pqkvb<WT>(d, l);
				base.step = b->seq;
				base.q_out = b->q;
				TRY((launch_rows<WT, BQKVB<WT>, true>({base, base.n, base.n_groups, q_dim, b->kv[l]}, b->x, c.dim, w.rms_att,
				                                      c.norm_eps, T, st)));
				break;
			}
			default: {
				PQKV<WT> base = make_pqkv<WT>(d, l);
				base.step = b->seq;
				base.q_out = b->q;
				TRY((launch_rows<WT, BQKV<WT>, true>({base, base.n, base.n_groups, q_dim, b->kv[l]}, b->x, c.dim, w.rms_att,
				                                     c.norm_eps, T, st)));
			}
			}
			TRY(enqueue_batch_attn(b, l));
			TRY((launch_rows<WT, RResidual<WT>, false>(make_rresidual<WT>(w.wo, q_dim, c.dim, b->x, c.dim), b->xb2, q_dim,
			                                           nullptr, 0.f, T, st)));
			TRY((launch_rows_glu<WT, true>(w.w1, w.w3, c.dim, c.hidden_dim, b->hb, c.hidden_dim, c.act, b->x, c.dim, w.rms_ffn,
			                               c.norm_eps, T, st)));
			TRY((launch_rows<WT, RResidual<WT>, false>(make_rresidual<WT>(w.w2, c.hidden_dim, c.dim, b->x, c.dim), b->hb,
			                                           c.hidden_dim, nullptr, 0.f, T, st)));
		}
		return launch_rows<WT, RStore<WT>, true>(make_rstore<WT>(d->wcls, c.dim, c.vocab_size, b->logits, c.vocab_size), b->x,
		                                         c.dim, d->rms_final, c.norm_eps, T, st);
	}
}

static int enqueue_batch_forward(yalm_batch_s *b) {
	return DISPATCH_WT(b->d->c.weight_dtype, enqueue_batch_forward_t, b);
}

static int batch_launches(const yalm_batch_s *b) {
	const int L = b->d->c.n_layers, attn = (b->flags & YALM_BATCH_ATTN_PER_SEQ) ? b->n_seq : 1;
	return 3 + L * (4 + attn + (b->d->gq.empty() ? 0 : 1));
}

static int batch_set(yalm_batch_s *b, const int *tokens, const int *pos, int reset_gen) {
	int tk[ROWS_MAX_T] = {0, 0, 0, 0}, ps[ROWS_MAX_T] = {0, 0, 0, 0};
	for (int s = 0; s < b->n_seq; ++s)
		tk[s] = tokens[s], ps[s] = pos[s];
	batch_set_kernel<<<1, 1, 0, b->d->stream>>>(b->seq, b->n_seq, tk[0], tk[1], tk[2], tk[3], ps[0], ps[1], ps[2], ps[3],
	                                            reset_gen);
	HIPCHK(hipGetLastError());
	return YALM_OK;
}

extern "C" int yalm_batch_forward(yalm_batch b, const int *tokens, const int *pos, float *logits_host) {
	ARGCHK(b && tokens && pos, "yalm_batch_forward: null argument");
	yalm_decoder_s *d = b->d;
	for (int s = 0; s < b->n_seq; ++s) {
		ARGCHK(tokens[s] >= 0 && tokens[s] < d->vocab_full, "yalm_batch_forward: token out of range");
		ARGCHK(pos[s] >= 0 && pos[s] < d->c.max_seq_len,
		       "yalm_batch_forward: pos must be in [0, max_seq_len) (a batched step never wraps the ring or rotates the sinks)");
	}
	TRY(batch_set(b, tokens, pos, 0));
	TRY(enqueue_batch_forward(b));
	if (logits_host) {
		const size_t bytes = sizeof(float) * (size_t)b->n_seq * d->c.vocab_size;
		HIPCHK(hipMemcpyAsync(b->logits_pinned, b->logits, bytes, hipMemcpyDeviceToHost, d->stream));
		HIPCHK(hipStreamSynchronize(d->stream));
		TRY(awo_check(d));
		memcpy(logits_host, b->logits_pinned, bytes);
	}
	return YALM_OK;
}

// The batched loop, greedy (smp == nullptr) or sampled: n_steps steps back to back, one read-back.
static int batch_generate(yalm_batch_s *b, const char *name, const int *tokens, const int *pos, int n_steps,
                          const yalm_sampling *smp, const float *uniforms, int *out_tokens, yalm_batch_stats *stats) {
	const std::string who(name);
	ARGCHK(b && tokens && pos && (out_tokens || n_steps == 0), who + ": null argument");
	yalm_decoder_s *d = b->d;
	ARGCHK(n_steps >= 0, who + ": bad n_steps");
	ARGCHK(n_steps <= d->tokens_cap, who + ": n_steps exceeds the token buffer (65536)");
	for (int s = 0; s < b->n_seq; ++s) {
		ARGCHK(tokens[s] >= 0 && tokens[s] < d->vocab_full, who + ": token out of range");
		ARGCHK(pos[s] >= 0 && (long long)pos[s] + n_steps <= d->c.max_seq_len,
		       who + ": pos + n_steps must not exceed max_seq_len (a batched step never wraps the ring or rotates the sinks)");
	}
	if (smp) {
		TRY(validate_sampling(smp, uniforms, b->n_seq * n_steps));
		ARGCHK(d->c.vocab_size <= SMP_MAX_N, who + ": vocabulary above 131072");
	}
	if (stats)
		stats->launches_per_step = batch_launches(b);
	if (n_steps == 0)
		return YALM_OK;
	hipStream_t st = d->stream;
	const int V = d->c.vocab_size, T = b->n_seq;
	if (smp) {
		HIPCHK(hipMemcpyAsync(b->smp_params, smp, sizeof(SampleParams), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(b->smp_u, uniforms, sizeof(float) * (size_t)T * n_steps, hipMemcpyHostToDevice, st));
	}
	TRY(batch_set(b, tokens, pos, 1));
	for (int i = 0; i < n_steps; ++i) {
		TRY(enqueue_batch_forward(b));
		if (smp) {
			if (V % 4 == 0)
				batch_sample_kernel<true><<<T, SMP_THREADS, 0, st>>>(b->logits, V, b->smp_params, b->smp_u, n_steps, b->seq,
				                                                    b->tok, d->tokens_cap);
			else
				batch_sample_kernel<false><<<T, SMP_THREADS, 0, st>>>(b->logits, V, b->smp_params, b->smp_u, n_steps, b->seq,
				                                                     b->tok, d->tokens_cap);
		} else if (V % 4 == 0) {
			batch_commit_kernel<true><<<T, 1024, 0, st>>>(b->logits, V, b->seq, b->tok, d->tokens_cap);
		} else {
			batch_commit_kernel<false><<<T, 1024, 0, st>>>(b->logits, V, b->seq, b->tok, d->tokens_cap);
		}
		HIPCHK(hipGetLastError());
	}
	for (int s = 0; s < T; ++s)
		HIPCHK(hipMemcpyAsync(out_tokens + (size_t)s * n_steps, b->tok.p[s], sizeof(int) * n_steps, hipMemcpyDeviceToHost,
		                      st));
	HIPCHK(hipStreamSynchronize(st));
	return awo_check(d);
}

extern "C" int yalm_batch_generate_greedy(yalm_batch b, const int *tokens, const int *pos, int n_steps, int *out_tokens,
                                          yalm_batch_stats *stats) {
	return batch_generate(b, "yalm_batch_generate_greedy", tokens, pos, n_steps, nullptr, nullptr, out_tokens, stats);
}

extern "C" int yalm_batch_generate_sampled(yalm_batch b, const int *tokens, const int *pos, int n_steps,
                                           const yalm_sampling *s, const float *uniforms, int *out_tokens,
                                           yalm_batch_stats *stats) {
	ARGCHK(s && (uniforms || n_steps == 0), "yalm_batch_generate_sampled: null argument");
	static const float none = 0.0f;
	return batch_generate(b, "yalm_batch_generate_sampled", tokens, pos, n_steps, s, uniforms ? uniforms : &none,
	                      out_tokens, stats);
}

extern "C" int yalm_batch_state(yalm_batch b, int *tokens, int *pos) {
	ARGCHK(b, "yalm_batch_state: null batch");
	HIPCHK(hipStreamSynchronize(b->d->stream));
	TRY(awo_check(b->d));
	std::vector<StepState> s(b->n_seq);
	HIPCHK(hipMemcpy(s.data(), b->seq, sizeof(StepState) * b->n_seq, hipMemcpyDeviceToHost));
	for (int i = 0; i < b->n_seq; ++i) {
		if (tokens)
			tokens[i] = s[i].token;
		if (pos)
			pos[i] = s[i].pos;
	}
	return YALM_OK;
}

extern "C" int yalm_device_step(yalm_decoder d, int *token, int *pos) {
	ARGCHK(d, "null decoder");
	StepState s;
	HIPCHK(hipStreamSynchronize(d->stream));
	TRY(awo_check(d));
	HIPCHK(hipMemcpy(&s, d->step, sizeof(s), hipMemcpyDeviceToHost));
	if (token)
		*token = s.token;
	if (pos)
		*pos = s.pos;
	return YALM_OK;
}

extern "C" int yalm_device_tokens(yalm_decoder d, int *out, int cap, int *n_total) {
	ARGCHK(d && n_total && cap >= 0 && (out || cap == 0), "yalm_device_tokens: bad argument");
	StepState s;
	HIPCHK(hipStreamSynchronize(d->stream));
	TRY(awo_check(d));
	HIPCHK(hipMemcpy(&s, d->step, sizeof(s), hipMemcpyDeviceToHost));
	*n_total = s.n_gen;
	const int n = std::min(std::min(s.n_gen, d->tokens_cap), cap);
	if (n > 0)
		HIPCHK(hipMemcpy(out, d->tokens, sizeof(int) * n, hipMemcpyDeviceToHost));
	return YALM_OK;
}

extern "C" int yalm_block(yalm_decoder d, int layer, int pos, int kv_sink, int kv_pos, int kv_len) {
	ARGCHK(d && layer >= 0 && layer < d->c.n_layers, "bad layer");
	ARGCHK(kv_len >= 1 && kv_len <= d->c.max_seq_len && kv_pos >= 0 && kv_pos < d->c.max_seq_len,
	       "bad kv indices");
	set_step_full_kernel<<<1, 64, 0, d->stream>>>(d->step, pos, kv_sink, kv_pos, kv_len, d->ipc ? 2 : 0, d->inv_freq,
	                                              d->c.head_dim / 2);
	HIPCHK(hipGetLastError());
	TRY(DISPATCH_WT(d->c.weight_dtype, enqueue_layer_t, d, layer, 0, false, true));
	if (d->ipc) { // the layer's W2 pushed its partial: collect the sum into x (a forward's next GEMV would)
		tpx_collect_kernel<<<TPX_COLLECT_WG, 256, 0, d->stream>>>(tpx_ex(d, 1), d->c.dim, 0, d->x);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipStreamSynchronize(d->stream));
	return awo_check(d);
}

extern "C" int yalm_get_x(yalm_decoder d, float *host) {
	ARGCHK(d && host, "null argument");
	HIPCHK(hipStreamSynchronize(d->stream));
	HIPCHK(hipMemcpy(host, d->x, sizeof(float) * d->c.dim, hipMemcpyDeviceToHost));
	return YALM_OK;
}

extern "C" int yalm_set_x(yalm_decoder d, const float *host) {
	ARGCHK(d && host, "null argument");
	HIPCHK(hipStreamSynchronize(d->stream));
	HIPCHK(hipMemcpy(d->x, host, sizeof(float) * d->c.dim, hipMemcpyHostToDevice));
	return YALM_OK;
}

extern "C" int yalm_get_logits(yalm_decoder d, float *host) {
	ARGCHK(d && host, "null argument");
	HIPCHK(hipStreamSynchronize(d->stream));
	HIPCHK(hipMemcpy(host, d->logits, sizeof(float) * d->vocab_full, hipMemcpyDeviceToHost));
	return YALM_OK;
}

// One launch of kernel_id on layer l: the forward's own launch functions with a local x (the
// timing hooks never take part in an exchange, except kernels 6 and 8); written out here are only
// the launches without a counterpart in the forward, each on its scratch step state.
template <class WT>
static int enqueue_one_t(yalm_decoder_s *d, int kernel_id, int l) {
	const yalm_config &c = d->c;
	switch (kernel_id) {
	case KID_QKV:
		return enqueue_qkv<WT>(d, l, -1);
	case KID_ATTN:
		return enqueue_attn(d, l, d->q, d->step, d->xb2);
	case KID_WO:
		return enqueue_wo<WT>(d, l, EX_LOCAL);
	case KID_GLU: // (experts: on the layer's last routing)
		return enqueue_glu<WT>(d, l, -1);
	case KID_W2:
		return enqueue_w2<WT>(d, l, EX_LOCAL);
	case KID_CLS:
		return enqueue_logits_t<WT>(d, -1, -1);
	case KID_EXCHANGE:
		return enqueue_exchange(d);
	case KID_ATTN_WO: // fused attention + Wo (IPC: pushing exchange 0 of the bumped sequence, unread)
		if constexpr (wt_fused_wo<WT>())
			return launch_attn_wo<WT>(d, l, 0);
		break;
	case KID_ROUTER:
		return enqueue_router<WT>(d, l);
	case KID_QK_NORM: // the q / k norm launch on whatever the last QKV launch left in qk_raw
		return launch_qk_norm(d, l, 1, d->step, d->q);
	case KID_SAMPLE: // the sampling launch on the current logits; commits into a scratch step state
		sample_kernel<<<1, SMP_THREADS, 0, d->stream>>>(d->logits, c.vocab_size, d->smp_params, d->smp_u, 1,
		                                                d->smp_step, nullptr, 0, nullptr, nullptr);
		HIPCHK(hipGetLastError());
		return YALM_OK;
	// the launches that end a 4-row speculative step, on the rows' current logits and a scratch step state
	case KID_SPEC_SAMPLE:
		if (c.vocab_size % 4 == 0)
			spec_sample_rows_kernel<true><<<SPEC_MAX_ROWS, SMP_THREADS, 0, d->stream>>>(
			    d->rlogits, c.vocab_size, c.vocab_size, d->smp_params, d->smp_u, 1, d->smp_step, d->spec, nullptr);
		else
			spec_sample_rows_kernel<false><<<SPEC_MAX_ROWS, SMP_THREADS, 0, d->stream>>>(
			    d->rlogits, c.vocab_size, c.vocab_size, d->smp_params, d->smp_u, 1, d->smp_step, d->spec, nullptr);
		HIPCHK(hipGetLastError());
		return YALM_OK;
	case KID_SPEC_ACCEPT:
		spec_accept_kernel<<<1, 64, 0, d->stream>>>(SPEC_MAX_ROWS, d->smp_step, d->spec, d->tokens, 0);
		HIPCHK(hipGetLastError());
		return YALM_OK;
	case KID_SPEC_VERIFY:
		spec_verify_kernel<<<1, 1024, 0, d->stream>>>(d->rlogits, c.vocab_size, SPEC_MAX_ROWS, d->smp_step, d->spec,
		                                              d->tokens, 0);
		HIPCHK(hipGetLastError());
		return YALM_OK;
	}
	set_err("bad kernel_id");
	return YALM_ERR_ARG;
}

extern "C" int yalm_graph_kernels(yalm_decoder d, int mode, int *kernels, int *nodes) {
	ARGCHK(d && kernels && mode >= 0 && mode < N_GRAPHS, "yalm_graph_kernels: bad argument");
	ARGCHK(!d->eager, "yalm_graph_kernels: the decoder launches eagerly (YALM_LAUNCH_EAGER)");
	if (mode == GRAPH_SAMPLED && (d->tp_size > 1 || d->comm || d->ipc)) {
		set_err("yalm_graph_kernels: no sampled step on a tensor-parallel decoder");
		return YALM_ERR_UNSUPPORTED;
	}
	TRY(ensure_graph(d, mode));
	return graph_kernel_count(d->graph[mode], kernels, nodes);
}

extern "C" int yalm_decoder_set_launch(yalm_decoder d, int flags) {
	ARGCHK(d, "null decoder");
	ARGCHK(!(flags & ~(YALM_LAUNCH_EAGER | YALM_LAUNCH_SYNC | YALM_LAUNCH_SEPARATE_ATTN_WO)), "unknown launch flag");
	HIPCHK(hipStreamSynchronize(d->stream));
	drop_graphs(d); // captured graphs bake the old launch sequence
	d->eager = flags & YALM_LAUNCH_EAGER;
	d->graph_sync = flags & YALM_LAUNCH_SYNC;
	d->attn_wo = d->attn_wo_ok && !(flags & YALM_LAUNCH_SEPARATE_ATTN_WO);
	return YALM_OK;
}

extern "C" int yalm_decoder_attn_wo(yalm_decoder d) {
	return d && d->attn_wo ? 1 : 0;
}

extern "C" int yalm_attn_wo_trace(yalm_decoder d, unsigned long long *host, size_t count, int *workgroups,
                                  int *attention_workgroups) {
	ARGCHK(d && host, "null argument");
	ARGCHK(d->attn_wo && d->awo_trace, "no attn_wo trace (create the decoder with YALM_ATTN_WO_TRACE=1)");
	HIPCHK(hipStreamSynchronize(d->stream));
	const size_t total = (size_t)AWO_TRACE_N * d->awo_nb;
	HIPCHK(hipMemcpy(host, d->awo_trace, sizeof(unsigned long long) * std::min(count, total), hipMemcpyDeviceToHost));
	if (workgroups)
		*workgroups = d->awo_nb;
	if (attention_workgroups)
		*attention_workgroups = d->c.n_kv_heads * (d->awo_S + d->c.n_heads / d->c.n_kv_heads - 1) + d->c.n_heads;
	return YALM_OK;
}

// Average ms per iteration of `iters` back-to-back enqueues of kernel_id on the
// decoder stream (HIP events). With `bump`, every iteration first advances the step
// epoch (one 1-thread kernel), so a fused attention + Wo launch sees fresh tags and
// its Wo waves really wait for the heads (without it the granules of the
// previous launch already match and the hand-off is not measured).
static int time_loop(yalm_decoder_s *d, int kernel_id, int iters, bool bump, bool kernel, float *ms_out) {
	hipEvent_t e0, e1;
	HIPCHK(hipEventCreate(&e0));
	HIPCHK(hipEventCreate(&e1));
	int r = YALM_OK;
	HIPCHK(hipEventRecord(e0, d->stream));
	for (int i = 0; i < iters && r == YALM_OK; ++i) {
		if (bump)
			epoch_bump_kernel<<<1, 1, 0, d->stream>>>(d->step, 1);
		// rotate layers so weights come from HBM, not the 256 MiB Infinity Cache
		if (kernel)
			r = DISPATCH_WT(d->c.weight_dtype, enqueue_one_t, d, kernel_id, (i + 1) % d->c.n_layers);
	}
	HIPCHK(hipEventRecord(e1, d->stream));
	HIPCHK(hipEventSynchronize(e1));
	float ms = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, e0, e1));
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	*ms_out = ms / iters;
	return r;
}

extern "C" int yalm_time_kernel(yalm_decoder d, int kernel_id, int iters, float *avg_ms) {
	ARGCHK(d && avg_ms && iters > 0 && kernel_id >= 0 && kernel_id <= KID_LAST && kernel_id != 7,
	       "bad argument (kernel ids 0-6, 8-14)");
	ARGCHK(kernel_id != KID_QK_NORM || qkv_form(d) == QKV_NORM, "kernel 11 (q / k norm) needs yalm_decoder_set_qk_norm");
	ARGCHK(kernel_id != KID_SAMPLE || (d->tp_size == 1 && !d->comm && !d->ipc && d->c.vocab_size <= SMP_MAX_N),
	       "kernel 10 (device sampling) needs a one-GPU decoder and a vocabulary of at most 131072");
	if (kernel_id >= KID_SPEC_SAMPLE) { // the speculative step's last launches: a decoder with a multi-row form, its row buffers
		TRY(rows_supported(d, "yalm_time_kernel (kernels 12-14)"));
		ARGCHK(d->c.vocab_size <= SMP_MAX_N, "kernels 12-14 need a vocabulary of at most 131072");
		TRY(rows_init(d));
	}
	ARGCHK(kernel_id != KID_ROUTER || moe_ffn(d), "kernel 9 (expert router) needs a mixture-of-experts decoder");
	ARGCHK(kernel_id != KID_EXCHANGE || d->comm || d->ipc,
	       "kernel 6 (tensor-parallel exchange) needs a tensor-parallel decoder");
	ARGCHK(kernel_id != KID_ATTN_WO || d->attn_wo, "kernel 8 (fused attention + Wo) needs yalm_decoder_attn_wo");
	// in-launch hand-offs and the IPC exchange: fresh tags per launch (one exchange per bump)
	const bool bump = kernel_id == KID_ATTN || kernel_id == KID_ATTN_WO || (kernel_id == KID_EXCHANGE && d->ipc);
	// the warm-up gets a fresh epoch too: under IPC it pushes exchange xbase + 0, whose slot
	// parity the previous forward's argmax exchange (2 L, even) used -- without the bump a
	// peer still reading that slot could see it overwritten (tp_exchange.h reuse rule)
	if (bump)
		epoch_bump_kernel<<<1, 1, 0, d->stream>>>(d->step, 1);
	TRY(DISPATCH_WT(d->c.weight_dtype, enqueue_one_t, d, kernel_id, 0)); // warm-up
	float ms = 0.f;
	TRY(time_loop(d, kernel_id, iters, bump, true, &ms));
	if (bump) { // minus the epoch bumps alone (one launch each), so one boundary per iteration stays in
		float mb = 0.f;
		TRY(time_loop(d, kernel_id, iters, true, false, &mb));
		ms = std::max(0.f, ms - mb);
	}
	TRY(awo_check(d));
	*avg_ms = ms;
	return YALM_OK;
}

extern "C" int yalm_set_gemv_config(yalm_decoder d, int kind, int threads, int unroll, int gpw) {
	ARGCHK(d && kind >= 0 && kind < GK_N, "bad decoder/kind");
	ARGCHK(threads == 0 || threads == 256 || threads == 512 || threads == 1024, "threads must be 0, 256, 512 or 1024");
	ARGCHK(unroll == 0 || unroll == 2 || unroll == 4 || unroll == 8, "unroll must be 0, 2, 4 or 8");
	ARGCHK(gpw >= 0, "gpw must be >= 0");
	d->gemv[kind] = GemvCfg{threads, unroll, gpw};
	// captured graphs bake the old geometry: drop them
	HIPCHK(hipStreamSynchronize(d->stream));
	drop_graphs(d);
	return YALM_OK;
}

template <class WT>
static const char *wt_name() {
	return WT::NAME;
}

extern "C" const char *yalm_kernel_name(yalm_decoder d, int kernel_id) {
	if (!d)
		return "";
	const char *wt = DISPATCH_WT(d->c.weight_dtype, wt_name);
	const std::string gk = std::string("gemv_rb_kernel<") + wt;
	std::string s;
	switch (kernel_id) {
	case KID_QKV:
		s = gk + qkv_policy_name(d);
		break;
	case KID_ATTN:
		s = "attn_decode_kernel<";
		break;
	case KID_WO:
		s = gk + WO_POLICY_NAME;
		break;
	case KID_GLU:
		s = gk + glu_policy_name(d);
		break;
	case KID_W2:
		s = gk + w2_policy_name(d);
		break;
	case KID_CLS:
		s = gk + CLS_POLICY_NAME;
		break;
	case KID_EXCHANGE:
		s = d->ipc ? "tpx_collect_kernel" : d->comm ? "AllReduce" : "";
		break;
	case KID_ATTN_WO:
		s = std::string("attn_wo_kernel<") + wt + ", ";
		break;
	case KID_ROUTER:
		s = router_kernel_name(d);
		if (!s.empty())
			s += wt;
		break;
	case KID_SAMPLE:
		s = "sample_kernel";
		break;
	case KID_QK_NORM:
		s = qkv_form(d) == QKV_NORM ? "qk_norm_rope_kernel<" : "";
		break;
	case KID_SPEC_SAMPLE:
		s = "spec_sample_rows_kernel<";
		break;
	case KID_SPEC_ACCEPT:
		s = "spec_accept_kernel";
		break;
	case KID_SPEC_VERIFY:
		s = "spec_verify_kernel";
		break;
	default:
		s = "";
	}
	d->kname = s;
	return d->kname.c_str();
}

namespace {
struct DevBuf { // a device allocation freed on scope exit
	void *p = nullptr;
	~DevBuf() {
		if (p)
			(void)hipFree(p);
	}
};
} // namespace

// ------------------------------------------------------------------ streaming envelope
// Pure read-only HBM stream (tools/stream_bench.hip): each wave sums `per_wave`
// contiguous 16-byte pieces with U nt loads in flight per lane; the result is
// consumed only to keep the loads alive.
template <int U>
__global__ __launch_bounds__(512) void stream_read_kernel(const u32x4_t *__restrict__ p, size_t n16, size_t per_wave,
                                                          unsigned *out) {
	const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) / 64;
	const int lane = threadIdx.x & 63;
	const size_t base = wave * per_wave;
	const size_t end = base + per_wave < n16 ? base + per_wave : n16;
	unsigned acc = 0;
	for (size_t i = base + lane; i < end; i += 64 * U) {
		u32x4_t v[U];
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const size_t j = i + (size_t)u * 64;
			v[u] = j < end ? load_nt16(p + j) : u32x4_t{0u, 0u, 0u, 0u};
		}
#pragma unroll
		for (int u = 0; u < U; ++u)
			acc ^= v[u][0] ^ v[u][1] ^ v[u][2] ^ v[u][3];
	}
	if (acc == 0x12345678u)
		out[0] = acc;
}

extern "C" int yalm_stream_envelope(size_t bytes, int iters, float *avg_ms) {
	ARGCHK(avg_ms && iters > 0 && bytes >= (1u << 20), "yalm_stream_envelope: bad argument");
	bytes &= ~(size_t)4095;
	DevBuf buf[2];
	unsigned *out = nullptr;
	for (auto &b : buf) {
		HIPCHK(hipMalloc(&b.p, bytes));
		HIPCHK(hipMemset(b.p, 1, bytes));
	}
	HIPCHK(hipMalloc((void **)&out, 64));
	hipEvent_t e0, e1;
	HIPCHK(hipEventCreate(&e0));
	HIPCHK(hipEventCreate(&e1));
	float best = 1e30f;
	const size_t n16 = bytes / 16;
	int r = YALM_OK;
	for (size_t pw_bytes : {16384ul, 32768ul, 65536ul}) {
		for (int U : {4, 8}) {
			const size_t per_wave = pw_bytes / 16;
			const size_t waves = (n16 + per_wave - 1) / per_wave;
			const int blocks = (int)((waves + 7) / 8);
			for (int pass = 0; pass < 2 && r == YALM_OK; ++pass) { // pass 0 warms up
				if (hipEventRecord(e0, nullptr) != hipSuccess)
					r = YALM_ERR_HIP;
				for (int it = 0; it < iters && r == YALM_OK; ++it) { // alternate buffers: 2x bytes > 256 MiB MALL
					const u32x4_t *src = (const u32x4_t *)buf[it & 1].p;
					if (U == 4)
						stream_read_kernel<4><<<blocks, 512>>>(src, n16, per_wave, out);
					else
						stream_read_kernel<8><<<blocks, 512>>>(src, n16, per_wave, out);
				}
				float ms = 0.f;
				if (r == YALM_OK && (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
				                     hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
					r = YALM_ERR_HIP;
				if (pass == 1 && r == YALM_OK)
					best = std::min(best, ms / iters);
			}
		}
	}
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	(void)hipFree(out);
	if (r != YALM_OK) {
		set_err("yalm_stream_envelope: HIP call failed");
		return r;
	}
	*avg_ms = best;
	return YALM_OK;
}

// ------------------------------------------------------------------ test API (host pointers)
namespace {
int up(DevBuf &b, const void *host, size_t bytes) {
	HIPCHK(hipMalloc(&b.p, bytes ? bytes : 4));
	if (host)
		HIPCHK(hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice));
	else
		HIPCHK(hipMemset(b.p, 0, bytes ? bytes : 4));
	return YALM_OK;
}
} // namespace

template <class WT>
static int matmul_t(float *out, const float *x, const void *w, int n, int d) {
	return launch_gemv<WT, PStore<WT, 1>, false>(make_store<WT, 1>(w, n, out, d), x, nullptr, 0.f, GK_GLU, GemvCfg{},
	                                             nullptr);
}

extern "C" int yalm_matmul(float *xout, const float *x, const void *w, int n, int d, int dtype) {
	ARGCHK(xout && x && w && n > 0 && d > 0, "bad argument");
	ARGCHK(dtype_ok(dtype), "bad dtype");
	ARGCHK(n % 16 == 0, "n must be a multiple of 16 (infer.cpp:66)");
	ARGCHK(dtype != YALM_Q4 || n % 32 == 0, "q4: n must be a multiple of 32");
	DevBuf dx, dw, dout;
	TRY(up(dx, x, sizeof(float) * n));
	TRY(up(dw, w, yalm_row_bytes(dtype, n) * (size_t)d));
	TRY(up(dout, nullptr, sizeof(float) * d));
	TRY(DISPATCH_WT(dtype, matmul_t, (float *)dout.p, (const float *)dx.p, dw.p, n, d));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(xout, dout.p, sizeof(float) * d, hipMemcpyDeviceToHost));
	return YALM_OK;
}

// One launch_rows call (the decoder's own) over device buffers; NORM on with a norm weight.
template <class WT, class P>
static int matmul_rows_launch(const P &p, const float *x, int xstride, const float *normw, float eps, int T) {
	return normw ? launch_rows<WT, P, true>(p, x, xstride, normw, eps, T, nullptr)
	             : launch_rows<WT, P, false>(p, x, xstride, nullptr, 0.f, T, nullptr);
}
template <class WT>
static int matmul_rows_t(float *out, const float *x, const void *w, const void *w3, const float *normw, float eps,
                         int T, int n, int d, int xstride, int ostride, int epilogue, int act) {
	if (epilogue == YALM_ROWS_GLU)
		return normw ? launch_rows_glu<WT, true>(w, w3, n, d, out, ostride, act, x, xstride, normw, eps, T, nullptr)
		             : launch_rows_glu<WT, false>(w, w3, n, d, out, ostride, act, x, xstride, nullptr, 0.f, T, nullptr);
	if (epilogue == YALM_ROWS_RESIDUAL)
		return matmul_rows_launch<WT>(make_rresidual<WT>(w, n, d, out, ostride), x, xstride, normw, eps, T);
	return matmul_rows_launch<WT>(make_rstore<WT>(w, n, d, out, ostride), x, xstride, normw, eps, T);
}

extern "C" int yalm_matmul_rows(float *out, const float *x, const void *w, const void *w3, const float *normw,
                                float eps, int T, int n, int d, int xstride, int ostride, int dtype, int epilogue,
                                int act) {
	if (dtype == YALM_Q4) {
		set_err(std::string("yalm_matmul_rows") + ROWS_Q4_WHY);
		return YALM_ERR_UNSUPPORTED;
	}
	ARGCHK(out && x && w && n > 0 && d > 0, "yalm_matmul_rows: bad argument");
	ARGCHK(dtype_ok(dtype), "yalm_matmul_rows: bad dtype");
	ARGCHK(T >= 1 && T <= ROWS_MAX_T, "yalm_matmul_rows: 1 <= T <= 4 rows");
	ARGCHK(n % 16 == 0, "yalm_matmul_rows: n must be a multiple of 16 (infer.cpp:66)");
	ARGCHK(xstride >= n && xstride % 4 == 0, "yalm_matmul_rows: xstride must be at least n and a multiple of 4");
	ARGCHK(ostride >= d && ostride % 4 == 0, "yalm_matmul_rows: ostride must be at least d and a multiple of 4");
	ARGCHK(epilogue == YALM_ROWS_STORE || epilogue == YALM_ROWS_RESIDUAL || epilogue == YALM_ROWS_GLU,
	       "yalm_matmul_rows: bad epilogue");
	ARGCHK(epilogue != YALM_ROWS_GLU || (w3 && (act == YALM_SILU || act == YALM_GELU)),
	       "yalm_matmul_rows: the GLU epilogue needs w3 and act GELU or SILU");
	const size_t wb = yalm_row_bytes(dtype, n) * (size_t)d;
	DevBuf dx, dw, dw3, dn, dout;
	TRY(up(dx, x, sizeof(float) * (size_t)T * xstride));
	TRY(up(dw, w, wb));
	if (epilogue == YALM_ROWS_GLU)
		TRY(up(dw3, w3, wb));
	if (normw)
		TRY(up(dn, normw, sizeof(float) * n));
	TRY(up(dout, out, sizeof(float) * (size_t)T * ostride));
	TRY(DISPATCH_WT_ROWS(dtype, matmul_rows_t, (float *)dout.p, (const float *)dx.p, dw.p, dw3.p, (const float *)dn.p, eps,
	                   T, n, d, xstride, ostride, epilogue, act));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(out, dout.p, sizeof(float) * (size_t)T * ostride, hipMemcpyDeviceToHost));
	return YALM_OK;
}

// ---- the single-row GEMV by itself: its plan, and one launch_gemv call on host arrays
static bool gemv_policy_qkv(int policy) {
	return policy == YALM_GEMV_QKV || policy == YALM_GEMV_QKVB || policy == YALM_GEMV_QKVN;
}
template <class WT>
static GemvPlan gemv_plan_dt(int policy, bool norm, int n, int n_groups, int kind, const GemvCfg &want) {
	switch (policy) {
	case YALM_GEMV_STORE2:
		return gemv_plan_of<WT, PStore<WT, 2>>(norm, n, n_groups, kind, want, false);
	case YALM_GEMV_RESIDUAL:
		return gemv_plan_of<WT, PResidual<WT, 1>>(norm, n, n_groups, kind, want, false);
	case YALM_GEMV_ADDTO:
		return gemv_plan_of<WT, PAddTo<WT, 1>>(norm, n, n_groups, kind, want, false);
	case YALM_GEMV_GLU:
		return gemv_plan_of<WT, PGlu<WT, 1>>(norm, n, n_groups, kind, want, false);
	case YALM_GEMV_QKV:
		return gemv_plan_of<WT, PQKV<WT>>(norm, n, n_groups, kind, want, false);
	case YALM_GEMV_QKVB:
		return gemv_plan_of<WT, PQKVB<WT>>(norm, n, n_groups, kind, want, false);
	case YALM_GEMV_QKVN:
		return gemv_plan_of<WT, PQKVN<WT>>(norm, n, n_groups, kind, want, false);
	default:
		return gemv_plan_of<WT, PStore<WT, 1>>(norm, n, n_groups, kind, want, false);
	}
}

static int gemv_cfg_check(const char *who, int dtype, int policy, int kind, int n, int threads, int unroll, int wpc,
                          int cus, int rows) {
	const std::string w(who);
	ARGCHK(dtype_ok(dtype), w + ": bad dtype");
	ARGCHK(policy >= YALM_GEMV_STORE1 && policy <= YALM_GEMV_QKVN, w + ": bad policy");
	ARGCHK(kind >= 0 && kind < GK_N, w + ": bad kind");
	ARGCHK(n > 0 && n % 16 == 0, w + ": n must be a multiple of 16 (infer.cpp:66)");
	ARGCHK(dtype != YALM_Q4 || n % 32 == 0, w + ": q4: n must be a multiple of 32");
	ARGCHK((threads == 0 || threads == 256 || threads == 512 || threads == 1024) &&
	           (unroll == 0 || unroll == 2 || unroll == 4 || unroll == 8) && wpc >= 0 && cus >= 0 &&
	           (rows == -1 || rows == 0),
	       w + ": threads 0 / 256 / 512 / 1024, unroll 0 / 2 / 4 / 8, wpc >= 0, cus >= 0, rows -1 / 0");
	return YALM_OK;
}

extern "C" int yalm_gemv_plan(int dtype, int policy, int kind, int n, int n_groups, int norm, int threads, int unroll,
                              int wpc, int cus, int rows, yalm_gemv_geometry *out) {
	TRY(gemv_cfg_check("yalm_gemv_plan", dtype, policy, kind, n, threads, unroll, wpc, cus, rows));
	ARGCHK(out && n_groups > 0, "yalm_gemv_plan: bad argument");
	GemvCfg want{threads, unroll, wpc};
	want.cus = cus;
	want.rows = rows;
	const GemvPlan g = DISPATCH_WT(dtype, gemv_plan_dt, policy, norm != 0, n, n_groups, kind, want);
	out->generic = g.generic;
	out->threads = g.threads;
	out->unroll = g.U;
	out->nb = g.nb;
	out->rows = g.rows;
	out->ngl_min = g.ngl_min;
	out->ngl_max = g.ngl_max;
	out->xregs = g.xregs;
	out->lds = g.lds;
	return YALM_OK;
}

namespace {
struct GemvOneDev { // the device side of one yalm_gemv_one call
	const float *x, *normw, *base, *bq, *bk, *bv;
	const void *w, *w3, *wq, *wk, *wv;
	float *out, *q_out, *raw;
	uint16_t *kc, *vc;
	const StepState *step;
};
} // namespace

template <class WT, class P>
static int gemv_one_launch(const yalm_gemv_args &a, const P &p, const GemvOneDev &v, const GemvCfg &cfg) {
	if (a.norm)
		return launch_gemv<WT, P, true>(p, v.x, v.normw, a.eps, a.kind, cfg, nullptr);
	return launch_gemv<WT, P, false>(p, v.x, nullptr, 0.f, a.kind, cfg, nullptr);
}
template <class WT>
static int gemv_one_t(const yalm_gemv_args &a, const GemvOneDev &v, const GemvCfg &cfg) {
	switch (a.policy) {
	case YALM_GEMV_STORE1:
		return gemv_one_launch<WT>(a, make_store<WT, 1>(v.w, a.n, v.out, a.d), v, cfg);
	case YALM_GEMV_STORE2:
		return gemv_one_launch<WT>(a, make_store<WT, 2>(v.w, a.n, v.out, a.d), v, cfg);
	case YALM_GEMV_RESIDUAL:
		return gemv_one_launch<WT>(a, make_residual<WT>(v.w, a.n, v.out, a.d), v, cfg);
	case YALM_GEMV_ADDTO:
		return launch_gemv<WT, PAddTo<WT, 1>, false>(make_addto<WT>(v.w, a.n, v.out, v.base, a.d), v.x, nullptr, 0.f,
		                                             a.kind, cfg, nullptr);
	case YALM_GEMV_GLU:
		return a.norm ? launch_glu<WT, true>(v.w, v.w3, a.n, v.out, a.d, a.act, v.x, v.normw, a.eps, a.kind, cfg, nullptr)
		              : launch_glu<WT, false>(v.w, v.w3, a.n, v.out, a.d, a.act, v.x, nullptr, 0.f, a.kind, cfg, nullptr);
	}
	// the QKV policies (inv_freq null: the epilogue reads the step's tables)
	const PQKV<WT> p = make_pqkv<WT>(v.wq, v.wk, v.wv, a.n, a.n_heads, a.n_kv_heads, a.head_dim, a.qkv_clip, nullptr,
	                                 v.step, v.q_out, v.kc, v.vc);
	if (a.policy == YALM_GEMV_QKV)
		return gemv_one_launch<WT>(a, p, v, cfg);
	if (a.policy == YALM_GEMV_QKVB)
		return gemv_one_launch<WT>(a, PQKVB<WT>{p, v.bq, v.bk, v.bv}, v, cfg);
	return gemv_one_launch<WT>(a, PQKVN<WT>{p, v.raw}, v, cfg);
}

extern "C" int yalm_gemv_one(const yalm_gemv_args *ap) {
	ARGCHK(ap, "yalm_gemv_one: bad argument");
	const yalm_gemv_args &a = *ap;
	TRY(gemv_cfg_check("yalm_gemv_one", a.dtype, a.policy, a.kind, a.n, a.threads, a.unroll, a.wpc, a.cus, a.rows));
	const bool qkv = gemv_policy_qkv(a.policy);
	ARGCHK(a.x && (!a.norm || a.normw), "yalm_gemv_one: bad argument");
	ARGCHK(!a.norm || a.policy != YALM_GEMV_ADDTO, "yalm_gemv_one: PAddTo has no normalising form");
	int n_groups = 0, q_dim = 0, kv_dim = 0;
	if (qkv) {
		ARGCHK(a.head_dim > 0 && a.head_dim % 2 == 0 && a.head_dim <= 256,
		       "yalm_gemv_one: head_dim must be even and at most 256");
		ARGCHK(a.n_heads > 0 && a.n_kv_heads > 0, "yalm_gemv_one: bad argument");
		q_dim = a.n_heads * a.head_dim;
		kv_dim = a.n_kv_heads * a.head_dim;
		ARGCHK(q_dim % 2 == 0 && kv_dim % 2 == 0, "yalm_gemv_one: q and kv dims must be even");
		ARGCHK(a.cache_rows >= 2 && a.kv_pos >= 0 && a.kv_pos < a.cache_rows,
		       "yalm_gemv_one: cache_rows must be at least 2 and above kv_pos");
		ARGCHK(a.kv_sink >= 0 && a.kv_sink <= a.kv_pos, "yalm_gemv_one: 0 <= kv_sink <= kv_pos");
		ARGCHK(a.wq && a.wk && a.wv && a.rope && a.rope_sink && a.kcache && a.vcache && a.q_out && a.q_len >= q_dim,
		       "yalm_gemv_one: bad argument");
		ARGCHK(a.policy != YALM_GEMV_QKVB || (a.bq && a.bk && a.bv), "yalm_gemv_one: PQKVB needs bq, bk and bv");
		ARGCHK(a.policy != YALM_GEMV_QKVN || (a.raw && a.raw_len >= q_dim + kv_dim),
		       "yalm_gemv_one: PQKVN needs raw of q_dim + kv_dim floats");
		n_groups = (q_dim + 2 * kv_dim) / 2;
	} else {
		ARGCHK(a.w && a.out && a.d > 0 && a.out_len >= a.d, "yalm_gemv_one: bad argument");
		ARGCHK(a.policy != YALM_GEMV_STORE2 || a.d % 2 == 0, "yalm_gemv_one: PStore<., 2> needs an even row count");
		ARGCHK(a.policy != YALM_GEMV_ADDTO || a.base, "yalm_gemv_one: PAddTo needs base");
		ARGCHK(a.policy != YALM_GEMV_GLU || (a.w3 && (a.act == YALM_SILU || a.act == YALM_GELU)),
		       "yalm_gemv_one: the GLU epilogue needs w3 and act GELU or SILU");
		n_groups = a.policy == YALM_GEMV_STORE2 ? a.d / 2 : a.d;
	}
	GemvCfg cfg{a.threads, a.unroll, a.wpc};
	cfg.cus = a.cus;
	cfg.rows = a.rows;
	const GemvPlan g = DISPATCH_WT(a.dtype, gemv_plan_dt, a.policy, a.norm != 0, a.n, n_groups, a.kind, cfg);
	ARGCHK(g.lds <= MOE_LDS_BYTES, "yalm_gemv_one: x and the partial slots do not fit the LDS");
	const size_t rb = yalm_row_bytes(a.dtype, a.n);
	DevBuf dx, dn, dw, dw3, dq, dk, dv, dout, dbase, dqo, draw, dkc, dvc, dbq, dbk, dbv, dstep;
	GemvOneDev v{};
	TRY(up(dx, a.x, sizeof(float) * a.n));
	v.x = (const float *)dx.p;
	if (a.norm) {
		TRY(up(dn, a.normw, sizeof(float) * a.n));
		v.normw = (const float *)dn.p;
	}
	const size_t cache_bytes = sizeof(uint16_t) * (size_t)a.cache_rows * kv_dim;
	if (qkv) {
		TRY(up(dq, a.wq, rb * q_dim));
		TRY(up(dk, a.wk, rb * kv_dim));
		TRY(up(dv, a.wv, rb * kv_dim));
		TRY(up(dqo, a.q_out, sizeof(float) * a.q_len));
		TRY(up(dkc, a.kcache, cache_bytes));
		TRY(up(dvc, a.vcache, cache_bytes));
		StepState h{};
		h.pos = (a.kv_pos + 1) % a.cache_rows; // another cache row: a row stored at pos, not kv_pos, shows
		h.kv_sink = a.kv_sink;
		h.kv_pos = a.kv_pos;
		h.kv_len = a.kv_pos + 1;
		memcpy(h.rope, a.rope, sizeof(float) * a.head_dim);
		memcpy(h.rope_sink, a.rope_sink, sizeof(float) * a.head_dim);
		TRY(up(dstep, &h, sizeof(h)));
		v.wq = dq.p;
		v.wk = dk.p;
		v.wv = dv.p;
		v.q_out = (float *)dqo.p;
		v.kc = (uint16_t *)dkc.p;
		v.vc = (uint16_t *)dvc.p;
		v.step = (const StepState *)dstep.p;
		if (a.policy == YALM_GEMV_QKVB) {
			TRY(up(dbq, a.bq, sizeof(float) * q_dim));
			TRY(up(dbk, a.bk, sizeof(float) * kv_dim));
			TRY(up(dbv, a.bv, sizeof(float) * kv_dim));
			v.bq = (const float *)dbq.p;
			v.bk = (const float *)dbk.p;
			v.bv = (const float *)dbv.p;
		}
		if (a.policy == YALM_GEMV_QKVN) {
			TRY(up(draw, a.raw, sizeof(float) * a.raw_len));
			v.raw = (float *)draw.p;
		}
	} else {
		TRY(up(dw, a.w, rb * a.d));
		v.w = dw.p;
		if (a.policy == YALM_GEMV_GLU) {
			TRY(up(dw3, a.w3, rb * a.d));
			v.w3 = dw3.p;
		}
		TRY(up(dout, a.out, sizeof(float) * a.out_len));
		v.out = (float *)dout.p;
		if (a.policy == YALM_GEMV_ADDTO) {
			TRY(up(dbase, a.base, sizeof(float) * a.d));
			v.base = (const float *)dbase.p;
		}
	}
	TRY(DISPATCH_WT(a.dtype, gemv_one_t, a, v, cfg));
	HIPCHK(hipDeviceSynchronize());
	if (qkv) {
		HIPCHK(hipMemcpy(a.q_out, dqo.p, sizeof(float) * a.q_len, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(a.kcache, dkc.p, cache_bytes, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(a.vcache, dvc.p, cache_bytes, hipMemcpyDeviceToHost));
		if (a.policy == YALM_GEMV_QKVN)
			HIPCHK(hipMemcpy(a.raw, draw.p, sizeof(float) * a.raw_len, hipMemcpyDeviceToHost));
	} else {
		HIPCHK(hipMemcpy(a.out, dout.p, sizeof(float) * a.out_len, hipMemcpyDeviceToHost));
	}
	return YALM_OK;
}

extern "C" int yalm_mha(float *xout, float *att, const uint16_t *kb, const uint16_t *vb, const float *q, int head_dim,
                        int kv_len, int max_seq_len, int n_heads, int n_kv_heads) {
	ARGCHK(xout && kb && vb && q, "null argument");
	ARGCHK(n_kv_heads > 0 && n_heads % n_kv_heads == 0 && kv_len >= 1 && kv_len <= max_seq_len, "bad shape");
	if (!attn_supported(head_dim, n_heads / n_kv_heads)) {
		set_err("unsupported head_dim / group size");
		return YALM_ERR_UNSUPPORTED;
	}
	const size_t kvn = (size_t)max_seq_len * n_kv_heads * head_dim;
	const int nsplit = attn_nsplit(max_seq_len);
	DevBuf dk, dv, dq, dout, datt, dpart, dstep, derr;
	TRY(up(dk, kb, kvn * 2));
	TRY(up(dv, vb, kvn * 2));
	TRY(up(dq, q, sizeof(float) * n_heads * head_dim));
	TRY(up(dout, nullptr, sizeof(float) * n_heads * head_dim));
	TRY(up(datt, att, sizeof(float) * (size_t)n_heads * max_seq_len));
	TRY(up(dpart, nullptr, sizeof(unsigned long long) * (size_t)n_heads * nsplit * (head_dim + 2)));
	TRY(up(dstep, nullptr, sizeof(StepState)));
	TRY(up(derr, nullptr, sizeof(unsigned)));
	set_step_full_kernel<<<1, 1>>>((StepState *)dstep.p, kv_len - 1, 0, kv_len - 1, kv_len);
	TRY(launch_attn(head_dim, n_heads, n_kv_heads, (const float *)dq.p, (const uint16_t *)dk.p,
	                (const uint16_t *)dv.p, (const StepState *)dstep.p, max_seq_len, (unsigned long long *)dpart.p, 0, 1,
	                (unsigned *)derr.p, att ? (float *)datt.p : nullptr, (float *)dout.p, nullptr));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(xout, dout.p, sizeof(float) * n_heads * head_dim, hipMemcpyDeviceToHost));
	if (att)
		HIPCHK(hipMemcpy(att, datt.p, sizeof(float) * (size_t)n_heads * max_seq_len, hipMemcpyDeviceToHost));
	unsigned e = 0;
	HIPCHK(hipMemcpy(&e, derr.p, sizeof(e), hipMemcpyDeviceToHost));
	if (e) {
		set_err("yalm_mha: the split-KV merger gave up waiting for a chunk");
		return YALM_ERR_HIP;
	}
	return YALM_OK;
}

extern "C" int yalm_argmax(const float *logits, int n, int n_shards, int *out) {
	ARGCHK(logits && out && n > 0 && n_shards >= 1 && n_shards <= 64 && n % n_shards == 0, "yalm_argmax: bad argument");
	DevBuf dl, dst, dpairs;
	TRY(up(dl, logits, sizeof(float) * (size_t)n));
	TRY(up(dst, nullptr, sizeof(StepState)));
	TRY(up(dpairs, nullptr, sizeof(float) * 2 * n_shards));
	StepState *st = (StepState *)dst.p;
	if (n_shards == 1) {
		argmax_kernel<<<1, 1024>>>((const float *)dl.p, n, st, nullptr, 0);
	} else { // the tensor-parallel path: per-shard first max as (value, global index), then the pick
		const int ns = n / n_shards;
		for (int r = 0; r < n_shards; ++r)
			argmax_kernel<<<1, 1024>>>((const float *)dl.p + (size_t)r * ns, ns, st, nullptr, 0,
			                           (float *)dpairs.p + 2 * r, r * ns);
		argmax_pick_kernel<<<1, 1>>>((const float *)dpairs.p, n_shards, st, nullptr, 0);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipDeviceSynchronize());
	StepState h;
	HIPCHK(hipMemcpy(&h, st, sizeof(h), hipMemcpyDeviceToHost));
	*out = h.token;
	return YALM_OK;
}

extern "C" int yalm_sample(const float *logits, int n, const yalm_sampling *s, const float *uniforms, int n_draws,
                           int *out_tokens, int *kept, uint64_t *weights_out) {
	ARGCHK(logits && out_tokens && n > 0 && n_draws > 0 && n_draws <= (1 << 16), "yalm_sample: bad argument");
	ARGCHK(n <= SMP_MAX_N, "yalm_sample: n above 131072");
	TRY(validate_sampling(s, uniforms, n_draws));
	DevBuf dl, dst, dprm, du, dtok, dkept, dw;
	TRY(up(dl, logits, sizeof(float) * (size_t)n));
	TRY(up(dst, nullptr, sizeof(StepState)));
	TRY(up(dprm, s, sizeof(SampleParams)));
	TRY(up(du, uniforms, sizeof(float) * n_draws));
	TRY(up(dtok, nullptr, sizeof(int) * n_draws));
	TRY(up(dkept, nullptr, sizeof(int) * n_draws));
	if (weights_out)
		TRY(up(dw, nullptr, sizeof(uint64_t) * (size_t)n));
	for (int i = 0; i < n_draws; ++i) // draw i reads uniforms[n_gen = i]; the weights are the same every time
		sample_kernel<<<1, SMP_THREADS>>>((const float *)dl.p, n, (const SampleParams *)dprm.p, (const float *)du.p,
		                                  n_draws, (StepState *)dst.p, (int *)dtok.p, n_draws, (int *)dkept.p,
		                                  i == 0 ? (unsigned long long *)dw.p : nullptr);
	HIPCHK(hipGetLastError());
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(out_tokens, dtok.p, sizeof(int) * n_draws, hipMemcpyDeviceToHost));
	if (kept)
		HIPCHK(hipMemcpy(kept, dkept.p, sizeof(int) * n_draws, hipMemcpyDeviceToHost));
	if (weights_out)
		HIPCHK(hipMemcpy(weights_out, dw.p, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
	return YALM_OK;
}

// Host-pointer hook: the sampled step's two launches as the loop makes them, n_gen = 0, stride n.
extern "C" int yalm_spec_sample_rows(const float *logits, int n, int T, const yalm_sampling *s, const float *uniforms,
                                     const int *drafts, int *drawn_out, int *kept_out, int *accepted_out) {
	ARGCHK(logits && drawn_out && accepted_out && n > 0, "yalm_spec_sample_rows: bad argument");
	ARGCHK(T >= 1 && T <= SPEC_MAX_ROWS, "yalm_spec_sample_rows: 1 <= T <= 4 rows");
	ARGCHK(T == 1 || drafts, "yalm_spec_sample_rows: null drafts");
	ARGCHK(n <= SMP_MAX_N, "yalm_spec_sample_rows: n above 131072");
	TRY(validate_sampling(s, uniforms, T));
	SpecState sp{};
	for (int k = 1; k < T; ++k)
		sp.draft[k] = drafts[k - 1];
	DevBuf dl, dst, dsp, dprm, du, dtok, dkept;
	TRY(up(dl, logits, sizeof(float) * (size_t)T * n));
	TRY(up(dst, nullptr, sizeof(StepState)));
	TRY(up(dsp, &sp, sizeof(sp)));
	TRY(up(dprm, s, sizeof(SampleParams)));
	TRY(up(du, uniforms, sizeof(float) * T));
	TRY(up(dtok, nullptr, sizeof(int) * SPEC_MAX_ROWS));
	TRY(up(dkept, nullptr, sizeof(int) * SPEC_MAX_ROWS));
	if (n % 4 == 0)
		spec_sample_rows_kernel<true><<<T, SMP_THREADS>>>((const float *)dl.p, n, n, (const SampleParams *)dprm.p,
		                                                 (const float *)du.p, T, (const StepState *)dst.p,
		                                                 (SpecState *)dsp.p, (int *)dkept.p);
	else
		spec_sample_rows_kernel<false><<<T, SMP_THREADS>>>((const float *)dl.p, n, n, (const SampleParams *)dprm.p,
		                                                  (const float *)du.p, T, (const StepState *)dst.p,
		                                                  (SpecState *)dsp.p, (int *)dkept.p);
	HIPCHK(hipGetLastError());
	spec_accept_kernel<<<1, 64>>>(T, (StepState *)dst.p, (SpecState *)dsp.p, (int *)dtok.p, SPEC_MAX_ROWS);
	HIPCHK(hipGetLastError());
	HIPCHK(hipDeviceSynchronize());
	StepState h;
	HIPCHK(hipMemcpy(&h, dst.p, sizeof(h), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(&sp, dsp.p, sizeof(sp), hipMemcpyDeviceToHost));
	for (int t = 0; t < T; ++t)
		drawn_out[t] = sp.drawn[t];
	if (kept_out)
		HIPCHK(hipMemcpy(kept_out, dkept.p, sizeof(int) * T, hipMemcpyDeviceToHost));
	*accepted_out = h.n_gen;
	return YALM_OK;
}

template <class WT>
static int ffn_t(float *out, const float *x, const void *w1, const void *w2, const void *w3, float *hb, int hidden,
                 int dim, int act) {
	TRY((launch_glu<WT, false>(w1, w3, dim, hb, hidden, act, x, nullptr, 0.f, GK_GLU, GemvCfg{}, nullptr)));
	return launch_gemv<WT, PStore<WT, 1>, false>(make_store<WT, 1>(w2, hidden, out, dim), hb, nullptr, 0.f, GK_GLU,
	                                             GemvCfg{}, nullptr);
}

extern "C" int yalm_ffn(float *xout, const float *x, const void *w1, const void *w2, const void *w3, int hidden_dim,
                        int dim, int act, int dtype) {
	ARGCHK(xout && x && w1 && w2 && w3 && hidden_dim > 0 && dim > 0, "bad argument");
	ARGCHK(dtype_ok(dtype), "bad dtype");
	ARGCHK(dim % 16 == 0 && hidden_dim % 16 == 0, "dims must be multiples of 16");
	ARGCHK(dtype != YALM_Q4 || (dim % 32 == 0 && hidden_dim % 32 == 0), "q4: dims must be multiples of 32");
	const size_t wb = yalm_row_bytes(dtype, dim) * (size_t)hidden_dim;   // w1, w3: hidden_dim rows of dim
	const size_t wb2 = yalm_row_bytes(dtype, hidden_dim) * (size_t)dim;  // w2: dim rows of hidden_dim
	DevBuf dx, d1, d2, d3, dhb, dout;
	TRY(up(dx, x, sizeof(float) * dim));
	TRY(up(d1, w1, wb));
	TRY(up(d2, w2, wb2));
	TRY(up(d3, w3, wb));
	TRY(up(dhb, nullptr, sizeof(float) * hidden_dim));
	TRY(up(dout, nullptr, sizeof(float) * dim));
	TRY(DISPATCH_WT(dtype, ffn_t, (float *)dout.p, (const float *)dx.p, d1.p, d2.p, d3.p, (float *)dhb.p, hidden_dim,
	                dim, act));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(xout, dout.p, sizeof(float) * dim, hipMemcpyDeviceToHost));
	return YALM_OK;
}

template <class WT>
static int moe_ffn_t(const MoeArgs &a, float *out, const float *x) {
	TRY((launch_moe_router<WT, false>(a, x, nullptr, 0.f, nullptr)));
	TRY((launch_moe_glu<WT, false>(a, x, nullptr, 0.f, GemvCfg{}, nullptr)));
	return launch_moe_w2<WT>(a, out, GemvCfg{}, nullptr); // out starts at 0: the sum without a residual
}

extern "C" int yalm_moe_ffn(float *xout, int *experts, float *weights, const float *x, const void *moegate,
                            const void *w1, const void *w2, const void *w3, int n_experts, int n_active, int hidden_dim,
                            int dim, int act, int dtype) {
	ARGCHK(xout && x && moegate && w1 && w2 && w3 && hidden_dim > 0 && dim > 0, "bad argument");
	if (dtype == YALM_Q4) {
		set_err("yalm_moe_ffn: q4 weights have no mixture-of-experts form");
		return YALM_ERR_UNSUPPORTED;
	}
	if (dtype == YALM_E4M3) {
		set_err("yalm_moe_ffn: e4m3 weights have no mixture-of-experts form");
		return YALM_ERR_UNSUPPORTED;
	}
	ARGCHK(dtype_ok(dtype), "bad dtype");
	ARGCHK(dim % 16 == 0 && hidden_dim % 16 == 0, "dims must be multiples of 16");
	ARGCHK(act == YALM_SILU || act == YALM_GELU, "bad activation");
	TRY(validate_moe(n_experts, n_active));
	const size_t wb = yalm_row_bytes(dtype, dim) * (size_t)n_experts * hidden_dim; // (E, hidden, dim); w2 (E, dim, hidden): as many
	DevBuf dx, dg, d1, d2, d3, dhb, dout, dsel, dwts;
	TRY(up(dx, x, sizeof(float) * dim));
	TRY(up(dg, moegate, yalm_row_bytes(dtype, dim) * (size_t)n_experts));
	TRY(up(d1, w1, wb));
	TRY(up(d2, w2, wb));
	TRY(up(d3, w3, wb));
	TRY(up(dhb, nullptr, sizeof(float) * (size_t)n_active * hidden_dim));
	TRY(up(dout, nullptr, sizeof(float) * dim));
	TRY(up(dsel, nullptr, sizeof(int) * n_active));
	TRY(up(dwts, nullptr, sizeof(float) * n_active));
	const MoeArgs a{dg.p, d1.p, d2.p, d3.p, n_experts, n_active, hidden_dim, dim, act, (int *)dsel.p, (float *)dwts.p,
	                (float *)dhb.p};
	TRY(DISPATCH_WT_EL(dtype, moe_ffn_t, a, (float *)dout.p, (const float *)dx.p));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(xout, dout.p, sizeof(float) * dim, hipMemcpyDeviceToHost));
	if (experts)
		HIPCHK(hipMemcpy(experts, dsel.p, sizeof(int) * n_active, hipMemcpyDeviceToHost));
	if (weights)
		HIPCHK(hipMemcpy(weights, dwts.p, sizeof(float) * n_active, hipMemcpyDeviceToHost));
	return YALM_OK;
}
