/*
 * yalm_hip.h — the drop-in C ABI of the MI355X (gfx950) decode engine.
 *
 * This header replaces the GPU-facing interface of the reference
 * (/root/reference/src/model.h:33-39, 70-79, 353-385 and the C++ members
 * compiled in src/infer.cu). It contains no HIP, CUDA or C++ types: every
 * entry point takes plain pointers, sizes and POD structs, so the reference's
 * own host (model.cpp, main.cpp, test.cpp) — or our C++20 mirror of it under
 * yalm_amd/host/ — binds it directly.
 *
 * Errors: every int-returning function returns YALM_OK (0) or a YALM_ERR_*
 * code; yalm_last_error() describes the last failure on the calling thread.
 * (The reference aborts on any runtime error, infer.cu:13-31; callers that
 * want that behaviour check the code and abort.)
 *
 * Threading: one decoder per stream; a decoder is not re-entrant (same as the
 * reference's InferenceState, model.h:84-190).
 */
#ifndef YALM_HIP_H
#define YALM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YALM_OK 0
#define YALM_ERR_HIP 1         /* a HIP runtime call failed */
#define YALM_ERR_ARG 2         /* bad argument / shape */
#define YALM_ERR_UNSUPPORTED 3 /* configuration the kernels do not implement */

/* DType codes follow the reference enum order (codec.h:15-25). */
enum { YALM_F32 = 0, YALM_F16 = 1, YALM_BF16 = 2, YALM_F8E5M2 = 3 };
/* ---------------- q4: 4-bit group-quantised weights ----------------
 * A storage format of this engine alone (code 16: outside the reference's DType range 0..8;
 * the reference rejects such a file). Symmetric 4-bit, one f16 scale per group of 32
 * consecutive elements of a weight row: an element is (u - 8) * s, u the nibble 0..15, s the
 * group's scale, whose low 3 mantissa bits are zero -- so every value is an exact f16 and a
 * q4 model has an exact f16 twin (the device the tests pin fp8 with). A matrix [rows][n],
 * n % 32 == 0, is rows rows of yalm_row_bytes(YALM_Q4, n) = round_up(n / 2 + n / 16, 16)
 * bytes: n / 32 16-byte nibble blocks (block b = elements 32 b .. 32 b + 31), then n / 32
 * f16 scales, then zero padding. A block is 4 little-endian 32-bit words; word j holds
 * elements 8 j .. 8 j + 7, element 8 j + i in the nibble at bits 4 * ((i >> 1) + 4 * (i & 1))
 * (models.q4_pack / q4_unpack). Every weight matrix of a q4 model, the embedding included,
 * has this layout; norms stay f32. Dense one-GPU decoders only: yalm_decoder_create,
 * yalm_forward, the greedy / sampled loops, yalm_block, yalm_prefill (through a per-layer
 * exact f16 upcast, as fp8), yalm_matmul, yalm_ffn, yalm_time_kernel, yalm_set_gemv_config.
 * Attention and Wo run as separate launches (yalm_attn_wo_plan returns 0).
 * YALM_ERR_UNSUPPORTED, with a yalm_last_error naming q4: yalm_decoder_create_moe,
 * yalm_decoder_create_tp, yalm_decoder_create_tp_ipc, yalm_moe_ffn, yalm_moe_ffn_rows.
 * YALM_ERR_ARG: a q4 config whose dim, hidden_dim or n_heads * head_dim is no multiple of 32. */
enum { YALM_Q4 = 16 };
/* ---------------- e4m3: row-scaled OCP E4M3 weights ----------------
 * A storage format of this engine alone (code 17: outside the reference's DType range; the
 * reference's F8E4M3 = 4 names a tensor of bare bytes, which this is not). A matrix [rows][n],
 * n % 16 == 0, is rows rows of yalm_row_bytes(YALM_E4M3, n) = n + 16 bytes: n codes (element e
 * at byte e), then one little-endian f32 scale s at byte n, then 12 zero bytes. A code is OCP
 * e4m3fn, S.EEEE.MMM with bias 7: subnormals m * 2^-9, maximum 448, no infinities, 0x7F and
 * 0xFF NaN. The value of an element is code * s. The quantiser (models.e4m3_quantize) writes
 * s = 2^k with -15 <= k <= 7 only and never a NaN code: for exactly those k every finite code
 * times s is an exact f16, so an e4m3 model has an exact f16 twin (models.e4m3_twin). The
 * decode kernels do not check the scale -- any finite f32 works there -- but the twin and the
 * prefill (whose upcast stores f16(code * s)) hold for the quantiser's scales only. Every
 * weight matrix of an e4m3 model, the embedding included, has this layout; norms, biases and
 * q / k norm gains stay f32. Dense one-GPU decoders only: yalm_decoder_create, yalm_forward,
 * the greedy / sampled loops, yalm_block, yalm_forward_rows, yalm_generate_speculative,
 * yalm_prefill (through a per-layer exact f16 upcast, as fp8), yalm_matmul, yalm_matmul_rows,
 * yalm_ffn, yalm_time_kernel, yalm_set_gemv_config. Attention and Wo fuse where the Wo row is
 * 4096 or 8192 codes (yalm_attn_wo_plan).
 * YALM_ERR_UNSUPPORTED, with a yalm_last_error naming e4m3: yalm_decoder_create_moe,
 * yalm_decoder_create_tp, yalm_decoder_create_tp_ipc, yalm_moe_ffn, yalm_moe_ffn_rows.
 * YALM_ERR_ARG: a config whose dim, hidden_dim or n_heads * head_dim is no multiple of 16. */
enum { YALM_E4M3 = 17 };
/* ActivationType (model.h:14-17) */
enum { YALM_GELU = 0, YALM_SILU = 1 };
/* InferenceMode (model.h:28-31) */
enum { YALM_HYDRATE_KV_CACHE = 0, YALM_OUTPUT_LOGITS = 1 };

/* Opaque stream handle; replaces cudaStream_t in init_cuda_stream (model.h:39). */
typedef struct yalm_stream_s *yalm_stream;
/* Opaque decoder: the device half of InferenceState + Model (model.h:84-190,
 * 303-327) — scratch buffers, KV caches, per-mode hipGraphs. */
typedef struct yalm_decoder_s *yalm_decoder;

/* Config (model.h:41-68). Same field meaning; the mixture-of-experts fields
 * (model.h:57-59) travel beside it in yalm_moe_config (yalm_decoder_create_moe),
 * so this struct keeps its layout. */
typedef struct yalm_config {
	int dim, hidden_dim, head_dim, n_layers, n_heads, n_kv_heads, vocab_size, max_seq_len;
	float rope_theta;
	int rotary_dim;
	float norm_eps;
	int act;          /* YALM_GELU / YALM_SILU */
	float qkv_clip;   /* FLT_MAX when absent (model.cpp:60-61) */
	int weight_dtype; /* YALM_F32 / YALM_F16 / YALM_F8E5M2 / YALM_Q4 / YALM_E4M3 */
} yalm_config;

/* Device pointers of one block (Block private fields, model.h:286-300). If
 * key_cache/value_cache are NULL the decoder allocates them (zeroed,
 * max_seq_len x n_kv_heads x head_dim f16 each). */
typedef struct yalm_block_weights {
	const float *rms_att, *rms_ffn;
	const void *wq, *wk, *wv, *wo, *w1, *w2, *w3;
	uint16_t *key_cache, *value_cache;
} yalm_block_weights;

/* Device pointers of the model (Model fields, model.h:303-311). wcls may equal
 * token_embedding (tied weights, model.cpp:370-377). blocks is a HOST array
 * of n_layers entries, copied by yalm_decoder_create. */
typedef struct yalm_model_weights {
	const void *token_embedding;
	const float *rms_final;
	const void *wcls;
	const yalm_block_weights *blocks;
} yalm_model_weights;

/* ---------------- device shim: replaces model.h:33-39 / infer.cu:59-90 ---------------- */
const char *yalm_last_error(void);
/* set_cuda_device (model.h:38): selects the HIP device for this thread. */
int yalm_set_device(int device);
/* upload_cuda (model.h:33): device alloc + H2D copy; returns NULL on failure. */
void *yalm_upload(const void *host, size_t size);
/* device alloc (zero-filled); returns NULL on failure. */
void *yalm_alloc(size_t size);
/* download_cuda (model.h:34): D2H copy into a caller buffer (the reference
 * allocated pinned memory and passed std::string through extern "C"). */
int yalm_download(void *host, const void *device, size_t size);
/* register_cuda_host / unregister_cuda_host (model.h:35, 37). */
int yalm_register_host(void *host, size_t size);
int yalm_unregister_host(void *host);
/* free_cuda (model.h:36). */
int yalm_free(void *device);
/* init_cuda_stream (model.h:39), with an opaque handle. */
int yalm_stream_create(yalm_stream *out);
int yalm_stream_destroy(yalm_stream s);
int yalm_stream_sync(yalm_stream s);
/* Fill n device elements of dtype with the deterministic synthetic
 * initialiser (uniform in [offset-scale, offset+scale); f32 adds offset).
 * Used to build random-weight models of real shapes in HBM without a PCIe
 * upload (bench.py). Same integer hash as the CPU oracle. */
int yalm_synth(void *device, size_t n, int dtype, uint64_t seed, float scale, float offset, yalm_stream s);
/* Bytes of one row of n elements of a weight matrix in dtype (q4: the padded row above; e4m3:
 * n + 16; 0 for an unknown dtype, a q4 n that is no multiple of 32 or an e4m3 n that is no
 * multiple of 16). Pure host arithmetic. */
size_t yalm_row_bytes(int dtype, int n);
/* yalm_synth for a q4 tensor [rows][n], which needs the row length (yalm_synth with YALM_Q4 is
 * YALM_ERR_ARG): nibble byte i of the tensor (row-major, nibble bytes only) is bits 40..47 of
 * the initialiser's hash of i, every scale is the restricted f16 nearest scale / 7 (the f16
 * nearest the f32 quotient, bits + 4 with the low 3 cleared), padding zero; the values are
 * uniform over (u - 8) * s, about [-8 / 7 scale, scale]. models.synth_q4_array is its numpy twin. */
int yalm_synth_q4(void *device, size_t rows, int n, uint64_t seed, float scale, yalm_stream s);
/* yalm_synth for an e4m3 tensor [rows][n] (yalm_synth with YALM_E4M3 is YALM_ERR_ARG): code
 * byte i of the tensor (row-major, code bytes only) is bits 40..47 of the initialiser's hash of
 * i, with the NaN codes made finite by clearing their lowest bit (0x7F -> 0x7E, 0xFF -> 0xFE);
 * every row's scale is 2^k for the smallest k in [-15, 7] with 448 * 2^k >= scale (7 if none),
 * the padding zero. models.synth_e4m3_array is its numpy twin. */
int yalm_synth_e4m3(void *device, size_t rows, int n, uint64_t seed, float scale, yalm_stream s);

/* ---------------- decoder: replaces Model::_forward_cuda / Block::_block_cuda ---------------- */
/* Creates the device state for one sequence (InferenceState::cuda,
 * model.cpp:323-345) on stream s (NULL = a private stream). Weight pointers
 * must stay valid for the decoder's lifetime. */
int yalm_decoder_create(const yalm_config *config, const yalm_model_weights *weights, yalm_stream s,
                        yalm_decoder *out);
int yalm_decoder_destroy(yalm_decoder d);
/* Model::forward (model.cpp:396-407 -> infer.cu:1021-1039): one token through
 * every block at position pos (sliding-window/sink indices as infer.cu:1081-
 * 1083). mode YALM_OUTPUT_LOGITS also computes the final norm + logits and,
 * if logits_host != NULL, copies vocab_size floats there before returning
 * (synchronous, like the reference's OUTPUT mode). YALM_HYDRATE_KV_CACHE is
 * asynchronous. Graph-replayed after the first call per mode. */
int yalm_forward(yalm_decoder d, int token, int pos, int mode, float *logits_host);
/* Device-resident greedy decode (-t 0; sampler.cpp:27-38 first-max argmax on
 * the device): feeds `token` at `pos`, then n_steps-1 more tokens each chosen
 * by argmax of the previous step; writes the n_steps argmax tokens to
 * out_tokens (host). No host round trip per token: each token's kernels are
 * launched back to back (eagerly: measured 0.3-0.5% faster than replaying the
 * per-token graph, whose kernel count yalm_graph_kernels still reports). */
int yalm_generate_greedy(yalm_decoder d, int token, int pos, int n_steps, int *out_tokens);
/* Device-side temperature / top-k / top-p sampling (csrc/sampler.h). The rule is in integers,
 * so the same logits, parameters and uniform give the same token whatever the reduction order:
 * m = the first-maximum logit; w_i = expf((l_i - m) / temperature) (sampler.cpp:50, f32),
 * q_i = (uint64) ldexpf(w_i, 40), 0 when w_i is not finite and positive; order = logit
 * descending (as order-preserving 32-bit keys), index ascending among equal logits; top_k > 0
 * keeps the first min(top_k, n) of that order (q sum S_k), top_p < 1 then the shortest prefix of
 * those whose q sum reaches min(S_k, max(1, ceil((double)top_p * S_k))); with S the kept q sum
 * and t = min(S, max(1, ceil((double)u * S))) the token is the first kept index, ascending,
 * whose inclusive kept prefix sum reaches t (sampler.cpp:53-57); S == 0: the first-maximum
 * argmax. top_k = 0 and top_p = 1 is the reference's temperature sampler up to rounding at the
 * boundaries of the cumulative distribution. */
typedef struct yalm_sampling {
	float temperature; /* > 0, finite */
	int top_k;         /* >= 0; 0 = off */
	float top_p;       /* in (0, 1]; 1 = off */
} yalm_sampling;
/* yalm_generate_greedy with the token of each step drawn by the rule above instead of the
 * argmax: one launch of one workgroup in the argmax launch's place (the step has the greedy
 * step's launch count, yalm_graph_kernels mode 3), parameters and uniforms read from device
 * memory. uniforms: host array of n_steps values in [0, 1], one consumed per step.
 * Dense and mixture-of-experts decoders, every weight dtype, any pos (the sliding window past
 * max_seq_len as in yalm_forward); yalm_device_step / yalm_device_tokens / yalm_enqueue_greedy
 * continue from it as after yalm_generate_greedy. YALM_ERR_ARG: temperature <= 0 or not
 * finite, top_k < 0, top_p outside (0, 1], a uniform outside [0, 1], n_steps above the token
 * buffer (65536), a vocabulary above 131072. YALM_ERR_UNSUPPORTED on tensor-parallel decoders
 * (yalm_decoder_create_tp / _tp_ipc): their vocabulary is sharded over the ranks. */
int yalm_generate_sampled(yalm_decoder d, int token, int pos, int n_steps, const yalm_sampling *s,
                          const float *uniforms, int *out_tokens);
/* Launch-only variant for benchmarking: enqueue n_steps greedy steps
 * continuing from the decoder's device-resident token/pos; no sync. */
int yalm_enqueue_greedy(yalm_decoder d, int n_steps);
/* Read back the device-resident next token / position after enqueue+sync. */
int yalm_device_step(yalm_decoder d, int *token, int *pos);
/* The greedy tokens produced on the device since the last yalm_generate_greedy
 * (that call's tokens, then every yalm_enqueue_greedy step, up to 65536):
 * copies min(*n_total, cap) of them to out (host) after a sync; *n_total = how many
 * were produced. Lets tensor-parallel ranks compare whole sequences (bench.py). */
int yalm_device_tokens(yalm_decoder d, int *out, int cap, int *n_total);
/* Block::block (model.cpp:213-265) for one layer, eagerly, on the decoder's
 * current activation x (the test hook for per-layer parity). */
int yalm_block(yalm_decoder d, int layer, int pos, int kv_sink, int kv_pos, int kv_len);
/* Host access to the decoder's activation x (dim floats) and logits. After a
 * YALM_HYDRATE_KV_CACHE forward of an IPC tensor-parallel decoder x is undefined
 * (that forward's last W2 partial is never exchanged: nothing reads it); after
 * yalm_block and OUTPUT forwards it is the full hidden state on every rank. */
int yalm_get_x(yalm_decoder d, float *host);
int yalm_set_x(yalm_decoder d, const float *host);
int yalm_get_logits(yalm_decoder d, float *host);
/* Average device time (ms) of one kernel of the forward, launched eagerly on
 * the decoder's stream `iters` times between HIP events (layers rotated so the
 * weights come from HBM). kernel_id: 0 = QKV GEMV, 1 = attention, 2 = Wo GEMV,
 * 3 = W1/W3 GEMV+GLU, 4 = W2 GEMV (a mixture-of-experts decoder: the expert launches;
 * 9 = its router), 5 = logits GEMV, 6 = one tensor-parallel
 * exchange of x (RCCL all-reduce or IPC exchange; collective: every rank calls it
 * with the same iters), 8 = the fused attention + Wo
 * launch (yalm_decoder_attn_wo; each timed launch gets a fresh step epoch, so its
 * Wo waves wait for the heads as in a real forward; the epoch-bump launches are
 * timed separately and subtracted), 10 = the sampling launch of yalm_generate_sampled on
 * the decoder's current logits, with the parameters of the last such call (before any:
 * temperature 1, no truncation) and its first uniform; it commits into a scratch step
 * state, not the decoder's; 11 = the q / k norm launch (yalm_decoder_set_qk_norm, which it
 * needs) on what the last QKV launch left; 12 / 13 = the draw and the accept launch of a 4-row
 * sampled speculative step, 14 = the verify launch of a greedy one, on the rows' current logits
 * and a scratch step state (decoders with a multi-row form). Used by bench.py for the roofline of the
 * dominant kernel. */
int yalm_time_kernel(yalm_decoder d, int kernel_id, int iters, float *avg_ms);
/* The same-process streaming envelope: average ms of one pure read-only pass over
 * `bytes` of HBM (16-byte non-temporal loads, the best of a few wave geometries,
 * `iters` back-to-back launches alternating two buffers so the 256 MiB Infinity
 * Cache cannot serve them). bench.py reports a kernel's time against it so the
 * roofline fraction is also stated relative to what THIS box streams. */
int yalm_stream_envelope(size_t bytes, int iters, float *avg_ms);
/* Override the GEMV launch geometry of one weight-streaming kernel kind
 * (0 = QKV, 1 = Wo, 2 = W1/W3, 3 = W2, 4 = logits): workgroup size
 * 256|512|1024, unroll (16-byte loads in flight per lane) 2|4|8, and `gpw` =
 * workgroups per CU of the row-block kernel; 0 = automatic.
 * Drops captured graphs (re-captured on next use). Tuning/ablation hook. */
int yalm_set_gemv_config(yalm_decoder d, int kind, int threads, int unroll, int gpw);
/* Kernel launches per forward of graph `mode` (0 = HYDRATE, 1 = OUTPUT_LOGITS, 2 = the
 * device greedy step, 3 = the device sampled step of yalm_generate_sampled): *kernels = kernel nodes of the captured per-token hipGraph (RCCL
 * collectives count as the kernels they capture), *nodes (may be NULL) = all nodes. Test
 * and measurement hook (tensor parallelism adds no exchange launches over IPC). */
int yalm_graph_kernels(yalm_decoder d, int mode, int *kernels, int *nodes);
/* Name of kernel_id's device function (to match rocprofv3 summaries). */
const char *yalm_kernel_name(yalm_decoder d, int kernel_id);
/* 1 if this decoder's launch path runs attention and the Wo projection (+ the
 * residual add) as ONE launch (attn_wo.h: the Wo weight stream overlaps the
 * attention; replaces attn + fused_matmul_add_residuals, infer.cu:338-524, 270):
 * head_dim 128, fp16 / fp8 weights with 1, 2, 4 or 8 KB (per-rank) Wo rows (e4m3: 4 or 8 KB of codes), and
 * not YALM_LAUNCH_SEPARATE_ATTN_WO. 0 = two separate launches. The split-KV
 * attention output is handed to the Wo workgroups as {value, epoch} granules. */
int yalm_decoder_attn_wo(yalm_decoder d);
/* Launch-mode switches of one decoder (default 0; drops captured graphs):
 * YALM_LAUNCH_EAGER every forward launches its kernels directly instead of replaying
 * the per-token graph (profilers that mis-handle graph replay); YALM_LAUNCH_SYNC a
 * stream sync after every replay (debugging); YALM_LAUNCH_SEPARATE_ATTN_WO separate
 * attention and Wo launches where the fused one would run (A/B and tests). The
 * production library reads no environment variable. */
#define YALM_LAUNCH_EAGER 1
#define YALM_LAUNCH_SYNC 2
#define YALM_LAUNCH_SEPARATE_ATTN_WO 4
int yalm_decoder_set_launch(yalm_decoder d, int flags);
/* The fused launch's plan for a (per-rank) config when `slots` workgroups of 256
 * threads are co-resident (occupancy x CUs): returns 1 and the key splits per kv head
 * and the grid size, or 0 = separate attention and Wo launches (unsupported shape, or
 * fewer than 2 key splits fit beside the mergers and Wo workgroups while contexts can
 * exceed head mode). Pure host arithmetic: no device is touched. */
int yalm_attn_wo_plan(const yalm_config *config, int slots, int *splits, int *grid);
/* Timeline of the most recent fused attention + Wo launch (decoder created with
 * YALM_ATTN_WO_TRACE=1): 16 stamps per workgroup at [w * 16 + k]: k < 8
 * s_memrealtime (100 MHz), k + 8 the shader clock (s_memtime) at the same point (k = 0: instead the
 * workgroup's place, HW_ID | XCC_ID << 32); k = 0 start, 1 hand-off signalled (attention; 0 if this workgroup did not
 * finish a kv head) or Wo slice landed (Wo; the trace waits for it), 2 poll passed (Wo) or
 * first K/V/q loads landed (attention; the trace waits for them), 3 end; attention units:
 * 4 scores of the last chunk, 5 its softmax, 6 P.V sums combined, 7 head outputs / partials
 * issued; merger workgroups (2 and 4 read 0): 5 gather issued, 7 every partial seen. A
 * phase a workgroup never reached reads 0. Workgroups [0, *attention_workgroups) are
 * attention units and mergers, the rest Wo. */
int yalm_attn_wo_trace(yalm_decoder d, unsigned long long *host, size_t count, int *workgroups,
                       int *attention_workgroups);

/* ---------------- model-family forms: scaled RoPE (Llama-3.1 / 3.2), q / k / v bias (Qwen2) ----------------
 * Both are set on a created decoder and are off by default: a decoder on which neither is
 * called launches exactly the kernels it launched before these entry points existed. The
 * reference reads neither form.
 *
 * RoPE scaling: the decoder's frequency table (head_dim / 2 pair frequencies; the decode
 * step's cos / sin table, the attention sinks' one-position rotation and the batched
 * prefill's table are all built from it) is recomputed on the host and uploaded after a
 * stream sync. type 1 = "llama3": per pair frequency f (the unscaled table's f32 value),
 * with the wavelength w = 2 pi / f:
 *   w < original_max_position / high_freq_factor      f stays
 *   w > original_max_position / low_freq_factor       f / factor
 *   otherwise  s = (original_max_position / w - low_freq_factor) / (high_freq_factor - low_freq_factor),
 *              (1 - s) f / factor + s f
 * in double, rounded once to f32. type 0 restores the unscaled table bit for bit. Every
 * decoder kind takes it. YALM_ERR_ARG: factor < 1, high_freq_factor <= low_freq_factor,
 * low_freq_factor <= 0, original_max_position <= 0, an unknown type. */
typedef struct yalm_rope_scaling {
	int type; /* 0 none, 1 llama3 */
	float factor, low_freq_factor, high_freq_factor;
	int original_max_position;
} yalm_rope_scaling;
int yalm_decoder_set_rope_scaling(yalm_decoder d, const yalm_rope_scaling *s);
/* The frequency table in use: head_dim / 2 floats to `host`. */
int yalm_decoder_get_inv_freq(yalm_decoder d, float *host);
/* q / k / v bias: v = clip(W . rmsnorm(x) + b), then RoPE (q, k), the f16 cache write (k, v)
 * and the q store as without a bias. bq, bk, bv: HOST arrays of n_layers DEVICE pointers to
 * f32 vectors, 8-byte aligned and caller-owned for the decoder's lifetime: bq[l] of
 * n_heads * head_dim, bk[l] / bv[l] of n_kv_heads * head_dim elements, in the row order of
 * wq / wk / wv. All three NULL removes the bias. Drops the captured graphs. Dense one-GPU
 * decoders of every weight dtype: decode, yalm_forward_rows / yalm_generate_speculative
 * (not q4, as without a bias) and yalm_prefill; a tensor-parallel or mixture-of-experts
 * decoder returns YALM_ERR_UNSUPPORTED. */
int yalm_decoder_set_qkv_bias(yalm_decoder d, const float *const *bq, const float *const *bk,
                              const float *const *bv);
/* q / k norm (Qwen3): an RMSNorm over each head of q and of k, after the projection and the
 * clip and before RoPE. With q, k, v = clip(W . rmsnorm(x)) as without it, for every head h of
 * q and of k:
 *   ss = sum_i a[h][i]^2 over the head's head_dim elements
 *   a'[h][i] = a[h][i] * (1 / sqrtf(ss / head_dim + norm_eps)) * g[i]
 * g = gq[l] for q and gk[l] for k (head_dim f32 values shared by the layer's heads; no bias),
 * norm_eps the config's. All f32 in this statement order; the sum is one wave's fixed-order
 * reduction, so the same input gives the same bits on every run. RoPE on a', the q store and
 * the f16 K cache write follow as without the norm; V is untouched, and so is the attention
 * sinks' one-position rotation (it turns rows that were normalised when they were written).
 * gq, gk: HOST arrays of n_layers DEVICE pointers, 8-byte aligned and caller-owned for the
 * decoder's lifetime. Both NULL removes the norm. Drops the captured graphs. Off by default:
 * a decoder on which it was never called launches what it launched before; with it, one more
 * launch per layer (qk_norm_rope_kernel, yalm_time_kernel id 11) between QKV and attention.
 * Dense one-GPU decoders of every weight dtype: decode and yalm_forward_rows /
 * yalm_generate_speculative (not q4, as without the norm), and yalm_prefill: its QKV GEMM
 * leaves raw f32 rows and one row kernel clips, norms, rotates and stores Q and the K / V cache
 * rows, in every precision form. YALM_ERR_UNSUPPORTED, naming the q / k
 * norm: a tensor-parallel or mixture-of-experts decoder, a decoder that has a q / k / v bias
 * (and yalm_decoder_set_qkv_bias on a decoder that has the norm).
 * YALM_ERR_ARG: exactly one array NULL, a NULL or misaligned (not 8-byte) entry. */
int yalm_decoder_set_qk_norm(yalm_decoder d, const float *const *gq, const float *const *gk);

/* ---------------- mixture of experts (Mixtral), one GPU ----------------
 * The reference runs MoE on the CPU only (infer.cpp:100-132, 347-384; its GPU path
 * asserts, infer.cu:865-867). Per layer: a router launch (rmsnorm(x) . moegate^T, then
 * the reference's top-k: K rounds of a first-maximum scan, softmax over the selected
 * logits) leaves the K expert indices and weights in device memory; one W1 | W3 + GLU
 * launch streams only the selected experts' rows of the stacked tensors; W2 of all
 * selected experts runs as one launch of row length K * hidden_dim when that fits the
 * LDS and hidden_dim is a multiple of 64 x the elements of a 16-byte load, else as one
 * launch per selected expert. 1 <= n_experts_active <= n_experts <= 64. */
typedef struct yalm_moe_config {
	int n_experts, n_experts_active;
} yalm_moe_config;
/* As yalm_decoder_create; blocks[l].w1 / w3 point at stacked (n_experts, hidden_dim, dim)
 * tensors, w2 at (n_experts, dim, hidden_dim); moegate: HOST array of n_layers device
 * pointers, each (n_experts, dim) in the weight dtype. yalm_forward,
 * yalm_generate_greedy, yalm_enqueue_greedy, yalm_block, yalm_get_x / yalm_set_x,
 * yalm_graph_kernels and yalm_decoder_set_launch work as on a dense decoder;
 * yalm_time_kernel ids 3 and 4 time the expert launches (on the layer's most recent
 * routing), id 9 the router; yalm_prefill / yalm_prefill_time run the batched expert
 * FFN (below, "batched prefill") under the dense prefill's shape rules. There is no
 * tensor-parallel form. */
int yalm_decoder_create_moe(const yalm_config *config, const yalm_moe_config *moe, const yalm_model_weights *weights,
                            const void *const *moegate, yalm_stream s, yalm_decoder *out);
/* The routing of the most recent forward / yalm_block: experts[n_layers * K] and
 * weights[n_layers * K] (host, either may be NULL), layer-major, in selection order
 * (descending logit). YALM_ERR_ARG on a dense decoder. */
int yalm_moe_routing(yalm_decoder d, int *experts, float *weights);

/* ---------------- tensor parallelism (BASELINE config 5) ----------------
 * Megatron row/column split of one model over tp_size GPUs, one process per
 * GPU: rank r holds Wq/Wk/Wv rows of heads [r*H/N, (r+1)*H/N) (kv heads
 * likewise), Wo columns of those heads, W1/W3 rows and W2 columns
 * [r*hidden/N, (r+1)*hidden/N), Wcls rows [r*vocab/N, ..); norms and the
 * embedding are replicated. Each layer then needs two all-reduces of x
 * (after Wo and after W2), captured in the per-token graph as RCCL
 * ncclAllReduce over xGMI; the greedy argmax gathers one (value, index) pair
 * per rank. Replaces the single-device forward of model.cpp:396-407 /
 * infer.cu:1021-1128 for multi-GPU; the reference has no multi-GPU path. */
/* 128-byte RCCL unique id, created by rank 0 and shared with the other ranks
 * out of band (bench.py: torch.distributed broadcast). */
int yalm_tp_unique_id(void *id_out);
/* config: the FULL model; weights: this rank's shards as above (blocks as in
 * yalm_decoder_create, KV caches for the local kv heads or null). Collective:
 * every rank calls it concurrently (ncclCommInitRank). All yalm_forward /
 * yalm_generate_greedy calls must then be made by every rank in lockstep;
 * logits (full vocabulary) and greedy tokens are identical on all ranks. */
int yalm_decoder_create_tp(const yalm_config *config, const yalm_model_weights *weights, int tp_rank, int tp_size,
                           const void *unique_id, yalm_stream s, yalm_decoder *out);
/* The same split with an IPC one-shot exchange instead of RCCL (no NCCL
 * communicator; also runs several ranks on ONE GPU, which RCCL refuses): each
 * rank allocates its exchange buffer (yalm_tp_ipc_alloc, config = full model,
 * s = the stream its decoder will run on) and shares the YALM_TP_HANDLE_BYTES
 * rank record out of band (the buffer's hipIpcMemHandle, the GPU's UUID and the
 * stream's CU mask); every rank then passes all tp_size records (rank order)
 * and the same stream s. Ranks on one GPU whose CU masks overlap get a one-wave
 * gate launch before each exchange consumer (they could otherwise hold the CUs a
 * peer's producer needs); one GPU per rank, or disjoint CU masks
 * (yalm_stream_create_cu_part), run the production sequence without it. The
 * decoder takes ownership of own_buf (1..8 ranks). Per exchange no launch of its own:
 * the producer (the fused attention + Wo launch, the W2 GEMV, the logits GEMV,
 * the argmax) pushes each value of this rank's partial into this rank's slot of
 * EVERY rank's buffer as an 8-byte {value, tag} granule (one system-scope store:
 * the data is its own ready flag); the consumer (the next normalising GEMV)
 * waits for every rank's granules while its weight stream starts and sums them
 * in rank order, so x is identical on every rank. Past 4 ranks a collect launch
 * sums x once before the consumer. The exchange sequence numbers live in the
 * decoder's step state, so every rank must make the same calls in lockstep. */
#define YALM_TP_HANDLE_BYTES 128
#define YALM_CU_MASK_WORDS 8 /* 256 CUs */
int yalm_tp_ipc_alloc(const yalm_config *config, int tp_size, yalm_stream s, void **buf, void *handle_out);
/* A stream restricted to CU block `part` of `n_parts` (CUs [part * ncu / n_parts,
 * (part + 1) * ncu / n_parts), spread by the driver over all XCDs): n_parts rank
 * processes on ONE GPU then run on disjoint CUs like n_parts small GPUs (the
 * one-GPU rehearsal of tensor parallelism; tests/test_gpu_mistral_dims.py, bench.py
 * --rehearse). Destroy with yalm_stream_destroy. */
int yalm_stream_create_cu_part(int part, int n_parts, yalm_stream *out);
int yalm_decoder_create_tp_ipc(const yalm_config *config, const yalm_model_weights *weights, int tp_rank, int tp_size,
                               void *own_buf, const void *handles, yalm_stream s, yalm_decoder *out);
/* Device-to-device 2D copy (hipMemcpy2D): shard slicing of weights resident in HBM. */
int yalm_copy_2d(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t width, size_t height);

/* ---------------- batched prefill (MFMA): the perplexity / prompt path ----------------
 * Replaces the reference's position-by-position forward loop over a prompt
 * (main.cpp:128-200 `-m perplexity`, main.cpp:95-101 prompt hydration,
 * Model::forward per position, model.cpp:396-407) with one pass per layer
 * over all n positions: rmsnorm + QKV GEMM + RoPE + fp16 KV-cache write, causal
 * GQA attention, Wo / W1|W3 / W2 GEMMs on the f16 MFMA units.
 * Fills the KV cache rows pos0 .. pos0 + n - 1 exactly where the decoder
 * expects them, so yalm_forward / yalm_generate_greedy can continue at
 * pos0 + n. logprobs (host, n floats, may be NULL): logprobs[i] =
 * log softmax(logits at position pos0 + i)[tokens[i + 1]] for i < n - 1 (the
 * quantity main.cpp:155 sums), logprobs[n - 1] = 0. Requires f16 weights (fp8, e4m3 and q4:
 * through an exact f16 upcast of one layer at a time),
 * dims multiple of 128, head_dim 64 | 128 and pos0 + n <= max_seq_len
 * (the sliding window past max_seq_len stays on the decode path).
 * Synchronous. Activations are rounded to f16 for the MFMA inputs: results
 * match the decode path within the tolerance stated in tests/test_gpu_prefill.py.
 * Range guard: where the reference's f32 activations would not fit an f16 operand,
 * a layer's GLU output (W2's A operand; trained checkpoints' "massive activations")
 * is stored with an exact power-of-two scale that W2's epilogue undoes, and the pass
 * runs again; any other operand out of range (the normalised x, Q) returns
 * YALM_ERR_UNSUPPORTED (the decode path keeps them in f32).
 * Mixture-of-experts decoders (yalm_decoder_create_moe): the attention half as above; the
 * FFN half routes all n rows (the decode router's arithmetic on each row of the f32
 * residual stream), groups the n * K (row, expert) entries by expert on the device
 * (stable: rows ascending inside an expert) and runs W1 | W3 + GLU and W2 as grouped GEMMs
 * over 256-row tiles of one expert each, then x[t] += sum_k weight_k * y[slot(t, k)] in
 * selection order, in f32, without atomics: two prefills of the same input give the same
 * bits. max_seq_len * n_experts_active <= 131072. */
int yalm_prefill(yalm_decoder d, const int *tokens, int n, int pos0, float *logprobs);
/* The last yalm_prefill's passes (1 = no operand out of range) and the number of
 * layers whose GLU output ran scaled. */
int yalm_prefill_info(yalm_decoder d, int *passes, int *scaled_layers);
/* The routing of the last yalm_prefill of n positions on a mixture-of-experts decoder:
 * experts / weights [n][n_layers][K] (host, either may be NULL), in selection order.
 * YALM_ERR_ARG on a dense decoder or before any prefill. */
int yalm_prefill_routing(yalm_decoder d, int *experts, float *weights);
/* Precision form of decoder d's prefill. YALM_PREFILL_FAST (default): f16 activation
 * operands (the K / V columns' over a split [hi | lo] operand). YALM_PREFILL_SPLIT: every
 * activation operand -- the normalised x, Q, the attention probabilities P, the attention
 * output, the GLU output -- as f16 [hi | lo] pairs (~22 significant bits, the f32 the
 * reference keeps, to ~2^-22), at twice the matrix work; the perplexity bar of SURVEY §7
 * (|d log ppl| <= 1e-3) then holds on peaked models too. The CLI's
 * -m perplexity uses SPLIT, prompt hydration FAST. */
#define YALM_PREFILL_FAST 0
#define YALM_PREFILL_SPLIT 1
int yalm_set_prefill_precision(yalm_decoder d, int mode);
/* Average device time (ms) of one n-position prefill with log-probs (synthetic
 * token ids), over `iters` back-to-back runs (bench_prefill.py). */
int yalm_prefill_time(yalm_decoder d, int n, int iters, float *avg_ms);
/* Test / ablation hook: the prefill GEMM forms of decoder d (d = NULL: of the
 * yalm_gemm_f16 test hook). spec = comma-separated key:value pairs, NULL or "" = the
 * defaults: qkv|wo|glu|w2|cls|test:<128|192|256|320> force that GEMM's tile width;
 * 8p:0 the 2-phase kernel; persist:0 one workgroup per tile; skinny:0 the large tiles
 * for T <= 64 too; qkv1:0 the q and k|v GEMMs as two launches; skl:0 the skinny GEMMs'
 * weights as register loads; wnorm:0 the row norms as one workgroup per row (default:
 * one wave per row). Every GEMM form is exact against the others (tests). An
 * unknown key is YALM_ERR_ARG. */
int yalm_set_prefill_forms(yalm_decoder d, const char *spec);

/* ---------------- multi-row forward and speculative greedy / sampled decode ----------------
 * Dense decoders on one GPU with f32, f16, fp8 (E5M2) or e4m3 weights. YALM_ERR_UNSUPPORTED, with a
 * yalm_last_error naming the reason: q4 weights, mixture-of-experts decoders
 * (yalm_decoder_create_moe), tensor-parallel decoders (yalm_decoder_create_tp / _tp_ipc). */
/* T tokens (1 <= T <= 4) at positions pos .. pos + T - 1 through every layer in ONE pass over
 * the weights (csrc/gemv_rows.h: each weight matrix is streamed once for all T rows; f32
 * activations and accumulation, as yalm_forward). Row t attends to keys 0 .. pos + t; the KV
 * rows pos .. pos + T - 1 are written where the decoder expects them, so yalm_forward /
 * yalm_generate_greedy can continue at pos + T. logits_host: [T][vocab_size] floats (then the
 * call is synchronous) or NULL. The device-resident (token, pos) of the greedy loop is set to
 * (tokens[0], pos) and does not advance, as after an OUTPUT_LOGITS forward. YALM_ERR_ARG: T
 * outside 1..4, a token out of range, pos < 0 or pos + T > max_seq_len (a multi-row step never
 * wraps the ring or rotates the sinks). */
int yalm_forward_rows(yalm_decoder d, const int *tokens, int T, int pos, float *logits_host);
/* Speculative greedy decode (csrc/spec.h). A step runs `rows` rows through yalm_forward_rows'
 * path: row 0 the token greedy decode would feed, rows k = 1..rows-1 drafted next tokens d_k (a
 * row without a draft is fed token 0). With m_t the first-maximum argmax of row t (the rule of
 * yalm_argmax), the step yields a = 1 + the longest prefix of drafts with d_k == m_(k-1) tokens,
 * m_0 .. m_(a-1): exactly the tokens of plain greedy decode. KV rows of rejected drafts are
 * overwritten by later steps.
 * The drafter, in integers. History H[0, m) = the caller's context followed by every token
 * produced so far; H[m - 1] is the token to feed next. For g = ngram_max down to ngram_min: take
 * the LARGEST i with i + g <= m - 1 and H[i, i + g) == H[m - g, m); the first g that has such an
 * i wins, and d_k = H[i + g + k - 1] for k = 1..rows-1 while that index is < m. Later drafts, and
 * all of them when nothing matches, are "none"; a none row is never accepted. The context is
 * capped at its last 65536 tokens.
 * draft_stream (test and benchmark hook): when non-NULL the drafts of a step are
 * draft_stream[p + k - 1], p = the tokens produced so far; none past draft_stream_len. */
typedef struct yalm_spec {
	int rows;                  /* 2..4 */
	int ngram_max, ngram_min;  /* 1 <= ngram_min <= ngram_max <= 4 */
	const int *draft_stream;   /* host, or NULL = the n-gram drafter */
	int draft_stream_len;
} yalm_spec;
typedef struct yalm_spec_stats {
	int spec_steps;        /* multi-row steps run */
	int accepted_drafts;   /* drafts whose token was delivered: spec_steps + accepted_drafts + plain_steps == n_tokens */
	int plain_steps;       /* plain steps (at and past the window's end) */
	int launches_per_step; /* kernel launches of one multi-row step: 4 + n_layers * (4 + rows), sampled: 5 + ... */
} yalm_spec_stats;
/* The contract of yalm_generate_greedy: feeds `token` at `pos`, writes exactly n_tokens tokens to
 * out_tokens (host), and the decoder then continues at pos + n_tokens (yalm_device_step,
 * yalm_enqueue_greedy, yalm_device_tokens) as after the greedy call. context (host, n_context
 * tokens, may be NULL with n_context 0 = the history starts at `token`) must end with `token`.
 * The host enqueues the steps in batches with no per-token round trip, reads the produced count
 * once per batch, drops what the last step accepted past n_tokens and sets the device (token,
 * pos) accordingly. A step needs pos + rows <= max_seq_len; from the first position where that
 * fails the call finishes with plain greedy steps, so it works at any pos. stats may be NULL.
 * YALM_ERR_ARG: rows outside 2..4, ngram bounds outside 1 <= min <= max <= 4, n_tokens above
 * the token buffer (65536), a context that does not end with token. */
int yalm_generate_speculative(yalm_decoder d, int token, int pos, int n_tokens, const yalm_spec *cfg,
                              const int *context, int n_context, int *out_tokens, yalm_spec_stats *stats);
/* Speculative sampled decode: yalm_generate_speculative with every row drawn by the rule of
 * yalm_generate_sampled instead of its argmax. Row t of a step is drawn with
 * uniforms[p + t], p = the tokens produced so far: the uniform of the output index the row would
 * fill. Draft d_k is accepted iff it equals the token drawn from row k - 1 (the drafter proposes
 * one token, not a distribution, so there is nothing to resample: a draft is accepted with
 * probability p(d_k)). Row k's input is then the token the plain sampled loop would have fed at
 * that index and its draw uses the uniform that loop would have used: the tokens are
 * yalm_generate_sampled's for the same uniforms, as the greedy call's are yalm_generate_greedy's.
 * Caveat: that equality holds when both paths see the same logits. The multi-row GEMV and the
 * decode GEMV sum in different orders, so a draw whose target lies within that rounding of a
 * boundary of the cumulative distribution can land on the neighbouring token in one path and not
 * in the other (both are valid draws; greedy has the same property at near-ties).
 * A step is: draft, rows, one launch of `rows` workgroups that draw (csrc/spec.h,
 * spec_sample_rows_kernel), one that accepts (spec_accept_kernel): 5 + n_layers * (4 + rows)
 * launches. Otherwise the contract of yalm_generate_speculative: batches with one count
 * read-back each, the overshoot dropped (rows past output index n_tokens - 1 read the last
 * uniform and their tokens are not delivered, so a following call's uniforms start at its own
 * index 0), a context that ends with `token`, and from the first position with pos + rows >
 * max_seq_len the plain steps of yalm_generate_sampled, which read uniforms[p] like every other
 * draw. uniforms: host, n_tokens values in [0, 1]. Same scope and refusals as the greedy call
 * (YALM_ERR_UNSUPPORTED: q4, mixture-of-experts, tensor-parallel); YALM_ERR_ARG: its argument
 * errors and those of yalm_generate_sampled (temperature, top_k, top_p, a uniform outside
 * [0, 1], a vocabulary above 131072). */
int yalm_generate_speculative_sampled(yalm_decoder d, int token, int pos, int n_tokens, const yalm_spec *cfg,
                                      const yalm_sampling *s, const float *uniforms, const int *context,
                                      int n_context, int *out_tokens, yalm_spec_stats *stats);
/* Speculative decode with a draft model: a second, smaller decoder `draft` on the SAME stream
 * proposes a token at every row of every step (csrc/spec.h). s == NULL is the greedy call (every
 * row's argmax, as yalm_generate_speculative); otherwise the sampled one (every row drawn with
 * uniforms[p + t] by output index, as yalm_generate_speculative_sampled, with its argument checks).
 * A step, all on the one stream with no host synchronisation:
 *   1. sync (1 launch): draft's device step = the target's current (token, pos), nothing produced.
 *      A token the draft does not have (>= its vocab_size) is fed as token 0 and the step's drafts
 *      are none: the draft's embedding is never read out of range.
 *   2. rows - 1 greedy forwards of `draft` from its device state (the path of yalm_enqueue_greedy):
 *      they yield d_1 .. d_(rows-1) and write its KV rows pos .. pos + rows - 2. Then one KV-only
 *      forward (the YALM_HYDRATE_KV_CACHE form at the state they left) feeds d_(rows-1) at
 *      pos + rows - 1.
 *   3. gather (1 launch): rows k = 1..rows-1 of the target's step get d_k; a d_k the target does
 *      not have (>= its vocab_size) is none. With draft_stream set the drafts are
 *      draft_stream[p + k - 1] instead, as in yalm_spec (the draft's forwards still run: a
 *      benchmark pays a draft model's true cost at a chosen acceptance).
 *   4. the rows forward and verify (or draw + accept) of the n-gram calls, unchanged.
 * The delivered tokens do not depend on the draft: a row of the multi-row GEMV depends on
 * neither the row count nor the other rows, so the call returns exactly the tokens of
 * yalm_generate_speculative / _sampled at the same rows (hence of the plain loops, with their
 * caveats). A stale, wrong or unhydrated draft cache only costs acceptance. After a step that
 * accepts a tokens the draft's KV rows pos .. pos + a - 1 hold the delivered tokens (accepted
 * drafts equal them); later rows are overwritten by later steps, as in the target. For drafts
 * worth accepting the caller hydrates positions [0, pos) on BOTH decoders (yalm_prefill or
 * yalm_forward on each).
 * Toward the target the contract of yalm_generate_speculative: batches of up to 64 steps with
 * one count read-back each, the overshoot dropped, and from the first p with p + rows >
 * max_seq_len the plain steps of the target alone (plain_steps; the draft does not run).
 * Afterwards the draft's device (token, pos) and token buffer are unspecified; its KV rows
 * [0, pos + n_tokens) are valid unless plain steps ran.
 * launches_per_step = (s ? 5 : 4) + n_layers * (4 + rows) [+ n_layers with the q / k norm]
 *                     + 1 + (rows - 1) * G + H,
 * the n-gram step with sync + gather in the drafter launch's place, G and H the kernel counts
 * of the draft's yalm_graph_kernels modes 2 (greedy) and 0 (KV-only).
 * Target: what yalm_forward_rows accepts. Draft: any dense one-GPU decoder, any weight format
 * (q4 included), with its own bias, q / k norm or RoPE scaling; the vocabulary sizes may differ.
 * YALM_ERR_UNSUPPORTED: a target the multi-row path refuses; a tensor-parallel or
 * mixture-of-experts draft. YALM_ERR_ARG: draft == d; decoders on different streams (create the
 * draft on yalm_decoder_get_stream(d)); the draft's max_seq_len below the target's; rows outside
 * 2..4; a null cfg; the argument errors of the n-gram calls. */
typedef struct yalm_spec_model {
	int rows;                 /* 2..4 */
	const int *draft_stream;  /* test / benchmark hook, host, or NULL: as in yalm_spec */
	int draft_stream_len;
} yalm_spec_model;
int yalm_generate_speculative_model(yalm_decoder d, yalm_decoder draft, int token, int pos, int n_tokens,
                                    const yalm_spec_model *cfg, const yalm_sampling *s, const float *uniforms,
                                    int *out_tokens, yalm_spec_stats *stats);
/* The stream decoder d enqueues on (its own, or the one it was created on). Not owned by the
 * caller when the decoder created it: do not destroy it. */
int yalm_decoder_get_stream(yalm_decoder d, yalm_stream *out);
/* Test hook (host pointers, synchronous, no decoder): the draw and the accept launch of a sampled
 * speculative step exactly as the loop makes them, on logits [T][n] (stride n, n <= 131072, 1 <=
 * T <= 4) with no token produced yet: row t is drawn with uniforms[t]; drafts[k - 1] = d_k for k
 * = 1..T-1, -1 for none (may be NULL when T == 1). drawn_out [T]: every row's token; kept_out
 * [T] (may be NULL): every row's kept-set size; *accepted_out = a, the tokens the step yields. */
int yalm_spec_sample_rows(const float *logits, int n, int T, const yalm_sampling *s, const float *uniforms,
                          const int *drafts, int *drawn_out, int *kept_out, int *accepted_out);
/* Test hook (host pointers, synchronous, no decoder): the drafter kernel on history[0, m),
 * 1 <= m <= 131072; drafts_out[k - 1] = d_k for k = 1..rows-1, -1 for none. */
int yalm_spec_draft(const int *history, int m, int rows, int ngram_max, int ngram_min, int *drafts_out);

/* ---------------- batched decode: up to four independent sequences per weight pass ----------------
 * A batch runs n_seq = 1..4 sequences through the multi-row path of yalm_forward_rows (csrc/batch.h):
 * every weight matrix is streamed ONCE per step for all sequences, and every row yields a token on
 * every step. Row s belongs to sequence s and to nothing else: it attends to its own KV cache, is
 * fed its own (token, pos) and appends to its own token buffer. A row of the multi-row GEMV depends
 * on neither the row count nor the other rows, so row s of a step equals yalm_forward_rows(T = 1)
 * of the same token at the same position over the same history, bit for bit (logits and the KV row).
 * Scope: that of yalm_forward_rows. Dense decoders on one GPU with f32, f16, fp8 (E5M2) or e4m3
 * weights, with or without a q / k / v bias or the q / k norm. YALM_ERR_UNSUPPORTED, with a
 * yalm_last_error naming the reason: q4 weights, mixture-of-experts decoders, tensor-parallel
 * decoders. A decoder that never creates a batch launches exactly what it launched before. */
typedef struct yalm_batch_s *yalm_batch;
/* The batch owns, per sequence: a KV cache set (n_layers x K and V, max_seq_len x n_kv_heads x
 * head_dim f16, the decoder's layout, zeroed), a device step state (token, pos, tokens produced), a
 * token buffer of the decoder's capacity (65536) and a split-KV partial buffer; and the [n_seq][..]
 * activation and logits buffers. It uses the decoder's stream, weights and model-family forms as
 * they are when a call is made. The decoder must outlive the batch: destroying the decoder first is
 * the caller's error (the batch then points at freed memory). yalm_batch_destroy syncs the stream.
 * YALM_ERR_ARG: n_seq outside 1..4. */
int yalm_batch_create(yalm_decoder d, int n_seq, yalm_batch *out);
int yalm_batch_destroy(yalm_batch b);
/* Copies KV rows [0, n_positions) of every layer from the DECODER's own caches into sequence seq
 * (seq == -1: into every sequence): device to device, asynchronous on the decoder's stream. This is
 * how prompts arrive -- hydrate the decoder with yalm_prefill / yalm_forward, then load -- and the
 * fork for several completions of one prompt. Rows from n_positions on are not touched.
 * YALM_ERR_ARG: n_positions outside [0, max_seq_len], seq outside -1 .. n_seq - 1. */
int yalm_batch_load(yalm_batch b, int seq, int n_positions);
/* One step without a commit. tokens, pos: host arrays of n_seq; row s feeds tokens[s] at pos[s],
 * attends to keys 0 .. pos[s] of sequence s's cache and writes that cache's row pos[s].
 * logits_host: [n_seq][vocab_size] floats (then the call is synchronous) or NULL. Each sequence's
 * device (token, pos) is set to (tokens[s], pos[s]) and does not advance, as after
 * yalm_forward_rows. YALM_ERR_ARG: a token out of range, pos[s] outside [0, max_seq_len). */
int yalm_batch_forward(yalm_batch b, const int *tokens, const int *pos, float *logits_host);
typedef struct yalm_batch_stats {
	int launches_per_step; /* kernel launches of one step: 3 + n_layers * 5 with the one-launch attention,
	                          3 + n_layers * (4 + n_seq) with YALM_BATCH_ATTN_PER_SEQ; the q / k norm adds
	                          n_layers */
} yalm_batch_stats;
/* n_steps steps enqueued back to back with no host round trip (the state is device-resident, as in
 * yalm_generate_greedy) and ONE read-back at the end. Sequence s starts by feeding tokens[s] at
 * pos[s]; each step commits row s's first-maximum argmax (the rule of yalm_argmax) to sequence s,
 * which continues at (that token, pos + 1). out_tokens: host [n_seq][n_steps]. stats may be NULL.
 * A step is begin, per layer QKV / attention / Wo / W1|W3 / W2, norm + logits, commit.
 * YALM_ERR_ARG: pos[s] + n_steps > max_seq_len for any s (a batched step never wraps the ring or
 * rotates the sinks: the sliding window past max_seq_len stays with the single-sequence loops), a
 * token out of range, n_steps above the token buffer (65536). */
int yalm_batch_generate_greedy(yalm_batch b, const int *tokens, const int *pos, int n_steps, int *out_tokens,
                               yalm_batch_stats *stats);
/* The same with row s of step i drawn by the rule of yalm_generate_sampled with
 * uniforms[s * n_steps + i] (host, [n_seq][n_steps] values in [0, 1]); one workgroup per row, in
 * the commit launch's place. YALM_ERR_ARG: the greedy call's, and those of yalm_generate_sampled
 * (temperature, top_k, top_p, a uniform outside [0, 1], a vocabulary above 131072). */
int yalm_batch_generate_sampled(yalm_batch b, const int *tokens, const int *pos, int n_steps, const yalm_sampling *s,
                                const float *uniforms, int *out_tokens, yalm_batch_stats *stats);
/* Every sequence's next (token, pos) after a sync: host arrays of n_seq, either may be NULL. */
int yalm_batch_state(yalm_batch b, int *tokens, int *pos);
/* Launch switch of one batch (default 0). YALM_BATCH_ATTN_PER_SEQ: one attention launch per
 * sequence (the decode kernel, as the verify step of yalm_generate_speculative runs it) where the
 * single launch for all sequences would run. Both forms give the same bits (A/B runs and tests). */
#define YALM_BATCH_ATTN_PER_SEQ 1
int yalm_batch_set_launch(yalm_batch b, int flags);
/* Test hook: the device pointers of sequence seq's K and V cache of `layer` and of its token buffer
 * (each may be NULL). Every one of these buffers has YALM_BATCH_GUARD_BYTES bytes of 0xA5 directly
 * before it and directly after its last byte, which nothing ever writes. */
#define YALM_BATCH_GUARD_BYTES 256
int yalm_batch_buffers(yalm_batch b, int seq, int layer, uint16_t **kcache, uint16_t **vcache, int **tokens);

/* ---------------- test API: replaces infer.cu:890-1019 (model.h:370-384) ---------------- */
/* Host pointers in and out; synchronous. dtype selects the weight type
 * (matmul_cuda<float|half|uint8_t>; YALM_Q4 / YALM_E4M3: w is d rows of yalm_row_bytes(dtype, n)). */
int yalm_matmul(float *xout, const float *x, const void *w, int n, int d, int dtype);
/* The geometry of one multi-row GEMV launch (gemv_rows.h: every weight matrix of yalm_forward_rows
 * and of the speculative verify step) over rows of n elements, n_groups wave groups (pairs of
 * output rows; GLU: one w1 / w3 row pair each) and T = 1..4 activation rows on `cus` CUs (0 =
 * this device's): kseg floats of x staged per row and segment (a whole number of the type's
 * 64-lane chunks, T * kseg * 4 <= 128 KiB), nseg segments, gpw groups per wave (1 when
 * segmented), the grid and the dynamic LDS bytes. Pure host arithmetic with cus > 0; outputs may
 * be NULL. YALM_ERR_UNSUPPORTED for YALM_Q4. */
int yalm_rows_plan(int dtype, int n, int n_groups, int T, int cus, int *kseg, int *nseg, int *gpw, int *blocks,
                   size_t *lds);
/* One multi-row GEMV launch, the decoder's own, at the plan of yalm_rows_plan: x [T][xstride]
 * (row t's n elements first), w d rows of n elements, out [T][ostride], uploaded as given and
 * returned whole (what the kernel does not write comes back as it went in). normw (n floats)
 * non-NULL: each x row is rmsnorm'ed with eps while it is staged. epilogue YALM_ROWS_STORE: out[t][j] =
 * w[j] . x[t]; YALM_ROWS_RESIDUAL: out[t][j] += w[j] . x[t]; YALM_ROWS_GLU: out[t][j] =
 * act(w[j] . x[t]) * (w3[j] . x[t]) (w3 and act are ignored otherwise). YALM_ERR_ARG: T outside
 * 1..4, n no multiple of 16, a stride below its row's length or no multiple of 4;
 * YALM_ERR_UNSUPPORTED for YALM_Q4. */
#define YALM_ROWS_STORE 0
#define YALM_ROWS_RESIDUAL 1
#define YALM_ROWS_GLU 2
int yalm_matmul_rows(float *out, const float *x, const void *w, const void *w3, const float *normw, float eps, int T,
                     int n, int d, int xstride, int ostride, int dtype, int epilogue, int act);
/* The geometry of one single-row (decode) GEMV launch, as the launcher itself computes it: over
 * n_groups wave groups of rows of n elements, for the epilogue `policy`, with (norm != 0) or without
 * the rmsnorm of x. kind 0..4 (QKV, Wo, W1|W3, W2, logits) selects the default {threads, unroll,
 * workgroups per CU} of the weight type; threads / unroll / wpc != 0 override it as
 * yalm_set_gemv_config does. cus: the CUs the grid is sized for (0 = this device's; pure host
 * arithmetic otherwise). rows: -1 = whole-row mode where the policy has it and the rows divide,
 * 0 = chunk order. A row that is no whole number of 64-lane chunks takes the generic kernel
 * (generic = 1: 256 threads, one group per wave; threads / unroll / wpc / cus / rows are ignored). */
#define YALM_GEMV_STORE1 0   /* out[i] = w[i] . x */
#define YALM_GEMV_STORE2 1   /* the same, two rows per group (even vocabularies) */
#define YALM_GEMV_RESIDUAL 2 /* out[i] += w[i] . x */
#define YALM_GEMV_ADDTO 3    /* out[i] = base[i] + w[i] . x */
#define YALM_GEMV_GLU 4      /* out[i] = act(w[i] . x) * (w3[i] . x) */
#define YALM_GEMV_QKV 5      /* clip, RoPE, q to q_out, K / V rows of the cache, sink rotation */
#define YALM_GEMV_QKVB 6     /* ... with a bias ahead of the clip */
#define YALM_GEMV_QKVN 7     /* ... q and k clipped and stored raw (ahead of the q / k norm launch) */
typedef struct {
	int generic;          /* 1: gemv_kernel, 0: gemv_rb_kernel */
	int threads, unroll;  /* block size, loads in flight per lane */
	int nb;               /* grid */
	int rows;             /* 1: whole-row mode */
	int ngl_min, ngl_max; /* groups of a workgroup: the fewest and the most */
	int xregs;            /* 1: x (and the norm weights) are loaded ahead of the weight stream */
	size_t lds;           /* dynamic LDS bytes */
} yalm_gemv_geometry;
int yalm_gemv_plan(int dtype, int policy, int kind, int n, int n_groups, int norm, int threads, int unroll, int wpc,
                   int cus, int rows, yalm_gemv_geometry *out);
/* One single-row GEMV launch, the decoder's own (the launcher the forward pass calls, at the plan of
 * yalm_gemv_plan), on host arrays, synchronous. x: n floats; normw: n floats when norm != 0 (x is
 * rmsnorm'ed with eps while it is staged). Store / residual / addto / GLU: w (and w3) are d rows,
 * out holds out_len >= d floats, base d floats. The QKV policies: wq is n_heads * head_dim rows, wk
 * and wv n_kv_heads * head_dim; rope and rope_sink are head_dim floats each, the (cos, sin) pairs
 * of this step and of the sinks' one-position rotation; kcache / vcache are cache_rows rows of
 * n_kv_heads * head_dim f16; q_out holds q_len floats, raw raw_len (QKVN), bq / bk / bv the
 * biases (QKVB). The step's `pos` is set to another cache row than kv_pos ((kv_pos + 1) %
 * cache_rows), so a row stored at pos shows. Everything the launch may write (out, q_out, raw, kcache, vcache) is uploaded as
 * given and returned whole: what the kernel does not write comes back as it went in.
 * YALM_ERR_ARG: n no multiple of 16 (q4: of 32), head_dim odd or above 256, odd q or kv dims,
 * cache_rows below 2 or at most kv_pos, kv_sink above kv_pos, a normalising PAddTo. */
typedef struct {
	int dtype, policy, kind;
	int n, d; /* row length; output rows (not the QKV policies) */
	int norm, act;
	float eps;
	int threads, unroll, wpc, cus, rows; /* as yalm_gemv_plan */
	const float *x, *normw;
	const void *w, *w3, *wq, *wk, *wv;
	float *out;
	const float *base;
	int out_len;
	int n_heads, n_kv_heads, head_dim, kv_sink, kv_pos, cache_rows;
	float qkv_clip;
	const float *rope, *rope_sink;
	uint16_t *kcache, *vcache;
	float *q_out, *raw;
	int q_len, raw_len;
	const float *bq, *bk, *bv;
} yalm_gemv_args;
int yalm_gemv_one(const yalm_gemv_args *args);
/* mha_cuda: xout (n_heads, head_dim), att (n_heads, max_seq_len) softmax
 * probabilities for t < kv_len. */
int yalm_mha(float *xout, float *att, const uint16_t *kb, const uint16_t *vb, const float *q, int head_dim, int kv_len,
             int max_seq_len, int n_heads, int n_kv_heads);
/* ffn_cuda: xout = W2 (act(W1 x) * W3 x). */
int yalm_ffn(float *xout, const float *x, const void *w1, const void *w2, const void *w3, int hidden_dim, int dim,
             int act, int dtype);

/* The MoE FFN of one block without the norm and the residual (host pointers,
 * synchronous): the router on x, then xout = sum_k weight_k * W2[e_k] (act(W1[e_k] x) *
 * W3[e_k] x) through the decoder's kernels; experts / weights (n_active each, may be
 * NULL) receive the routing. */
int yalm_moe_ffn(float *xout, int *experts, float *weights, const float *x, const void *moegate, const void *w1,
                 const void *w2, const void *w3, int n_experts, int n_active, int hidden_dim, int dim, int act,
                 int dtype);

/* Device greedy sampling (sampler.cpp:27-38 sample_argmax: strict '>' scan, the
 * FIRST maximum wins, 0 when nothing exceeds -FLT_MAX): *out = argmax of n host
 * logits through argmax_kernel, the kernel of the -t 0 decode loop. n_shards > 1
 * runs the tensor-parallel form instead: one per-shard first max as a (value,
 * global index) pair over each n / n_shards slice, then argmax_pick_kernel. */
int yalm_argmax(const float *logits, int n, int n_shards, int *out);

/* Device sampling test hook (host pointers, synchronous): n_draws draws from the n <= 131072
 * logits by the rule of yalm_generate_sampled, one launch of its kernel per draw, draw i with
 * uniforms[i]. kept (n_draws, may be NULL): the kept-set size of each draw; weights_out (n,
 * may be NULL): the q_i the kernel used. */
int yalm_sample(const float *logits, int n, const yalm_sampling *s, const float *uniforms, int n_draws,
                int *out_tokens, int *kept, uint64_t *weights_out);

/* Prefill building blocks (host pointers, synchronous):
 * c[M][N] f32 = a[M][K] f16 · w[N][K]^T f16 (the MFMA GEMM; N % 128 == 0, K % 64 == 0). */
int yalm_gemm_f16(float *c, const uint16_t *a, const uint16_t *w, int M, int N, int K);
/* The grouped GEMM of the mixture-of-experts prefill: c[r] = a[r] . w[expert_of_row[r]]^T,
 * w (E, N, K) f16, through the device grouping pass, the M-tile table and the grouped tile
 * kernels (plain store in slot order, scattered back to row order); follows the forms of
 * yalm_set_prefill_forms(NULL, ...). */
int yalm_moe_gemm_f16(float *c, const uint16_t *a, const uint16_t *w, const int *expert_of_row, int M, int N, int K,
                      int E);
/* The batched router and the whole grouped expert FFN on T already-normalised rows x
 * [T][dim] f32 (no norm, no residual): xout [T][dim], experts / weights [T][n_active] (may
 * be NULL). f16 or fp8 (E5M2) weights, dims multiples of 128. */
int yalm_moe_ffn_rows(float *xout, int *experts, float *weights, const float *x, int T, const void *moegate,
                      const void *w1, const void *w2, const void *w3, int n_experts, int n_active, int hidden_dim,
                      int dim, int act, int dtype);
/* Causal GQA attention of T query rows at positions pos0 .. pos0 + T - 1:
 * q [T][n_heads * head_dim] f16, kc / vc [pos0 + T][n_kv_heads * head_dim] f16,
 * o [T][n_heads * head_dim] f16 (infer.cpp:216-248 per row and head). */
int yalm_attn_prefill(uint16_t *o, const uint16_t *q, const uint16_t *kc, const uint16_t *vc, int T, int pos0,
                      int n_heads, int n_kv_heads, int head_dim);
/* The same launch as a decoder's prefill makes, with the buffers a decoder has around it:
 * kc / vc are [cache_rows][n_kv_heads * head_dim] with cache_rows >= pos0 + T (rows past
 * pos0 + T are stale cache the kernel must not read), o is [o_rows][W] with o_rows >= T; its
 * incoming content is uploaded first and all o_rows rows come back (rows past T must return
 * untouched). W = n_heads * head_dim, or twice that when split != 0: the split-operand form,
 * q is [T][W] too, and the rows of q and o are f16 [hi | lo] halves. YALM_ERR_ARG on a bad
 * argument. */
int yalm_attn_prefill_rows(uint16_t *o, int o_rows, const uint16_t *q, const uint16_t *kc, const uint16_t *vc,
                           int cache_rows, int T, int pos0, int n_heads, int n_kv_heads, int head_dim, int split);

#ifdef __cplusplus
}
#endif
#endif
