// model.h — C++20 host API with the reference's shape (Config, InferenceState,
// Block, Model: /root/reference/src/model.h:41-327) over the MI355X engine's
// C ABI (include/yalm_hip.h). No HIP/CUDA types appear here: the reference
// leaked cudaStream_t / cudaGraph_t into this header (model.h:4, 39, 70-79);
// the device state lives behind the opaque yalm_decoder.
//
// Device::HIP replaces Device::CUDA. The CPU device is the reference's own
// infer.cpp path and is not part of this engine;
// forward() on a CPU-resident model raises.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/yalm_hip.h"
#include "codec.h"

namespace yalm {

constexpr int KV_SINKS = 2; // model.h:12

enum class ActivationType { GELU, SILU };
enum class LayerNormType { RMSNorm };
enum class Device { CPU, HIP };
enum class InferenceMode { HYDRATE_KV_CACHE, OUTPUT_LOGITS };

struct YalmRuntimeError : std::runtime_error {
	using std::runtime_error::runtime_error;
};
// Throws with yalm_last_error() when a C-ABI call fails.
void check(int rc, const char *what);

struct Config {
	int dim = 0, hidden_dim = 0, head_dim = 0, n_layers = 0, n_heads = 0, n_kv_heads = 0, vocab_size = 0,
	    max_seq_len = 0;
	float rope_theta = 10000.f;
	int rotary_dim = 0;
	float norm_eps = 1e-5f;
	ActivationType act = ActivationType::GELU;
	LayerNormType norm_type = LayerNormType::RMSNorm;
	float qkv_clip = 3.40282347e38f;
	int n_experts = 0, n_experts_active = 0;
	DType weight_dtype = DType::F16;
	// this engine's own metadata keys (absent: off): a q / k / v bias (Qwen2; tensors
	// attn.{wq,wk,wv}.bias, F32) and the Llama-3.1 / 3.2 "llama3" RoPE scaling
	bool qkv_bias = false;
	yalm_rope_scaling rope_scaling{};
	// ... and the per-head RMSNorm on q and k ahead of RoPE (Qwen3; tensors
	// attn.{q_norm,k_norm}.weight, F32 of head_dim)
	bool qk_norm = false;

	// model.cpp:17-75 (max_seq_len = min(meta, 4096) unless context != 0)
	void from_yalm(YALMData &yalm, int context = 0);
	// Algorithmic HBM bytes for one token at position pos (the
	// classifier counted at the weight dtype, unlike model.cpp:99's fp32).
	size_t active_bytes(size_t pos) const;
	yalm_config to_c() const;
};

struct InferenceState {
	explicit InferenceState(std::shared_ptr<Config> config);
	~InferenceState();
	InferenceState(const InferenceState &) = delete;
	InferenceState &operator=(const InferenceState &) = delete;

	float *logits() const {
		return _logits; // host memory, valid after an OUTPUT_LOGITS forward
	}
	void cuda(); // reference name (model.cpp:323); selects the HIP device
	void hip() {
		cuda();
	}
	Device device() const {
		return _device;
	}
	InferenceMode mode() const {
		return _mode;
	}
	void set_mode(InferenceMode m) {
		_mode = m;
	}
	yalm_decoder decoder() const {
		return _decoder;
	}

private:
	friend struct Model;
	std::shared_ptr<Config> _config;
	Device _device = Device::CPU;
	InferenceMode _mode = InferenceMode::OUTPUT_LOGITS;
	float *_logits = nullptr;
	yalm_decoder _decoder = nullptr;
	yalm_batch _batch = nullptr; // batched decode (Model::generate_batch_sampled), created on first use
	int _batch_n = 0;
};

struct Block {
	Block(int layer_i, std::shared_ptr<Config> config, const Tensor *rms_att_weight, const Tensor *rms_ffn_weight,
	      const Tensor *wq, const Tensor *wk, const Tensor *wv, const Tensor *wo, const Tensor *w1, const Tensor *w2,
	      const Tensor *w3, const Tensor *moegate);
	~Block();
	void cuda(); // device weight upload (model.cpp:185-211)
	yalm_block_weights device_weights() const;
	const void *moegate() const { return _moegate; } // (n_experts, dim) router weights, null when dense
	// the layer's q / k / v bias (Config::qkv_bias): checked F32 vectors, uploaded by cuda()
	void set_qkv_bias(const Tensor *bq, const Tensor *bk, const Tensor *bv);
	const float *bias(int i) const { return (const float *)_bias[i]; } // 0 q, 1 k, 2 v; null without a bias
	// the layer's q / k norm weights (Config::qk_norm): checked F32 vectors of head_dim, uploaded by cuda()
	void set_qk_norm(const Tensor *gq, const Tensor *gk);
	const float *qk_norm(int i) const { return (const float *)_qk_norm[i]; } // 0 q, 1 k; null without the norm

private:
	int _layer_i = 0;
	std::shared_ptr<Config> _config;
	Device _device = Device::CPU;
	const void *_rms_att = nullptr, *_rms_ffn = nullptr;
	const void *_wq = nullptr, *_wk = nullptr, *_wv = nullptr, *_wo = nullptr, *_w1 = nullptr, *_w2 = nullptr,
	           *_w3 = nullptr;
	const void *_bias[3] = {nullptr, nullptr, nullptr};
	const void *_qk_norm[2] = {nullptr, nullptr};
	const void *_moegate = nullptr; // with experts, _w1 / _w2 / _w3 are the stacked (n_experts, ...) tensors
	std::vector<void *> _owned;
};

struct Model {
	std::shared_ptr<Config> config;
	std::vector<std::shared_ptr<Block>> blocks;
	const void *token_embedding_table = nullptr;
	const void *rms_final_weight = nullptr;
	const void *wcls = nullptr;

	Model(YALMData &yalm, int context = 0);
	~Model();
	Model(const Model &) = delete;
	Model &operator=(const Model &) = delete;

	// Model::forward (model.cpp:396-407). OUTPUT_LOGITS leaves logits in s.logits().
	void forward(InferenceState &s, int token, int pos, InferenceMode mode = InferenceMode::OUTPUT_LOGITS);
	// Greedy (-t 0) step on the device: forward + first-max argmax without
	// copying logits to the host. Returns the next token.
	int forward_greedy(InferenceState &s, int token, int pos);
	// Sampled step on the device (yalm_generate_sampled, one step): forward, then temperature /
	// top-k (0 = off) / top-p (1 = off) sampling of the logits with the uniform u in [0, 1];
	// only the token comes back. Returns the next token.
	int forward_sampled(InferenceState &s, int token, int pos, float temperature, int top_k, float top_p, float u);
	// n greedy tokens by speculative steps of `rows` rows (yalm_generate_speculative, n-gram
	// drafts of 3 down to 1 tokens from `context`, which ends with `token`): the tokens of
	// forward_greedy, several per pass over the weights where the drafts hit. steps / accepted /
	// plain (may be null) are incremented by the call's counts.
	void generate_speculative(InferenceState &s, int token, int pos, int n, int rows, const int *context, int n_context,
	                          int *out, int *steps, int *accepted, int *plain);
	// The same with every row drawn on the device (yalm_generate_speculative_sampled): the tokens
	// of forward_sampled step by step with uniforms[j] for token j (n of them, each in [0, 1]).
	void generate_speculative_sampled(InferenceState &s, int token, int pos, int n, int rows, float temperature,
	                                  int top_k, float top_p, const float *uniforms, const int *context, int n_context,
	                                  int *out, int *steps, int *accepted, int *plain);
	// Speculative steps whose drafts come from a second, smaller model (yalm_generate_speculative_model):
	// `draft` / `ds` propose a token at every row. uniforms == nullptr: greedy, the tokens of
	// generate_speculative; else n uniforms, the tokens of generate_speculative_sampled. ds's decoder
	// must sit on s's stream (draft.share_stream(ds, s) before anything else runs on ds), and the
	// caller hydrates positions [0, pos) on both states.
	void generate_speculative_model(InferenceState &s, Model &draft, InferenceState &ds, int token, int pos, int n,
	                                int rows, float temperature, int top_k, float top_p, const float *uniforms, int *out,
	                                int *steps, int *accepted, int *plain);
	// Creates s's decoder (for this model) on the stream of `other`'s decoder, which must exist
	// (any forward on it creates it) and outlive s. Throws if s already has a decoder.
	void share_stream(InferenceState &s, const InferenceState &other);
	// n_seq completions side by side (yalm_batch_generate_sampled: one pass over the weights per
	// step for all of them). load >= 0: first copy KV rows [0, load) of the state's own cache into
	// every sequence (the prompt, hydrated once by forward / prefill). Sequence q feeds tokens[q] at
	// pos[q] and draws step i with uniforms[q * n + i]; out is [n_seq][n]. A later call with load
	// < 0 continues the same sequences. Dense models on one GPU, not q4 (yalm_batch_create).
	void generate_batch_sampled(InferenceState &s, int n_seq, int load, const int *tokens, const int *pos, int n,
	                            float temperature, int top_k, float top_p, const float *uniforms, int *out);
	// Batched MFMA prefill of tokens[0..n) at positions pos0.. (yalm_prefill):
	// fills the KV cache; logprobs (may be null) gets log p(tokens[i+1]) per
	// position; split: the split-operand precision form (yalm_set_prefill_precision).
	// Mixture-of-experts models take the same call (the grouped expert FFN, moe_prefill.h).
	// Returns false when this model's shape/dtype has no prefill path (f16 / fp8 / q4 / e4m3
	// weights, dims multiple of 128, head_dim 64|128), its activations leave the
	// prefill's f16 operand range, or YALM_NO_PREFILL=1; the caller then runs the
	// per-position forward.
	bool prefill(InferenceState &s, const int *tokens, int n, int pos0, float *logprobs, bool split = false);
	void cuda(); // Model::cuda (model.cpp:380-394)
	void hip() {
		cuda();
	}
	Device device() const {
		return _device;
	}

private:
	void ensure_decoder(InferenceState &s, yalm_stream stream = nullptr);
	Device _device = Device::CPU;
	bool _tied = false;
	std::vector<void *> _owned;
};

} // namespace yalm
