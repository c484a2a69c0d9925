#include "model.h"

#include <cstdlib>

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <iostream>

namespace yalm {

void check(int rc, const char *what) {
	if (rc != YALM_OK)
		throw YalmRuntimeError(std::string(what) + ": " + yalm_last_error());
}

static int meta_int(const Json &md, const char *k) {
	return std::stoi(md.at(k).as_string());
}

void Config::from_yalm(YALMData &yalm, int context) {
	const Json &md = yalm.metadata;
	dim = meta_int(md, "dim");
	hidden_dim = meta_int(md, "hidden_dim");
	head_dim = meta_int(md, "head_dim");
	n_layers = meta_int(md, "n_layers");
	n_heads = meta_int(md, "n_heads");
	n_kv_heads = meta_int(md, "n_kv_heads");
	vocab_size = meta_int(md, "vocab_size");
	n_experts = md.contains("n_experts") ? meta_int(md, "n_experts") : 0;
	n_experts_active = md.contains("n_experts_active") ? meta_int(md, "n_experts_active") : 0;
	max_seq_len = std::min(meta_int(md, "max_seq_len"), 4096);
	if (context)
		max_seq_len = context;
	rope_theta = std::stof(md.at("rope_theta").as_string());
	rotary_dim = meta_int(md, "rotary_dim");
	norm_eps = std::stof(md.value("norm_eps", "1e-5"));
	const std::string act_str = md.value("act_type", "gelu");
	if (act_str == "gelu") {
		act = ActivationType::GELU;
	} else if (act_str == "silu") {
		act = ActivationType::SILU;
	} else {
		std::cerr << "unsupported act_type, defaulting to gelu" << std::endl;
		act = ActivationType::GELU;
	}
	if (md.value("norm_type", "rmsnorm") != "rmsnorm")
		std::cerr << "unsupported norm_type, defaulting to rmsnorm" << std::endl;
	norm_type = LayerNormType::RMSNorm;
	qkv_clip = md.contains("qkv_clip") ? std::stof(md.at("qkv_clip").as_string()) : FLT_MAX;
	const std::string dtype = md.at("dtype").as_string();
	if (dtype == "fp32")
		weight_dtype = DType::F32;
	else if (dtype == "fp16")
		weight_dtype = DType::F16;
	else if (dtype == "fp8")
		weight_dtype = DType::F8E5M2;
	else if (dtype == "q4")
		weight_dtype = DType::Q4;
	else if (dtype == "e4m3")
		weight_dtype = DType::E4M3;
	else
		throw std::runtime_error("FATAL: unsupported dtype: " + dtype);
	if (n_experts > 0 && !(n_experts_active >= 1 && n_experts_active <= n_experts && n_experts <= 64))
		throw std::runtime_error("FATAL: mixture of experts needs 1 <= n_experts_active <= n_experts <= 64");
	if (weight_dtype == DType::Q4 && n_experts > 0)
		throw std::runtime_error("FATAL: q4 weights have no mixture-of-experts form");
	if (weight_dtype == DType::E4M3 && n_experts > 0)
		throw std::runtime_error("FATAL: e4m3 weights have no mixture-of-experts form");
	const std::string qb = md.value("qkv_bias", "0");
	qkv_bias = !(qb.empty() || qb == "0" || qb == "False" || qb == "false");
	if (qkv_bias && n_experts > 0)
		throw std::runtime_error("FATAL: a q / k / v bias has no mixture-of-experts form");
	const std::string qn = md.value("qk_norm", "0");
	qk_norm = !(qn.empty() || qn == "0" || qn == "False" || qn == "false");
	if (qk_norm && n_experts > 0)
		throw std::runtime_error("FATAL: the q / k norm has no mixture-of-experts form");
	if (qk_norm && qkv_bias)
		throw std::runtime_error("FATAL: the q / k norm does not run together with a q / k / v bias");
	rope_scaling = yalm_rope_scaling{};
	if (md.contains("rope_scaling_type")) {
		if (md.at("rope_scaling_type").as_string() != "llama3")
			throw std::runtime_error("FATAL: unsupported rope_scaling_type: " + md.at("rope_scaling_type").as_string());
		rope_scaling.type = 1;
		rope_scaling.factor = std::stof(md.at("rope_scaling_factor").as_string());
		rope_scaling.low_freq_factor = std::stof(md.at("rope_low_freq_factor").as_string());
		rope_scaling.high_freq_factor = std::stof(md.at("rope_high_freq_factor").as_string());
		rope_scaling.original_max_position = meta_int(md, "rope_original_max_position");
	}
	if (weight_dtype == DType::Q4 && (dim % 32 || hidden_dim % 32 || (n_heads * head_dim) % 32))
		throw std::runtime_error("FATAL: q4 needs dim, hidden_dim and n_heads * head_dim multiples of 32");
}

// the C ABI's code of a weight dtype (the reference's enum order, but q4 and e4m3)
static int dtype_code(DType dt) {
	return dt == DType::Q4 ? YALM_Q4 : dt == DType::E4M3 ? YALM_E4M3 : (int)dt;
}

// bytes of one row of n weights (q4: nibble blocks + scales + padding; e4m3: codes + scale + padding)
static size_t weight_row_bytes(DType dt, size_t n) {
	return yalm_row_bytes(dtype_code(dt), (int)n);
}

size_t Config::active_bytes(size_t pos) const {
	const size_t q_dim = (size_t)n_heads * head_dim;
	const size_t rb_dim = weight_row_bytes(weight_dtype, dim), rb_q = weight_row_bytes(weight_dtype, q_dim),
	             rb_h = weight_row_bytes(weight_dtype, hidden_dim);
	size_t per_block = 2 * dim * sizeof(float);
	per_block += q_dim * rb_dim;
	per_block += 2 * (size_t)n_kv_heads * head_dim * rb_dim;
	per_block += (size_t)dim * rb_q;
	if (qkv_bias)
		per_block += (q_dim + 2 * (size_t)n_kv_heads * head_dim) * sizeof(float);
	if (qk_norm)
		per_block += 2 * (size_t)head_dim * sizeof(float);
	if (n_experts > 0) { // model.cpp:85-87: the router and the active experts
		per_block += (size_t)n_experts * rb_dim;
		per_block += (size_t)n_experts_active * (2 * hidden_dim * rb_dim + dim * rb_h);
	} else {
		per_block += 2 * (size_t)hidden_dim * rb_dim + (size_t)dim * rb_h;
	}
	const size_t kv_len = std::min((size_t)max_seq_len, pos + 1);
	per_block += 2 * kv_len * n_kv_heads * head_dim * sizeof(f16_t);
	return rb_dim + n_layers * per_block + dim * sizeof(float) + (size_t)vocab_size * rb_dim;
}

yalm_config Config::to_c() const {
	yalm_config c{};
	c.dim = dim;
	c.hidden_dim = hidden_dim;
	c.head_dim = head_dim;
	c.n_layers = n_layers;
	c.n_heads = n_heads;
	c.n_kv_heads = n_kv_heads;
	c.vocab_size = vocab_size;
	c.max_seq_len = max_seq_len;
	c.rope_theta = rope_theta;
	c.rotary_dim = rotary_dim;
	c.norm_eps = norm_eps;
	c.act = act == ActivationType::SILU ? YALM_SILU : YALM_GELU;
	c.qkv_clip = qkv_clip;
	c.weight_dtype = dtype_code(weight_dtype);
	return c;
}

// model.cpp:104-132
static const void *check_tensor(const Tensor *t, DType dt, std::array<int, 4> shape) {
	if (!t)
		throw std::runtime_error("FATAL: missing tensor");
	if (t->dtype != dt || t->shape != shape)
		throw std::runtime_error("FATAL: tensor mismatch for " + t->name + " (got " + dtype_to_string(t->dtype) +
		                         ", expected " + dtype_to_string(dt) + ")");
	return t->data;
}

// a weight matrix [rows][n] in the model's weight dtype; q4 / e4m3: a U8 tensor [rows, row bytes]
static const void *check_weight(const Tensor *t, DType dt, int rows, int n) {
	if (dt == DType::Q4 || dt == DType::E4M3)
		return check_tensor(t, DType::U8, {rows, (int)weight_row_bytes(dt, n), 0, 0});
	return check_tensor(t, dt, {rows, n, 0, 0});
}

static const Tensor *get_tensor(const YALMData &y, const std::string &key) {
	auto it = y.tensors.find(key);
	if (it == y.tensors.end())
		throw std::runtime_error("FATAL: missing tensor: " + key);
	return &it->second;
}

InferenceState::InferenceState(std::shared_ptr<Config> config) : _config(std::move(config)) {
	_logits = new float[_config->vocab_size]();
}

InferenceState::~InferenceState() {
	if (_batch) // before the decoder it runs on
		yalm_batch_destroy(_batch);
	if (_decoder)
		yalm_decoder_destroy(_decoder);
	if (_device == Device::HIP)
		yalm_unregister_host(_logits);
	delete[] _logits;
}

void InferenceState::cuda() {
	if (_device != Device::CPU)
		return;
	_device = Device::HIP;
	// pinned logits so the OUTPUT copy is a straight DMA (model.cpp:338)
	check(yalm_register_host(_logits, sizeof(float) * _config->vocab_size), "register logits");
}

Block::Block(int layer_i, std::shared_ptr<Config> config, const Tensor *rms_att_weight, const Tensor *rms_ffn_weight,
             const Tensor *wq, const Tensor *wk, const Tensor *wv, const Tensor *wo, const Tensor *w1, const Tensor *w2,
             const Tensor *w3, const Tensor *moegate)
    : _layer_i(layer_i), _config(std::move(config)) {
	const Config &c = *_config;
	const DType dt = c.weight_dtype;
	_rms_att = check_tensor(rms_att_weight, DType::F32, {c.dim, 0, 0, 0});
	_rms_ffn = check_tensor(rms_ffn_weight, DType::F32, {c.dim, 0, 0, 0});
	_wq = check_weight(wq, dt, c.n_heads * c.head_dim, c.dim);
	_wk = check_weight(wk, dt, c.n_kv_heads * c.head_dim, c.dim);
	_wv = check_weight(wv, dt, c.n_kv_heads * c.head_dim, c.dim);
	_wo = check_weight(wo, dt, c.dim, c.n_heads * c.head_dim);
	if (c.n_experts > 0) { // model.cpp:160-164
		_moegate = check_tensor(moegate, dt, {c.n_experts, c.dim, 0, 0});
		_w1 = check_tensor(w1, dt, {c.n_experts, c.hidden_dim, c.dim, 0});
		_w2 = check_tensor(w2, dt, {c.n_experts, c.dim, c.hidden_dim, 0});
		_w3 = check_tensor(w3, dt, {c.n_experts, c.hidden_dim, c.dim, 0});
	} else {
		_w1 = check_weight(w1, dt, c.hidden_dim, c.dim);
		_w2 = check_weight(w2, dt, c.dim, c.hidden_dim);
		_w3 = check_weight(w3, dt, c.hidden_dim, c.dim);
	}
}

void Block::set_qkv_bias(const Tensor *bq, const Tensor *bk, const Tensor *bv) {
	const Config &c = *_config;
	_bias[0] = check_tensor(bq, DType::F32, {c.n_heads * c.head_dim, 0, 0, 0});
	_bias[1] = check_tensor(bk, DType::F32, {c.n_kv_heads * c.head_dim, 0, 0, 0});
	_bias[2] = check_tensor(bv, DType::F32, {c.n_kv_heads * c.head_dim, 0, 0, 0});
}

void Block::set_qk_norm(const Tensor *gq, const Tensor *gk) {
	const Config &c = *_config;
	_qk_norm[0] = check_tensor(gq, DType::F32, {c.head_dim, 0, 0, 0});
	_qk_norm[1] = check_tensor(gk, DType::F32, {c.head_dim, 0, 0, 0});
}

Block::~Block() {
	for (void *p : _owned)
		yalm_free(p);
}

static const void *upload(std::vector<void *> &owned, const void *host, size_t bytes) {
	void *d = yalm_upload(host, bytes);
	if (!d)
		throw YalmRuntimeError(std::string("upload: ") + yalm_last_error());
	owned.push_back(d);
	return d;
}

void Block::cuda() {
	if (_device != Device::CPU)
		return;
	const Config &c = *_config;
	const size_t q_dim = (size_t)c.n_heads * c.head_dim, kv_dim = (size_t)c.n_kv_heads * c.head_dim;
	const size_t rb_dim = weight_row_bytes(c.weight_dtype, c.dim), rb_q = weight_row_bytes(c.weight_dtype, q_dim),
	             rb_h = weight_row_bytes(c.weight_dtype, c.hidden_dim);
	_rms_att = upload(_owned, _rms_att, c.dim * sizeof(float));
	_rms_ffn = upload(_owned, _rms_ffn, c.dim * sizeof(float));
	_wq = upload(_owned, _wq, q_dim * rb_dim);
	_wk = upload(_owned, _wk, kv_dim * rb_dim);
	_wv = upload(_owned, _wv, kv_dim * rb_dim);
	_wo = upload(_owned, _wo, c.dim * rb_q);
	const size_t ne = c.n_experts > 0 ? c.n_experts : 1; // the whole expert stacks (the reference uploads none)
	_w1 = upload(_owned, _w1, ne * c.hidden_dim * rb_dim);
	_w2 = upload(_owned, _w2, ne * c.dim * rb_h);
	_w3 = upload(_owned, _w3, ne * c.hidden_dim * rb_dim);
	if (_moegate)
		_moegate = upload(_owned, _moegate, (size_t)c.n_experts * rb_dim);
	if (_bias[0]) {
		_bias[0] = upload(_owned, _bias[0], q_dim * sizeof(float));
		_bias[1] = upload(_owned, _bias[1], kv_dim * sizeof(float));
		_bias[2] = upload(_owned, _bias[2], kv_dim * sizeof(float));
	}
	if (_qk_norm[0]) {
		_qk_norm[0] = upload(_owned, _qk_norm[0], c.head_dim * sizeof(float));
		_qk_norm[1] = upload(_owned, _qk_norm[1], c.head_dim * sizeof(float));
	}
	_device = Device::HIP;
	// The KV cache is allocated (zeroed) by the decoder in HBM: no host copy
	// to upload (model.cpp:208-210 uploads a zero host array).
}

yalm_block_weights Block::device_weights() const {
	yalm_block_weights w{};
	w.rms_att = (const float *)_rms_att;
	w.rms_ffn = (const float *)_rms_ffn;
	w.wq = _wq;
	w.wk = _wk;
	w.wv = _wv;
	w.wo = _wo;
	w.w1 = _w1;
	w.w2 = _w2;
	w.w3 = _w3;
	return w;
}

Model::Model(YALMData &yalm, int context) {
	config = std::make_shared<Config>();
	config->from_yalm(yalm, context);
	std::cout << "loading model with dtype: " << dtype_to_string(config->weight_dtype) << std::endl;
	const Config &c = *config;
	token_embedding_table = check_weight(get_tensor(yalm, "model.embed.weight"), c.weight_dtype, c.vocab_size, c.dim);
	for (int i = 0; i < c.n_layers; ++i) {
		const std::string p = "model.layers." + std::to_string(i) + ".";
		blocks.emplace_back(std::make_shared<Block>(
		    i, config, get_tensor(yalm, p + "attn.norm.weight"), get_tensor(yalm, p + "mlp.norm.weight"),
		    get_tensor(yalm, p + "attn.wq.weight"), get_tensor(yalm, p + "attn.wk.weight"),
		    get_tensor(yalm, p + "attn.wv.weight"), get_tensor(yalm, p + "attn.wo.weight"),
		    get_tensor(yalm, p + "mlp.w1.weight"), get_tensor(yalm, p + "mlp.w2.weight"),
		    get_tensor(yalm, p + "mlp.w3.weight"), c.n_experts > 0 ? get_tensor(yalm, p + "moegate.weight") : nullptr));
		if (c.qkv_bias)
			blocks.back()->set_qkv_bias(get_tensor(yalm, p + "attn.wq.bias"), get_tensor(yalm, p + "attn.wk.bias"),
			                            get_tensor(yalm, p + "attn.wv.bias"));
		if (c.qk_norm)
			blocks.back()->set_qk_norm(get_tensor(yalm, p + "attn.q_norm.weight"), get_tensor(yalm, p + "attn.k_norm.weight"));
	}
	rms_final_weight = check_tensor(get_tensor(yalm, "model.norm.weight"), DType::F32, {c.dim, 0, 0, 0});
	_tied = yalm.tensors.count("model.output.weight") == 0;
	wcls = _tied ? token_embedding_table
	             : check_weight(get_tensor(yalm, "model.output.weight"), c.weight_dtype, c.vocab_size, c.dim);
}

Model::~Model() {
	blocks.clear();
	for (void *p : _owned)
		yalm_free(p);
}

void Model::cuda() {
	if (_device != Device::CPU)
		return;
	check(yalm_set_device(0), "set device");
	const Config &c = *config;
	const size_t emb_bytes = (size_t)c.vocab_size * weight_row_bytes(c.weight_dtype, c.dim);
	token_embedding_table = upload(_owned, token_embedding_table, emb_bytes);
	for (auto &b : blocks)
		b->cuda();
	rms_final_weight = upload(_owned, rms_final_weight, c.dim * sizeof(float));
	// tied classifier: alias the uploaded embedding (the reference uploads it twice, model.cpp:388/393)
	wcls = _tied ? token_embedding_table : upload(_owned, wcls, emb_bytes);
	_device = Device::HIP;
}

void Model::ensure_decoder(InferenceState &s, yalm_stream stream) {
	if (s.device() != _device)
		throw std::runtime_error("FATAL: inference state device mismatch");
	if (_device != Device::HIP)
		throw std::runtime_error("this engine runs on the HIP device only: call model.cuda(); state.cuda() "
		                         "(the CPU path is the reference's own -d cpu)");
	if (s._decoder)
		return;
	std::vector<yalm_block_weights> bw;
	for (auto &b : blocks)
		bw.push_back(b->device_weights());
	yalm_model_weights mw{token_embedding_table, (const float *)rms_final_weight, wcls, bw.data()};
	const yalm_config cc = config->to_c();
	if (config->n_experts > 0) {
		std::vector<const void *> gates;
		for (auto &b : blocks)
			gates.push_back(b->moegate());
		const yalm_moe_config mc{config->n_experts, config->n_experts_active};
		check(yalm_decoder_create_moe(&cc, &mc, &mw, gates.data(), stream, &s._decoder), "decoder create");
	} else {
		check(yalm_decoder_create(&cc, &mw, stream, &s._decoder), "decoder create");
	}
	if (config->rope_scaling.type)
		check(yalm_decoder_set_rope_scaling(s._decoder, &config->rope_scaling), "rope scaling");
	if (config->qkv_bias) {
		std::vector<const float *> b[3];
		for (auto &blk : blocks)
			for (int i = 0; i < 3; ++i)
				b[i].push_back(blk->bias(i));
		check(yalm_decoder_set_qkv_bias(s._decoder, b[0].data(), b[1].data(), b[2].data()), "qkv bias");
	}
	if (config->qk_norm) {
		std::vector<const float *> g[2];
		for (auto &blk : blocks)
			for (int i = 0; i < 2; ++i)
				g[i].push_back(blk->qk_norm(i));
		check(yalm_decoder_set_qk_norm(s._decoder, g[0].data(), g[1].data()), "q / k norm");
	}
}

void Model::forward(InferenceState &s, int token, int pos, InferenceMode mode) {
	ensure_decoder(s);
	s.set_mode(mode);
	check(yalm_forward(s._decoder, token, pos,
	                   mode == InferenceMode::OUTPUT_LOGITS ? YALM_OUTPUT_LOGITS : YALM_HYDRATE_KV_CACHE,
	                   mode == InferenceMode::OUTPUT_LOGITS ? s._logits : nullptr),
	      "forward");
}

bool Model::prefill(InferenceState &s, const int *tokens, int n, int pos0, float *logprobs, bool split) {
	const char *off = getenv("YALM_NO_PREFILL");
	if ((off && atoi(off) != 0) || n <= 0)
		return false;
	ensure_decoder(s);
	check(yalm_set_prefill_precision(s._decoder, split ? YALM_PREFILL_SPLIT : YALM_PREFILL_FAST), "prefill precision");
	const int r = yalm_prefill(s._decoder, tokens, n, pos0, logprobs);
	if (r == YALM_ERR_UNSUPPORTED)
		return false;
	check(r, "prefill");
	return true;
}

int Model::forward_greedy(InferenceState &s, int token, int pos) {
	ensure_decoder(s);
	int next = 0;
	check(yalm_generate_greedy(s._decoder, token, pos, 1, &next), "greedy step");
	return next;
}

void Model::generate_speculative(InferenceState &s, int token, int pos, int n, int rows, const int *context,
                                 int n_context, int *out, int *steps, int *accepted, int *plain) {
	ensure_decoder(s);
	const yalm_spec cfg{rows, 3, 1, nullptr, 0};
	yalm_spec_stats st{};
	check(yalm_generate_speculative(s._decoder, token, pos, n, &cfg, context, n_context, out, &st), "speculative steps");
	if (steps)
		*steps += st.spec_steps;
	if (accepted)
		*accepted += st.accepted_drafts;
	if (plain)
		*plain += st.plain_steps;
}

void Model::share_stream(InferenceState &s, const InferenceState &other) {
	if (s._decoder)
		throw std::runtime_error("share_stream: the inference state already has a decoder");
	if (!other._decoder)
		throw std::runtime_error("share_stream: the other inference state has no decoder yet (run a forward on it)");
	yalm_stream st = nullptr;
	check(yalm_decoder_get_stream(other._decoder, &st), "decoder stream");
	ensure_decoder(s, st);
}

void Model::generate_speculative_model(InferenceState &s, Model &draft, InferenceState &ds, int token, int pos, int n,
                                       int rows, float temperature, int top_k, float top_p, const float *uniforms,
                                       int *out, int *steps, int *accepted, int *plain) {
	ensure_decoder(s);
	draft.ensure_decoder(ds);
	const yalm_spec_model cfg{rows, nullptr, 0};
	const yalm_sampling sp{temperature, top_k, top_p};
	yalm_spec_stats st{};
	check(yalm_generate_speculative_model(s._decoder, ds._decoder, token, pos, n, &cfg, uniforms ? &sp : nullptr, uniforms,
	                                      out, &st),
	      "speculative steps with a draft model");
	if (steps)
		*steps += st.spec_steps;
	if (accepted)
		*accepted += st.accepted_drafts;
	if (plain)
		*plain += st.plain_steps;
}

void Model::generate_speculative_sampled(InferenceState &s, int token, int pos, int n, int rows, float temperature,
                                         int top_k, float top_p, const float *uniforms, const int *context,
                                         int n_context, int *out, int *steps, int *accepted, int *plain) {
	ensure_decoder(s);
	const yalm_spec cfg{rows, 3, 1, nullptr, 0};
	const yalm_sampling sp{temperature, top_k, top_p};
	yalm_spec_stats st{};
	check(yalm_generate_speculative_sampled(s._decoder, token, pos, n, &cfg, &sp, uniforms, context, n_context, out, &st),
	      "speculative sampled steps");
	if (steps)
		*steps += st.spec_steps;
	if (accepted)
		*accepted += st.accepted_drafts;
	if (plain)
		*plain += st.plain_steps;
}

void Model::generate_batch_sampled(InferenceState &s, int n_seq, int load, const int *tokens, const int *pos, int n,
                                   float temperature, int top_k, float top_p, const float *uniforms, int *out) {
	ensure_decoder(s);
	if (s._batch && s._batch_n != n_seq) {
		check(yalm_batch_destroy(s._batch), "batch destroy");
		s._batch = nullptr;
	}
	if (!s._batch) {
		check(yalm_batch_create(s._decoder, n_seq, &s._batch), "batch create");
		s._batch_n = n_seq;
	}
	if (load >= 0)
		check(yalm_batch_load(s._batch, -1, load), "batch load");
	const yalm_sampling sp{temperature, top_k, top_p};
	check(yalm_batch_generate_sampled(s._batch, tokens, pos, n, &sp, uniforms, out, nullptr), "batched sampled steps");
}

int Model::forward_sampled(InferenceState &s, int token, int pos, float temperature, int top_k, float top_p, float u) {
	ensure_decoder(s);
	const yalm_sampling sp{temperature, top_k, top_p};
	int next = 0;
	check(yalm_generate_sampled(s._decoder, token, pos, 1, &sp, &u, &next), "sampled step");
	return next;
}

} // namespace yalm
