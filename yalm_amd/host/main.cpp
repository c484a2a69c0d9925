// main.cpp — yalm-compatible CLI over the MI355X engine (flags and modes of
// /root/reference/src/main.cpp:17-428): completion, perplexity and passkey,
// -d device switch (cpu | cuda | hip prefixes), -m -n -t -i -f -T -l.
// -t 0 runs the greedy loop with the argmax on the device; -k / -p (top-k, top-p) select
// device sampling for -t > 0: only the token comes back per step. -s <rows> runs the greedy
// (-t 0) or the device-sampled (-t > 0 with -k / -p) completion by speculative steps of 2..4
// rows with n-gram drafts from the prompt and the output so far: the same tokens, several per
// pass over the weights where drafts hit. -D <draft checkpoint> (with -s) takes the drafts from a
// second, smaller model of the same family instead: it proposes a token at every row.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>

#include "model.h"
#include "sampler.h"
#include "tokenizer.h"

using namespace yalm;

static uint64_t now_ms() {
	return (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
	           std::chrono::system_clock::now().time_since_epoch())
	    .count();
}

[[noreturn]] static void error_usage() {
	fprintf(stderr, "Usage:   yalm <checkpoint> [options]\n");
	fprintf(stderr, "Example: yalm model.yalm -i \"Q: What is the meaning of life?\"\n");
	fprintf(stderr, "Options:\n");
	fprintf(stderr, "  -h Display this help message\n");
	fprintf(stderr, "  -d [cpu,cuda,hip] which device to use (default - hip; cuda is an alias)\n");
	fprintf(stderr, "  -m [completion,passkey,perplexity] which mode to run in (default - completion)\n");
	fprintf(stderr, "  -T <int> sliding window context length (0 - max)\n");
	fprintf(stderr, "\nPerplexity mode options:\n  Choose one:\n    -i <string> input prompt\n");
	fprintf(stderr, "    -f <filepath> input file with prompt\n");
	fprintf(stderr, "Completion mode options:\n");
	fprintf(stderr, "  -n <int>    number of steps to run for in completion mode, default 256. 0 = max_seq_len, "
	                "-1 = infinite\n");
	fprintf(stderr, "  -t <float> temperature (default - 1.0)\n");
	fprintf(stderr, "  -k <int>   top-k: sample among the k most likely tokens (0 - off); samples on the device\n");
	fprintf(stderr, "  -p <float> top-p: sample from the smallest set of most likely tokens whose probability\n"
	                "             reaches p, in (0, 1] (1 - off); samples on the device\n");
	fprintf(stderr, "  -s <int>   speculative decode with this many rows per step, 2..4 (0 - off, the default);\n"
	                "             needs -t 0 (greedy), or -t > 0 with -k or -p (sampled on the device: the\n"
	                "             same tokens as without -s)\n");
	fprintf(stderr, "  -D <path>  draft model checkpoint for -s: a smaller model of the same family (loaded with the\n"
	                "             same -T) proposes every row's draft in place of the n-gram lookup; needs -s\n");
	fprintf(stderr, "  -N <int>   completions of one prompt decoded together, 2..4 (0 - off, the default): one pass\n"
	                "             over the weights per step for all of them; needs -t > 0 with -k or -p (greedy\n"
	                "             completions would be identical); not with -s\n");
	fprintf(stderr, "  Choose one:\n    -i <string> input prompt\n    -f <filepath> input file with prompt\n");
	fprintf(stderr, "Passkey mode options:\n  -n <int>    number of junk lines to insert (default - 250)\n");
	fprintf(stderr, "  -l <int>    passkey position (-1 - random)\n");
	exit(1);
}

static bool print_token_ids() {
	const char *e = getenv("YALM_PRINT_TOKENS");
	return e && atoi(e) != 0;
}

// The sampler's seed: the clock, as the reference (main.cpp constructs Sampler(config,
// get_timestamp_ms())); YALM_SEED fixes it for reproducible runs (tests: the passkey
// value and position come from std::rand after Sampler's srand).
static uint64_t sampler_seed() {
	const char *e = getenv("YALM_SEED");
	return e ? strtoull(e, nullptr, 10) : now_ms();
}

static void setup_device(const std::string &device, Model &model, InferenceState &state) {
	if (device == "cpu") {
		fprintf(stderr, "error: -d cpu is the reference's own CPU backend (src/infer.cpp); this engine implements "
		                "the MI355X device path only. Use -d hip (or cuda).\n");
		exit(1);
	}
	std::cout << "Using HIP (MI355X)" << std::endl;
	model.cuda();
	state.cuda();
}

static std::vector<int> encode_prompt(const Tokenizer &tok, const std::string &prompt, bool show) {
	const uint64_t t0 = now_ms();
	std::vector<int> enc = tok.encode(prompt, true);
	const double s = (now_ms() - t0) / 1000.0;
	if (show)
		std::cout << tok.encoding_to_debug_string(enc) << std::endl;
	printf("Encoding stats: (%zu tokens, throughput: %.5gtok/s, latency: %.5gs/tok, total: %.5gs)\n\n", enc.size(),
	       enc.size() / s, s / enc.size(), s);
	return enc;
}

static void run_completion(const std::string &path, const std::string &device, const std::string &prompt,
                           int context, int num_steps, float temperature, bool device_sampling, int top_k,
                           float top_p, int spec_rows, int n_completions, const std::string &draft_path) {
	YALMData data;
	if (data.from_file(path) != 0) {
		fprintf(stderr, "error: cannot load %s\n", path.c_str());
		exit(1);
	}
	Model model(data, context);
	InferenceState state(model.config);
	Sampler sampler(model.config, sampler_seed());
	Tokenizer tokenizer(data);
	std::cout << "Model active bytes with full context window: " << model.config->active_bytes(model.config->max_seq_len)
	          << std::endl;
	if (num_steps == 0)
		num_steps = model.config->max_seq_len;
	setup_device(device, model, state);
	model.forward(state, 0, 0); // warm-up: captures the graph, touches all weights

	std::vector<int> encoding = encode_prompt(tokenizer, prompt, true);
	const bool greedy = temperature == 0.0f;
	// -k / -p: the token is drawn on the device (Model::forward_sampled) from one
	// std::rand() / (float)RAND_MAX per generated token, the stream Sampler's constructor seeded
	const bool sampled = device_sampling && !greedy;
	auto uniform = [] { return std::rand() / (float)RAND_MAX; };
	const uint64_t start = now_ms();
	size_t read_bytes = 0;
	int next = 0;
	// hydrate all but the last prompt token in one batched prefill when the
	// model has that path (yalm_prefill) and there are at least 3 of them (one or
	// two positions are as fast as per-token forwards: profiles/r4m_delay_prefill.txt); the
	// last token goes through the per-token forward, which produces its logits /
	// greedy argmax
	size_t first = 0;
	if (encoding.size() >= 4 && (int)encoding.size() - 1 <= model.config->max_seq_len &&
	    model.prefill(state, encoding.data(), (int)encoding.size() - 1, 0, nullptr)) {
		first = encoding.size() - 1;
		for (size_t pos = 0; pos < first; ++pos)
			read_bytes += model.config->active_bytes(pos);
	}
	// -D: the draft model, its decoder on the target's stream, hydrated with the same prompt
	// (declared after the target's state: it is destroyed first, while the stream still exists)
	YALMData draft_data;
	std::unique_ptr<Model> draft_model;
	std::unique_ptr<InferenceState> draft_state;
	if (!draft_path.empty()) {
		if (draft_data.from_file(draft_path) != 0) {
			fprintf(stderr, "error: cannot load %s\n", draft_path.c_str());
			exit(1);
		}
		draft_model = std::make_unique<Model>(draft_data, context);
		draft_state = std::make_unique<InferenceState>(draft_model->config);
		draft_model->cuda();
		draft_state->cuda();
		draft_model->share_stream(*draft_state, state);
		const int dv = draft_model->config->vocab_size;
		if (dv != model.config->vocab_size)
			fprintf(stderr, "[yalm] note: the draft's vocabulary (%d) differs from the model's (%d); tokens one of them "
			                "lacks are never drafted\n", dv, model.config->vocab_size);
		std::vector<int> fed(encoding.begin(), encoding.end() - 1); // a token the draft lacks is fed as token 0
		for (int &t : fed)
			t = t < dv ? t : 0;
		if (!(fed.size() >= 3 && (int)fed.size() <= draft_model->config->max_seq_len &&
		      draft_model->prefill(*draft_state, fed.data(), (int)fed.size(), 0, nullptr)))
			for (size_t pos = 0; pos < fed.size(); ++pos)
				draft_model->forward(*draft_state, fed[pos], (int)pos, InferenceMode::HYDRATE_KV_CACHE);
	}
	// YALM_SEED (tests): re-seeded before the first draw, as in run_passkey, because the HIP
	// runtime's initialisation above draws from std::rand too
	if (sampled && getenv("YALM_SEED"))
		std::srand((unsigned)sampler_seed());
	for (size_t pos = first; pos < encoding.size(); ++pos) {
		const bool last = pos + 1 == encoding.size();
		if (last && (spec_rows > 0 || n_completions > 0))
			break; // the speculative / batched loop below feeds the last prompt token itself
		if (last && greedy)
			next = model.forward_greedy(state, encoding[pos], (int)pos);
		else if (last && sampled)
			next = model.forward_sampled(state, encoding[pos], (int)pos, temperature, top_k, top_p, uniform());
		else
			model.forward(state, encoding[pos], (int)pos,
			              last ? InferenceMode::OUTPUT_LOGITS : InferenceMode::HYDRATE_KV_CACHE);
		read_bytes += model.config->active_bytes(pos);
	}
	const uint64_t end_hydrate = now_ms();
	std::string ids;
	int spec_steps = 0, spec_accepted = 0, spec_plain = 0;
	// -s: the tokens come in chunks of SPEC_CHUNK (one call each: no per-token round trip inside)
	constexpr int SPEC_CHUNK = 16;
	for (int done = 0, stop = 0; spec_rows > 0 && !stop && (done < num_steps || num_steps == -1);) {
		const int chunk = num_steps == -1 ? SPEC_CHUNK : std::min(SPEC_CHUNK, num_steps - done);
		int out[SPEC_CHUNK];
		const int pos = (int)encoding.size() - 1;
		float u[SPEC_CHUNK];
		if (sampled) // one draw per token of the chunk, in order: token j consumes the j-th draw, as without -s
			for (int j = 0; j < chunk; ++j)
				u[j] = uniform();
		if (draft_model)
			model.generate_speculative_model(state, *draft_model, *draft_state, encoding.back(), pos, chunk, spec_rows,
			                                 temperature, top_k, top_p, sampled ? u : nullptr, out, &spec_steps,
			                                 &spec_accepted, &spec_plain);
		else if (sampled) {
			model.generate_speculative_sampled(state, encoding.back(), pos, chunk, spec_rows, temperature, top_k, top_p, u,
			                                   encoding.data(), (int)encoding.size(), out, &spec_steps, &spec_accepted,
			                                   &spec_plain);
		} else
			model.generate_speculative(state, encoding.back(), pos, chunk, spec_rows, encoding.data(),
			                           (int)encoding.size(), out, &spec_steps, &spec_accepted, &spec_plain);
		for (int j = 0; j < chunk && !stop; ++j, ++done) {
			std::cout << tokenizer.decode_one(encoding.back(), out[j]) << std::flush;
			ids += std::to_string(out[j]) + " ";
			read_bytes += model.config->active_bytes(encoding.size() - 1);
			encoding.push_back(out[j]);
			stop = out[j] == tokenizer.eos_id || out[j] == tokenizer.eot_id;
		}
	}
	// -N: the prompt's KV rows, hydrated once above, are loaded into every sequence of a batch; the
	// sequences then decode together in chunks of BATCH_CHUNK steps (one call each). The seeded
	// host RNG hands out the uniforms chunk by chunk, inside a chunk sequence by sequence
	// (sequence 0's BATCH_CHUNK draws, then sequence 1's, ...), a finished sequence included: its
	// row keeps running and its tokens are dropped, so the others' draws do not depend on it.
	// A batched step never leaves the window: the completions end at max_seq_len.
	if (n_completions > 0) {
		constexpr int BATCH_CHUNK = 16;
		const int N = n_completions, pos0 = (int)encoding.size() - 1;
		const int room = model.config->max_seq_len - pos0;
		const int total = num_steps == -1 ? room : std::min(num_steps, room);
		std::vector<std::vector<int>> seqs(N);
		std::vector<int> tok(N, encoding.back()), pos(N, pos0), stopped(N, 0);
		for (int done = 0; done < total && std::count(stopped.begin(), stopped.end(), 0) > 0;) {
			const int chunk = std::min(BATCH_CHUNK, total - done);
			std::vector<float> u((size_t)N * chunk);
			std::vector<int> out((size_t)N * chunk);
			for (int q = 0; q < N; ++q)
				for (int j = 0; j < chunk; ++j)
					u[(size_t)q * chunk + j] = uniform();
			model.generate_batch_sampled(state, N, done == 0 ? pos0 : -1, tok.data(), pos.data(), chunk, temperature, top_k,
			                             top_p, u.data(), out.data());
			for (int q = 0; q < N; ++q) {
				for (int j = 0; j < chunk && !stopped[q]; ++j) {
					const int t = out[(size_t)q * chunk + j];
					seqs[q].push_back(t);
					stopped[q] = t == tokenizer.eos_id || t == tokenizer.eot_id;
				}
				tok[q] = out[(size_t)q * chunk + chunk - 1];
				pos[q] += chunk;
			}
			done += chunk;
		}
		size_t produced = 0;
		for (int q = 0; q < N; ++q) {
			printf("--- completion %d of %d ---\n", q + 1, N);
			int prev = encoding.back();
			std::string line;
			for (int t : seqs[q]) {
				std::cout << tokenizer.decode_one(prev, t);
				line += std::to_string(t) + " ";
				prev = t;
			}
			std::cout << "\n" << std::endl;
			if (print_token_ids())
				fprintf(stderr, "TOKENS[%d]: %s\n", q, line.c_str());
			produced += seqs[q].size();
		}
		const double el = (now_ms() - start) / 1000.0;
		printf("Generation stats:\n  %zu prompt + %zu generated tokens in %d completions\n  throughput: %.5gtok/s\n"
		       "  hydrate: %.5gs\n  total: %.5gs\n\n",
		       encoding.size(), produced, N, (encoding.size() + produced) / el, (end_hydrate - start) / 1000.0, el);
		return;
	}
	for (int i = 0; spec_rows == 0 && (i < num_steps || num_steps == -1); ++i) {
		const int token = greedy || sampled ? next : sampler.sample(state, temperature);
		std::cout << tokenizer.decode_one(encoding.back(), token) << std::flush;
		ids += std::to_string(token) + " ";
		encoding.push_back(token);
		if (token == tokenizer.eos_id || token == tokenizer.eot_id)
			break;
		const int pos = (int)encoding.size() - 1;
		if (greedy)
			next = model.forward_greedy(state, token, pos);
		else if (sampled) {
			if (i + 1 == num_steps)
				break; // no further token: no further forward, and exactly one draw per generated token
			next = model.forward_sampled(state, token, pos, temperature, top_k, top_p, uniform());
		} else
			model.forward(state, token, pos);
		read_bytes += model.config->active_bytes(pos);
	}
	std::cout << "\n" << std::endl;
	if (print_token_ids())
		fprintf(stderr, "TOKENS: %s\n", ids.c_str());
	const double el = (now_ms() - start) / 1000.0;
	printf("Generation stats:\n  %zu tokens\n  throughput: %.5gtok/s\n  latency: %.5gs/tok\n  hydrate: %.5gs\n"
	       "  bandwidth: %.5gGB/s\n  total: %.5gs\n\n",
	       encoding.size(), encoding.size() / el, el / encoding.size(), (end_hydrate - start) / 1000.0,
	       (double)read_bytes / 1e9 / el, el);
	if (spec_rows > 0)
		printf("  speculative: %d steps of %d rows, %d accepted drafts, %d plain steps\n\n", spec_steps, spec_rows,
		       spec_accepted, spec_plain);
	if (draft_model)
		printf("  draft model: %s, %d of its %d drafts accepted\n\n", draft_path.c_str(), spec_accepted,
		       spec_steps * (spec_rows - 1));
}

static void run_perplexity(const std::string &path, const std::string &device, const std::string &prompt,
                           int context) {
	YALMData data;
	if (data.from_file(path) != 0) {
		fprintf(stderr, "error: cannot load %s\n", path.c_str());
		exit(1);
	}
	Model model(data, context);
	InferenceState state(model.config);
	Sampler sampler(model.config, sampler_seed());
	Tokenizer tokenizer(data);
	std::cout << "Model active bytes with full context window: " << model.config->active_bytes(model.config->max_seq_len)
	          << std::endl;
	setup_device(device, model, state);
	model.forward(state, 0, 0);
	std::vector<int> encoding = encode_prompt(tokenizer, prompt, true);
	double sum_logprob = 0.0, ss_logprob = 0.0;
	const uint64_t start = now_ms();
	size_t read_bytes = 0;
	const size_t N = encoding.size() - 1;
	// positions inside the context window in one batched prefill (per-position
	// log p from a vocab-tiled log-softmax on the device); the rest, past
	// max_seq_len (sliding window), position by position as in the reference
	size_t pos = 0;
	const size_t B = std::min(encoding.size(), (size_t)model.config->max_seq_len);
	std::vector<float> lps(B);
	// the split-operand precision form: every activation operand carries the f32 the
	// reference keeps to ~2^-22, so the perplexity is the reference's; a
	// model whose activations do not fit the prefill's operands (YALM_ERR_UNSUPPORTED) runs
	// position by position below, as the reference does
	if (B >= 2 && model.prefill(state, encoding.data(), (int)B, 0, lps.data(), true)) {
		for (; pos + 1 < B; ++pos) {
			const double lp = lps[pos];
			sum_logprob += lp;
			ss_logprob += lp * lp;
			read_bytes += model.config->active_bytes(pos);
		}
		std::cout << "\r Computing perplexity..." << pos << "/" << N << " (batched prefill)" << std::flush;
	}
	for (; pos + 1 < encoding.size(); ++pos) {
		std::cout << "\r Computing perplexity..." << pos + 1 << "/" << N << std::flush;
		model.forward(state, encoding[pos], (int)pos);
		read_bytes += model.config->active_bytes(pos);
		const double lp = std::log(sampler.sample_prob(encoding[pos + 1], state));
		sum_logprob += lp;
		ss_logprob += lp * lp;
	}
	std::cout << std::endl;
	const double el = (now_ms() - start) / 1000.0;
	const double ppl = std::exp(-sum_logprob / N);
	const double err = ppl * std::sqrt((ss_logprob - sum_logprob * sum_logprob / N) / N / N);
	printf("Stats:\n  %zu tokens\n  perplexity: %.5g ± %.5g\n  throughput: %.5gtok/s\n  latency: %.5gs/tok\n"
	       "  bandwidth: %.5gGB/s\n  total: %.5gs\n\n",
	       N, ppl, err, N / el, el / N, (double)read_bytes / 1e9 / el, el);
}

static void run_passkey(const std::string &path, const std::string &device, int context, int n_junk,
                        int passkey_pos) {
	YALMData data;
	if (data.from_file(path) != 0) {
		fprintf(stderr, "error: cannot load %s\n", path.c_str());
		exit(1);
	}
	Model model(data, context);
	InferenceState state(model.config);
	Sampler sampler(model.config, sampler_seed());
	Tokenizer tokenizer(data);
	std::cout << "Model active bytes with full context window: " << model.config->active_bytes(model.config->max_seq_len)
	          << std::endl;
	setup_device(device, model, state);
	model.forward(state, 0, 0);
	const std::string PREFIX = "There is an important info hidden inside a lot of irrelevant text. "
	                           "Find it and memorize them. I will quiz you about the important information there.";
	const std::string SUFFIX = " What is the pass key? The pass key is";
	// YALM_SEED (tests): re-seeded here, because the HIP runtime's initialisation above draws
	// from std::rand too (two runs with the same seed otherwise got different passkeys)
	if (getenv("YALM_SEED"))
		std::srand((unsigned)sampler_seed());
	const int passkey = std::rand() % 50000 + 1;
	const int ppos = passkey_pos == -1 ? std::rand() % n_junk : passkey_pos;
	std::string prompt = PREFIX;
	for (int i = 0; i < n_junk; i++) {
		if (i % n_junk == ppos)
			prompt += " The pass key is " + std::to_string(passkey) + ". Remember it. " + std::to_string(passkey) +
			          " is the pass key.";
		prompt += " The grass is green. The sky is blue. The sun is yellow. Here we go. There and back again.";
	}
	prompt += SUFFIX;
	std::vector<int> encoding = encode_prompt(tokenizer, prompt, false);
	printf("Passkey test:\n  prompt: %zu tokens\n  passkey: %d\n  passkey token index: ~%d\n\n", encoding.size(),
	       passkey, (int)(((float)ppos) / n_junk * encoding.size()));
	const size_t N = encoding.size();
	if (print_token_ids()) {
		std::string pids;
		for (int t : encoding)
			pids += std::to_string(t) + " ";
		fprintf(stderr, "PROMPT: %s\n", pids.c_str());
	}
	// the positions inside the context window before the last one in one batched prefill
	// (yalm_prefill; the reference hydrates them one forward each, main.cpp:228-232); the
	// rest -- past max_seq_len (sliding window + sinks) and the last prompt token, whose
	// logits start the answer -- one forward each
	size_t first = 0;
	const size_t H = std::min(N - 1, (size_t)model.config->max_seq_len);
	if (H >= 3 && model.prefill(state, encoding.data(), (int)H, 0, nullptr))
		first = H;
	for (size_t pos = first; pos < N; ++pos) {
		std::cout << "\r Running passkey test..." << pos + 1 << "/" << N << std::flush;
		model.forward(state, encoding[pos], (int)pos,
		              pos + 1 == N ? InferenceMode::OUTPUT_LOGITS : InferenceMode::HYDRATE_KV_CACHE);
	}
	std::cout << std::endl << SUFFIX << std::flush;
	if (const char *dump = getenv("YALM_DUMP_LOGITS")) { // test hook: the logits the answer starts from
		FILE *f = fopen(dump, "wb");
		if (!f || fwrite(state.logits(), sizeof(float), model.config->vocab_size, f) != (size_t)model.config->vocab_size) {
			fprintf(stderr, "error: cannot write %s\n", dump);
			exit(1);
		}
		fclose(f);
	}
	std::string ids;
	for (size_t pos = N; pos < N + 16; ++pos) {
		const int token = sampler.sample_argmax(state);
		std::cout << tokenizer.decode_one(encoding.back(), token) << std::flush;
		ids += std::to_string(token) + " ";
		encoding.push_back(token);
		if (token == tokenizer.eos_id || token == tokenizer.eot_id)
			break;
		model.forward(state, token, (int)pos);
	}
	std::cout << std::endl;
	if (print_token_ids())
		fprintf(stderr, "TOKENS: %s\n", ids.c_str());
}

int main(int argc, char *argv[]) {
	std::string checkpoint, device = "hip", mode = "completion", prompt, prompt_path, draft_path;
	int context = 0, num_steps = 256, n_junk = 250, passkey_pos = -1, top_k = 0, spec_rows = 0, n_completions = 0;
	float temperature = 1.0f, top_p = 1.0f;
	bool device_sampling = false;
	if (argc < 2)
		error_usage();
	checkpoint = argv[1];
	for (int i = 2; i < argc; i += 2) {
		if (i + 1 >= argc || argv[i][0] != '-' || strlen(argv[i]) != 2)
			error_usage();
		const std::string v = argv[i + 1];
		switch (argv[i][1]) {
		case 'h': error_usage();
		case 'm':
			if (std::string("completion").starts_with(v))
				mode = "completion";
			else if (std::string("passkey").starts_with(v))
				mode = "passkey";
			else if (std::string("perplexity").starts_with(v))
				mode = "perplexity";
			else
				error_usage();
			break;
		case 'd':
			if (std::string("cpu").starts_with(v))
				device = "cpu";
			else if (std::string("cuda").starts_with(v) || std::string("hip").starts_with(v))
				device = "hip";
			else
				error_usage();
			break;
		case 'i': prompt = v; break;
		case 't': temperature = std::stof(v); break;
		case 'k':
			top_k = std::stoi(v);
			device_sampling = true;
			break;
		case 'p':
			top_p = std::stof(v);
			device_sampling = true;
			break;
		case 's': spec_rows = std::stoi(v); break;
		case 'N': n_completions = std::stoi(v); break;
		case 'D': draft_path = v; break;
		case 'f': prompt_path = v; break;
		case 'T': context = std::stoi(v); break;
		case 'l': passkey_pos = std::stoi(v); break;
		case 'n':
			num_steps = std::stoi(v);
			n_junk = num_steps;
			break;
		default: error_usage();
		}
	}
	// -s: completion mode, with -t 0 (greedy) or with -t > 0 and -k / -p (the device draw); the
	// host sampler (-t > 0 alone) reads the logits of one row and has no speculative form
	if (spec_rows != 0 && (spec_rows < 2 || spec_rows > 4 || (temperature != 0.0f && !device_sampling) ||
	                       temperature < 0.0f || mode != "completion"))
		error_usage();
	// -D: the drafter of -s (whose checks above then cover the mode and the sampling)
	if (!draft_path.empty() && spec_rows == 0)
		error_usage();
	// -N: completion mode, sampled on the device (-t > 0 with -k or -p): greedy completions of one
	// prompt would be identical, and the host sampler reads one row's logits
	if (n_completions != 0 && (n_completions < 2 || n_completions > 4 || !(temperature > 0.0f) || !device_sampling ||
	                           spec_rows != 0 || mode != "completion"))
		error_usage();
	const int has_prompt = prompt.size() > 0, has_path = prompt_path.size() > 0;
	if (mode == "completion" || mode == "perplexity") {
		if (has_prompt + has_path != 1)
			error_usage();
		if (has_path) {
			std::ifstream f(prompt_path);
			if (!f.is_open()) {
				std::cerr << "Error: could not open file " << prompt_path << std::endl;
				return 1;
			}
			std::stringstream buf;
			buf << f.rdbuf();
			prompt = buf.str();
		}
	} else if (passkey_pos != -1 && (passkey_pos >= n_junk || passkey_pos < 0)) {
		std::cerr << "Error: passkey position must be between 0 and " << n_junk - 1 << std::endl;
		return 1;
	}
	fprintf(stderr, "[yalm] Using checkpoint: %s\n", checkpoint.c_str());
	try {
		if (mode == "completion")
			run_completion(checkpoint, device, prompt, context, num_steps, temperature, device_sampling, top_k, top_p,
			               spec_rows, n_completions, draft_path);
		else if (mode == "passkey")
			run_passkey(checkpoint, device, context, n_junk, passkey_pos);
		else
			run_perplexity(checkpoint, device, prompt, context);
	} catch (const std::exception &e) {
		fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
	return 0;
}
