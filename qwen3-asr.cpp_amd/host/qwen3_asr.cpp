// qwen3_asr.cpp -- Qwen3ASR (include/qwen3_asr.h) over the C-ABI.
// Mirrors src/qwen3_asr.cpp:21-327: same error strings, same result fields;
// mel / encode / prefill / greedy decode run on the GPU through qasr_run.
#include "qwen3_asr.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>

#include "qasr_host.h"

namespace qwen3_asr {

// per-token callback trampoline (qasr_set_token_callback): the reference calls
// progress_callback(n_generated, max_tokens) after every token and prints every
// 10th (src/qwen3_asr.cpp:255-291); a batch reports its first clip
struct TokenCb {
    const progress_callback_t *cb;
    int max_tokens;
    bool print;
};
static void token_cb(void *user, int seq, int n_generated, int32_t) {
    const TokenCb *t = (const TokenCb *)user;
    if (seq != 0) return;
    if (t->cb && *t->cb) (*t->cb)(n_generated, t->max_tokens);
    if (t->print && n_generated % 10 == 0) fprintf(stderr, "Generated %d tokens...\n", n_generated);
}

// the stream's callback: every clip's tokens (seq = the clip's id), so a
// progress callback sees each clip's running count in turn
static void stream_token_cb(void *user, int seq, int n_generated, int32_t) {
    const TokenCb *t = (const TokenCb *)user;
    if (t->cb && *t->cb) (*t->cb)(n_generated, t->max_tokens);
    if (t->print && n_generated % 10 == 0) fprintf(stderr, "Clip %d: generated %d tokens...\n", seq, n_generated);
}

static int64_t now_ms() {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

Qwen3ASR::Qwen3ASR() = default;

Qwen3ASR::~Qwen3ASR() {
    if (ctx_) qasr_ctx_free(ctx_);
    if (model_) qasr_model_free(model_);
}

bool Qwen3ASR::load_model(const std::string &model_path) {
    const int64_t t0 = now_ms();
    if (model_) { qasr_model_free(model_); model_ = nullptr; }
    if (qasr_model_load(model_path.c_str(), device_, &model_) != 0) {
        error_msg_ = std::string("Failed to load model: ") + qasr_last_error();
        model_ = nullptr;
        return false;
    }
    qasr_hparams hp;
    qasr_model_hparams(model_, &hp);
    config_.vocab_size = hp.vocab_size;
    config_.hidden_size = hp.hidden_size;
    config_.n_decoder_layers = hp.dec_layers;
    config_.n_attention_heads = hp.n_heads;
    config_.n_key_value_heads = hp.n_kv_heads;
    config_.intermediate_size = hp.dec_ffn;
    config_.head_dim = hp.head_dim;
    config_.rms_norm_eps = hp.rms_eps;
    config_.rope_theta = hp.rope_theta;
    config_.eos_token_id = hp.eos_id;
    config_.audio_start_token_id = hp.audio_start_id;
    config_.audio_end_token_id = hp.audio_end_id;
    config_.audio_pad_token_id = hp.audio_pad_id;
    fprintf(stderr, "Model loaded in %lld ms\n", (long long)(now_ms() - t0));
    return true;
}

// The shape a context is recreated with when (batch, n_ctx) does not fit the
// current (cur_b, cur_l): the union of both only while its KV cells (slots x
// positions) are no more than the larger of the two shapes' own -- a long
// single clip after a many-slot stream gets (1, its length), not (slots, its
// length), which multiplies the cache (128 slots x 16k positions of
// a 20-min file is ~240 GB of KV at 0.6B).
extern "C" void qasr_ctx_grow_shape(int cur_b, int cur_l, int batch, int n_ctx, int *nb, int *nl) {
    const long long cur = (long long)cur_b * cur_l, want = (long long)batch * n_ctx;
    const int ub = std::max(batch, cur_b), ul = std::max(n_ctx, cur_l);
    if ((long long)ub * ul <= std::max(cur, want)) { *nb = ub; *nl = ul; }
    else { *nb = batch; *nl = n_ctx; }
}

bool Qwen3ASR::ensure_ctx(int batch, int n_ctx) {
    if (ctx_ && ctx_batch_ >= batch && ctx_len_ >= n_ctx) return true;
    if (ctx_) { qasr_ctx_free(ctx_); ctx_ = nullptr; }
    int nb = 0, nl = 0;
    qasr_ctx_grow_shape(ctx_batch_, ctx_len_, batch, n_ctx, &nb, &nl);
    if (qasr_ctx_create(model_, nb, nl, &ctx_) != 0) {
        error_msg_ = std::string("Failed to initialize KV cache: ") + qasr_last_error();
        ctx_ = nullptr;
        return false;
    }
    ctx_batch_ = nb;
    ctx_len_ = nl;
    return true;
}

// context option token_logprobs as the call asks (set only on a change: setting drops the decode graphs)
bool Qwen3ASR::set_logprobs(bool on) {
    int cur = 0;
    if (qasr_ctx_get_option(ctx_, "token_logprobs", &cur) == 0 && (cur != 0) == on) return true;
    if (qasr_ctx_set_option(ctx_, "token_logprobs", on ? 1 : 0) != 0) {
        error_msg_ = std::string("Failed to set token_logprobs: ") + qasr_last_error();
        return false;
    }
    return true;
}

// context option top_k likewise
bool Qwen3ASR::set_top_k(int k) {
    int cur = 0;
    if (qasr_ctx_get_option(ctx_, "top_k", &cur) == 0 && cur == k) return true;
    if (qasr_ctx_set_option(ctx_, "top_k", k) != 0) {
        error_msg_ = std::string("Failed to set top_k: ") + qasr_last_error();
        return false;
    }
    return true;
}

// context option beam_width likewise (0 and 1 both mean greedy)
bool Qwen3ASR::set_beam_width(int w) {
    int cur = 0;
    if (qasr_ctx_get_option(ctx_, "beam_width", &cur) == 0 && cur == w) return true;
    if (qasr_ctx_set_option(ctx_, "beam_width", w) != 0) {
        error_msg_ = std::string("Failed to set beam_width: ") + qasr_last_error();
        return false;
    }
    return true;
}

// sampling as the call asks (qasr_set_sampling: no graph is dropped either way)
bool Qwen3ASR::set_sampling(const transcribe_params &params) {
    qasr_sampling sp{params.temperature, params.min_p, params.seed, params.n_best};
    if (qasr_set_sampling(ctx_, params.temperature > 0.f ? &sp : nullptr) != 0) {
        error_msg_ = std::string("Failed to set sampling: ") + qasr_last_error();
        return false;
    }
    return true;
}

// decoding constraints as the call asks (qasr_set_constraints: no graph is dropped either way)
static bool constraints_asked(const transcribe_params &params) {
    return params.no_repeat_ngram != 0 || params.repetition_penalty != 1.f || !params.suppress_tokens.empty() || !params.token_bias.empty() ||
           !params.hotwords.empty();
}

bool Qwen3ASR::set_constraints(const transcribe_params &params) {
    std::vector<int32_t> ids;
    std::vector<float> bias;
    auto put = [&](int32_t id, float b) {
        for (size_t i = 0; i < ids.size(); i++)
            if (ids[i] == id) { bias[i] = b; return; }
        ids.push_back(id);
        bias.push_back(b);
    };
    for (const auto &tb : params.token_bias) put(tb.first, tb.second);
    for (const int32_t id : params.suppress_tokens) put(id, -INFINITY);
    qasr_constraints k{params.no_repeat_ngram, params.repetition_penalty, params.penalty_last_n, (int32_t)ids.size(), ids.data(), bias.data()};
    if (qasr_set_constraints(ctx_, constraints_asked(params) ? &k : nullptr) != 0) {
        error_msg_ = std::string("Failed to set decoding constraints: ") + qasr_last_error();
        return false;
    }
    return true;
}

// hotwords as the call asks (qasr_set_phrases: every text in both tokenisations)
bool Qwen3ASR::set_hotwords(const transcribe_params &params) {
    std::vector<int32_t> ids, len;
    std::vector<float> boost;
    for (size_t i = 0; i < params.hotwords.size(); i++) {
        int32_t v[2 * QASR_PHRASE_LEN_MAX], l[2];
        const int n = qasr_phrase_tokenize(model_, params.hotwords[i].c_str(), v, l, 2 * QASR_PHRASE_LEN_MAX);
        if (n < 0) {
            error_msg_ = std::string("Failed to tokenize hotword \"") + params.hotwords[i] + "\": " + qasr_last_error();
            return false;
        }
        const float b = i < params.hotword_boosts.size() && params.hotword_boosts[i] > 0.f ? params.hotword_boosts[i] : params.hotword_boost;
        for (int k = 0, at = 0; k < n; at += l[k], k++) {
            ids.insert(ids.end(), v + at, v + at + l[k]);
            len.push_back(l[k]);
            boost.push_back(b);
        }
    }
    const qasr_phrases p{(int32_t)len.size(), ids.data(), len.data(), boost.data()};
    if (qasr_set_phrases(ctx_, len.empty() ? nullptr : &p) != 0) {
        error_msg_ = std::string("Failed to set hotwords: ") + qasr_last_error();
        return false;
    }
    return true;
}

transcribe_result Qwen3ASR::transcribe(const std::string &audio_path, const transcribe_params &params) {
    transcribe_result result;
    if (!model_) { result.error_msg = "Model not loaded"; return result; }
    std::vector<float> samples;
    int sr = 0;
    if (!load_audio_file(audio_path, samples, sr)) {
        result.error_msg = "Failed to load audio file: " + audio_path;
        return result;
    }
    if (sr != 16000 && params.resample) return transcribe(samples.data(), (int)samples.size(), sr, params);
    if (sr != 16000) {
        result.error_msg = "Audio must be 16kHz, got " + std::to_string(sr) + " Hz";
        return result;
    }
    return transcribe_internal(samples.data(), (int)samples.size(), params);
}

// samples at sample_rate: transcribe_internal with the resampler in front
transcribe_result Qwen3ASR::transcribe(const float *samples, int n_samples, int sample_rate, const transcribe_params &params) {
    transcribe_result result;
    if (!model_) { result.error_msg = "Model not loaded"; return result; }
    return transcribe_internal(samples, n_samples, params, sample_rate);
}

transcribe_result Qwen3ASR::transcribe(const float *samples, int n_samples, const transcribe_params &params) {
    transcribe_result result;
    if (!model_) { result.error_msg = "Model not loaded"; return result; }
    return transcribe_internal(samples, n_samples, params);
}

// the results of the last qasr_run / qasr_run_staged of out.size() clips (toks [B][max_tokens], nt [B]) as the call
// asked for them: per-token values, alternatives, beam and sampling hypotheses, texts.  A message: every clip failed
static std::string collect_run(qasr_ctx *ctx, qasr_model *model, const transcribe_params &params, const std::vector<int32_t> &toks,
                               const std::vector<int> &nt, const qasr_timings &tm, int64_t t0, std::vector<transcribe_result> &out) {
    const int B = (int)out.size();
    const int W = params.beam_width >= 2 ? params.beam_width : 1;
    const bool beam = W >= 2, sampling = params.temperature > 0.f;
    const int NB = sampling ? std::max(params.n_best, 1) : 1;
    const bool many = sampling && NB >= 2;
    const bool want_lp = params.token_logprobs && !beam && !many;
    std::vector<float> lps;
    if (want_lp) {
        lps.resize((size_t)B * params.max_tokens);
        if (qasr_get_logprobs(ctx, lps.data(), B, params.max_tokens) != 0) {
            return std::string("Decoding failed: ") + qasr_last_error();
        }
    }
    const int K = beam || many ? 0 : params.top_k;
    std::vector<int32_t> alt_id;
    std::vector<float> alt_lp;
    if (K > 0) {
        alt_id.resize((size_t)B * params.max_tokens * K);
        alt_lp.resize(alt_id.size());
        if (qasr_get_topk(ctx, alt_id.data(), alt_lp.data(), B, params.max_tokens, K) != 0) {
            return std::string("Decoding failed: ") + qasr_last_error();
        }
    }
    const int64_t t1 = now_ms();
    for (int b = 0; b < B; b++) {
        transcribe_result &r = out[b];
        r.tokens.assign(toks.begin() + (long)b * params.max_tokens, toks.begin() + (long)b * params.max_tokens + nt[b]);
        if (want_lp)
            r.token_logprobs.assign(lps.begin() + (long)b * params.max_tokens, lps.begin() + (long)b * params.max_tokens + nt[b]);
        if (K > 0) {
            const long o = (long)b * params.max_tokens * K;
            r.alt_tokens.assign(alt_id.begin() + o, alt_id.begin() + o + (long)nt[b] * K);
            r.alt_logprobs.assign(alt_lp.begin() + o, alt_lp.begin() + o + (long)nt[b] * K);
        }
        auto detok = [&](const std::vector<int32_t> &t) {
            const int len = qasr_detokenize(model, t.data(), (int)t.size(), nullptr, 0);
            std::string text(std::max(len, 0) + 1, '\0');
            qasr_detokenize(model, t.data(), (int)t.size(), &text[0], (int)text.size());
            text.resize(std::max(len, 0));
            return text;
        };
        r.text = detok(r.tokens);
        if (beam) {
            std::vector<int32_t> bt((size_t)W * params.max_tokens);
            std::vector<int> bn(W), bf(W);
            std::vector<float> bs(W);
            const int nh = qasr_get_beams(ctx, b, bt.data(), nullptr, bn.data(), bs.data(), bf.data(), W, params.max_tokens);
            if (nh < 0) {
                r.error_msg = std::string("Decoding failed: ") + qasr_last_error();
                continue;
            }
            for (int i = 0; i < nh; i++) {
                beam_hypothesis h;
                h.tokens.assign(bt.begin() + (long)i * params.max_tokens, bt.begin() + (long)i * params.max_tokens + bn[i]);
                h.text = detok(h.tokens);
                h.sum_logprob = bs[i];
                h.finished = bf[i] != 0;
                r.beams.push_back(std::move(h));
            }
        }
        if (sampling) {
            std::vector<int32_t> st((size_t)NB * params.max_tokens);
            std::vector<float> sl(st.size()), ss(NB);
            std::vector<int> sn(NB);
            const int nh = qasr_get_samples(ctx, b, st.data(), sl.data(), sn.data(), ss.data(), NB, params.max_tokens);
            if (nh < 0) {
                r.error_msg = std::string("Decoding failed: ") + qasr_last_error();
                continue;
            }
            for (int i = 0; i < nh; i++) {
                sample_hypothesis h;
                h.tokens.assign(st.begin() + (long)i * params.max_tokens, st.begin() + (long)i * params.max_tokens + sn[i]);
                h.token_logprobs.assign(sl.begin() + (long)i * params.max_tokens, sl.begin() + (long)i * params.max_tokens + sn[i]);
                h.text = detok(h.tokens);
                h.sum_logprob = ss[i];
                r.samples.push_back(std::move(h));
            }
        }
        r.success = true;
        r.t_mel_ms = (int64_t)tm.t_mel_ms;
        r.t_encode_ms = (int64_t)tm.t_encode_ms;
        r.t_decode_ms = (int64_t)(tm.t_prefill_ms + tm.t_decode_ms);
        r.t_total_ms = t1 - t0;
    }
    return std::string();
}

// one clip through qasr_run: the stage timings and --profile sections of the
// reference's transcribe_internal (src/qwen3_asr.cpp:81-160)
// rates: the clips' sample rates (null: 16 kHz), resampled on the device before the mel stage
std::vector<transcribe_result> Qwen3ASR::transcribe_run(const std::vector<std::vector<float>> &clips,
                                                        const transcribe_params &params, const std::vector<int> *rates) {
    const int B = (int)clips.size();
    std::vector<transcribe_result> out(B);
    if (!model_) { for (auto &r : out) r.error_msg = "Model not loaded"; return out; }
    int maxP = 0;
    std::vector<const float *> ptr(B);
    std::vector<int> n(B);
    for (int b = 0; b < B; b++) {
        ptr[b] = clips[b].data();
        n[b] = (int)clips[b].size();
        int n16 = n[b];   // the prompt comes from the samples at 16 kHz
        if (rates && (n16 = qasr_resample_len(n[b], (*rates)[b])) < 0) {
            for (auto &r : out) r.error_msg = std::string("Failed to resample audio: ") + qasr_last_error();
            return out;
        }
        maxP = std::max(maxP, qasr_prompt_len(qasr_encoder_frames(qasr_mel_frames(n16))));
    }
    const int64_t t0 = now_ms();
    std::vector<int32_t> sys;
    if (!params.system_prompt.empty()) {
        const int k = qasr_tokenize(model_, params.system_prompt.c_str(), nullptr, 0);
        sys.resize(std::max(k, 0));
        qasr_tokenize(model_, params.system_prompt.c_str(), sys.data(), k);
    }
    // beam search: W decode rows a clip, no per-token progress, its values through qasr_get_beams
    const int W = params.beam_width >= 2 ? params.beam_width : 1;
    const bool beam = W >= 2;
    // sampling: n_best decode rows a clip; n_best >= 2 delivers its values through qasr_get_samples alone
    const bool sampling = params.temperature > 0.f;
    const int NB = sampling ? std::max(params.n_best, 1) : 1;
    const bool many = sampling && NB >= 2;
    if (!ensure_ctx(B * std::max(W, NB), maxP + (int)sys.size() + params.max_tokens) || !set_logprobs(params.token_logprobs) ||
        !set_top_k(params.top_k) || !set_beam_width(params.beam_width) || !set_sampling(params) || !set_constraints(params) || !set_hotwords(params)) {
        for (auto &r : out) r.error_msg = error_msg_;
        return out;
    }
    qasr_set_system_prompt(ctx_, sys.data(), (int)sys.size());
    qasr_set_profile(ctx_, profile_ ? 1 : 0);   // resets the sections: the report covers this call
    std::vector<int32_t> toks((size_t)B * params.max_tokens);
    std::vector<int> nt(B);
    qasr_timings tm{};
    TokenCb tcb{&progress_callback_, params.max_tokens, params.print_progress};
    const bool per_token = !beam && !many && (progress_callback_ || params.print_progress);
    qasr_set_token_callback(ctx_, per_token ? token_cb : nullptr, per_token ? &tcb : nullptr);
    const int rc = rates ? qasr_transcribe_batch_rate(ctx_, ptr.data(), n.data(), rates->data(), B, params.max_tokens, 0, toks.data(), nt.data(), &tm)
                         : qasr_transcribe_batch(ctx_, ptr.data(), n.data(), B, params.max_tokens, 0, toks.data(), nt.data(), &tm);
    qasr_set_token_callback(ctx_, nullptr, nullptr);
    if (rc != 0) {
        for (auto &r : out) r.error_msg = std::string("Decoding failed: ") + qasr_last_error();
        return out;
    }
    if (profile_) {
        const int len = qasr_profile_report(ctx_, nullptr, 0);
        std::string rep(std::max(len, 0) + 1, '\0');
        qasr_profile_report(ctx_, &rep[0], (int)rep.size());
        rep.resize(std::max(len, 0));
        profile_report_ = rep;
    }
    const std::string err = collect_run(ctx_, model_, params, toks, nt, tm, t0, out);
    if (!err.empty())
        for (auto &r : out) r.error_msg = err;
    return out;
}

// several clips: the continuous-batching stream (qasr_run_stream), up to
// max_batch() slots; each clip succeeds or fails on its own, with the
// reference's per-call error strings
std::vector<transcribe_result> Qwen3ASR::transcribe_batch(const std::vector<std::vector<float>> &clips,
                                                          const transcribe_params &params) {
    return batch_impl(clips, nullptr, params);
}

std::vector<transcribe_result> Qwen3ASR::transcribe_batch(const std::vector<std::vector<float>> &clips, const std::vector<int> &rates,
                                                          const transcribe_params &params) {
    if (rates.size() != clips.size())
        return std::vector<transcribe_result>(clips.size(), [] { transcribe_result r; r.error_msg = "One sample rate per clip"; return r; }());
    return batch_impl(clips, &rates, params);
}

std::vector<transcribe_result> Qwen3ASR::batch_impl(const std::vector<std::vector<float>> &clips, const std::vector<int> *rates,
                                                    const transcribe_params &params) {
    if (clips.size() <= 1) return transcribe_run(clips, params, rates);
    // the stream has neither beam search, sampling nor decoding constraints: whole runs of as many clips as max_batch() rows hold
    if (params.beam_width >= 2 || params.temperature > 0.f || constraints_asked(params)) {
        std::vector<transcribe_result> out;
        const size_t per = (size_t)std::max(1, max_batch_ / std::max(1, params.beam_width >= 2 ? params.beam_width : params.n_best));
        for (size_t i = 0; i < clips.size(); i += per) {
            std::vector<std::vector<float>> part(clips.begin() + i, clips.begin() + std::min(clips.size(), i + per));
            std::vector<int> prates;
            if (rates) prates.assign(rates->begin() + i, rates->begin() + std::min(clips.size(), i + per));
            for (auto &r : transcribe_run(part, params, rates ? &prates : nullptr)) out.push_back(std::move(r));
        }
        return out;
    }
    if (!model_) return std::vector<transcribe_result>(clips.size(), [] { transcribe_result r; r.error_msg = "Model not loaded"; return r; }());
    std::vector<transcribe_result> out(clips.size());
    int maxP = 0;
    for (size_t i = 0; i < clips.size(); i++) {   // (a clip at an unsupported rate fails alone in the stream: it sizes nothing)
        const int n16 = rates ? qasr_resample_len((int)clips[i].size(), (*rates)[i]) : (int)clips[i].size();
        maxP = std::max(maxP, qasr_prompt_len(qasr_encoder_frames(qasr_mel_frames(std::max(n16, 0)))));
    }
    const int n_sys = params.system_prompt.empty() ? 0 : std::max(qasr_tokenize(model_, params.system_prompt.c_str(), nullptr, 0), 0);
    size_t next = 0;
    const bool ok = stream_impl(
        [&](int &id, std::vector<float> &pcm, int &rate) {
            if (next >= clips.size()) return false;
            id = (int)next;
            if (rates) rate = (*rates)[next];
            pcm = clips[next++];
            return true;
        },
        rates != nullptr, [&](int id, transcribe_result r) { out[id] = std::move(r); }, params, maxP + n_sys + params.max_tokens,
        std::min((int)clips.size(), max_batch_));
    if (!ok)
        for (auto &r : out)
            if (!r.success && r.error_msg.empty()) r.error_msg = error_msg_;
    return out;
}

namespace {
struct StreamCtx {
    const std::function<bool(int &, std::vector<float> &, int &)> *fetch;
    const std::function<void(int, transcribe_result)> *sink;
    qasr_model *model;
    std::vector<float> pcm;
    int64_t t0;
    qasr_ctx *lp_ctx;   // non-null: transcribe_params::token_logprobs
    qasr_ctx *tk_ctx;   // non-null: transcribe_params::top_k, its value in top_k
    int top_k;
    const std::vector<int> *staged = nullptr;   // transcribe_long: the pool entries to decode, in order
    size_t staged_next = 0;
};
// (the staged stream: the clip is pool entry id, already in HBM)
int stream_fetch_staged(void *u, int *) {
    StreamCtx *s = (StreamCtx *)u;
    return s->staged_next < s->staged->size() ? (*s->staged)[s->staged_next++] : -1;
}
int stream_fetch_rate(void *u, const float **pcm, int *n, int *rate, int *) {
    StreamCtx *s = (StreamCtx *)u;
    int id = -1, sr = 16000;
    if (!(*s->fetch)(id, s->pcm, sr) || id < 0) return -1;
    *pcm = s->pcm.data();
    *n = (int)s->pcm.size();
    if (rate) *rate = sr;
    return id;
}
int stream_fetch(void *u, const float **pcm, int *n, int *budget) { return stream_fetch_rate(u, pcm, n, nullptr, budget); }
void stream_sink(void *u, int id, int status, const int32_t *toks, int n) {
    StreamCtx *s = (StreamCtx *)u;
    transcribe_result r;
    if (status != 0) {
        r.error_msg = std::string("Decoding failed: ") + qasr_last_error();
    } else {
        r.tokens.assign(toks, toks + n);
        if (s->lp_ctx) {
            r.token_logprobs.resize(n);
            if (qasr_stream_logprobs(s->lp_ctx, r.token_logprobs.data(), n) != n) r.token_logprobs.clear();
        }
        if (s->tk_ctx) {
            r.alt_tokens.resize((size_t)n * s->top_k);
            r.alt_logprobs.resize((size_t)n * s->top_k);
            if (qasr_stream_topk(s->tk_ctx, r.alt_tokens.data(), r.alt_logprobs.data(), n, s->top_k) != n) {
                r.alt_tokens.clear();
                r.alt_logprobs.clear();
            }
        }
        const int len = qasr_detokenize(s->model, toks, n, nullptr, 0);
        std::string text(std::max(len, 0) + 1, '\0');
        qasr_detokenize(s->model, toks, n, &text[0], (int)text.size());
        text.resize(std::max(len, 0));
        r.text = text;
        r.success = true;
        r.t_total_ms = now_ms() - s->t0;   // (completion time within the stream)
    }
    (*s->sink)(id, std::move(r));
}
}  // namespace

bool Qwen3ASR::transcribe_stream(const std::function<bool(int &id, std::vector<float> &pcm)> &fetch,
                                 const std::function<void(int id, transcribe_result result)> &sink,
                                 const transcribe_params &params, int n_ctx, int slots) {
    return stream_impl([&](int &id, std::vector<float> &pcm, int &) { return fetch(id, pcm); }, false, sink, params, n_ctx, slots);
}

bool Qwen3ASR::transcribe_stream_rate(const std::function<bool(int &id, std::vector<float> &pcm, int &rate)> &fetch,
                                      const std::function<void(int id, transcribe_result result)> &sink,
                                      const transcribe_params &params, int n_ctx, int slots) {
    return stream_impl(fetch, true, sink, params, n_ctx, slots);
}

// with_rates: the fetch's rate is honoured (qasr_run_stream_rate); else every clip is 16 kHz PCM (qasr_run_stream)
bool Qwen3ASR::stream_impl(const std::function<bool(int &id, std::vector<float> &pcm, int &rate)> &fetch, bool with_rates,
                           const std::function<void(int id, transcribe_result result)> &sink, const transcribe_params &params,
                           int n_ctx, int slots) {
    if (!model_) { error_msg_ = "Model not loaded"; return false; }
    std::vector<int32_t> sys;
    if (!params.system_prompt.empty()) {
        const int k = qasr_tokenize(model_, params.system_prompt.c_str(), nullptr, 0);
        sys.resize(std::max(k, 0));
        qasr_tokenize(model_, params.system_prompt.c_str(), sys.data(), k);
    }
    // context length: n_ctx, or the prompt of a 30 s clip (the reference's
    // chunking unit) plus the budget -- longer clips fail alone ("Context length")
    const int need = n_ctx > 0 ? n_ctx : qasr_prompt_len(qasr_encoder_frames(qasr_mel_frames(30 * 16000))) + (int)sys.size() + params.max_tokens;
    const int S = slots > 0 ? std::min(slots, max_batch_) : max_batch_;
    if (params.beam_width >= 2) { error_msg_ = "The stream has no beam search (transcribe_params::beam_width)"; return false; }
    if (params.temperature > 0.f) { error_msg_ = "The stream has no sampling (transcribe_params::temperature)"; return false; }
    if (constraints_asked(params)) { error_msg_ = "The stream has neither decoding constraints nor hotwords (transcribe_params::no_repeat_ngram ... hotwords)"; return false; }
    if (!ensure_ctx(S, need) || !set_logprobs(params.token_logprobs) || !set_top_k(params.top_k) || !set_beam_width(0) ||
        !set_sampling(params) || !set_constraints(params) || !set_hotwords(params))
        return false;
    qasr_set_system_prompt(ctx_, sys.data(), (int)sys.size());
    qasr_set_profile(ctx_, profile_ ? 1 : 0);   // the report covers the whole stream
    TokenCb tcb{&progress_callback_, params.max_tokens, params.print_progress};
    const bool per_token = progress_callback_ || params.print_progress;
    qasr_set_token_callback(ctx_, per_token ? stream_token_cb : nullptr, per_token ? &tcb : nullptr);
    StreamCtx sc{&fetch, &sink, model_, {}, now_ms(), params.token_logprobs ? ctx_ : nullptr,
                 params.top_k > 0 ? ctx_ : nullptr, params.top_k};
    const int rc = with_rates ? qasr_run_stream_rate(ctx_, S, stream_fetch_rate, stream_sink, &sc, params.max_tokens, 0, nullptr)
                              : qasr_run_stream(ctx_, S, stream_fetch, stream_sink, &sc, params.max_tokens, 0, nullptr);
    qasr_set_token_callback(ctx_, nullptr, nullptr);
    if (rc != 0) { error_msg_ = std::string("Decoding failed: ") + qasr_last_error(); return false; }
    if (profile_) {
        const int len = qasr_profile_report(ctx_, nullptr, 0);
        std::string rep(std::max(len, 0) + 1, '\0');
        qasr_profile_report(ctx_, &rep[0], (int)rep.size());
        rep.resize(std::max(len, 0));
        profile_report_ = rep;
    }
    return true;
}

// a recording of any length: staged once (qasr_stage_long: resampled and cut on the device, every segment a pool entry
// into the recording), then the segments that are not silent decoded from the pool
long_result Qwen3ASR::transcribe_long(const float *samples, int n_samples, int sample_rate, const transcribe_params &params,
                                      const qasr_segment_params *seg_params) {
    long_result out;
    if (!model_) { out.error_msg = "Model not loaded"; return out; }
    const qasr_segment_params seg = seg_params ? *seg_params : qasr_segment_params{3000, 1000, 5, -1.0};
    if (qasr_segment_validate(&seg) != 0) { out.error_msg = std::string("Segmentation failed: ") + qasr_last_error(); return out; }
    std::vector<int32_t> sys;
    if (!params.system_prompt.empty()) {
        const int k = qasr_tokenize(model_, params.system_prompt.c_str(), nullptr, 0);
        sys.resize(std::max(k, 0));
        qasr_tokenize(model_, params.system_prompt.c_str(), sys.data(), k);
    }
    const int W = params.beam_width >= 2 ? params.beam_width : 1;
    const int NB = params.temperature > 0.f ? std::max(params.n_best, 1) : 1;
    const bool grouped = W >= 2 || params.temperature > 0.f || constraints_asked(params);   // (what the stream refuses)
    // the longest segment: max_frames frames and the recording's tail of less than a frame
    const int need = qasr_prompt_len(qasr_encoder_frames(qasr_mel_frames(seg.max_frames * 160 + 159))) + (int)sys.size() + params.max_tokens;
    const int rows = grouped ? std::max(W, NB) * std::max(1, max_batch_ / std::max(W, NB)) : max_batch_;
    if (!ensure_ctx(rows, need) || !set_logprobs(params.token_logprobs) || !set_top_k(params.top_k) ||
        !set_beam_width(grouped ? params.beam_width : 0) || !set_sampling(params) || !set_constraints(params) || !set_hotwords(params)) {
        out.error_msg = error_msg_;
        return out;
    }
    qasr_set_system_prompt(ctx_, sys.data(), (int)sys.size());
    qasr_set_profile(ctx_, profile_ ? 1 : 0);
    const int64_t t0 = now_ms();
    const int rate = sample_rate > 0 ? sample_rate : 16000;
    const int K = qasr_stage_long(ctx_, &samples, &n_samples, rate == 16000 ? nullptr : &rate, 1, &seg);
    if (K < 0) { out.error_msg = std::string("Segmentation failed: ") + qasr_last_error(); return out; }
    std::vector<long long> start(K);
    std::vector<int> len(K), silent(K);
    if (qasr_get_segments(ctx_, 0, start.data(), len.data(), nullptr, silent.data(), K) != K) {
        out.error_msg = std::string("Segmentation failed: ") + qasr_last_error();
        return out;
    }
    out.segments.resize(K);
    std::vector<int> todo;
    for (int k = 0; k < K; k++) {
        long_segment &s = out.segments[k];
        s.start_s = (double)start[k] / 16000.0;
        s.end_s = (double)(start[k] + len[k]) / 16000.0;
        s.silent = silent[k] != 0;
        if (s.silent) s.result.success = true;
        else todo.push_back(k);
    }
    if (grouped) {
        const size_t per = (size_t)std::max(1, max_batch_ / std::max(W, NB));
        for (size_t i = 0; i < todo.size(); i += per) {
            const int B = (int)std::min(per, todo.size() - i);
            std::vector<int32_t> toks((size_t)B * params.max_tokens);
            std::vector<int> nt(B);
            qasr_timings tm{};
            std::vector<transcribe_result> res(B);
            std::string err;
            if (qasr_run_staged(ctx_, todo.data() + i, B, params.max_tokens, 0, toks.data(), nt.data(), &tm) != 0)
                err = std::string("Decoding failed: ") + qasr_last_error();
            else
                err = collect_run(ctx_, model_, params, toks, nt, tm, t0, res);
            for (int b = 0; b < B; b++) {
                if (!err.empty()) res[b].error_msg = err;
                out.segments[todo[i + b]].result = std::move(res[b]);
            }
        }
    } else if (!todo.empty()) {
        const std::function<void(int, transcribe_result)> sink = [&](int id, transcribe_result r) { out.segments[id].result = std::move(r); };
        TokenCb tcb{&progress_callback_, params.max_tokens, params.print_progress};
        const bool per_token = progress_callback_ || params.print_progress;
        qasr_set_token_callback(ctx_, per_token ? stream_token_cb : nullptr, per_token ? &tcb : nullptr);
        StreamCtx sc{nullptr, &sink, model_, {}, t0, params.token_logprobs ? ctx_ : nullptr, params.top_k > 0 ? ctx_ : nullptr, params.top_k, &todo, 0};
        const int rc = qasr_run_stream_staged(ctx_, std::min((int)todo.size(), max_batch_), stream_fetch_staged, stream_sink, &sc, params.max_tokens, 0, nullptr);
        qasr_set_token_callback(ctx_, nullptr, nullptr);
        if (rc != 0) { out.error_msg = std::string("Decoding failed: ") + qasr_last_error(); return out; }
    }
    if (profile_) {
        const int plen = qasr_profile_report(ctx_, nullptr, 0);
        std::string rep(std::max(plen, 0) + 1, '\0');
        qasr_profile_report(ctx_, &rep[0], (int)rep.size());
        rep.resize(std::max(plen, 0));
        profile_report_ = rep;
    }
    out.success = true;
    for (const long_segment &s : out.segments) {
        if (!s.result.success) {
            out.success = false;
            if (out.error_msg.empty()) out.error_msg = s.result.error_msg.empty() ? "A segment was not decoded" : s.result.error_msg;
        }
        if (s.result.text.empty()) continue;
        if (!out.text.empty()) out.text += ' ';
        out.text += s.result.text;
    }
    return out;
}

// sample_rate 0: 16 kHz PCM; else the resampler in front (qasr_transcribe_batch_rate)
transcribe_result Qwen3ASR::transcribe_internal(const float *samples, int n_samples, const transcribe_params &params, int sample_rate) {
    std::vector<std::vector<float>> one(1, std::vector<float>(samples, samples + n_samples));
    const std::vector<int> rate(1, sample_rate);
    transcribe_result r = transcribe_run(one, params, sample_rate ? &rate : nullptr)[0];
    if (r.success && params.print_timing) {
        fprintf(stderr, "\nTiming:\n");
        fprintf(stderr, "  Mel spectrogram: %lld ms\n", (long long)r.t_mel_ms);
        fprintf(stderr, "  Audio encoding:  %lld ms\n", (long long)r.t_encode_ms);
        fprintf(stderr, "  Text decoding:   %lld ms\n", (long long)r.t_decode_ms);
        fprintf(stderr, "  Total:           %lld ms\n", (long long)r.t_total_ms);
        fprintf(stderr, "  Tokens generated: %zu\n", r.tokens.size());
    }
    return r;
}

std::string Qwen3ASR::token_text(int32_t id) const {
    if (!model_) return std::string();
    const int len = qasr_detokenize(model_, &id, 1, nullptr, 0);
    std::string text(std::max(len, 0) + 1, '\0');
    qasr_detokenize(model_, &id, 1, &text[0], (int)text.size());
    text.resize(std::max(len, 0));
    return text;
}

std::vector<score_result> Qwen3ASR::score(const float *samples, int n_samples, const std::vector<std::string> &texts,
                                          const transcribe_params &params) {
    std::vector<score_result> out(texts.size());
    auto fail_all = [&](const std::string &msg) {
        for (auto &r : out)
            if (!r.success) r.error_msg = msg;
        return out;
    };
    if (!model_) return fail_all("Model not loaded");
    if (texts.empty()) return out;
    std::vector<int32_t> sys;
    if (!params.system_prompt.empty()) {
        const int k = qasr_tokenize(model_, params.system_prompt.c_str(), nullptr, 0);
        sys.resize(std::max(k, 0));
        qasr_tokenize(model_, params.system_prompt.c_str(), sys.data(), k);
    }
    int longest = 0;
    for (size_t i = 0; i < texts.size(); i++) {
        const int k = std::max(qasr_tokenize(model_, texts[i].c_str(), nullptr, 0), 0);
        out[i].tokens.resize(k);
        qasr_tokenize(model_, texts[i].c_str(), out[i].tokens.data(), k);
        longest = std::max(longest, k);
    }
    const int P = qasr_prompt_len(qasr_encoder_frames(qasr_mel_frames(n_samples))) + (int)sys.size();
    const int per = std::min<int>(QASR_SCORE_MAX_HYP, (int)texts.size());
    if (!ensure_ctx(per, P + longest + 1)) return fail_all(error_msg_);
    qasr_set_system_prompt(ctx_, sys.data(), (int)sys.size());
    if (qasr_stage_audio(ctx_, &samples, &n_samples, 1) != 0) return fail_all(std::string("Scoring failed: ") + qasr_last_error());
    for (size_t i0 = 0; i0 < texts.size(); i0 += per) {   // more than 8 texts: in groups
        const int S = (int)std::min<size_t>(per, texts.size() - i0);
        std::vector<int> clips(S, 0), nt(S);
        std::vector<int32_t> toks;
        for (int s = 0; s < S; s++) {
            nt[s] = (int)out[i0 + s].tokens.size();
            toks.insert(toks.end(), out[i0 + s].tokens.begin(), out[i0 + s].tokens.end());
        }
        const size_t total = toks.size() + S;
        std::vector<float> lp(total), glp(total), sums(S);
        std::vector<int32_t> gid(total);
        const int rc = qasr_score(ctx_, clips.data(), toks.data(), nt.data(), S, 1, lp.data(), gid.data(), glp.data(), sums.data(), nullptr);
        size_t o = 0;
        for (int s = 0; s < S; s++) {
            score_result &r = out[i0 + s];
            const size_t k = (size_t)nt[s] + 1;
            if (rc < 0) {
                r.error_msg = std::string("Scoring failed: ") + qasr_last_error();
            } else {
                r.tokens.push_back(config_.eos_token_id);
                r.token_logprobs.assign(lp.begin() + o, lp.begin() + o + k);
                r.greedy_tokens.assign(gid.begin() + o, gid.begin() + o + k);
                r.greedy_logprobs.assign(glp.begin() + o, glp.begin() + o + k);
                r.sum_logprob = sums[s];
                r.success = true;
            }
            o += k;
        }
    }
    return out;
}

void Qwen3ASR::set_progress_callback(progress_callback_t callback) { progress_callback_ = std::move(callback); }

bool load_audio_file(const std::string &path, std::vector<float> &samples, int &sample_rate) {
    std::string err;
    if (!qasr::load_wav(path, samples, sample_rate, err)) {
        fprintf(stderr, "Error: %s\n", err.c_str());
        return false;
    }
    return true;
}

}  // namespace qwen3_asr
