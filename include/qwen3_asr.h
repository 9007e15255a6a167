// qwen3_asr.h -- C++17 pipeline API, kept verbatim from the reference's
// src/qwen3_asr.h:15-116 (transcribe_params / transcribe_result / Qwen3ASR),
// implemented over the C-ABI of libqasr.so (include/qasr_capi.h) instead of
// ggml graphs.  Existing callers of the reference library recompile against
// this header unchanged.
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "audio_encoder.h"
#include "audio_injection.h"
#include "mel_spectrogram.h"
#include "qasr_capi.h"
#include "text_decoder.h"

namespace qwen3_asr {

// src/qwen3_asr.h:15-34
struct transcribe_params {
    int32_t max_tokens = 1024;
    std::string language = "";       // accepted, ignored (as src/qwen3_asr.cpp:211)
    std::string system_prompt = "";
    int32_t n_threads = 4;            // accepted for API compatibility (no host threads on the hot path)
    bool print_progress = false;
    bool print_timing = true;
    // MI355X addition (trailing, default off): also return every token's log-probability
    // (context option "token_logprobs" of qasr_capi.h; no reference counterpart)
    bool token_logprobs = false;
    // MI355X addition (trailing, default off): also return every token's top_k (1..8) alternatives
    // (context option "top_k" of qasr_capi.h; no reference counterpart)
    int32_t top_k = 0;
    // MI355X addition (trailing, default off): beam search of this width (2..8) instead of greedy decoding
    // (context option "beam_width" of qasr_capi.h; no reference counterpart).  0 and 1 are greedy.  A beam run
    // reports no per-token progress and fills neither token_logprobs nor alt_tokens: its values are in
    // transcribe_result::beams
    int32_t beam_width = 0;
    // MI355X addition (trailing, default off): temperature sampling (qasr_set_sampling of qasr_capi.h; no reference
    // counterpart).  temperature > 0 draws every token from softmax(logits / temperature) among the tokens at least
    // min_p times as probable as the greedy one, seeded; n_best (1..8) hypotheses a clip, in
    // transcribe_result::samples.  Excludes beam_width >= 2; n_best >= 2 reports no per-token progress and fills
    // neither token_logprobs nor alt_tokens
    float temperature = 0.f;
    float min_p = 0.f;
    uint64_t seed = 0;
    int32_t n_best = 1;
    // MI355X addition (trailing, default off): decoding constraints (qasr_set_constraints of qasr_capi.h; no reference
    // counterpart), applied to every step's logits before a token is chosen.  no_repeat_ngram n (1..8): no n-gram of
    // tokens occurs twice; repetition_penalty p (0 < p <= 10, 1 = off) over the last penalty_last_n tokens (0 = all);
    // suppress_tokens are never emitted; token_bias adds to the listed tokens' logits (at most 1024 tokens in both
    // lists together, a token in both is suppressed).  Excludes beam_width >= 2 and transcribe_stream
    int32_t no_repeat_ngram = 0;
    float repetition_penalty = 1.f;
    int32_t penalty_last_n = 0;
    std::vector<int32_t> suppress_tokens;
    std::vector<std::pair<int32_t, float>> token_bias;
    // MI355X addition (trailing, default off): hotword boosting (qasr_set_phrases of qasr_capi.h; no reference
    // counterpart).  Each hotword is tokenised with and without a leading space (qasr_phrase_tokenize, at most 16
    // tokens a variant); while the last tokens spell the beginning of one, its next token's logit gets the boost
    // (0 < boost <= 100).  hotword_boosts, where given, holds a boost per hotword (an entry <= 0, or a missing
    // one: hotword_boost).  Excludes beam_width >= 2 and transcribe_stream
    std::vector<std::string> hotwords;
    float hotword_boost = 5.f;
    std::vector<float> hotword_boosts;
    // MI355X addition (trailing, default off): transcribe(audio_path) takes a file at any rate the resampler supports
    // (qasr_stage_audio_rate of qasr_capi.h: 8, 11.025, 12, 22.05, 24, 32, 44.1, 48, 88.2, 96, 176.4, 192 kHz ...)
    // and resamples it to 16 kHz on the device, in front of the mel stage; off, such a file is an error
    bool resample = false;
};

// MI355X addition: one hypothesis of a beam run
struct beam_hypothesis {
    std::vector<int32_t> tokens;   // a trailing EOS popped
    std::string text;
    float sum_logprob = 0.f;       // the EOS step included
    bool finished = false;         // ended in EOS (else the token budget ran out)
};

// MI355X addition: one hypothesis of a sampling run
struct sample_hypothesis {
    std::vector<int32_t> tokens;          // a trailing EOS popped
    std::string text;
    std::vector<float> token_logprobs;    // log softmax(logits)[token] at T = 1, one per token
    float sum_logprob = 0.f;              // the EOS step included
};

// src/qwen3_asr.h:37-49
struct transcribe_result {
    std::string text;
    std::vector<int32_t> tokens;
    bool success = false;
    std::string error_msg;
    int64_t t_load_ms = 0;
    int64_t t_mel_ms = 0;
    int64_t t_encode_ms = 0;
    int64_t t_decode_ms = 0;   // prefill + greedy loop, as the reference's decode_greedy
    int64_t t_total_ms = 0;
    // MI355X addition (trailing): with transcribe_params::token_logprobs, log softmax(logits)[token]
    // of every entry of tokens (same length); empty otherwise
    std::vector<float> token_logprobs;
    // MI355X addition (trailing): with transcribe_params::top_k = K > 0, the K largest logits of every
    // token's step as ids and log-probabilities, flat [tokens.size()][K] (entry 0 of a step is the
    // token itself); empty otherwise
    std::vector<int32_t> alt_tokens;
    std::vector<float> alt_logprobs;
    // MI355X addition (trailing): with transcribe_params::beam_width >= 2, every hypothesis of the clip,
    // best first (tokens / text above are beams[0]'s); empty otherwise
    std::vector<beam_hypothesis> beams;
    // MI355X addition (trailing): with transcribe_params::temperature > 0, the clip's n_best hypotheses in sample
    // order (tokens / text above are samples[0]'s); empty otherwise
    std::vector<sample_hypothesis> samples;
};

// MI355X addition (trailing): one text scored as a transcript of a clip (Qwen3ASR::score) -- the
// log-probability the model gives every token of the text, and the EOS after it, given the audio
struct score_result {
    std::vector<int32_t> tokens;          // the text's ids, then the EOS
    std::vector<float> token_logprobs;    // log softmax(logits)[token], one per entry of tokens
    std::vector<int32_t> greedy_tokens;   // the model's own argmax at each position
    std::vector<float> greedy_logprobs;   // ... and its log-probability
    float sum_logprob = 0.f;              // float32 sum of token_logprobs, in order
    bool success = false;
    std::string error_msg;
};

// MI355X addition (trailing): a long recording cut at its pauses (Qwen3ASR::transcribe_long)
struct long_segment {
    double start_s = 0.0, end_s = 0.0;   // within the recording, at 16 kHz
    bool silent = false;                 // qasr_segment_params::skip_ratio found it silent: not decoded, empty text
    transcribe_result result;
};
struct long_result {
    std::string text;                    // the segments' texts joined by one space (empty ones left out)
    std::vector<long_segment> segments;
    bool success = false;
    std::string error_msg;
};

using progress_callback_t = std::function<void(int tokens_generated, int max_tokens)>;

// src/qwen3_asr.h:55-116
class Qwen3ASR {
public:
    Qwen3ASR();
    ~Qwen3ASR();
    Qwen3ASR(const Qwen3ASR &) = delete;
    Qwen3ASR &operator=(const Qwen3ASR &) = delete;

    bool load_model(const std::string &model_path);
    transcribe_result transcribe(const std::string &audio_path, const transcribe_params &params = transcribe_params());
    transcribe_result transcribe(const float *samples, int n_samples, const transcribe_params &params = transcribe_params());
    void set_progress_callback(progress_callback_t callback);
    const std::string &get_error() const { return error_msg_; }
    bool is_loaded() const { return model_ != nullptr; }
    const text_decoder_config &get_config() const { return config_; }

    // MI355X additions: device selection, batched transcription, and the
    // --profile report (src/timing.h sections, device time, of the last call)
    void set_device(int device) { device_ = device; }
    // several clips: continuous batching over max_batch() KV-cache slots (a
    // finished clip's slot is refilled at once); results in input order, each
    // clip's success / error_msg its own
    std::vector<transcribe_result> transcribe_batch(const std::vector<std::vector<float>> &clips,
                                                    const transcribe_params &params = transcribe_params());
    // a work queue: fetch(id, pcm) -> false when empty (called whenever a slot
    // frees; a counter shared by several Qwen3ASR objects, one per device,
    // balances them dynamically); sink(id, result) as each clip finishes.
    // n_ctx: the context length (0: a 30 s clip's prompt + max_tokens);
    // slots: 0 = max_batch().  false: the run itself failed (get_error()).
    // Per clip only t_total_ms is set (its completion time within the stream:
    // the stages of different clips overlap); the progress callback sees
    // every clip's running count; --profile's report covers the whole stream.
    bool transcribe_stream(const std::function<bool(int &id, std::vector<float> &pcm)> &fetch,
                           const std::function<void(int id, transcribe_result result)> &sink,
                           const transcribe_params &params = transcribe_params(), int n_ctx = 0, int slots = 0);
    // MI355X additions: the same three for clips at other sample rates (one rate per clip), resampled to 16 kHz on
    // the device (qasr_transcribe_batch_rate / qasr_run_stream_rate); an unsupported rate fails its clip alone
    transcribe_result transcribe(const float *samples, int n_samples, int sample_rate, const transcribe_params &params = transcribe_params());
    std::vector<transcribe_result> transcribe_batch(const std::vector<std::vector<float>> &clips, const std::vector<int> &rates,
                                                    const transcribe_params &params = transcribe_params());
    bool transcribe_stream_rate(const std::function<bool(int &id, std::vector<float> &pcm, int &rate)> &fetch,
                                const std::function<void(int id, transcribe_result result)> &sink,
                                const transcribe_params &params = transcribe_params(), int n_ctx = 0, int slots = 0);
    void set_max_batch(int slots) { max_batch_ = slots > 0 ? slots : 1; }
    int max_batch() const { return max_batch_; }
    void set_profile(bool on) { profile_ = on; }
    const std::string &profile_report() const { return profile_report_; }
    // the text of one token id (empty without a model): for listing transcribe_result::alt_tokens
    std::string token_text(int32_t id) const;
    // teacher-forced scoring (qasr_score of qasr_capi.h; no reference counterpart): each text goes through
    // the model's tokenizer verbatim, the EOS is appended and scored; params.system_prompt is honoured, the
    // other fields are not used.  The clip's mel, encoder and prompt prefill run once per group of at most
    // 8 texts; results in input order, each text's success / error_msg its own
    std::vector<score_result> score(const float *samples, int n_samples, const std::vector<std::string> &texts,
                                    const transcribe_params &params = transcribe_params());

    // a recording of any length (qasr_stage_long of qasr_capi.h; no reference counterpart): uploaded once, resampled
    // on the device when sample_rate is not 16000, cut at its quietest points on the device (seg_params; null: cuts
    // at most 30 s apart, nothing skipped), every segment a pool entry into the recording.  Silent segments are not
    // decoded (empty text, success); the others go through the staged stream over max_batch() slots, or -- with
    // beam_width >= 2, sampling, constraints or hotwords, which the stream refuses -- through qasr_run_staged in
    // groups that fit max_batch().  The context length is that of a max_frames clip plus max_tokens
    long_result transcribe_long(const float *samples, int n_samples, int sample_rate, const transcribe_params &params = transcribe_params(),
                                const qasr_segment_params *seg_params = nullptr);

private:
    transcribe_result transcribe_internal(const float *samples, int n_samples, const transcribe_params &params, int sample_rate = 0);
    bool ensure_ctx(int batch, int n_ctx);
    bool set_logprobs(bool on);
    bool set_top_k(int k);
    bool set_beam_width(int w);
    bool set_sampling(const transcribe_params &params);
    bool set_constraints(const transcribe_params &params);
    bool set_hotwords(const transcribe_params &params);
    std::vector<transcribe_result> transcribe_run(const std::vector<std::vector<float>> &clips, const transcribe_params &params,
                                                  const std::vector<int> *rates = nullptr);
    std::vector<transcribe_result> batch_impl(const std::vector<std::vector<float>> &clips, const std::vector<int> *rates,
                                              const transcribe_params &params);
    bool stream_impl(const std::function<bool(int &id, std::vector<float> &pcm, int &rate)> &fetch, bool with_rates,
                     const std::function<void(int id, transcribe_result result)> &sink, const transcribe_params &params, int n_ctx,
                     int slots);

    qasr_model *model_ = nullptr;
    qasr_ctx *ctx_ = nullptr;
    int ctx_batch_ = 0, ctx_len_ = 0, device_ = 0, max_batch_ = 16;
    text_decoder_config config_;
    std::string error_msg_;
    progress_callback_t progress_callback_;
    bool profile_ = false;
    std::string profile_report_;
};

bool load_audio_file(const std::string &path, std::vector<float> &samples, int &sample_rate);

}  // namespace qwen3_asr
