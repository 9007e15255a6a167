/*
 * qasr_capi.h -- C-ABI of the MI355X-native Qwen3-ASR engine (libqasr.so).
 *
 * The reference has no plugin registry; its hot-path boundary is the C++
 * class API listed below.  Each entry point here replaces one of those calls
 * (SURVEY.md §8(b)); plain pointers and sizes only, no torch / HIP types.
 *
 *   qasr_model_load / qasr_model_free
 *       <- Qwen3ASR::load_model           src/qwen3_asr.cpp:21-42
 *          (AudioEncoder::load_model      src/audio_encoder.cpp:42-83,
 *           TextDecoder::load_model       src/text_decoder.cpp:38-114,
 *           GGUFLoader::load              src/gguf_loader.cpp:17-53)
 *   qasr_ctx_create / qasr_ctx_free
 *       <- TextDecoder::init_kv_cache     src/text_decoder.cpp:337-386
 *   qasr_mel, qasr_mel_engine_run
 *       <- log_mel_spectrogram            src/mel_spectrogram.h:53-55 / .cpp:484-628
 *   qasr_mel_filters
 *       <- generate_mel_filters           src/mel_spectrogram.h:42-43 / .cpp:352-395
 *   qasr_encode, qasr_encode_conv
 *       <- AudioEncoder::encode           src/audio_encoder.h:27 / .cpp:312-601
 *          AudioEncoder::encode_conv_only src/audio_encoder.h:30
 *   qasr_prefill
 *       <- TextDecoder::forward_with_audio src/text_decoder.h:134-137 / .cpp:588-684
 *   qasr_decode_step
 *       <- TextDecoder::forward           src/text_decoder.h:125-126 / .cpp:583-586
 *          + Qwen3ASR::sample_greedy      src/qwen3_asr.cpp:305-317 (fused argmax)
 *   qasr_transcribe_batch / qasr_stage_audio + qasr_run
 *       <- Qwen3ASR::transcribe_internal  src/qwen3_asr.cpp:81-149
 *          + decode_greedy                src/qwen3_asr.cpp:216-303
 *   qasr_detokenize / qasr_tokenize
 *       <- TextDecoder::decode_tokens / tokenize src/text_decoder.cpp:1069-1103
 *   qasr_align, qasr_align_json          (ForcedAligner model files)
 *       <- ForcedAligner::align           src/forced_aligner.cpp:1636-1720
 *          (encode_audio :591-924, forward_decoder :1088-1169,
 *           extract_timestamp_classes :1280-1306)
 *   qasr_align_tokenize <- ForcedAligner::tokenize_with_timestamps :1564-1609
 *   qasr_model_load_korean_dict <- ForcedAligner::load_korean_dict :1543-1562
 *   qasr_fix_timestamps <- ForcedAligner::fix_timestamp_classes :1183-1265
 *   qasr_get_step_logprobs, qasr_get_logprobs, qasr_stream_logprobs
 *       no reference counterpart: sample_greedy keeps the token id and drops
 *       the logits; these return log softmax(logits)[argmax] of every greedy
 *       token (context option "token_logprobs")
 *   qasr_get_step_topk, qasr_get_topk, qasr_stream_topk
 *       no reference counterpart: the K largest logits of every greedy step
 *       as (id, log-probability) pairs (context option "top_k")
 *   qasr_kv_fork, qasr_get_beams, qasr_prefill_slots
 *       no reference counterpart: beam search (context option "beam_width") --
 *       the KV-cache fork that lets a cache slot continue another slot's
 *       history, the hypotheses of the last beam run, and a prefill into
 *       chosen cache slots
 *   qasr_prefill_score, qasr_score
 *       no reference counterpart: teacher-forced scoring -- the log-probability
 *       of every token of a transcript the caller brings, from an LM head
 *       over many rows that never writes its logits
 *   qasr_set_phrases, qasr_get_phrases, qasr_phrases_validate, qasr_phrase_tokenize
 *       no reference counterpart: hotword boosting -- a list of token
 *       sequences the decoder prefers, matched on the device against every
 *       row's last tokens as one more edit of the constraint stage
 *
 * Conventions (mirroring the reference's):
 *   - return value: 0 = OK, nonzero = error; message via qasr_last_error().
 *     Nothing throws across the boundary.
 *   - host pointers are caller-owned; outputs are written into caller
 *     buffers sized by the documented formula (query helpers provided).
 *   - a context owns its device buffers, KV cache and HIP stream; calls on
 *     one context are stream-ordered and NOT thread-safe (one context per
 *     host thread), exactly as the reference's objects.
 *   - layouts: mel [128][T] mel-major; features [N][1024] row-major; logits
 *     [151936] fp32 (last row only); token ids int32.
 */
#ifndef QASR_CAPI_H
#define QASR_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qasr_model qasr_model;
typedef struct qasr_ctx qasr_ctx;

#define QASR_OK 0
#define QASR_ERR_ARG 1
#define QASR_ERR_IO 2
#define QASR_ERR_FORMAT 3
#define QASR_ERR_DEVICE 4
#define QASR_ERR_STATE 5

typedef struct {
    /* audio encoder (src/gguf_loader.h:15-25) */
    int32_t enc_layers, d_model, enc_heads, enc_ffn, conv_channels, n_mel;
    float enc_eps;
    /* text decoder (src/text_decoder.h:15-31) */
    int32_t vocab_size, hidden_size, dec_layers, n_heads, n_kv_heads, head_dim, dec_ffn;
    float rms_eps, rope_theta;
    int32_t eos_id, pad_id, audio_start_id, audio_end_id, audio_pad_id;
    int32_t weight_type; /* ggml type of the 2-D linear weights: 1 = F16, 8 = Q8_0 */
    /* Qwen3-ForcedAligner files (src/forced_aligner.h:36-73): classify_num > 0 */
    int32_t classify_num, timestamp_token_id;
} qasr_hparams;

typedef struct {
    double t_mel_ms, t_encode_ms, t_prefill_ms, t_decode_ms, t_total_ms;  /* device (HIP event) time */
    int32_t n_decode_steps;
} qasr_timings;

/* ---- errors / version ---------------------------------------------------- */
const char *qasr_last_error(void);                 /* thread-local last message */
const char *qasr_version(void);
int qasr_device_count(int *n);
/* Self-check of the exact prefill attention's expf (fa_exact.hip px_expf_nonpos,
 * the device expf's instruction sequence without its overflow clamp) against the
 * device expf on every non-positive fp32 input (2^31 + 1 values) on `device`:
 * *mismatches = the number of differing results (0 = the kernel's weights are
 * ggml's expf bits).  No reference counterpart (a property of this build). */
int qasr_check_expf_nonpos(int device, uint64_t *mismatches);

/* ---- model ---------------------------------------------------------------- */
/* device >= 0: upload weights to that HIP device.  device = QASR_HOST_ONLY:
 * parse + validate the GGUF and load the tokenizer only (no GPU needed);
 * such a model serves hparams/text calls but cannot create a context. */
#define QASR_HOST_ONLY (-1)
int qasr_model_load(const char *gguf_path, int device, qasr_model **out);
void qasr_model_free(qasr_model *m);
int qasr_model_hparams(const qasr_model *m, qasr_hparams *out);
/* device bytes held by the weight arena */
int64_t qasr_model_device_bytes(const qasr_model *m);

/* ---- context -------------------------------------------------------------- */
/* max_batch: clips per call; max_ctx: decoder positions per sequence
 * (prompt + max_tokens, src/qwen3_asr.cpp:223). */
int qasr_ctx_create(qasr_model *m, int max_batch, int max_ctx, qasr_ctx **out);
void qasr_ctx_free(qasr_ctx *c);

/* ---- size helpers (host-only arithmetic) ---------------------------------- */
int qasr_mel_frames(int n_samples);               /* n/160 (src/mel_spectrogram.cpp:517-522) */
int qasr_encoder_frames(int n_mel_frames);        /* src/audio_encoder.cpp:304-343 */
int qasr_prompt_len(int n_audio_frames);          /* n + 15 (src/qwen3_asr.cpp:170-209) */
/* build the reference chat prompt (no system prompt); returns P, writes
 * ids[P] and the first <|audio_pad|> index to *audio_pos. */
int qasr_build_prompt(const qasr_model *m, int n_audio_frames, int32_t *ids, int *audio_pos);

/* ---- stages (host buffers in/out; each call synchronises its stream) ---- */
/* B clips: pcm[b] has n[b] samples; mel_out receives B blocks of [128][T_b]
 * back to back, T_b = qasr_mel_frames(n[b]). */
int qasr_mel(qasr_ctx *c, const float *const *pcm, const int *n, int B, float *mel_out);
/* mel: B blocks [128][T_b] back to back; feats: [sum N_b][hidden] */
int qasr_encode(qasr_ctx *c, const float *mel, const int *T, int B, float *feats);
/* conv front-end + positional embedding only: [sum N_b][d_model] */
int qasr_encode_conv(qasr_ctx *c, const float *mel, const int *T, int B, float *out);
/* AudioEncoder::encode_no_chunk (src/audio_encoder.cpp:603-852): the conv stack
 * over each clip's T_b frames as ONE chunk (no 100-frame split), sinusoidal PE
 * positions 0 .. N_b - 1, then the same transformer; feats [sum N_b][hidden]
 * with N_b = qasr_encoder_frames_no_chunk(T_b).  ASR models only. */
int qasr_encode_no_chunk(qasr_ctx *c, const float *mel, const int *T, int B, float *feats);
int qasr_encoder_frames_no_chunk(int n_mel_frames);
/* Prefill B sequences from n_past = 0 (the KV cache of sequence b is reset).
 * ids: sum P_b tokens back to back; feats: sum N_b rows of [hidden];
 * audio_pos[b]: first pad index (splice rows [audio_pos, audio_pos+N_b));
 * logits_last (optional) [B][vocab]; argmax (optional) [B]. */
int qasr_prefill(qasr_ctx *c, const int32_t *ids, const int *P, const float *feats,
                 const int *audio_pos, const int *N, int B, float *logits_last, int32_t *argmax);
/* A chunk of P[b] tokens after n_past[b] cached ones (no audio splice), one
 * causal prefill over the cache and the chunk; logits of each chunk's last
 * row.  <- TextDecoder::forward(tokens, n_tokens > 1, n_past > 0)
 *    src/text_decoder.h:125-126 / .cpp:392-581, 583-586 */
int qasr_prefill_chunk(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, int B,
                       float *logits_last, int32_t *argmax);
/* The same chunk with audio rows spliced in (feats: sum N_b rows of [hidden];
 * rows [audio_pos[b], audio_pos[b] + N_b) of chunk b when they fit in it).
 * <- TextDecoder::forward_with_audio(tokens, n, audio, n_audio, pos, n_past)
 *    at any n_past, src/text_decoder.cpp:588-644 (splice :431-459) */
int qasr_prefill_chunk_audio(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, const float *feats,
                             const int *audio_pos, const int *N, int B, float *logits_last, int32_t *argmax);
/* One decode step for B sequences at positions n_past[b] (token tok[b]). */
int qasr_decode_step(qasr_ctx *c, const int32_t *tok, const int *n_past, int B,
                     float *logits, int32_t *argmax);

/* ---- standalone log-mel (no model) ----------------------------------------- */
/* log_mel_spectrogram of src/mel_spectrogram.h:53-55 without a model: an
 * engine keeps the DFT / window tables and a filterbank on one device and runs
 * the context's mel kernels.  filters: [128][201] (NULL: the built-in
 * generate_mel_filters values); mel_out: [128][qasr_mel_frames(n)].  One
 * engine per host thread. */
typedef struct qasr_mel_engine qasr_mel_engine;
int qasr_mel_engine_create(int device, qasr_mel_engine **out);
void qasr_mel_engine_free(qasr_mel_engine *e);
int qasr_mel_engine_run(qasr_mel_engine *e, const float *pcm, int n, const float *filters, float *mel_out);
/* host: generate_mel_filters(128, 400, 16000) (src/mel_spectrogram.cpp:352-395) -> out[128][201] */
int qasr_mel_filters(float *out);

/* ---- whole path ----------------------------------------------------------- */
/* Stage PCM into device HBM (one H2D copy); qasr_run then works from HBM.
 * Any number of clips may be staged (a pool); qasr_run needs B <= max_batch,
 * qasr_run_staged runs subsets of a larger pool. */
int qasr_stage_audio(qasr_ctx *c, const float *const *pcm, const int *n, int B);
/* Greedy transcription of staged clips clips[0..B) (indices into the last
 * qasr_stage_audio call, B <= max_batch) as one batch, from HBM; outputs as
 * qasr_run.  The multi-GPU sharded driver stages a rank's whole shard once
 * and runs it batch by batch (bench.py --utterances). */
int qasr_run_staged(qasr_ctx *c, const int *clips, int B, int max_tokens, int ignore_eos, int32_t *tokens,
                    int *n_tokens, qasr_timings *t);
/* Greedy transcription of the staged clips: tokens [B][max_tokens],
 * n_tokens[B] (trailing EOS popped as src/qwen3_asr.cpp:298-300).
 * ignore_eos != 0: fixed budget of max_tokens steps (throughput mode). */
int qasr_run(qasr_ctx *c, int max_tokens, int ignore_eos, int32_t *tokens, int *n_tokens,
             qasr_timings *t);
/* Optional system-prompt token ids inserted by qasr_run after
 * "<|im_start|>system\n" (src/qwen3_asr.cpp:186-190); n = 0 clears. */
int qasr_set_system_prompt(qasr_ctx *c, const int32_t *ids, int n);
int qasr_transcribe_batch(qasr_ctx *c, const float *const *pcm, const int *n, int B, int max_tokens,
                          int ignore_eos, int32_t *tokens, int *n_tokens, qasr_timings *t);

/* ---- continuous batching ---------------------------------------------------- */
/* Greedy transcription of a queue of clips through `slots` KV-cache slots
 * (1..max_batch; 0 = max_batch) decoding as one batch: a slot whose clip ends (EOS unless ignore_eos, or its token
 * budget) is refilled from the queue at the next chunk boundary (<= 8 decode
 * steps; 1 with a token callback), so a batch never waits for its longest
 * member.  Clip results equal qasr_run's for the same clip.
 *   fetch(user, &pcm, &n_samples, &max_tokens): the next clip -> its id
 *       (>= 0), 16 kHz mono samples (read before fetch is called again) and
 *       its budget (preset to the call's max_tokens); < 0: the queue is empty
 *       (fetch is not called again).  A shared counter behind fetch makes a
 *       dynamic work queue across contexts, threads or processes.
 *   sink(user, id, status, tokens, n_tokens): once per fetched clip, in
 *       completion order: status 0 with the tokens (trailing EOS popped, as
 *       qasr_run), or a QASR_ERR_* code for that clip alone (no audio frames,
 *       context length exceeded, bad arguments) with qasr_last_error() set
 *       during the call; the run goes on with the other clips.
 * The token callback (qasr_set_token_callback) receives the clip id as seq.
 * Returns non-zero only for failures of the run itself (device errors). */
typedef int (*qasr_fetch_fn)(void *user, const float **pcm, int *n_samples, int *max_tokens);
typedef void (*qasr_sink_fn)(void *user, int id, int status, const int32_t *tokens, int n_tokens);
typedef struct {
    int32_t n_clips, n_errors, n_prefills;  /* clips delivered, clips rejected, refill prefills */
    int64_t n_steps;                        /* decode steps (each over all the slots) */
    int64_t slot_steps, live_steps;         /* slot-steps run, of which decoding a live clip */
    double t_prefill_ms, t_decode_ms, t_total_ms;  /* host wall time: refills, decode chunks, call */
    double t_mel_ms, t_encode_ms;           /* device time (HIP events) of the refills' mel / encoder stages,
                                               parts of t_prefill_ms */
    int64_t kv_keys;                        /* sum over decode steps and slots of the keys each slot's attention
                                               read (n_kv): the steps' K / V cache bytes = kv_keys x layers x
                                               n_kv_heads x 128 x 2 B x 2 */
} qasr_stream_stats;
int qasr_run_stream(qasr_ctx *c, int slots, qasr_fetch_fn fetch, qasr_sink_fn sink, void *user, int max_tokens, int ignore_eos,
                    qasr_stream_stats *stats);
/* The same over the staged pool (qasr_stage_audio; inputs already in HBM):
 * fetch(user, &max_tokens) returns the next clip's id (>= 0), or < 0 when the
 * queue is empty; the clip is staged clip id.  An id outside the pool fails
 * that clip (QASR_ERR_ARG through the sink) unless the context option
 * "staged_wrap" is 1: then it is staged clip id % (pool size), so an utterance
 * set larger than the pool reuses its clips, each under its own id. */
typedef int (*qasr_fetch_staged_fn)(void *user, int *max_tokens);
int qasr_run_stream_staged(qasr_ctx *c, int slots, qasr_fetch_staged_fn fetch, qasr_sink_fn sink, void *user,
                           int max_tokens, int ignore_eos, qasr_stream_stats *stats);

/* ---- per-context options (no reference counterpart: MI355X launch tuning) -- */
/* Batch-1 decode runs two fused launches per layer whose roles wait on each
 * other in-launch.  Options, defaulted from the environment
 * variable in brackets at qasr_ctx_create:
 *   "fuse_ffn" [QASR_FUSE_FFN], "fuse_qkv" [QASR_FUSE_QKV], "fuse_o" [QASR_FUSE_O]
 *       1/0: the fused launch or the separate launches (same arithmetic)
 *   "ffn_delay", "ffn_wdelay", "qkv_delay", "o_delay"  in-launch delays (~0.2 us units)
 *   "kvw_delay" [QASR_KVW_DELAY], "k_stagger" [QASR_K_STAGGER], "vt_stagger" [QASR_VT_STAGGER]
 *       the QKV + attention launch's memory requests in the order the attention chain
 *       needs them (same units; 0: every request at its role's start)
 *   "att_spl1" [QASR_ATT_SPL1]   batch <= 8 attention key split: 0 auto, 64, 128
 *   "poll_limit" [QASR_POLL_LIMIT]  bounded in-launch waits (polls); a wait that
 *       runs out makes the call fail with QASR_ERR_DEVICE
 *   "handoff_fence" [QASR_HANDOFF_FENCE]  1: agent-scope release/acquire fences
 *       around every in-launch hand-off (diagnostic)
 *   "dec_layers"  diagnostic: decode steps run only the first n decoder layers (0 = all)
 * Read-only: "slots_ffn", "slots_qkv" (co-resident workgroups of the fused
 * kernels on the context's device).  Setting an option drops captured decode
 * graphs.  Unknown names: QASR_ERR_ARG. */
int qasr_ctx_set_option(qasr_ctx *c, const char *name, int value);
int qasr_ctx_get_option(const qasr_ctx *c, const char *name, int *value);
/* diagnostic copy of decode-step state (after qasr_decode_step): "x" fp32
 * [max_batch][hidden] residual stream, "act" fp16 [max_batch][ffn] SwiGLU
 * output, "qkv" fp32 [max_batch][q+k+v], "att" fp16 [max_batch][n_head*128] */
int qasr_debug_read(qasr_ctx *c, const char *buffer, void *dst, int64_t bytes);

/* ---- token log-probabilities (no reference counterpart) -------------------- */
/* Context option "token_logprobs" [QASR_TOKEN_LOGPROBS], default 0: every
 * greedy step also computes log softmax(logits)[token] of the token it chose,
 * over the whole vocabulary row, on the device (decode batches of 9..128 rows
 * of 1024-wide f16 models: inside the one-launch LM head; every other path:
 * one more small launch over the fp32 logits).  Tokens are the same with the
 * option on or off.  With it off, or before a call of the kind named has run
 * with it on, the three calls return QASR_ERR_STATE; a null or short buffer is
 * QASR_ERR_ARG.
 *   qasr_get_step_logprobs: the value of each row's argmax of the last
 *       qasr_prefill* / qasr_decode_step (B >= that call's B; B values written)
 *   qasr_get_logprobs: the last qasr_run / qasr_run_staged /
 *       qasr_transcribe_batch; out [B][max_tokens] row-major, row b's first
 *       n_tokens[b] entries aligned with its returned tokens (a popped trailing
 *       EOS drops its value too); B and max_tokens at least the run's batch
 *       and longest row
 *   qasr_stream_logprobs: only inside a qasr_sink_fn call of qasr_run_stream*
 *       with status 0: the values of the clip being delivered (one per token
 *       passed to the sink); returns their count (>= 0), or minus an error code */
int qasr_get_step_logprobs(qasr_ctx *c, float *out, int B);
int qasr_get_logprobs(qasr_ctx *c, float *out, int B, int max_tokens);
int qasr_stream_logprobs(qasr_ctx *c, float *out, int cap);

/* ---- top-K token alternatives (no reference counterpart) ------------------- */
/* Context option "top_k" [QASR_TOP_K], 0 .. QASR_TOPK_MAX, default 0 (a value
 * outside the range is QASR_ERR_ARG): with K > 0 every greedy step also yields,
 * per row, the K largest logits of the vocabulary row as (id, logprob) pairs in
 * descending order of the fp32 logit, equal logits by lower id first -- entry 0
 * is the greedy token -- with logprob = logit - logsumexp(row), the value
 * "token_logprobs" reports for entry 0 (bit-identical with both options on).
 * The selection runs on the device -- a small launch over the step's fp32
 * logits, which the step then writes, or inside the one-launch LM head of
 * decode batches -- and nothing is copied to the host but the pairs.  Tokens are
 * the same with the option on or off; it is independent of "token_logprobs".
 * Setting it invalidates earlier results.  Aligner models ignore it.  (The order
 * is that of the greedy argmax key, which compares the fp32 bits: -0.0 sorts
 * below +0.0, where a sort by value would call them equal.)  "lmh_topk"
 * [QASR_LMH_TOPK] is a diagnostic switch between the two device paths at decode
 * batches of 9..64 rows (0 / 2: never / always inside the LM head; default 1:
 * the faster one for this K); results do not depend on it beyond rounding.
 * K must equal the option's value (else QASR_ERR_ARG).  With the option off, or
 * before a call of the kind named has run with it on, the three calls return
 * QASR_ERR_STATE; a null or short buffer is QASR_ERR_ARG.
 *   qasr_get_step_topk: the last qasr_prefill* / qasr_decode_step; ids and
 *       logprobs [B][K] row-major (B >= that call's B; that call's rows written)
 *   qasr_get_topk: the last qasr_run / qasr_run_staged / qasr_transcribe_batch;
 *       ids and logprobs [B][max_tokens][K], row b's first n_tokens[b] steps
 *       aligned with its returned tokens (a popped trailing EOS drops its
 *       alternatives too); B and max_tokens at least the run's batch and
 *       longest row
 *   qasr_stream_topk: only inside a qasr_sink_fn call of qasr_run_stream* with
 *       status 0: the alternatives of the clip being delivered, [n][K] for its n
 *       tokens (cap_tokens >= n); returns n (>= 0), or minus an error code */
#define QASR_TOPK_MAX 8
int qasr_get_step_topk(qasr_ctx *c, int32_t *ids, float *logprobs, int B, int K);
int qasr_get_topk(qasr_ctx *c, int32_t *ids, float *logprobs, int B, int max_tokens, int K);
int qasr_stream_topk(qasr_ctx *c, int32_t *ids, float *logprobs, int cap_tokens, int K);

/* ---- beam search (no reference counterpart) --------------------------------- */
/* Context option "beam_width" [QASR_BEAM_WIDTH], 0 .. QASR_BEAM_MAX, default 0 (a
 * value outside the range is QASR_ERR_ARG); 0 and 1 are greedy decoding, exactly
 * the path without the option.  With W >= 2, qasr_run / qasr_run_staged /
 * qasr_transcribe_batch decode every clip by beam search of width W: B clips use
 * decode rows b * W .. b * W + W - 1 (B * W > max_batch is QASR_ERR_ARG), a step
 * keeps the W best continuations of a clip's rows by summed log-probability, a
 * continuation that ends in EOS among the step's W best is set aside as finished
 * (at most W; W finished end the clip), and at the end the finished and, when the
 * token budget ran out first, the live hypotheses are ranked by sum / length
 * (DESIGN.md "Beam search" gives the rule to the tie).  tokens / n_tokens return
 * each clip's best hypothesis, a trailing EOS popped as in greedy runs.  The beam
 * step and the cache fork run on the device inside the replayed step graph.  The
 * run's internal top-K uses K = W; option "top_k" keeps its value.  While W >= 2:
 * qasr_run_stream* and a run with a token callback set return QASR_ERR_STATE, and
 * so do qasr_get_logprobs / qasr_get_topk after a beam run.  Aligner models ignore
 * the option.
 *
 * qasr_get_beams: all hypotheses of clip `clip` of the last beam run, best first.
 *   tokens / logprobs: [cap_hyp][max_tokens] (logprobs may be NULL)
 *   n_tokens / sum_logprob / finished: [cap_hyp]
 * Returns their number (1..W) or minus an error code.  A popped EOS is not in
 * tokens but is counted in sum_logprob.
 *
 * qasr_kv_fork: rows are forked inside groups of `group` consecutive rows (1..8; B
 * a multiple of group, B <= max_batch; parent[b] in the same group as b).  After
 * the call, for every row b, positions [from[b], to[b]) of cache slot b -- K, V
 * and V^T, every decoder layer and kv head -- hold what slot parent[b] held at
 * those positions BEFORE the call.  Swaps, cycles and several rows sharing one
 * parent are all valid.  Everything else is unchanged: positions outside the
 * range, also inside a partly covered 8-key V^T block; the read-ahead slack of
 * V^T; slots >= B.  parent[b] == b or from[b] >= to[b] is a no-op for that row.
 * Stream-ordered on the context's stream.  Bad arguments: QASR_ERR_ARG.
 *
 * qasr_prefill_slots: qasr_prefill with sequence b's prompt written to KV-cache
 * slot slots[b] (0 .. max_batch - 1); logits, argmax and the step's top-K stay
 * indexed by b. */
#define QASR_BEAM_MAX 8
int qasr_kv_fork(qasr_ctx *c, const int *parent, const int *from, const int *to, int B, int group);
int qasr_get_beams(qasr_ctx *c, int clip, int32_t *tokens, float *logprobs, int *n_tokens, float *sum_logprob, int *finished,
                   int cap_hyp, int max_tokens);
int qasr_prefill_slots(qasr_ctx *c, const int32_t *ids, const int *P, const float *feats, const int *audio_pos, const int *N,
                       const int *slots, int B, float *logits_last, int32_t *argmax);

/* ---- teacher-forced scoring (no reference counterpart) ----------------------- */
/* The log-probability the model gives a transcript the caller brings: for a scored row whose input
 * is token t of a sequence and whose target is the token that follows it,
 *   logprob = logit[target] - logsumexp(logits of the row, whole vocabulary)
 * together with the row's greedy token (the argmax, ties to the lower id, as every greedy step) and
 * that token's log-probability.  The LM head over the scored rows folds the log-sum-exp, the target's
 * logit and the argmax into its GEMM epilogue (csrc/score_head.hip; DESIGN.md "Teacher-forced
 * scoring"): no logits are written and nothing but three values a row reaches the host.  Results are
 * bit-reproducible.  Neither call is captured or touches a step graph; options "token_logprobs",
 * "top_k" and "beam_width" do not change their results.  ASR models only (aligner models:
 * QASR_ERR_STATE).  Both return the number of values written (>= 0) or minus an error code.
 *
 * qasr_prefill_score (stage level): qasr_prefill / _chunk / _chunk_audio / _slots in one call --
 *   n_past, feats (with audio_pos and N) and slots may each be NULL, with the meaning they have there
 *   (n_past NULL: every sequence from position 0) -- plus targets[sum P_b]: the row of ids[t] is scored
 *   against targets[t] (0 .. vocab - 1); targets[t] < 0: the row is not scored.  The outputs are
 *   compacted in row order, one entry per scored row (cap >= their number, else QASR_ERR_ARG).  The
 *   call also does everything the unscored call does (the last rows' argmax, the decode state).
 *
 * qasr_score (whole path, over the pool of qasr_stage_audio): sequence s is the hypothesis
 *   tokens[off_s .. off_s + n_tokens[s]) (off_s = the sum of the earlier n_tokens) of staged clip
 *   clips[s].  Entry k < n_tokens[s] of a sequence is the log-probability of its token k given the
 *   clip's prompt and its tokens 0 .. k - 1; with include_eos != 0 one more entry scores the EOS token
 *   after the last one.  Outputs: n_tokens[s] + (include_eos != 0) entries a sequence, back to back, in
 *   input order (the caller sizes them so); sum_logprob [S] (optional): the float32 sum of each
 *   sequence's entries in order.  The clips named need not be adjacent or sorted: mel, encoder and the
 *   prompt's prefill run once per distinct clip, the prompt's KV rows are forked to the clip's other
 *   hypotheses (qasr_kv_fork's kernel) and every hypothesis's tokens run as one chunk prefill in a
 *   cache slot of their own.  A clip may have at most QASR_SCORE_MAX_HYP hypotheses a call; with D
 *   distinct clips and G the largest number of hypotheses of one clip, D * G <= max_batch.
 *   n_tokens[s] = 0 scores the EOS alone (include_eos) or yields nothing for that sequence.
 *   Errors: null or short buffers, a token >= vocab, a clip index outside the pool, more than
 *   QASR_SCORE_MAX_HYP hypotheses of one clip, D * G > max_batch, and prompt + n_tokens[s] + 1 > max_ctx
 *   ("Context length exceeded") are QASR_ERR_ARG; no staged audio, an aligner model, and option
 *   "fa_exact_prefill" = 0 (the chunk after cached tokens needs it) are QASR_ERR_STATE.
 *   t (optional): t_decode_ms is the scoring after the prompts' prefill (fork, chunk prefill, heads).
 *   After either call the decode state and, after qasr_score, the KV slots are unspecified: the next
 *   decode starts from a prefill, as qasr_run* does. */
#define QASR_SCORE_MAX_HYP 8
int qasr_prefill_score(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, const float *feats,
                       const int *audio_pos, const int *N, const int *slots, int B, const int32_t *targets,
                       float *logprobs, int32_t *greedy_ids, float *greedy_logprobs, int cap);
int qasr_score(qasr_ctx *c, const int *clips, const int32_t *tokens, const int *n_tokens, int S, int include_eos,
               float *logprobs, int32_t *greedy_ids, float *greedy_logprobs, float *sum_logprob, qasr_timings *t);

/* Per-token callback (Qwen3ASR::set_progress_callback, src/qwen3_asr.cpp:255-291):
 * called synchronously on the caller's thread after every greedy token of
 * qasr_run / qasr_run_staged -- the prefill's token first (n_generated = 1) --
 * for every sequence still decoding, in sequence order.  Each step then
 * synchronises the stream (the token must reach the host), so a callback
 * costs throughput; NULL removes it.  The callback must not start another
 * qasr_run / qasr_run_staged / qasr_run_stream* / qasr_decode_step on any
 * context of the same GPU: a batch-1 run holds that device's fused-launch
 * lock (not recursive) while it calls back. */
int qasr_set_token_callback(qasr_ctx *c, void (*cb)(void *user, int seq, int n_generated, int32_t token), void *user);

/* ---- measurement ---------------------------------------------------------- */
/* --profile (src/timing.h QWEN3_TIMER sections, src/main.cpp:409-411): on = 1
 * records per-section device time (HIP events) of every qasr_run --
 * mel_spectrogram, audio_encoding.{total,conv_chunk,transformer},
 * decode.initial_forward, decode.token (one per step), transcribe.total --
 * accumulated until the next qasr_set_profile (which resets).  The run also
 * carries roctx ranges "qasr.run" / "qasr.decode" for rocprofv3 --marker-trace. */
int qasr_set_profile(qasr_ctx *c, int on);
/* the report in QWEN3_TIMER_REPORT's layout; returns its length, writes at
 * most cap-1 bytes + NUL */
int qasr_profile_report(qasr_ctx *c, char *out, int cap);
/* Probe one launch group of every greedy decode step of qasr_run with HIP
 * events on the context's stream: kernel 1 = LM head + fused argmax; 2 = the
 * QKV projection + attention (+ o-projection) of decoder layer "probe_layer"
 * (option, default 14) -- at batch 1 the fused qkv_attn1_kernel; 3 = that
 * layer's FFN (batch 1: ffn1_kernel).  The rest of each step replays as two
 * graphs around it (one extra graph launch per step); 0 disables.  Setting a
 * probe resets the totals; bytes_per_launch = mean algorithmic HBM bytes of
 * the probed launches (weights + the layer's K/V rows at each step's n_kv).
 * 4 = at decode batches (9..128 rows) that layer's attention launch alone
 * (decode_attn_seq_kernel: K / V^T rows + q / output rows), by the device
 * clock (qasr_get_probe_device). */
int qasr_set_probe(qasr_ctx *c, int kernel);
int qasr_get_probe(qasr_ctx *c, double *total_ms, int64_t *launches, double *bytes_per_launch);
/* The same launches timed by the device clock (first workgroup start -> last
 * workgroup end, 100 MHz s_memrealtime, folded in-kernel by the batch <= 8
 * decode kernels and the decode-batch attention): the kernels' own duration, without the ~2.5 us of dispatch
 * and event processing an event pair around one launch includes. */
int qasr_get_probe_device(qasr_ctx *c, double *total_ms, int64_t *launches);

/* ---- forced alignment (Qwen3-ForcedAligner model files) ------------------- */
/* Device part of ForcedAligner::align for one clip: text_ids are the words'
 * BPE ids, each word followed by two timestamp tokens (qasr_align_tokenize);
 * classes[i] = argmax class of the i-th timestamp token (x 80 ms), *n_ts =
 * their number (writes at most cap).  The context needs max_ctx >=
 * qasr_align_prompt_len.  t: t_mel_ms, t_encode_ms, t_prefill_ms (= decode). */
int qasr_align(qasr_ctx *c, const float *pcm, int n_samples, const int32_t *text_ids, int n_text,
               int32_t *classes, int cap, int *n_ts, qasr_timings *t);
/* words -> ids with timestamps; language "korean" uses the loaded dictionary
 * (qasr_model_load_korean_dict), else whitespace words.  Returns the number of
 * ids (writes at most cap); *n_words = number of words. */
int qasr_align_tokenize(const qasr_model *m, const char *text, const char *language, int32_t *ids, int cap,
                        int *n_words);
/* the words of that split, joined by '\n' (words never contain whitespace);
 * returns the length, writes at most cap-1 bytes + NUL */
int qasr_align_words(const qasr_model *m, const char *text, const char *language, char *out, int cap);
int qasr_model_load_korean_dict(qasr_model *m, const char *path);
/* Host policy of the Qwen3ASR class (no reference counterpart): the shape a
 * context (cur_b slots x cur_l positions) is recreated with for a call that
 * needs (batch, n_ctx) -- the union of both while its KV cells do not exceed
 * the larger shape's own, else exactly (batch, n_ctx). */
void qasr_ctx_grow_shape(int cur_b, int cur_l, int batch, int n_ctx, int *nb, int *nl);
/* LIS repair of raw classes (in -> out, n values) */
int qasr_fix_timestamps(const int32_t *classes, int n, int32_t *out);
/* prompt length of an alignment: n_text + 2 + pads(mel frames of n_samples) */
int qasr_align_prompt_len(int n_samples, int n_text);
/* The whole alignment -> the CLI's JSON document {"words": [{"word", "start",
 * "end"}...]} (src/main.cpp:257-276).  Returns its length (or minus the error
 * code on failure); writes at most cap-1 bytes + NUL. */
int qasr_align_json(qasr_ctx *c, const float *pcm, int n_samples, const char *text, const char *language,
                    char *out, int cap, qasr_timings *t);
/* B clips in one aligner pass (mel + windowed encoder of all clips, one
 * prefill of the B prompts, one classify GEMM over every timestamp row): the
 * B documents of qasr_align_json as one JSON array, in input order; each
 * clip's classes equal its single-clip run.  B <= the context's max_batch.
 * Returns the length (or minus the error code); writes at most cap-1 + NUL.
 * <- the --transcribe-align pipeline over many files, src/main.cpp:416-500 */
int qasr_align_json_batch(qasr_ctx *c, const float *const *pcm, const int *n_samples, const char *const *text, int B,
                          const char *language, char *out, int cap, qasr_timings *t);

/* ---- text (host) ---------------------------------------------------------- */
/* UTF-8 text for ids (special <|..|> and [PAD..] tokens skipped); returns the
 * byte length (excluding NUL), writes at most cap-1 bytes + NUL. */
int qasr_detokenize(const qasr_model *m, const int32_t *ids, int n, char *out, int cap);
/* byte-level BPE; returns number of ids (writes at most cap). */
int qasr_tokenize(const qasr_model *m, const char *text, int32_t *ids, int cap);

/* ---- host utilities (no device needed) ------------------------------------ */
/* PCM16 RIFF reader (src/mel_spectrogram.cpp:130-221); returns n or -1.
 * out may be NULL to query n. */
int qasr_load_wav(const char *path, float *out, int max_n, int *sample_rate);
int qasr_write_wav(const char *path, const float *pcm, int n, int sample_rate);
/* deterministic synthetic clip: seed 1000+i recipe */
int qasr_synth_pcm(uint64_t seed, int n_samples, float *out);
/* synthetic GGUF with the reference tensor names/shapes/dtypes.
 * config: "full" (Qwen3-ASR-0.6B dims) or "tiny" (test dims);
 * wtype: 1 = f16, 8 = q8_0 for linear weights. */
int qasr_write_synthetic_gguf(const char *path, const char *config, uint64_t seed, int wtype);
/* version of that writer's output: bumped whenever the file it writes for a
 * given (config, seed, wtype) changes, so a cached synthetic model is keyed on it */
int qasr_synthetic_gguf_version(void);

/* ---- test only: one kernel launcher on caller-supplied arrays --------------- */
/* (csrc/kernel_harness.hip; tests/kernel_util.py holds the bindings.)  Every
 * pointer is a host pointer; a null input is not passed on, a null output is not
 * allocated.  Per call: each input is uploaded with `guard` extra rows after its
 * last row filled with 0xFF bytes (fp16 / fp32 NaN; 0x7F for int8 quants); each
 * output is allocated with `guard` rows before and after its rows, every byte
 * pre-filled with 0xFF, and copied back whole ((rows + 2 * guard) * ld elements)
 * after the launch.  The launch goes on the null stream and is synchronised.
 * Returns QASR_OK with `declined` = 1 and `msg` set where the launcher took no
 * kernel (a false return or a take_declined message), QASR_ERR_DEVICE on a HIP
 * error; `tag` names the kernel that ran (kernels.h note_kernel). */
typedef struct {
    int32_t launcher;        /* 0 launch_gemm (AM_DENSE), 1 launch_gemm_q8, 2 launch_gemm_skinny, 3 launch_gemm_skinny_q8 */
    int32_t epi;             /* GemmEpi */
    int32_t M, N, K;
    int32_t lda, ldw, ldad, ldr, ldo, ldo16, ldoq;
    int32_t regs_staged, n_valid, skinny_inflight, wdef;
    int32_t guard;
    int32_t pe_rows;         /* rows of pe [pe_rows][N] */
    const uint16_t *A;       /* fp16 [M][lda] */
    const uint16_t *W;       /* fp16 [N][ldw] */
    const int8_t *Aq;        /* int8 [M][lda] */
    const float *Ad;         /* [M][ldad] */
    const int8_t *Wq;        /* int8 [N][ldw] */
    const uint16_t *Wd;      /* fp16 [N][K / 32] */
    const float *bias;       /* [N] */
    const float *res;        /* [M][ldr] */
    const float *pe;
    const int32_t *pe_pos;   /* [M] */
    float *out_f32;          /* [M + 2 guard][ldo] */
    uint16_t *out_f16;       /* [M + 2 guard][ldo16] */
    int8_t *out_q;           /* [M + 2 guard][ldoq] */
    float *out_d;            /* [M + 2 guard][ldoq / 32] */
    uint64_t *amax;          /* [M + 2 guard] packed argmax keys (rows zero before the launch) */
    uint16_t *gelu_out;      /* [65536]: the engine's GELU table as the launch used it */
    int32_t declined;
    char tag[64];
    char msg[256];
} qasr_kt_gemm_args;
int qasr_kt_gemm(int device, qasr_kt_gemm_args *a);

typedef struct {
    int32_t epi;             /* GemmEpi */
    int32_t M, N, K;         /* N = output columns */
    int32_t wrows;           /* weight rows: N, or 2 N for the SwiGLU epilogues */
    int32_t ldx, ldxh, ldr, ldo, ldo16;
    int32_t embd_rows, hist_stride;
    int32_t guard;
    int32_t launches;        /* >= 1: the same launch repeated on the same device state */
    float eps;
    const float *x;          /* fp32 [M][ldx] */
    const uint16_t *xh;      /* fp16 [M][ldxh] */
    const float *norm_w;     /* [K] */
    const uint16_t *W;       /* fp16 [wrows][K] */
    const int8_t *Wq;        /* int8 [wrows][K], with Wd */
    const uint16_t *Wd;      /* fp16 [wrows][K / 32] */
    const float *bias;       /* [N] */
    const float *res;        /* [M][ldr] */
    const int32_t *embd_ids; /* [M] */
    const uint16_t *embd;    /* fp16 [embd_rows][K] */
    float *x_store;          /* [M + 2 guard][ldx] */
    float *out_f32;          /* [M + 2 guard][ldo] */
    uint16_t *out_f16;       /* [M + 2 guard][ldo16] */
    uint64_t *amax;          /* [8] in (zero at rest) / out */
    /* EPI_ARGMAX bookkeeping group: all or none; in / out */
    uint32_t *done;          /* [1] */
    int32_t *tok_out;        /* [8] */
    int32_t *hist;           /* [M][hist_stride] */
    int32_t *step;           /* [1] */
    int32_t *pos;            /* [8] */
    int32_t declined;
    char tag[64];
    char msg[256];
} qasr_kt_gemv_args;
int qasr_kt_gemv(int device, qasr_kt_gemv_args *a);

typedef struct {
    int32_t M, K, ldx, gather_C, guard;
    const float *x32;        /* one of x32 / x16: [M][ldx] */
    const uint16_t *x16;
    int8_t *q;               /* [M + 2 guard][K] */
    float *d;                /* [M + 2 guard][K / 32] */
} qasr_kt_quant_args;
int qasr_kt_quantize_q8(int device, qasr_kt_quant_args *a);

/* kv_fork_kernel on caller-supplied caches: kc / vc [layers][slots + guard][n_kv_head][max_ctx][128] and
 * vt [layers][slots + guard][n_kv_head][128 * vt_ctx] fp16, where vt_ctx = max_ctx rounded up to 64 plus 384
 * and the last `guard` slots of every layer are guard slots the caller filled with 0xFF; in / out, whole */
typedef struct {
    int32_t layers, n_kv_head, max_ctx, slots, guard;
    int32_t B, group, blocks;      /* blocks: 8-key blocks of the grid (0 = up to max_ctx) */
    const int32_t *parent, *from, *to;   /* [B] */
    uint16_t *kc, *vc, *vt;
    int32_t declined;
} qasr_kt_kv_fork_args;
int qasr_kt_kv_fork(int device, qasr_kt_kv_fork_args *a);

/* beam_select_kernel on caller-supplied state: G groups of W rows, every group at step t.  In: ids / lps
 * [G * W][W] (at t = 0 the kernel reads row g for group g).  In / out: cum, the finished table (fin_*
 * [G * W]), n_fin / done [G].  Out, each [1 + 2 guard][G * W] with the guard rows 0xFF: tok, parent, from, to
 * and the history slot h_par / h_id / h_lp.  t_out [G]: the groups' step index after the launch. */
typedef struct {
    int32_t W, G, t, eos, guard;
    const int32_t *ids;
    const float *lps;
    const int32_t *P;              /* [G] */
    float *cum;
    int32_t *fin_row, *fin_t;
    float *fin_sum, *fin_lp;
    int32_t *n_fin, *done, *t_out;
    int32_t *tok, *parent, *from, *to, *h_par, *h_id;
    float *h_lp;
    int32_t declined;
} qasr_kt_beam_select_args;
int qasr_kt_beam_select(int device, qasr_kt_beam_select_args *a);

/* launch_score_head on caller-supplied arrays (csrc/score_head.hip), `launches` (>= 1) times on the same
 * device state.  In, each with `guard` rows of 0xFF after its last row: A fp16 [R][lda], W fp16 [N][ldw],
 * target [R].  Out, each [R + 2 guard] with the guard entries 0xFF before the launch: lp, gid, glp.  The
 * scratch is filled with 0xFF bytes before the first launch. */
typedef struct {
    int32_t R, N, K, lda, ldw, n_valid;
    int32_t cols_fast;       /* ScoreHeadArgs::cols_fast */
    int32_t guard, launches;
    const uint16_t *A;
    const uint16_t *W;
    const int32_t *target;
    float *lp;
    int32_t *gid;
    float *glp;
    int32_t declined;
    char tag[64];
    char msg[256];
} qasr_kt_score_args;
int qasr_kt_score_head(int device, qasr_kt_score_args *a);

/* ---- temperature sampling with n-best ---------------------- */
/* With sampling on, every token a prefill or decode step yields is drawn on the device from
 * softmax(logits / temperature) restricted to the tokens whose probability is at least min_p times the
 * greedy token's (seeded Gumbel-max; the rule is normative, DESIGN.md §5.5 and tests/sample_util.py).  A
 * draw is identified by (seed, clip, sample, t) and depends on nothing else: not on its row, its batch or
 * the grid.  clip = the staged pool index in qasr_run / qasr_run_staged, sample = 0 .. n_best - 1, t = the
 * token's index within its hypothesis (0 = drawn from the prefill's logits).
 * temperature in (0, 100], min_p in [0, 1], n_best in 1 .. QASR_SAMPLE_MAX, else QASR_ERR_ARG; NULL or
 * temperature <= 0 turns sampling off (nothing of the greedy paths changes).  Changing temperature, min_p
 * or seed re-captures no step graph.  While sampling is on, qasr_run_stream* and option beam_width >= 2
 * are refused with QASR_ERR_STATE; aligner models ignore it; qasr_score / qasr_prefill_score are unaffected.
 * Log-probabilities (option token_logprobs, qasr_get_samples) are log softmax(logits)[token] at T = 1, the
 * model's own value; option top_k is unchanged (entry 0 stays the greedy token, which need not be the drawn one). */
#define QASR_SAMPLE_MAX 8
typedef struct {
    float temperature, min_p;
    uint64_t seed;
    int32_t n_best;
} qasr_sampling;
int qasr_set_sampling(qasr_ctx *c, const qasr_sampling *s);
int qasr_get_sampling(const qasr_ctx *c, qasr_sampling *out);
/* Stage level: the identities rows 0 .. B - 1 of qasr_prefill* / qasr_decode_step draw with, t advancing by
 * one per draw (n_best plays no part there; their `argmax` output then carries the drawn token).  A context
 * starts with row b = (clip b, sample 0, t 0).  QASR_ERR_STATE while sampling is off. */
int qasr_set_sample_streams(qasr_ctx *c, const int32_t *clip, const int32_t *sample, const int32_t *t, int B);
/* The n_best hypotheses of clip `clip` (index into the run's clips) of the last sampling qasr_run, in sample
 * order: tokens / logprobs [cap_hyp][max_tokens] (logprobs may be NULL), n_tokens / sum_logprob [cap_hyp].
 * A trailing EOS is popped from the tokens and log-probabilities but counted in the fp32 in-order sum, as
 * in qasr_get_beams.  The run's own tokens / n_tokens are sample 0's.  After an n_best >= 2 run
 * qasr_get_logprobs / qasr_get_topk return QASR_ERR_STATE.  Returns the count, or minus an error code
 * (QASR_ERR_STATE after a run with sampling off). */
int qasr_get_samples(qasr_ctx *c, int clip, int32_t *tokens, float *logprobs, int *n_tokens, float *sum_logprob, int cap_hyp,
                     int max_tokens);

/* test only: launch_sample (csrc/sample.hip) on caller-supplied arrays, `launches` (>= 1) times; t is uploaded
 * again before every launch, so repeated launches draw the same tokens.  In: logits [R / src_div][ld] with
 * `guard` rows of 0xFF after the last row, greedy [R / src_div] (each inside [0, n_valid)), clip / sample / t
 * [R].  Out, each [R + 2 guard] with the guard entries 0xFF before the launch: tok, key (the winning fp32 key),
 * hist (one history slot).  t_out [R]: t after the last launch; skey_out [R]: the key scratch after it (zero
 * at rest; it lies between two 4 KiB fences of 0xFF the launch must leave alone).  slices: 0 = the
 * launcher's choice.  dump_n > 0: no draw; dump [dump_n] = G(u_n) for n = dump_n0 .. dump_n0 + dump_n - 1
 * (n < 2^23), the device's value of the rule's steps 2 and 3. */
typedef struct {
    int32_t R, ld, n_valid, src_div, slices, guard, launches;
    float inv_T, cut;
    uint64_t seed;
    const float *logits;
    const int32_t *greedy, *clip, *sample, *t;
    int32_t *tok;
    float *key;
    int32_t *hist, *t_out;
    uint64_t *skey_out;
    uint32_t dump_n0, dump_n;
    float *dump;
    int32_t declined;
    char tag[64];
    char msg[256];
} qasr_kt_sample_args;
int qasr_kt_sample(int device, qasr_kt_sample_args *a);

/* ---- decoding constraints ---------------------------------- */
/* With constraints on, the fp32 logits of every prefill and decode step are edited on the device before a
 * token is chosen, and the token is chosen again from the edited row (the rule is normative, DESIGN.md §5.6
 * and tests/constrain_util.py; every operation is one rounded fp32 operation, so it is exact).  For a row
 * with raw logits l and history h[0 .. t) (the tokens the engine returned for that row since its last
 * prefill, the prefill's own token included), in this order:
 *   1. repetition_penalty p != 1: every distinct token v among the last penalty_last_n tokens of h (0: all
 *      of h) gets l[v] > 0 ? l[v] * (1 / p) : l[v] * p;
 *   2. every listed token gets l[bias_ids[k]] += bias[k] (-inf suppresses the token);
 *   3. no_repeat_ngram n >= 1: every token that would complete an n-gram h already holds gets -inf (n = 1
 *      bans every token seen);
 *   4. the token is the largest value of the edited row, equal values by lower id.
 * The edited row replaces the step's logits everywhere: the `logits` output of qasr_prefill* and
 * qasr_decode_step, option token_logprobs (log softmax of the edited row), option top_k (entry 0 is the
 * constrained token) and the sampler (qasr_set_sampling draws from the edited row).
 * Covered: qasr_prefill*, qasr_decode_step, qasr_run, qasr_run_staged, qasr_transcribe_batch, with sampling at
 * any n_best, f16 and Q8_0 models.  At stage level the history is the engine's own record of what its calls
 * returned: qasr_decode_step continues the history of the last prefill whatever tokens the caller feeds back
 * (QASR_ERR_STATE once it holds max_ctx tokens).  While constraints are on, qasr_run_stream* and option
 * beam_width >= 2 are refused with QASR_ERR_STATE; qasr_score / qasr_prefill_score are unaffected; aligner
 * models ignore the setting.  Changing the values re-captures no step graph; with constraints off nothing of
 * the other paths changes. */
#define QASR_NGRAM_MAX 8
#define QASR_BIAS_MAX 1024
typedef struct {
    int32_t no_repeat_ngram;      /* 0 = off, 1 .. QASR_NGRAM_MAX */
    float repetition_penalty;     /* 0 < p <= 10, 1 = off */
    int32_t penalty_last_n;       /* >= 0, 0 = the whole history */
    int32_t n_bias;               /* 0 .. QASR_BIAS_MAX */
    const int32_t *bias_ids;      /* [n_bias] distinct ids in [0, vocab) */
    const float *bias;            /* [n_bias] each finite or -inf */
} qasr_constraints;
/* Host only (no device): 0, or QASR_ERR_ARG with a message naming the violated range.  vocab <= 0: the ids'
 * upper bound is not checked. */
int qasr_constraints_validate(const qasr_constraints *k, int vocab);
/* NULL, or no_repeat_ngram = 0, repetition_penalty = 1 and n_bias = 0 together, turns constraints off; any
 * n_bias > 0 turns them on.  QASR_ERR_ARG as qasr_constraints_validate; QASR_ERR_STATE for a model whose
 * vocabulary exceeds 2^20. */
int qasr_set_constraints(qasr_ctx *c, const qasr_constraints *k);
/* The setting in force (n_bias = 0 and the neutral values while off).  ids / bias [cap] receive the bias list
 * where they are non-NULL (cap < n_bias: QASR_ERR_ARG); out's two pointers are set to ids / bias. */
int qasr_get_constraints(const qasr_ctx *c, qasr_constraints *out, int32_t *ids, float *bias, int cap);

/* test only: launch_constrain (csrc/constrain.hip) on caller-supplied arrays, `launches` (>= 1) times, each from
 * the same device state (the logits are uploaded again before every launch).  In: logits [R / src_div][ld],
 * greedy [R / src_div] (each inside [0, n_valid)), hist [R][hist_stride] (ids inside [0, n_valid)), t (0 ..
 * hist_stride - 1: the history length and the slot written) and the parameters.  Out: tok [R + 2 guard] and
 * hist_slot [R + 2 guard] (the history slot t of every row; the rest of the history must come back unchanged,
 * which the call checks) with the guard entries 0xFF before the launch; logits_out [R / src_div + 2 guard][ld],
 * the edited rows between guard rows of 0xFF; skey_out / flag_out [R / src_div]: the scratch after the last
 * launch (zero at rest; each lies between two 4 KiB fences of 0xFF the launch must leave alone).  slices: 0 =
 * the launcher's choice. */
typedef struct {
    int32_t R, ld, n_valid, src_div, slices, guard, launches, hist_stride, t;
    int32_t no_repeat_ngram;
    float repetition_penalty;
    int32_t penalty_last_n, n_bias;
    const int32_t *bias_ids;
    const float *bias;
    const float *logits;
    const int32_t *greedy, *hist;
    int32_t *tok, *hist_slot;
    float *logits_out;
    uint64_t *skey_out;
    int32_t *flag_out;
    int32_t declined;
    char tag[64];
    char msg[256];
} qasr_kt_constrain_args;
int qasr_kt_constrain(int device, qasr_kt_constrain_args *a);

/* ---- hotword boosting -------------------------------------- */
/* A phrase list makes the decoder prefer given token sequences (hotwords, phrase hints, contextual biasing).
 * It is one more edit of the constraint stage above, step 2b between the bias (2) and the ban (3), and the rule
 * is as normative and as exact (tests/phrase_util.py).  For a row with history h[0 .. t): phrase
 * k matches at position j (0 <= j < len_k) when j <= t and the row's last j tokens are the phrase's first j
 * (j = 0 always matches); a match makes token ph_k[j] a candidate with bonus boost_k, and every token with a
 * candidate gets l[x] += the largest of its candidates' bonuses: one rounded fp32 add a boosted column, after
 * the bias and before the ban (a banned column stays -inf).  There is no cumulative score and nothing is taken
 * back when a phrase is not completed.
 * Phrases alone turn the constraint stage on; everything said above of the stage holds: the edited row is what
 * the logits output, token_logprobs, top_k and the sampler read; qasr_run_stream* and beam_width >= 2 are
 * refused with QASR_ERR_STATE while phrases are on; scoring is unaffected; aligner models ignore the setting.
 * Changing the list, or turning phrases on or off while the stage stays on, re-captures no step graph. */
#define QASR_PHRASE_MAX 4096
#define QASR_PHRASE_LEN_MAX 16
typedef struct {
    int32_t n_phrases;     /* 0 .. QASR_PHRASE_MAX */
    const int32_t *ids;    /* the phrases' tokens back to back, each in [0, vocab) */
    const int32_t *len;    /* [n_phrases] each 1 .. QASR_PHRASE_LEN_MAX */
    const float *boost;    /* [n_phrases] each finite, 0 < b <= 100 */
} qasr_phrases;
/* Host only (no device): 0, or QASR_ERR_ARG with a message naming the violated range.  vocab <= 0: the ids'
 * upper bound is not checked.  Duplicates and phrases that are prefixes or suffixes of one another are allowed. */
int qasr_phrases_validate(const qasr_phrases *p, int vocab);
/* NULL or n_phrases = 0 turns phrases off.  QASR_ERR_ARG as qasr_phrases_validate, and for a list whose trie
 * exceeds 65,536 edges (65,537 nodes); QASR_ERR_STATE for a model whose vocabulary exceeds 2^20. */
int qasr_set_phrases(qasr_ctx *c, const qasr_phrases *p);
/* The list in force (n_phrases = 0 while off).  ids [cap_ids], len / boost [cap_phrases] receive it where they
 * are non-NULL (too small: QASR_ERR_ARG); out's pointers are set to them. */
int qasr_get_phrases(const qasr_ctx *c, qasr_phrases *out, int32_t *ids, int32_t *len,
                     float *boost, int cap_ids, int cap_phrases);
/* host only: the tokenisations a hotword text needs -- of `text` (outer white space trimmed)
 * and of " " + text, the second dropped when equal; returns their number (1 or 2), or minus
 * an error code (empty text, a variant longer than 16 tokens, short buffers).  ids receives the variants back to
 * back, len [2] their lengths. */
int qasr_phrase_tokenize(const qasr_model *m, const char *text, int32_t *ids, int32_t *len,
                         int cap_ids);

/* test only: qasr_kt_constrain with a phrase list (compiled by csrc/phrase_host.h): the same arrays, guard rows,
 * fences and re-armed scratch; scanned_out [R / src_div] receives per logits row whether it took the scan (its
 * raw argmax was edited) or the fast path. */
typedef struct {
    int32_t R, ld, n_valid, src_div, slices, guard, launches, hist_stride, t;
    int32_t no_repeat_ngram;
    float repetition_penalty;
    int32_t penalty_last_n, n_bias;
    const int32_t *bias_ids;
    const float *bias;
    const float *logits;
    const int32_t *greedy, *hist;
    int32_t *tok, *hist_slot;
    float *logits_out;
    uint64_t *skey_out;
    int32_t *flag_out;
    int32_t n_phrases;
    const int32_t *ph_ids, *ph_len;
    const float *ph_boost;
    int32_t *scanned_out;
    int32_t declined;
    char tag[64];
    char msg[256];
} qasr_kt_phrases_args;
int qasr_kt_phrases(int device, qasr_kt_phrases_args *a);

/* ---- audio at other sample rates: the resampler to 16 kHz ----------------
 * Every other entry point takes 16 kHz mono float PCM.  The *_rate entry points take a rate per
 * clip and resample on the device, in front of the mel stage, by one rule (csrc/resample_host.h
 * states it in full): a polyphase Kaiser-windowed sinc with L = 16000 / gcd, M = rate / gcd,
 * Z = 32 zero crossings a side, BETA = 9, cut-off 0.96 x the lower Nyquist, fp32 taps, fp64
 * accumulation in tap order.  The device result equals the host rule bit for bit for finite
 * input.  A clip at 16000 is copied unchanged.  Supported: 4000 <= rate <= 192000 with
 * L <= 640 (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400,
 * 192000, ...); any other rate is QASR_ERR_ARG with the rate in qasr_last_error().
 * `rate` may be NULL: every clip is at 16000 (the call is then the plain one).
 *
 * host only (no device is touched):
 *   qasr_resample_plan   L, M and H (taps a phase = 2H + 1) of a rate; 16000: 1, 1, 0
 *   qasr_resample_len    output samples of n_in input samples, (n_in * L + M - 1) / M; minus an
 *                        error code for an unsupported rate, n_in < 0 or a result past INT_MAX
 *   qasr_resample_taps   the table h[L][2H + 1] into out (cap floats); returns its size (cap 0:
 *                        the size alone), or minus an error code
 *   qasr_resample_host   the rule on the CPU: out receives qasr_resample_len(n, rate) samples;
 *                        returns that count, or minus an error code
 * stage level, as qasr_mel (host buffers in and out, synchronises):
 *   qasr_resample        B clips -> out, the resampled clips back to back
 *   qasr_resample_last_us  device time of the last qasr_resample's kernel launch on this context, in
 *                        microseconds (HIP events around the launch alone), or minus an error code
 * whole path:
 *   qasr_stage_audio_rate       as qasr_stage_audio; the pool then holds the 16 kHz clips, so
 *                               qasr_run, qasr_run_staged, qasr_score and qasr_run_stream_staged
 *                               serve it unchanged
 *   qasr_transcribe_batch_rate  qasr_stage_audio_rate + qasr_run
 *   qasr_run_stream_rate        qasr_run_stream whose fetch also returns the clip's rate; prompt
 *                               and context checks use the resampled length, and an unsupported
 *                               rate fails that clip alone through the sink */
int qasr_resample_plan(int rate, int *L, int *M, int *H);
int qasr_resample_len(int n_in, int rate);
int qasr_resample_taps(int rate, float *out, int cap);
int qasr_resample_host(const float *pcm, int n, int rate, float *out);
int qasr_resample(qasr_ctx *c, const float *const *pcm, const int *n, const int *rate, int B, float *out);
int qasr_resample_last_us(qasr_ctx *c);
int qasr_stage_audio_rate(qasr_ctx *c, const float *const *pcm, const int *n, const int *rate, int B);
int qasr_transcribe_batch_rate(qasr_ctx *c, const float *const *pcm, const int *n, const int *rate, int B,
                               int max_tokens, int ignore_eos, int32_t *tokens, int *n_tokens, qasr_timings *t);
typedef int (*qasr_fetch_rate_fn)(void *user, const float **pcm, int *n_samples, int *rate, int *max_tokens);
int qasr_run_stream_rate(qasr_ctx *c, int slots, qasr_fetch_rate_fn fetch, qasr_sink_fn sink, void *user,
                         int max_tokens, int ignore_eos, qasr_stream_stats *stats);

/* test only: the resample kernel on B packed clips (pcm: the raw clips back to back, n_in / rate [B]) with the
 * library's tap tables.  The device input is followed by `guard` floats of 0xFF bytes (NaN); out receives, per
 * clip, `guard` floats of 0xFF, the clip's qasr_resample_len outputs and `guard` floats of 0xFF again
 * ([sum n_out + 2 * guard * B] floats).  launches 2: a second launch on the same device state into out2.
 * tile receives the outputs a workgroup computes. */
typedef struct {
    int32_t B, guard, launches;
    const int32_t *n_in, *rate;
    const float *pcm;
    float *out, *out2;
    int32_t tile;
} qasr_kt_resample_args;
int qasr_kt_resample(int device, qasr_kt_resample_args *a);

/* ---- long recordings: pause segmentation into zero-copy pool clips --------
 * A recording longer than one decoder context is uploaded once, cut on the device at its
 * quietest points, and every piece becomes a pool entry that points into the recording: no PCM
 * is copied and no clip is staged a second time.  The rule (csrc/segment_host.h states it in
 * full), for a recording of n samples at 16 kHz, F = n / 160 frames:
 *   e[f] = sum of the frame's 160 squared samples, fp64, ascending;
 *   s[f] = sum of e over [max(0, f - H), min(F - 1, f + H)], fp64, ascending (H = smooth_half);
 *   a = 0; while F - a > max_frames: the next cut is the frame of
 *     [a + min_frames, min(a + max_frames, F - min_frames)] with the smallest s, equal values to
 *     the LARGER frame; a = the cut;
 *   segment k covers samples [160 cut_k, 160 cut_k+1), the last one ends at n; every recording has
 *     at least one segment;
 *   peak[k] = the maximum of s over the segment's frames (0 without frames), peak_rec the maximum
 *     over the recording; with skip_ratio >= 0 segment k is silent iff
 *     peak[k] <= skip_ratio * peak_rec; skip_ratio < 0: never silent.
 * The device results equal the host rule exactly (cuts) and bit for bit (e, s, peaks) for finite
 * input.  Ranges: 1 <= min_frames, 2 * min_frames <= max_frames <= 2^20, 0 <= smooth_half <= 64,
 * skip_ratio not NaN; anything else is QASR_ERR_ARG with the range in qasr_last_error().
 * Defaults: 3000, 1000, 5, -1.  params NULL: the defaults.
 *
 * host only (no device is touched):
 *   qasr_segment_validate  0, or QASR_ERR_ARG
 *   qasr_segment_host      the rule on the CPU: start frame, peak and silent flag of up to cap
 *                          segments (each array may be NULL); returns the segment count (which may
 *                          exceed cap: nothing past cap is written), or minus an error code
 * stage level, as qasr_resample (host buffers in and out, synchronises; the pool is untouched):
 *   qasr_segment           B recordings at 16 kHz.  e, s: [sum F] back to back (each may be NULL);
 *                          cuts, peak, silent: [B][cap] (each may be NULL); n_seg [B]; peak_rec [B]
 *                          (may be NULL).  A recording with more than cap segments is QASR_ERR_ARG.
 *   qasr_segment_last_us   device time of the last qasr_segment's launches on this context in
 *                          microseconds (HIP events around the launches alone); cut_us (may be
 *                          NULL) receives the cut kernel's share.  Minus an error code on failure.
 * whole path:
 *   qasr_stage_long        B recordings (rate NULL: 16 kHz; else per recording, resampled on the
 *                          device as qasr_stage_audio_rate) -> the pool becomes all segments in
 *                          recording order, entry = recording offset + 160 * cut.  Returns the
 *                          segment count, or minus an error code.  qasr_run_staged,
 *                          qasr_run_stream_staged, qasr_score and beam, sampling and constraint
 *                          runs then serve the pool as they do any other; qasr_run keeps its
 *                          B <= max_batch check.  A later qasr_stage_audio* clears the table.
 *   qasr_get_segments      the table of recording rec (0 .. B - 1 of the last qasr_stage_long): start
 *                          (16 kHz samples from the recording's own start), n_samples, peak, silent
 *                          of up to cap segments (each array may be NULL); returns the count of
 *                          that recording's segments, or minus an error code (QASR_ERR_STATE
 *                          before a qasr_stage_long and after a qasr_stage_audio*).  Segment j of
 *                          recording r is pool entry (segments of the recordings before r) + j.
 * Aligner models: qasr_stage_long and qasr_get_segments are QASR_ERR_STATE. */
typedef struct {
    int32_t max_frames, min_frames, smooth_half;
    double skip_ratio;
} qasr_segment_params;
int qasr_segment_validate(const qasr_segment_params *p);
int qasr_segment_host(const float *pcm, int n, const qasr_segment_params *p, int *cuts, double *peak, int *silent, int cap);
int qasr_segment(qasr_ctx *c, const float *const *pcm, const int *n, int B, const qasr_segment_params *p, double *e, double *s,
                 int *cuts, double *peak, int *silent, int *n_seg, double *peak_rec, int cap);
int qasr_segment_last_us(qasr_ctx *c, int *cut_us);
int qasr_stage_long(qasr_ctx *c, const float *const *pcm, const int *n, const int *rate, int B, const qasr_segment_params *p);
int qasr_get_segments(qasr_ctx *c, int rec, long long *start, int *n_samples, double *peak, int *silent, int cap);

/* test only: the segmentation kernels on B packed recordings (pcm: the recordings back to back, n [B]; a
 * recording starts wherever the one before it ends).  The device input is followed by `guard` floats of 0xFF
 * bytes (NaN).  Every output sits between `guard` elements of 0xFF bytes and comes back whole:
 * e, s [guard + sum F + guard] doubles; cuts [guard + B * cap + guard] ints and peak likewise in doubles
 * (recording b's slots at b * cap); n_seg [guard + B + guard] ints, peak_rec likewise in doubles.
 * cap must be >= F / min_frames + 1 for every recording.  launches 2: a second pair of launches on the same
 * device state into the *2 outputs.  tile receives the frames a workgroup of the energy kernel computes. */
typedef struct {
    int32_t B, guard, launches, cap;
    qasr_segment_params prm;
    const int32_t *n;
    const float *pcm;
    double *e, *s, *peak, *peak_rec;
    int32_t *cuts, *n_seg;
    double *e2, *s2, *peak2, *peak_rec2;
    int32_t *cuts2, *n_seg2;
    int32_t tile;
} qasr_kt_segment_args;
int qasr_kt_segment(int device, qasr_kt_segment_args *a);

/* test only: the norm, RoPE and prefill / encoder attention launchers on caller-supplied arrays (csrc/kernel_harness.hip;
 * tests/attn_util.py holds the bindings).  The conventions of qasr_kt_gemm: inputs with `guard` rows of 0xFF bytes (NaN)
 * after their last row, outputs [rows + 2 guard][ld] pre-filled with 0xFF and returned whole, arguments validated before
 * any launch (QASR_ERR_ARG), `declined` = 1 with `msg` where the launcher took no kernel (nothing written). */
typedef struct {
    int32_t kind;            /* 0 launch_layernorm_f16, 1 launch_rmsnorm_f16, 2 launch_rmsnorm_q8 */
    int32_t M, D;
    int32_t ldx, xrows;      /* x [xrows][ldx]; kind 0: ldx == D; xrows >= M, row_idx entries in [0, xrows) */
    int32_t guard;
    float eps;
    const float *x;
    const int32_t *row_idx;  /* kind 1: [M] or null */
    const float *w, *b;      /* [D]; kind 0: either may be null, b unused by kinds 1 / 2 */
    uint16_t *y;             /* kinds 0 / 1: one of y, y32 [M + 2 guard][D] */
    float *y32;
    int8_t *yq;              /* kind 2: [M + 2 guard][D] and yd [M + 2 guard][D / 32] */
    float *yd;
    int32_t declined;
    char msg[256];
} qasr_kt_norm_args;
int qasr_kt_norm(int device, qasr_kt_norm_args *a);

/* launch_qkv_post.  The caches are in / out between fences (qasr_kt_kv_fork): kc / vc [slots][n_kv_head][max_ctx][128],
 * vt [slots][n_kv_head][128 * vt_ctx(max_ctx)] fp16, as the caller filled them (0xFF), back whole.  row_seq in
 * [0, slots), row_pos in [0, min(max_ctx, max_pos)). */
typedef struct {
    int32_t rows, n_head, n_kv_head, max_ctx, slots, max_pos, guard;
    float eps;
    const float *qkv;        /* [rows][(n_head + 2 n_kv_head) * 128] */
    const int32_t *row_seq, *row_pos;
    const float *q_norm, *k_norm;   /* [128] */
    const float *rope;       /* [max_pos][64][2] (cos, sin) */
    uint16_t *q_out;         /* [rows + 2 guard][n_head * 128] */
    float *q32, *k32;        /* both or neither: [rows + 2 guard][n_head * 128], [rows + 2 guard][n_kv_head * 128] */
    uint16_t *kc, *vc, *vt;
    int32_t declined;
    char msg[256];
} qasr_kt_qkv_post_args;
int qasr_kt_qkv_post(int device, qasr_kt_qkv_post_args *a);

/* launch_enc_attention: qkv [rows][3 D] fp32, segments [seg_start, seg_start + seg_len) inside the rows, seg_len in
 * 1 .. max_len; D != 64 H is QASR_ERR_ARG here (the launcher throws).  One of out / out32 [rows + 2 guard][D]. */
typedef struct {
    int32_t rows, D, H, n_seg, max_len, f32_mfma, guard;
    const float *qkv;
    const int32_t *seg_start, *seg_len;
    uint16_t *out;
    float *out32;
    int32_t declined;
    char msg[256];
} qasr_kt_enc_attention_args;
int qasr_kt_enc_attention(int device, qasr_kt_enc_attention_args *a);

/* launch_prefill_attention (exact 0) or launch_prefill_attention_exact (exact 1).  q fp16 [rows][n_head * 128]; kc / vc
 * [slots][n_kv_head][max_ctx][128] fp16, uploaded with kKvPadRows (kernels.h) rows of 0xFF (fp16 NaN) after the last
 * region -- the exact kernel stages V up to 127 rows past a sequence's last key -- between fences, and verified
 * unchanged after the launch.  Sequence s: rows seq_row0[s] .. + seq_len[s] - 1 (1 .. max_len of them), cache slot
 * seq_slot[s], keys 0 .. seq_pos0[s] + seq_len[s] - 1 <= max_ctx - 1.  q32 / k32 (exact only, both, without seq_pos0):
 * fp32 [rows][n_head * 128] / [rows][n_kv_head * 128].  One of out / out32 [rows + 2 guard][n_head * 128]. */
typedef struct {
    int32_t exact, rows, n_head, n_kv_head, max_ctx, slots, n_seq, max_len, guard;
    float scale;
    const uint16_t *q;
    const uint16_t *kc, *vc;
    const int32_t *seq_row0, *seq_len, *seq_slot;
    const int32_t *seq_pos0; /* or null */
    const float *q32, *k32;  /* or null */
    uint16_t *out;
    float *out32;
    int32_t declined;
    char msg[256];
} qasr_kt_prefill_attention_args;
int qasr_kt_prefill_attention(int device, qasr_kt_prefill_attention_args *a);

/* The decode attention launchers that do not wait in-launch (never the fused batch-1 launch: qcnt, gran, sgran,
 * att_done, trace, stamp and err are always null).  mode 0: launch_decode_attention; 1: the same in scores mode,
 * scores [B * n_head + 2 guard][max_ctx] out (masked positions keep the sentinel); 2: the scores launch, then
 * launch_decode_attention_exact; 3: launch_decode_attention_exact_seq (false -> declined); 4: the chain alone,
 * launch_decode_attention_exact on scores_in [B * n_head][max_ctx] (any whole n_head / n_kv_head; qkv, norms, rope,
 * kc and vc unused and may be null).
 * Row b is cache slot b: kc / vc [B][n_kv_head][max_ctx][128] (uploaded with kKvPadRows rows of 0xFF after the last
 * region), vt [B][n_kv_head][128 * vt_ctx(max_ctx)] fp16, in / out between fences.  part is sized from
 * decode_max_splits() and counter [B][n_kv_head] is zero on entry, both between fences; a counter that is not zero
 * again after a launch is QASR_ERR_STATE.  repeat 2 (modes 0, 2, 3): a second launch on the same part and counter,
 * the caches restored in between (and required equal after both), into the *_b outputs.
 * Before any launch (QASR_ERR_ARG): 0 <= pos[b] < min(max_ctx, max_pos); grid_splits * 64 > max pos; the launch's
 * split count <= decode_max_splits(); exactly one of out / out32 / outq + outd (mode 1: scores instead)
 * [B + 2 guard][n_head * 128] (outd: [..][n_head * 4]).
 * tag: the kernels taken, e.g. "decode_split<64>", "decode_seq<0>+decode_exact<1>". */
typedef struct {
    int32_t mode, B, n_head, n_kv_head, max_ctx, max_pos, grid_splits, spl1, spl_batch, stream_blocks, kv_nt, fx_seq, repeat, guard;
    float scale, eps;
    const int32_t *pos;      /* [B] */
    const float *qkv;        /* [B][(n_head + 2 n_kv_head) * 128] */
    const float *q_norm, *k_norm;   /* [128] */
    const float *rope;       /* [max_pos][64][2] (cos, sin) */
    const float *scores_in;  /* mode 4 */
    uint16_t *kc, *vc, *vt;
    float *scores;           /* mode 1 */
    uint16_t *out, *out_b;
    float *out32, *out32_b;
    int8_t *outq, *outq_b;
    float *outd, *outd_b;
    int32_t declined;
    char tag[64];
    char msg[256];
} qasr_kt_decode_attention_args;
int qasr_kt_decode_attention(int device, qasr_kt_decode_attention_args *a);

/* The conv front end (tests/conv_util.py holds the bindings).  layer 1: launch_conv1 over mel; 2 / 3: launch_gemm in
 * AM_CONV2 / AM_CONV3 with EPI_GELU_F16, N = C, K = 9 C, ldw = conv_kpad(C) = 9 C rounded up to 128, ldo16 = C,
 * row_start taken from the chunks' row2 / row3 -- called directly, through no context.  chunks: ChunkDesc of
 * csrc/kernels.h field for field, every field filled by the caller.
 * The input -- mel, in_len floats (layer 1), or the activation the layer reads, [in_len][C] fp16 (act1 / act2) -- is
 * uploaded between guard_in elements (floats / rows of C) of 0xFF bytes on both sides, so a tap that should have been
 * padding reads NaN inside the allocation at the first and the last chunk too; the caller passes at least the widest
 * row of the input image + 1 (mel: a clip's frames + 1).  W: layer 1 fp16 [C][9]; layers 2 / 3 fp16 [C][conv_kpad(C)],
 * the padding columns as the caller chose them (zero where the 8-phase tile is expected: its contract; NaN
 * elsewhere), with `guard` rows of 0xFF after it; bias [C].  out: [out_rows + 2 guard][C] fp16 as qasr_kt_gemm's.
 * Before any launch (QASR_ERR_ARG): every chunk's reads and writes lie inside in_len / out_rows, the output rows of
 * the chunks are consecutive from 0 and out_rows is their sum (layers 2 / 3: find_chunk's contract). */
typedef struct {
    int64_t mel_off;
    int32_t T, L, Lv, W1, W2, W3, row1, row2, row3, enc_row;
} qasr_kt_chunk;
typedef struct {
    int32_t layer;           /* 1, 2, 3 */
    int32_t C, regs_staged, n_chunks;
    int32_t in_len, out_rows;
    int32_t guard, guard_in;
    int32_t max_w1;          /* layer 1: the grid's width (the engine: the widest chunk's W1) */
    const qasr_kt_chunk *chunks;
    const float *mel;        /* layer 1 */
    const uint16_t *act;     /* layers 2 / 3 */
    const uint16_t *W;
    const float *bias;
    uint16_t *out;
    uint16_t *gelu_out;      /* [65536] */
    int32_t declined;
    char tag[64];
    char msg[256];
} qasr_kt_conv_args;
int qasr_kt_conv(int device, qasr_kt_conv_args *a);

#ifdef __cplusplus
}
#endif
#endif
