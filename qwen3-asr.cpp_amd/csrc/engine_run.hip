// engine_run.hip -- the whole-pipeline drivers: qasr_run over the staged clips
// (front end, greedy loop, result assembly) and the continuous-batching stream,
// with the readers of their per-token log-probabilities.
#include <rocprofiler-sdk-roctx/roctx.h>

#include <chrono>
#include <functional>

#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

qasr::eng::RoctxRange::RoctxRange(const char *name) { roctxRangePushA(name); }
qasr::eng::RoctxRange::~RoctxRange() { roctxRangePop(); }

extern "C" int qasr_stage_audio(qasr_ctx *c, const float *const *pcm, const int *n, int B) {
    if (!c || !pcm || !n || B <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->m->device));
    c->seg_valid = false;   // (the pool is no qasr_stage_long's from here on)
    c->staged_n.assign(n, n + B);
    c->staged_off.assign(B, 0);
    for (int b = 0; b < B; b++)
        if (n[b] < 0) return fail(QASR_ERR_ARG, "negative length");
    const int rc = pack_pcm(c, pcm, n, B, c->staged_off);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// ------------------------------------------------------------- front end
// mel -> encoder -> prompts -> prefill for the clips at d_pcm + off[r] (n[r]
// samples each), the prefill into KV-cache slots `slots` (nullptr: clip r ->
// slot r).  Events are recorded on the context stream before the mel, after
// it, after the encoder and (e_prefill, optional) after the prefill.
// check_prompt(r, P, audio_pos) sees every prompt before the prefill is
// launched; a non-zero return ends the call with it.
static int front_end(qasr_ctx *c, const float *d_pcm, const std::vector<long> &off, const std::vector<int> &n, hipEvent_t e_start,
                     hipEvent_t e_mel, hipEvent_t e_enc, hipEvent_t e_prefill, const std::vector<int> *slots,
                     const std::function<int(int, int, int)> &check_prompt, FrontEnd &o) {
    const int R = (int)n.size();
    hipStream_t s = c->st;
    std::vector<long> mo;
    std::vector<int> T;
    int rc;
    HIPCHK(hipEventRecord(e_start, s));
    if ((rc = run_mel(c, off, n, mo, T, d_pcm))) return rc;
    HIPCHK(hipEventRecord(e_mel, s));
    if ((rc = run_encoder(c, c->mel.as<float>(), mo, T, false, o.Nb))) return rc;
    HIPCHK(hipEventRecord(e_enc, s));
    std::vector<int32_t> ids;
    o.P.assign(R, 0);
    o.audio_pos.assign(R, 0);
    for (int r = 0; r < R; r++) {
        std::vector<int32_t> p = build_prompt(c->m->hp, o.Nb[r], c->sys_ids, &o.audio_pos[r]);
        o.P[r] = (int)p.size();
        if ((rc = check_prompt(r, o.P[r], o.audio_pos[r]))) return rc;
        ids.insert(ids.end(), p.begin(), p.end());
    }
    if ((rc = run_prefill(c, ids, o.P, c->feats.as<float>(), o.audio_pos, o.Nb, false, slots))) return rc;
    if (e_prefill) HIPCHK(hipEventRecord(e_prefill, s));
    return 0;
}

// ---------------------------------------------------------------- qasr_run
// greedy loop (src/qwen3_asr.cpp:270-296): step k feeds token k at position P+k-1.
// Leaves the device token history in hist ([B][hist_cap]) and the steps run in steps.
int qasr::eng::greedy_loop(qasr_ctx *c, int B, int max_tokens, int ignore_eos, std::vector<int32_t> &hist, int &steps) {
    const Hparams &hp = c->m->hp;
    hipStream_t s = c->st;
    int rc;
    hist.resize((size_t)B * c->hist_cap);
    steps = 0;
    RoctxRange dec_range("qasr.decode");
    // profile: an event after every step (decode.token); k = 0-based step
    auto step = [&](int k) -> int {
        int r = launch_step(c, B, k);
        if (r || !c->profile_on) return r;
        while ((int)c->step_ev.size() <= k) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            c->step_ev.push_back(e);
        }
        HIPCHK(hipEventRecord(c->step_ev[k], s));
        return 0;
    };
    if (c->tok_cb) {
        // per-token callback (src/qwen3_asr.cpp:255-291): every token reaches
        // the host as it is produced -- one synchronisation per step
        std::vector<char> live(B, 1);
        std::vector<int32_t> tok(B);
        auto deliver = [&](int n_gen) -> int {
            HIPCHK(hipMemcpyAsync(tok.data(), c->d_tok, B * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (int b = 0; b < B; b++) {
                if (!live[b]) continue;
                c->tok_cb(c->tok_cb_user, b, n_gen, tok[b]);
                if (!ignore_eos && tok[b] == hp.eos_id) live[b] = 0;
            }
            return 0;
        };
        if ((rc = deliver(1))) return rc;
        int k = 1;
        for (; k < max_tokens && std::count(live.begin(), live.end(), 1) > 0; k++) {
            if ((rc = step(k - 1)) || (rc = deliver(k + 1))) return rc;
        }
        steps = k - 1;
        HIPCHK(hipMemcpyAsync(hist.data(), c->d_hist, hist.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    } else if (ignore_eos) {
        for (int k = 1; k < max_tokens; k++)
            if ((rc = step(k - 1))) return rc;
        steps = max_tokens - 1;
        HIPCHK(hipMemcpyAsync(hist.data(), c->d_hist, hist.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    } else {
        const int chunk = 8;
        auto all_done = [&](int done) -> int {   // 1 = every sequence has emitted EOS
            if (hipMemcpyAsync(hist.data(), c->d_hist, hist.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                return -1;
            for (int b = 0; b < B; b++) {
                bool fin = false;
                for (int k = 0; k <= done && !fin; k++) fin = hist[(size_t)b * c->hist_cap + k] == hp.eos_id;
                if (!fin) return 0;
            }
            return 1;
        };
        int done = 0, st = 0;
        while (done + 1 < max_tokens && (st = all_done(done)) == 0) {
            const int todo = std::min(chunk, max_tokens - 1 - done);
            for (int k = 0; k < todo; k++)
                if ((rc = step(done + k))) return rc;
            done += todo;
        }
        if (st < 0) return fail(QASR_ERR_DEVICE, "device copy failed in decode loop");
        HIPCHK(hipMemcpyAsync(hist.data(), c->d_hist, hist.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        steps = done;
    }
    return 0;
}

// the stage timings of a run from its events (t may be null)
int qasr::eng::run_timings(qasr_ctx *c, int steps, qasr_timings *t) {
    if (!t) return 0;
    float a, b2, c2, d;
    (void)hipEventElapsedTime(&a, c->ev[EV_START], c->ev[EV_MEL]);
    (void)hipEventElapsedTime(&b2, c->ev[EV_MEL], c->ev[EV_ENC]);
    (void)hipEventElapsedTime(&c2, c->ev[EV_ENC], c->ev[EV_PREFILL]);
    (void)hipEventElapsedTime(&d, c->ev[EV_PREFILL], c->ev[EV_END]);
    t->t_mel_ms = a; t->t_encode_ms = b2; t->t_prefill_ms = c2; t->t_decode_ms = d;
    t->t_total_ms = (double)a + b2 + c2 + d;
    t->n_decode_steps = steps;
    return 0;
}

// after the timed span of a run: the device error word, probe and profile
// records, then the history's rows as the caller's tokens (and their
// log-probabilities, option token_logprobs) and the stage timings
int qasr::eng::run_results(qasr_ctx *c, int B, int max_tokens, int ignore_eos, const std::vector<int32_t> &hist, int steps,
                           int32_t *tokens, int *n_tokens, qasr_timings *t) {
    const Hparams &hp = c->m->hp;
    hipStream_t s = c->st;
    int rc;
    if ((rc = check_dev_err(c))) return rc;
    if ((rc = probe_collect(c, B, steps))) return rc;
    // option token_logprobs: columns 0 .. steps of the history parallel to d_hist (after the timed span)
    const bool lp = c->fuse.token_logprobs != 0;
    const int lp_cols = std::min(steps + 1, max_tokens);
    std::vector<float> lph;
    c->lp_run_B = 0;
    if (lp) {
        lph.resize((size_t)B * lp_cols);
        HIPCHK(hipMemcpy2DAsync(lph.data(), (size_t)lp_cols * 4, c->d_lphist, (size_t)c->hist_cap * 4, (size_t)lp_cols * 4, B,
                                hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        c->lp_run.assign((size_t)B * max_tokens, 0.f);
        c->lp_run_n.assign(B, 0);
    }
    // option top_k: the same columns of its two histories, K entries a step
    const int K = c->fuse.top_k;
    std::vector<int32_t> tkid;
    std::vector<float> tklp;
    c->tk_run_B = 0;
    if (K) {
        tkid.resize((size_t)B * lp_cols * K);
        tklp.resize(tkid.size());
        HIPCHK(hipMemcpy2DAsync(tkid.data(), (size_t)lp_cols * K * 4, c->d_tkhid, (size_t)c->hist_cap * K * 4, (size_t)lp_cols * K * 4,
                                B, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpy2DAsync(tklp.data(), (size_t)lp_cols * K * 4, c->d_tkhlp, (size_t)c->hist_cap * K * 4, (size_t)lp_cols * K * 4,
                                B, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        c->tk_run_id.assign((size_t)B * max_tokens * K, -1);
        c->tk_run_lp.assign((size_t)B * max_tokens * K, 0.f);
        c->tk_run_n.assign(B, 0);
    }
    if (c->profile_on) {   // the reference's QWEN3_TIMER sections (src/timing.h), device time
        auto add = [&](const char *name, hipEvent_t e0, hipEvent_t e1) -> int {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            auto &v = c->prof[name];
            v.first += ms;
            v.second += 1;
            return 0;
        };
        if ((rc = add("mel_spectrogram", c->ev[EV_START], c->ev[EV_MEL])) ||
            (rc = add("audio_encoding.total", c->ev[EV_MEL], c->ev[EV_ENC])) ||
            (rc = add("audio_encoding.conv_chunk", c->ev[EV_MEL], c->ev[EV_ENC_CONV])) ||
            (rc = add("audio_encoding.transformer", c->ev[EV_ENC_CONV], c->ev[EV_ENC])) ||
            (rc = add("decode.initial_forward", c->ev[EV_ENC], c->ev[EV_PREFILL])) ||
            (rc = add("transcribe.total", c->ev[EV_START], c->ev[EV_END])))
            return rc;
        for (int k = 0; k < steps; k++)
            if ((rc = add("decode.token", k ? c->step_ev[k - 1] : c->ev[EV_PREFILL], c->step_ev[k]))) return rc;
    }
    if (c->d_trace) {   // dev trace dump: raw [6][4096][8] u64
        std::vector<unsigned long long> tr(qasr_ctx::kTraceBytes / 8);
        HIPCHK(hipMemcpy(tr.data(), c->d_trace, tr.size() * 8, hipMemcpyDeviceToHost));
        if (FILE *f = fopen(c->trace_path.c_str(), "wb")) {
            (void)fwrite(tr.data(), 8, tr.size(), f);
            fclose(f);
        }
    }
    for (int b = 0; b < B; b++) {
        int nt = 0;
        for (int k = 0; k <= steps && k < max_tokens; k++) {
            const int32_t tk = hist[(size_t)b * c->hist_cap + k];
            if (lp) c->lp_run[(size_t)b * max_tokens + nt] = lph[(size_t)b * lp_cols + k];
            for (int j = 0; j < K; j++) {
                c->tk_run_id[((size_t)b * max_tokens + nt) * K + j] = tkid[((size_t)b * lp_cols + k) * K + j];
                c->tk_run_lp[((size_t)b * max_tokens + nt) * K + j] = tklp[((size_t)b * lp_cols + k) * K + j];
            }
            tokens[(size_t)b * max_tokens + nt++] = tk;
            if (!ignore_eos && tk == hp.eos_id) break;
        }
        if (!ignore_eos && nt > 0 && tokens[(size_t)b * max_tokens + nt - 1] == hp.eos_id) nt--;   // (its value goes with it)
        n_tokens[b] = nt;
        if (lp) c->lp_run_n[b] = nt;
        if (K) c->tk_run_n[b] = nt;
    }
    if (lp) { c->lp_run_B = B; c->lp_run_T = max_tokens; }
    if (K) { c->tk_run_B = B; c->tk_run_T = max_tokens; }
    if ((rc = run_timings(c, steps, t))) return rc;
    return 0;
}

// the front end over the staged clips of a run (slots: prefill_layers' slot map), with the reference's two prompt checks
int qasr::eng::front_end_staged(qasr_ctx *c, int max_tokens, const std::vector<int> *slots, FrontEnd &fe) {
    auto check_prompt = [&](int, int P, int audio_pos) -> int {   // the reference's two messages
        if (audio_pos < 0) return fail(QASR_ERR_ARG, "No audio_pad token found in input sequence");
        if (P + max_tokens > c->max_ctx) return fail(QASR_ERR_ARG, "Context length exceeded (prompt + max_tokens > max_ctx)");
        return 0;
    };
    return front_end(c, c->pcm.as<float>(), c->staged_off, c->staged_n, c->ev[EV_START], c->ev[EV_MEL], c->ev[EV_ENC],
                     c->ev[EV_PREFILL], slots, check_prompt, fe);
}

extern "C" int qasr_run(qasr_ctx *c, int max_tokens, int ignore_eos, int32_t *tokens, int *n_tokens, qasr_timings *t) {
    if (!c || max_tokens <= 0 || !tokens || !n_tokens) return fail(QASR_ERR_ARG, "bad arguments");
    const int B = (int)c->staged_n.size();
    if (B == 0) return fail(QASR_ERR_STATE, "no staged audio");
    if (constraints_on(c) && c->fuse.beam_width >= 2)
        return fail(QASR_ERR_STATE, "decoding constraints and beam search (option beam_width >= 2) exclude each other");
    if (sampling_on(c)) return sample_run(c, max_tokens, ignore_eos, tokens, n_tokens, t);
    c->last_run_sampled = false;
    if (c->fuse.beam_width >= 2 && !c->m->hp.aligner) return beam_run(c, max_tokens, ignore_eos, tokens, n_tokens, t);
    c->last_run_beam = false;
    if (B > c->max_batch) return fail(QASR_ERR_ARG, "staged clips exceed the context's max_batch (qasr_run_staged runs subsets)");
    HIPCHK(hipSetDevice(c->m->device));
    std::unique_lock<std::mutex> dev_lk;
    if (takes_fused(c, B)) {
        dev_lk = std::unique_lock<std::mutex>(device_lock(c->m->device));
        // the fused launches re-arm the next layer's counters as they go; within
        // a run the launch mode only moves from fused to separate (longer
        // contexts), so zero them once here, whatever the previous run left
        if (int rc = reset_counters(c)) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    RoctxRange run_range("qasr.run");   // host-side ranges for rocprofv3 --marker-trace
    int rc;
    FrontEnd fe;
    if ((rc = front_end_staged(c, max_tokens, nullptr, fe))) return rc;
    c->run_P = fe.P;
    if ((rc = decode_graph(c, B, false, *std::max_element(fe.P.begin(), fe.P.end())))) return rc;
    if ((rc = probe_arm(c, max_tokens - 1))) return rc;
    std::vector<int32_t> hist;
    int steps = 0;
    if ((rc = greedy_loop(c, B, max_tokens, ignore_eos, hist, steps))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_END], c->st));
    HIPCHK(hipEventSynchronize(c->ev[EV_END]));
    return run_results(c, B, max_tokens, ignore_eos, hist, steps, tokens, n_tokens, t);
}

extern "C" int qasr_run_staged(qasr_ctx *c, const int *clips, int B, int max_tokens, int ignore_eos, int32_t *tokens,
                               int *n_tokens, qasr_timings *t) {
    if (!c || !clips || B <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    if (B > c->max_batch) return fail(QASR_ERR_ARG, "subset exceeds the context's max_batch");
    std::vector<int> n(B);
    std::vector<long> off(B);
    for (int b = 0; b < B; b++) {
        if (clips[b] < 0 || clips[b] >= (int)c->staged_n.size()) return fail(QASR_ERR_ARG, "staged clip index out of range");
        n[b] = c->staged_n[clips[b]];
        off[b] = c->staged_off[clips[b]];
    }
    std::swap(n, c->staged_n);
    std::swap(off, c->staged_off);
    c->run_clip_ids.assign(clips, clips + B);   // (a sampling run keys its draws by the pool index)
    const int rc = qasr_run(c, max_tokens, ignore_eos, tokens, n_tokens, t);
    c->run_clip_ids.clear();
    std::swap(n, c->staged_n);   // the staged pool stays for the next subset
    std::swap(off, c->staged_off);
    return rc;
}

// ------------------------------------------------------ continuous batching
// qasr_run_stream: `slots` KV-cache slots (<= max_batch) decode together;
// a slot whose clip ends (EOS, or its token budget) is refilled at the next
// chunk boundary -- mel + encoder + prefill of the next clips from `fetch`
// into exactly the freed slots (prefill_layers' slot map), the other slots'
// caches untouched -- so a batch never idles on its longest member (the
// reference decodes one utterance at a time, src/qwen3_asr.cpp:270-296; the
// tokens of a clip depend only on its own rows).  Every chunk of <= 8 steps
// (1 with a token callback) replays the step graphs of qasr_run, then the
// host reads the chunk's tokens, delivers finished clips to `sink` and
// re-uploads the slots' (token, position) state.  A slot with no clip is
// parked at position 0 (its writes stay inside its own cache slot).
namespace {
struct StreamSlot {
    int id = -1, P = 0, budget = 0;
    std::vector<int32_t> toks;
    std::vector<float> lps;   // option token_logprobs: one per token
    std::vector<int32_t> tkid;   // option top_k: K per token
    std::vector<float> tklp;
};
}  // namespace

// next(clip) -> false when the queue is empty; a clip is host samples (pcm, n)
// or a clip of the staged pool (staged >= 0); host samples may come at another rate (qasr_run_stream_rate), which
// the refill resamples on the device
struct StreamClip {
    int id = -1, budget = 0, n = 0, staged = -1, rate = qasr::kResampleOutRate;
    const float *pcm = nullptr;
};
static int run_stream(qasr_ctx *c, int slots, const std::function<bool(StreamClip &)> &next, qasr_sink_fn sink, void *user,
                      int max_tokens, int ignore_eos, qasr_stream_stats *stats) {
    if (!c || !sink || max_tokens <= 0 || slots < 0 || slots > c->max_batch) return fail(QASR_ERR_ARG, "bad arguments");
    if (c->fuse.beam_width >= 2 && !c->m->hp.aligner) return fail(QASR_ERR_STATE, "the continuous-batching stream has no beam search (option beam_width >= 2)");
    if (sampling_on(c)) return fail(QASR_ERR_STATE, "the continuous-batching stream has no sampling (qasr_set_sampling)");
    if (constraints_on(c)) return fail(QASR_ERR_STATE, "the continuous-batching stream has no decoding constraints (qasr_set_constraints)");
    HIPCHK(hipSetDevice(c->m->device));
    const int S = slots ? slots : c->max_batch;
    std::unique_lock<std::mutex> dev_lk;
    if (takes_fused(c, S)) {
        dev_lk = std::unique_lock<std::mutex>(device_lock(c->m->device));
        if (int rc = reset_counters(c)) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    const Hparams &hp = c->m->hp;
    hipStream_t s = c->st;
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t0) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    qasr_stream_stats st{};
    // device time of each refill's mel and encoder stages (the utterance set's encoder roofline)
    struct StageEvents {
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~StageEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));
    std::vector<StreamSlot> sl(S);
    bool open = true;
    int rc;
    const bool lp = c->fuse.token_logprobs != 0;
    c->lp_sink = nullptr;
    const int K = c->fuse.top_k;
    c->tk_sink_id = nullptr;
    c->tk_sink_lp = nullptr;
    // a finished clip: trailing EOS popped (src/qwen3_asr.cpp:298-300)
    auto deliver = [&](StreamSlot &x) {
        std::vector<int32_t> &t = x.toks;
        if (!ignore_eos && !t.empty() && t.back() == hp.eos_id) {
            t.pop_back();
            if (lp) x.lps.pop_back();
            if (K) { x.tkid.resize(x.tkid.size() - K); x.tklp.resize(x.tklp.size() - K); }
        }
        if (lp) c->lp_sink = &x.lps;   // qasr_stream_logprobs, for the length of the call
        if (K) { c->tk_sink_id = &x.tkid; c->tk_sink_lp = &x.tklp; }   // qasr_stream_topk likewise
        sink(user, x.id, 0, t.data(), (int)t.size());
        c->lp_sink = nullptr;
        c->tk_sink_id = nullptr;
        c->tk_sink_lp = nullptr;
        st.n_clips++;
        x.id = -1;
        x.toks.clear();
        x.lps.clear();
        x.tkid.clear();
        x.tklp.clear();
    };
    auto reject = [&](int id, int code, const char *msg) {   // per-clip error: the message is qasr_last_error() inside sink
        fail(code, msg);
        sink(user, id, code, nullptr, 0);
        st.n_errors++;
    };
    // fill free slots from the queue until every slot holds a live clip or the queue is empty
    auto refill = [&]() -> int {
        bool refilled = false;
        for (;;) {
            std::vector<int> freeS;
            for (int i = 0; i < S; i++)
                if (sl[i].id < 0) freeS.push_back(i);
            if (freeS.empty() || !open) return 0;
            if (refilled && c->fuse.refill_group > 0) return 0;   // one group a refill: decode steps come between groups
            if (c->fuse.refill_group > 0 && (int)freeS.size() > c->fuse.refill_group) freeS.resize(c->fuse.refill_group);
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<int> ids, ns, budgets, slots;
            std::vector<int> raw_n, rates;   // host clips as fetched; ns holds their lengths at 16 kHz
            bool resample = false;
            std::vector<float> pcm;   // host clips of this refill, packed (-> c->spcm)
            std::vector<long> off;
            bool staged = false;
            while (ids.size() < freeS.size()) {
                StreamClip k;
                k.budget = max_tokens;
                if (!next(k)) { open = false; break; }
                const int id = k.id;
                if (k.staged >= 0) {
                    if (k.staged >= (int)c->staged_n.size()) { reject(id, QASR_ERR_ARG, "staged clip index out of range"); continue; }
                    k.n = c->staged_n[k.staged];
                }
                const int raw = k.n;
                if (k.staged < 0 && k.rate != qasr::kResampleOutRate && k.n >= 0) {   // every check below sees the output length
                    if ((k.n = qasr_resample_len(raw, k.rate)) < 0) { const std::string why = qasr_last_error(); reject(id, QASR_ERR_ARG, why.c_str()); continue; }
                }
                const int P = qasr_prompt_len(encoder_frames(mel_frames(std::max(k.n, 0)))) + (int)c->sys_ids.size();
                if (k.n < 0 || (k.staged < 0 && k.n > 0 && !k.pcm) || k.budget <= 0) { reject(id, QASR_ERR_ARG, "bad clip (length, samples or budget)"); continue; }
                if (encoder_frames(mel_frames(k.n)) <= 0) { reject(id, QASR_ERR_ARG, "No audio_pad token found in input sequence"); continue; }
                if (P + k.budget > c->max_ctx) { reject(id, QASR_ERR_ARG, "Context length exceeded (prompt + max_tokens > max_ctx)"); continue; }
                staged = k.staged >= 0;   // (one kind per run: the caller's API)
                ids.push_back(id);
                ns.push_back(k.n);
                budgets.push_back(k.budget);
                if (staged) {
                    off.push_back(c->staged_off[k.staged]);
                } else {
                    off.push_back((long)pcm.size());
                    pcm.insert(pcm.end(), k.pcm, k.pcm + raw);
                    raw_n.push_back(raw);
                    rates.push_back(k.rate);
                    resample = resample || k.rate != qasr::kResampleOutRate;
                }
                slots.push_back(freeS[ids.size() - 1]);
            }
            if (ids.empty()) return 0;
            const int R = (int)ids.size();
            if (!staged && resample) {   // raw clips -> c->rsin, resampled (16 kHz clips copied) into c->spcm
                ResampleLayout lay;
                if ((rc = resample_layout(raw_n.data(), rates.data(), R, lay)) || (rc = ensure(c, c->rsin, std::max<size_t>(pcm.size(), 1) * 4)) ||
                    (rc = ensure(c, c->spcm, std::max<long>(lay.out_tot, 1) * 4)))
                    return rc;
                HIPCHK(hipMemcpyAsync(c->rsin.p, pcm.data(), pcm.size() * 4, hipMemcpyHostToDevice, s));
                if ((rc = run_resample(c, lay, c->rsin.as<float>(), c->spcm.as<float>()))) return rc;
                off = lay.out_off;
            } else if (!staged) {
                if ((rc = ensure(c, c->spcm, std::max<size_t>(pcm.size(), 1) * 4))) return rc;
                HIPCHK(hipMemcpyAsync(c->spcm.p, pcm.data(), pcm.size() * 4, hipMemcpyHostToDevice, s));
            }
            FrontEnd fe;
            auto check_prompt = [&](int r, int P, int audio_pos) -> int {   // (such clips were rejected one by one above)
                if (audio_pos < 0 || P + budgets[r] > c->max_ctx) return fail(QASR_ERR_STATE, "prompt length differs from its estimate");
                return 0;
            };
            if ((rc = front_end(c, staged ? c->pcm.as<float>() : c->spcm.as<float>(), off, ns, ev.e[0], ev.e[1], ev.e[2], nullptr,
                                &slots, check_prompt, fe)))
                return rc;
            std::vector<int32_t> first(R);
            std::vector<float> first_lp(R);
            HIPCHK(hipMemcpyAsync(first.data(), c->d_tok, R * 4, hipMemcpyDeviceToHost, s));
            if (lp) HIPCHK(hipMemcpyAsync(first_lp.data(), c->d_lp, R * 4, hipMemcpyDeviceToHost, s));
            std::vector<int32_t> first_tkid((size_t)R * K);
            std::vector<float> first_tklp((size_t)R * K);
            if (K) {
                HIPCHK(hipMemcpyAsync(first_tkid.data(), c->d_tkid, (size_t)R * K * 4, hipMemcpyDeviceToHost, s));
                HIPCHK(hipMemcpyAsync(first_tklp.data(), c->d_tklp, (size_t)R * K * 4, hipMemcpyDeviceToHost, s));
            }
            HIPCHK(hipStreamSynchronize(s));   // (pcm host vector in flight until here)
            if ((rc = check_dev_err(c))) return rc;
            refilled = true;
            st.n_prefills++;
            st.t_prefill_ms += ms_since(t0);
            float mel_ms = 0.f, enc_ms = 0.f;
            HIPCHK(hipEventElapsedTime(&mel_ms, ev.e[0], ev.e[1]));
            HIPCHK(hipEventElapsedTime(&enc_ms, ev.e[1], ev.e[2]));
            st.t_mel_ms += mel_ms;
            st.t_encode_ms += enc_ms;
            for (int r = 0; r < R; r++) {
                StreamSlot &x = sl[slots[r]];
                x.id = ids[r];
                x.P = fe.P[r];
                x.budget = budgets[r];
                x.toks.assign(1, first[r]);
                x.lps.assign(lp ? 1 : 0, first_lp[r]);
                x.tkid.assign(first_tkid.begin() + (size_t)r * K, first_tkid.begin() + (size_t)(r + 1) * K);
                x.tklp.assign(first_tklp.begin() + (size_t)r * K, first_tklp.begin() + (size_t)(r + 1) * K);
                if (c->tok_cb) c->tok_cb(c->tok_cb_user, x.id, 1, first[r]);
                if ((!ignore_eos && first[r] == hp.eos_id) || x.budget == 1) deliver(x);
            }
        }
    };
    std::vector<int> pos(S), nkv(S), tok(S);
    std::vector<int32_t> hist;
    std::vector<float> lph;
    std::vector<int32_t> tkhid;
    std::vector<float> tkhlp;
    if ((rc = decode_graph(c, S, false, 0))) return rc;
    for (;;) {
        if ((rc = refill())) return rc;
        int live = 0, chunk = c->tok_cb ? 1 : 8, maxpos = 0, hi = 0;
        for (int i = 0; i < S; i++) {
            const StreamSlot &x = sl[i];
            if (x.id < 0) { pos[i] = 0; nkv[i] = 1; tok[i] = 0; continue; }   // parked
            live++;
            hi = i + 1;
            pos[i] = x.P + (int)x.toks.size() - 1;   // the last token is fed at this position
            nkv[i] = pos[i] + 1;
            tok[i] = x.toks.back();
            chunk = std::min(chunk, x.budget - (int)x.toks.size());
            maxpos = std::max(maxpos, pos[i]);
        }
        if (live == 0) break;
        // option live_prefix: decode only the slots up to the last live one (rounded up to 16 rows, at least
        // 16 -- the batch kernels' shapes), so a context filling in refill groups or draining at the end of the
        // queue does not run every step at full width; the slots past it are parked and untouched
        const int Bq = c->fuse.live_prefix && S > 8 ? std::min(S, std::max(16, (hi + 15) / 16 * 16)) : S;
        if ((rc = decode_graph(c, Bq, false, 0))) return rc;
        HIPCHK(hipMemcpyAsync(c->d_pos, pos.data(), S * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->d_nkv, nkv.data(), S * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->d_tok, tok.data(), S * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(c->d_step, 0, 4, s));
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < chunk; k++) {
            if ((rc = launch_whole_step(c, Bq, split_bucket(c, maxpos + k)))) return rc;   // (probes are qasr_run's)
        }
        hist.resize((size_t)S * chunk);
        // (a decode step advances d_step, then writes hist[step]: the chunk's tokens are columns 1..chunk)
        HIPCHK(hipMemcpy2DAsync(hist.data(), chunk * 4, c->d_hist + 1, (size_t)c->hist_cap * 4, chunk * 4, S, hipMemcpyDeviceToHost, s));
        if (lp) {   // the same columns of the rows this chunk decoded (the slots past Bq hold earlier chunks' values)
            lph.resize((size_t)S * chunk);
            HIPCHK(hipMemcpy2DAsync(lph.data(), chunk * 4, c->d_lphist + 1, (size_t)c->hist_cap * 4, chunk * 4, Bq, hipMemcpyDeviceToHost, s));
        }
        if (K) {   // likewise, K entries a step
            tkhid.resize((size_t)S * chunk * K);
            tkhlp.resize(tkhid.size());
            HIPCHK(hipMemcpy2DAsync(tkhid.data(), (size_t)chunk * K * 4, c->d_tkhid + K, (size_t)c->hist_cap * K * 4, (size_t)chunk * K * 4,
                                    Bq, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpy2DAsync(tkhlp.data(), (size_t)chunk * K * 4, c->d_tkhlp + K, (size_t)c->hist_cap * K * 4, (size_t)chunk * K * 4,
                                    Bq, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));   // (the pos / nkv / tok host vectors in flight until here)
        if ((rc = check_dev_err(c))) return rc;
        st.t_decode_ms += ms_since(t0);
        st.n_steps += chunk;
        st.slot_steps += (int64_t)S * chunk;
        for (int i = 0; i < S; i++) st.kv_keys += (int64_t)nkv[i] * chunk + (int64_t)chunk * (chunk - 1) / 2;   // step k: n_kv + k
        for (int i = 0; i < S; i++) {
            StreamSlot &x = sl[i];
            if (x.id < 0) continue;
            for (int k = 0; k < chunk; k++) {
                const int32_t t = hist[(size_t)i * chunk + k];
                x.toks.push_back(t);
                if (lp) x.lps.push_back(lph[(size_t)i * chunk + k]);
                if (K) {
                    const size_t o = ((size_t)i * chunk + k) * K;
                    x.tkid.insert(x.tkid.end(), tkhid.begin() + o, tkhid.begin() + o + K);
                    x.tklp.insert(x.tklp.end(), tkhlp.begin() + o, tkhlp.begin() + o + K);
                }
                st.live_steps++;
                if (c->tok_cb) c->tok_cb(c->tok_cb_user, x.id, (int)x.toks.size(), t);
                if ((!ignore_eos && t == hp.eos_id) || (int)x.toks.size() >= x.budget) {
                    deliver(x);
                    break;
                }
            }
        }
    }
    st.t_total_ms = ms_since(t_start);
    if (stats) *stats = st;
    return 0;
}

extern "C" int qasr_run_stream(qasr_ctx *c, int slots, qasr_fetch_fn fetch, qasr_sink_fn sink, void *user, int max_tokens,
                               int ignore_eos, qasr_stream_stats *stats) {
    if (!fetch) return fail(QASR_ERR_ARG, "bad arguments");
    return run_stream(c, slots, [&](StreamClip &k) { return (k.id = fetch(user, &k.pcm, &k.n, &k.budget)) >= 0; }, sink, user,
                      max_tokens, ignore_eos, stats);
}

extern "C" int qasr_run_stream_rate(qasr_ctx *c, int slots, qasr_fetch_rate_fn fetch, qasr_sink_fn sink, void *user, int max_tokens,
                                    int ignore_eos, qasr_stream_stats *stats) {
    if (!fetch) return fail(QASR_ERR_ARG, "bad arguments");
    return run_stream(c, slots, [&](StreamClip &k) { return (k.id = fetch(user, &k.pcm, &k.n, &k.rate, &k.budget)) >= 0; }, sink,
                      user, max_tokens, ignore_eos, stats);
}

extern "C" int qasr_run_stream_staged(qasr_ctx *c, int slots, qasr_fetch_staged_fn fetch, qasr_sink_fn sink, void *user,
                                      int max_tokens, int ignore_eos, qasr_stream_stats *stats) {
    if (!fetch) return fail(QASR_ERR_ARG, "bad arguments");
    const int pool = (int)c->staged_n.size();
    return run_stream(c, slots, [&](StreamClip &k) {
        k.id = fetch(user, &k.budget);
        // ids past the pool reuse its clips only when asked for (option staged_wrap); else run_stream
        // rejects them as out of range
        k.staged = k.id >= 0 && pool > 0 && c->fuse.staged_wrap ? k.id % pool : k.id;
        return k.id >= 0;
    }, sink, user, max_tokens, ignore_eos, stats);
}

extern "C" int qasr_get_logprobs(qasr_ctx *c, float *out, int B, int max_tokens) {
    if (!c || !out || B <= 0 || max_tokens <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    if (!c->fuse.token_logprobs) return fail(QASR_ERR_STATE, "option token_logprobs is off");
    if (c->last_run_beam) return fail(QASR_ERR_STATE, "the last run was a beam run: its values are qasr_get_beams'");
    if (c->last_run_sampled && c->last_run_nbest >= 2) return fail(QASR_ERR_STATE, "the last run drew n_best >= 2 samples: their values are qasr_get_samples'");
    if (!c->lp_run_B) return fail(QASR_ERR_STATE, "no run has finished with option token_logprobs on");
    if (B < c->lp_run_B) return fail(QASR_ERR_ARG, "buffer holds fewer rows than the last run's batch");
    for (int b = 0; b < c->lp_run_B; b++)
        if (c->lp_run_n[b] > max_tokens) return fail(QASR_ERR_ARG, "buffer rows shorter than the last run's tokens");
    for (int b = 0; b < c->lp_run_B; b++)
        for (int k = 0; k < c->lp_run_n[b]; k++) out[(size_t)b * max_tokens + k] = c->lp_run[(size_t)b * c->lp_run_T + k];
    return 0;
}

// (a count on success, so errors are minus the code, as qasr_align_json)
extern "C" int qasr_stream_logprobs(qasr_ctx *c, float *out, int cap) {
    if (!c || cap < 0 || (cap > 0 && !out)) return -fail(QASR_ERR_ARG, "bad arguments");
    if (!c->fuse.token_logprobs) return -fail(QASR_ERR_STATE, "option token_logprobs is off");
    if (!c->lp_sink) return -fail(QASR_ERR_STATE, "qasr_stream_logprobs is valid only inside a qasr_sink_fn call");
    const int n = (int)c->lp_sink->size();
    if (cap < n) return -fail(QASR_ERR_ARG, "buffer shorter than the clip's tokens");
    for (int k = 0; k < n; k++) out[k] = (*c->lp_sink)[k];
    return n;
}

extern "C" int qasr_get_topk(qasr_ctx *c, int32_t *ids, float *logprobs, int B, int max_tokens, int K) {
    if (!c || !ids || !logprobs || B <= 0 || max_tokens <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    if (!c->fuse.top_k) return fail(QASR_ERR_STATE, "option top_k is off");
    if (K != c->fuse.top_k) return fail(QASR_ERR_ARG, "K differs from option top_k");
    if (c->last_run_beam) return fail(QASR_ERR_STATE, "the last run was a beam run: its values are qasr_get_beams'");
    if (c->last_run_sampled && c->last_run_nbest >= 2) return fail(QASR_ERR_STATE, "the last run drew n_best >= 2 samples: qasr_get_samples reads them");
    if (!c->tk_run_B) return fail(QASR_ERR_STATE, "no run has finished with option top_k on");
    if (B < c->tk_run_B) return fail(QASR_ERR_ARG, "buffer holds fewer rows than the last run's batch");
    for (int b = 0; b < c->tk_run_B; b++)
        if (c->tk_run_n[b] > max_tokens) return fail(QASR_ERR_ARG, "buffer rows shorter than the last run's tokens");
    for (int b = 0; b < c->tk_run_B; b++)
        for (size_t k = 0; k < (size_t)c->tk_run_n[b] * K; k++) {
            ids[(size_t)b * max_tokens * K + k] = c->tk_run_id[(size_t)b * c->tk_run_T * K + k];
            logprobs[(size_t)b * max_tokens * K + k] = c->tk_run_lp[(size_t)b * c->tk_run_T * K + k];
        }
    return 0;
}

// (a count on success, so errors are minus the code, as qasr_stream_logprobs)
extern "C" int qasr_stream_topk(qasr_ctx *c, int32_t *ids, float *logprobs, int cap_tokens, int K) {
    if (!c || cap_tokens < 0 || (cap_tokens > 0 && (!ids || !logprobs))) return -fail(QASR_ERR_ARG, "bad arguments");
    if (!c->fuse.top_k) return -fail(QASR_ERR_STATE, "option top_k is off");
    if (K != c->fuse.top_k) return -fail(QASR_ERR_ARG, "K differs from option top_k");
    if (!c->tk_sink_id) return -fail(QASR_ERR_STATE, "qasr_stream_topk is valid only inside a qasr_sink_fn call");
    const int n = (int)(c->tk_sink_id->size() / K);
    if (cap_tokens < n) return -fail(QASR_ERR_ARG, "buffer shorter than the clip's tokens");
    for (size_t k = 0; k < (size_t)n * K; k++) {
        ids[k] = (*c->tk_sink_id)[k];
        logprobs[k] = (*c->tk_sink_lp)[k];
    }
    return n;
}

extern "C" int qasr_set_token_callback(qasr_ctx *c, void (*cb)(void *user, int seq, int n_generated, int32_t token), void *user) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    c->tok_cb = cb;
    c->tok_cb_user = user;
    return 0;
}

extern "C" int qasr_set_system_prompt(qasr_ctx *c, const int32_t *ids, int n) {
    if (!c || n < 0 || (n > 0 && !ids)) return fail(QASR_ERR_ARG, "bad arguments");
    c->sys_ids.assign(ids, ids + n);
    return 0;
}

extern "C" int qasr_transcribe_batch(qasr_ctx *c, const float *const *pcm, const int *n, int B, int max_tokens, int ignore_eos,
                                     int32_t *tokens, int *n_tokens, qasr_timings *t) {
    int rc = qasr_stage_audio(c, pcm, n, B);
    if (rc) return rc;
    return qasr_run(c, max_tokens, ignore_eos, tokens, n_tokens, t);
}
