// engine_sample.hip -- temperature sampling: qasr_set_sampling and the per-row draw identities,
// the sampler step that ends a prefill or decode step while sampling is on, qasr_run with sampling (n_best = 1:
// the ordinary loop; n_best = N >= 2: clip g owns rows g * N .. g * N + N - 1, one prefill a clip, one KV-cache
// fork after the first draw, then the ordinary loop over G * N independent rows) and the sample reader.
#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

static_assert(QASR_SAMPLE_MAX == QASR_BEAM_MAX, "an n_best run forks with the beam's group limit");

// ------------------------------------------------------------------ state
static int ensure_sample(qasr_ctx *c) {
    if (c->sd.skey) return 0;   // (the last one allocated below)
    const size_t rows = (size_t)c->max_batch;
    qasr_ctx::SampleDev d;
    int rc;
    if ((rc = dev_alloc(c, (void **)&d.sc, sizeof(SampleScalars))) || (rc = dev_alloc(c, (void **)&d.clip, rows * 4)) ||
        (rc = dev_alloc(c, (void **)&d.sample, rows * 4)) || (rc = dev_alloc(c, (void **)&d.t, rows * 4)) ||
        (rc = dev_alloc(c, (void **)&d.skey, rows * 8)))
        return rc;
    // until qasr_set_sample_streams says otherwise: row b draws as (clip b, sample 0) from t = 0
    std::vector<int> id(rows), zero(rows, 0);
    for (size_t b = 0; b < rows; b++) id[b] = (int)b;
    HIPCHK(hipMemcpy(d.clip, id.data(), rows * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.sample, zero.data(), rows * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.t, zero.data(), rows * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d.skey, 0, rows * 8));
    c->sd = d;
    return 0;
}

extern "C" int qasr_set_sampling(qasr_ctx *c, const qasr_sampling *s) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    if (!s || s->temperature <= 0.f) {   // off: no kernel, graph or result of the greedy paths changes
        c->samp.temperature = 0.f;
        return 0;
    }
    if (!(s->temperature <= 100.f)) return fail(QASR_ERR_ARG, "sampling: temperature must be in (0, 100]");
    if (!(s->min_p >= 0.f && s->min_p <= 1.f)) return fail(QASR_ERR_ARG, "sampling: min_p must be in [0, 1]");
    if (s->n_best < 1 || s->n_best > QASR_SAMPLE_MAX) return fail(QASR_ERR_ARG, "sampling: n_best must be in 1..8");
    HIPCHK(hipSetDevice(c->m->device));
    if (int rc = ensure_sample(c)) return rc;
    SampleScalars sc;
    sc.inv_T = 1.0f / s->temperature;
    sc.cut = s->min_p > 0.f ? s->temperature * logf(s->min_p) : -INFINITY;
    sc.seed_lo = (uint32_t)(s->seed & 0xffffffffull);
    sc.seed_hi = (uint32_t)(s->seed >> 32);
    // (device memory: a captured step serves any temperature, min_p or seed)
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipMemcpy(c->sd.sc, &sc, sizeof sc, hipMemcpyHostToDevice));
    c->samp = *s;
    return 0;
}

extern "C" int qasr_get_sampling(const qasr_ctx *c, qasr_sampling *out) {
    if (!c || !out) return fail(QASR_ERR_ARG, "bad arguments");
    *out = c->samp;
    return 0;
}

int qasr::eng::sample_set_streams(qasr_ctx *c, const std::vector<int> &clip, const std::vector<int> &sample, const std::vector<int> &t) {
    const size_t n = clip.size() * 4;
    int rc;
    if ((rc = stage_pinned(c, clip.data(), n, c->sd.clip)) || (rc = stage_pinned(c, sample.data(), n, c->sd.sample)) ||
        (rc = stage_pinned(c, t.data(), n, c->sd.t)))
        return rc;
    HIPCHK(hipMemsetAsync(c->sd.skey, 0, (size_t)c->max_batch * 8, c->st));   // (zero at rest whatever an earlier failed call left)
    return 0;
}

extern "C" int qasr_set_sample_streams(qasr_ctx *c, const int32_t *clip, const int32_t *sample, const int32_t *t, int B) {
    if (!c || !clip || !sample || !t || B <= 0 || B > c->max_batch) return fail(QASR_ERR_ARG, "bad arguments");
    if (!sampling_on(c)) return fail(QASR_ERR_STATE, "sampling is off (qasr_set_sampling)");
    for (int b = 0; b < B; b++)
        if (clip[b] < 0 || sample[b] < 0 || t[b] < 0) return fail(QASR_ERR_ARG, "sample streams: negative clip, sample or t");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    if (int rc = sample_set_streams(c, std::vector<int>(clip, clip + B), std::vector<int>(sample, sample + B), std::vector<int>(t, t + B)))
        return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// ------------------------------------------------------------ sampler step
int qasr::eng::sample_step(qasr_ctx *c, int B, int src_div) {
    const int V = c->m->hp.vocab;
    if (B > c->max_batch) return fail(QASR_ERR_ARG, "sampling: rows exceed the context's max_batch");
    SampleArgs a{};
    a.logits = c->d_logits; a.ld = V; a.n_valid = V;
    // (constraints on: the draw is from the edited rows, whose maxima are the constraint stage's tokens per logits row)
    a.greedy = constraints_on(c) ? c->cd.gtok : c->d_tok;
    a.clip = c->sd.clip; a.sample = c->sd.sample; a.t = c->sd.t;
    a.sc = c->sd.sc; a.skey = c->sd.skey;
    a.tok = c->d_tok; a.hist = c->d_hist; a.hist_stride = c->hist_cap; a.step = c->d_step;
    a.R = B; a.src_div = src_div;
    if (!launch_sample(a, std::max(c->fuse.sample_slices, 0), c->st)) return fail(QASR_ERR_STATE, "sampling: the launcher declined " + std::to_string(B) + " rows");
    // the drawn token's log-probability under the model's own distribution (T = 1)
    launch_token_logprob(c->d_logits, V, B, 0, c->d_tok, c->d_step, c->d_lp, c->d_lphist, c->hist_cap, c->st, src_div);
    return 0;
}

// ------------------------------------------------------------- sampling run
namespace {
// c->samp_run_N is non-zero only inside a sampling run: the prefill's draw and the graph keys read it
struct SampleScope {
    qasr_ctx *c;
    SampleScope(qasr_ctx *c_, int N) : c(c_) { c->samp_run_N = N; }
    ~SampleScope() { c->samp_run_N = 0; }
};
}  // namespace

int qasr::eng::sample_collect(qasr_ctx *c, int G, int N, const std::vector<int32_t> &hist, int steps, int max_tokens, int ignore_eos) {
    const int B = G * N, cols = std::min(steps + 1, max_tokens), eos = c->m->hp.eos_id;
    std::vector<float> lph((size_t)B * cols);
    HIPCHK(hipMemcpy2DAsync(lph.data(), (size_t)cols * 4, c->d_lphist, (size_t)c->hist_cap * 4, (size_t)cols * 4, B, hipMemcpyDeviceToHost,
                            c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->samp_res.assign(G, std::vector<qasr_ctx::SampleHyp>(N));
    for (int r = 0; r < B; r++) {
        qasr_ctx::SampleHyp &h = c->samp_res[r / N][r % N];
        for (int k = 0; k < cols; k++) {
            const int32_t tk = hist[(size_t)r * c->hist_cap + k];
            const float lp = lph[(size_t)r * cols + k];
            h.sum += lp;   // fp32, in order; a popped EOS still counts
            if (!ignore_eos && tk == eos) break;
            h.tokens.push_back(tk);
            h.logprobs.push_back(lp);
        }
    }
    return 0;
}

int qasr::eng::sample_run(qasr_ctx *c, int max_tokens, int ignore_eos, int32_t *tokens, int *n_tokens, qasr_timings *t) {
    const int N = c->samp.n_best, G = (int)c->staged_n.size(), B = G * N;
    if (c->fuse.beam_width >= 2) return fail(QASR_ERR_STATE, "sampling and beam search (option beam_width >= 2) exclude each other");
    if (N >= 2 && c->tok_cb) return fail(QASR_ERR_STATE, "a token callback is set: an n_best >= 2 run delivers no tokens before it ends");
    if (B > c->max_batch) return fail(QASR_ERR_ARG, "staged clips x n_best exceed the context's max_batch");
    HIPCHK(hipSetDevice(c->m->device));
    std::unique_lock<std::mutex> dev_lk;
    if (takes_fused(c, B)) {   // (as qasr_run)
        dev_lk = std::unique_lock<std::mutex>(device_lock(c->m->device));
        if (int rc = reset_counters(c)) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    c->last_run_beam = false;
    c->last_run_sampled = true;
    c->last_run_nbest = N;
    c->samp_res.clear();
    hipStream_t s = c->st;
    int rc;
    RoctxRange run_range("qasr.run");
    SampleScope scope(c, N);
    // the draws' identities: row g * N + i is (clip g's pool index, sample i), every hypothesis from t = 0
    std::vector<int> clip(B), smp(B), t0(B, 0);
    for (int r = 0; r < B; r++) {
        clip[r] = c->run_clip_ids.empty() ? r / N : c->run_clip_ids[r / N];
        smp[r] = r % N;
    }
    if ((rc = sample_set_streams(c, clip, smp, t0))) return rc;
    // n_best >= 2: only row 0 of a group is prefilled (slot g * N, logits row g); the prefill's draw covers all B rows
    std::vector<int> slots(G);
    for (int g = 0; g < G; g++) slots[g] = g * N;
    FrontEnd fe;
    if ((rc = front_end_staged(c, max_tokens, N >= 2 ? &slots : nullptr, fe))) return rc;
    const int maxP = *std::max_element(fe.P.begin(), fe.P.end());
    c->run_P.resize(B);
    for (int r = 0; r < B; r++) c->run_P[r] = fe.P[r / N];
    if (N >= 2) {
        // every row's decode position (the prefill wrote entries 0 .. G - 1), then one fork of [0, P) to the other rows
        std::vector<int> pos(B), nkv(B), tab(3 * (size_t)B);
        for (int r = 0; r < B; r++) {
            pos[r] = fe.P[r / N];
            nkv[r] = pos[r] + 1;
            tab[r] = r / N * N;
            tab[(size_t)B + r] = 0;
            tab[2 * (size_t)B + r] = fe.P[r / N];
        }
        if ((rc = stage_pinned(c, pos.data(), (size_t)B * 4, c->d_pos)) || (rc = stage_pinned(c, nkv.data(), (size_t)B * 4, c->d_nkv)) ||
            (rc = upload(c, c->fork_args, tab)))
            return rc;
        const int *d = c->fork_args.as<int>();
        if (!launch_kv_fork(fork_args(c, d, d + B, d + 2 * B, B, N, (maxP + 7) / 8), s))
            return fail(QASR_ERR_STATE, "sampling: the KV-cache fork declined n_best = " + std::to_string(N));
    }
    if ((rc = decode_graph(c, B, false, maxP)) || (rc = probe_arm(c, max_tokens - 1))) return rc;
    std::vector<int32_t> hist;
    int steps = 0;
    if ((rc = greedy_loop(c, B, max_tokens, ignore_eos, hist, steps))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_END], s));
    HIPCHK(hipEventSynchronize(c->ev[EV_END]));
    if (N == 1) {
        if ((rc = run_results(c, B, max_tokens, ignore_eos, hist, steps, tokens, n_tokens, t))) return rc;
        return sample_collect(c, G, 1, hist, steps, max_tokens, ignore_eos);
    }
    if ((rc = check_dev_err(c)) || (rc = probe_collect(c, B, steps))) return rc;
    c->lp_run_B = c->tk_run_B = 0;
    if ((rc = sample_collect(c, G, N, hist, steps, max_tokens, ignore_eos))) return rc;
    for (int g = 0; g < G; g++) {   // the run's tokens are sample 0's: what an n_best = 1 run returns
        const qasr_ctx::SampleHyp &h = c->samp_res[g][0];
        n_tokens[g] = (int)h.tokens.size();
        std::copy(h.tokens.begin(), h.tokens.end(), tokens + (size_t)g * max_tokens);
    }
    return run_timings(c, steps, t);
}

// (a count on success, so errors are minus the code, as qasr_get_beams)
extern "C" int qasr_get_samples(qasr_ctx *c, int clip, int32_t *tokens, float *logprobs, int *n_tokens, float *sum_logprob, int cap_hyp,
                                int max_tokens) {
    if (!c || !tokens || !n_tokens || !sum_logprob || cap_hyp <= 0 || max_tokens <= 0) return -fail(QASR_ERR_ARG, "bad arguments");
    if (!c->last_run_sampled || c->samp_res.empty()) return -fail(QASR_ERR_STATE, "no sampling run has finished (qasr_set_sampling)");
    if (clip < 0 || clip >= (int)c->samp_res.size()) return -fail(QASR_ERR_ARG, "clip index outside the last sampling run");
    const std::vector<qasr_ctx::SampleHyp> &hs = c->samp_res[clip];
    if ((int)hs.size() > cap_hyp) return -fail(QASR_ERR_ARG, "buffers hold fewer hypotheses than the clip has");
    for (const auto &h : hs)
        if ((int)h.tokens.size() > max_tokens) return -fail(QASR_ERR_ARG, "buffer rows shorter than the hypotheses");
    for (size_t i = 0; i < hs.size(); i++) {
        std::copy(hs[i].tokens.begin(), hs[i].tokens.end(), tokens + i * max_tokens);
        if (logprobs) std::copy(hs[i].logprobs.begin(), hs[i].logprobs.end(), logprobs + i * max_tokens);
        n_tokens[i] = (int)hs[i].tokens.size();
        sum_logprob[i] = hs[i].sum;
    }
    return (int)hs.size();
}
