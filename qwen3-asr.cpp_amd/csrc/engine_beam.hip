// engine_beam.hip -- beam search (option beam_width = W >= 2, DESIGN.md "Beam search"): the KV-cache
// fork entry, the beam loop of qasr_run and the hypothesis reader.  Clip g owns rows g * W .. g * W + W - 1
// of the decode step; every step ends with beam_select_kernel and kv_fork_kernel (beam.hip) inside the
// replayed graph, so the loop synchronises with the host no more often than the greedy one.
#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

// ------------------------------------------------------------------- fork
KvForkArgs qasr::eng::fork_args(qasr_ctx *c, const int *parent, const int *from, const int *to, int B, int group, int blocks) {
    KvForkArgs a{};
    a.kc = c->kc; a.vc = c->vc; a.vt = c->vt;
    a.layers = c->m->hp.dec_layers; a.n_kv_head = c->m->hp.n_kv_head; a.max_ctx = c->max_ctx; a.slots = c->max_batch;
    a.parent = parent; a.from = from; a.to = to;
    a.B = B; a.group = group; a.blocks = blocks;
    return a;
}

extern "C" int qasr_kv_fork(qasr_ctx *c, const int *parent, const int *from, const int *to, int B, int group) {
    if (!c || !parent || !from || !to) return fail(QASR_ERR_ARG, "bad arguments");
    if (group < 1 || group > QASR_BEAM_MAX || B <= 0 || B % group != 0 || B > c->max_batch)
        return fail(QASR_ERR_ARG, "kv_fork: group in 1..8, B a multiple of it and at most max_batch");
    int hi = 0;
    for (int b = 0; b < B; b++) {
        if (parent[b] < 0 || parent[b] >= B || parent[b] / group != b / group) return fail(QASR_ERR_ARG, "kv_fork: parent outside the row's group");
        if (parent[b] == b || from[b] >= to[b]) continue;
        if (from[b] < 0 || to[b] > c->max_ctx) return fail(QASR_ERR_ARG, "kv_fork: range outside [0, max_ctx]");
        hi = std::max(hi, to[b]);
    }
    if (!hi) return 0;   // every row a no-op
    HIPCHK(hipSetDevice(c->m->device));
    std::vector<int> tab(3 * (size_t)B);
    std::copy(parent, parent + B, tab.begin());
    std::copy(from, from + B, tab.begin() + B);
    std::copy(to, to + B, tab.begin() + 2 * B);
    if (int rc = upload(c, c->fork_args, tab)) return rc;
    const int *d = c->fork_args.as<int>();
    if (!launch_kv_fork(fork_args(c, d, d + B, d + 2 * B, B, group, (hi + 7) / 8), c->st))
        return fail(QASR_ERR_STATE, "kv_fork: the launcher declined its shape");
    HIPCHK(hipGetLastError());
    return 0;
}

// -------------------------------------------------------------- beam step
int qasr::eng::beam_step(qasr_ctx *c, int G, int blocks) {
    const int W = c->beam_W;
    const qasr_ctx::BeamDev &b = c->bm;
    BeamSelectArgs a{};
    a.tk_id = c->d_tkid; a.tk_lp = c->d_tklp;
    a.cum = b.cum; a.fin_row = b.fin_row; a.fin_t = b.fin_t; a.fin_sum = b.fin_sum; a.fin_lp = b.fin_lp;
    a.n_fin = b.n_fin; a.done = b.done; a.t = b.t; a.P = b.P;
    a.tok = c->d_tok; a.parent = b.parent; a.from = b.from; a.to = b.to;
    a.h_par = b.h_par; a.h_id = b.h_id; a.h_lp = b.h_lp;
    a.hist_stride = c->max_batch; a.hist_base = 0;
    a.W = W; a.G = G; a.eos = b.eos;
    if (!launch_beam_select(a, c->st) || !launch_kv_fork(fork_args(c, b.parent, b.from, b.to, G * W, W, blocks), c->st))
        return fail(QASR_ERR_STATE, "beam step: a launcher declined W = " + std::to_string(W));
    return 0;
}

// --------------------------------------------------------------- beam run
namespace {
// c->beam_W is non-zero only inside a beam run: the step emitter, the prefill's top-K and the graph keys read it
struct BeamScope {
    qasr_ctx *c;
    BeamScope(qasr_ctx *c_, int W) : c(c_) { c->beam_W = W; }
    ~BeamScope() { c->beam_W = 0; }
};
}  // namespace

int qasr::eng::beam_run(qasr_ctx *c, int max_tokens, int ignore_eos, int32_t *tokens, int *n_tokens, qasr_timings *t) {
    const int W = c->fuse.beam_width, G = (int)c->staged_n.size(), B = G * W;
    const Hparams &hp = c->m->hp;
    if (c->tok_cb) return fail(QASR_ERR_STATE, "a token callback is set: beam search delivers no tokens before the run ends");
    if (B > c->max_batch) return fail(QASR_ERR_ARG, "staged clips x beam_width exceed the context's max_batch");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    c->last_run_beam = true;
    c->beam_res.clear();
    c->lp_run_B = c->tk_run_B = 0;
    hipStream_t s = c->st;
    int rc;
    RoctxRange run_range("qasr.run");   // host-side ranges for rocprofv3 --marker-trace, as qasr_run's
    BeamScope scope(c, W);
    // only row 0 of a group is prefilled: clip g's prompt goes to slot g * W, its logits to row g
    std::vector<int> slots(G);
    for (int g = 0; g < G; g++) slots[g] = g * W;
    FrontEnd fe;
    if ((rc = front_end_staged(c, max_tokens, &slots, fe))) return rc;
    c->run_P = fe.P;
    const int maxP = *std::max_element(fe.P.begin(), fe.P.end());
    // the group state at rest, and every row's decode position (the prefill wrote entries 0 .. G - 1 of them)
    const qasr_ctx::BeamDev &bm = c->bm;
    std::vector<float> cum(B, -INFINITY);
    std::vector<int> pos(B), nkv(B), zero(G, 0);
    const int32_t eos = ignore_eos ? -1 : hp.eos_id;   // (device memory: the captured step serves either setting)
    for (int g = 0; g < G; g++) {
        cum[(size_t)g * W] = 0.f;
        for (int i = 0; i < W; i++) {
            pos[(size_t)g * W + i] = fe.P[g];
            nkv[(size_t)g * W + i] = fe.P[g] + 1;
        }
    }
    if ((rc = stage_pinned(c, cum.data(), (size_t)B * 4, bm.cum)) || (rc = stage_pinned(c, pos.data(), (size_t)B * 4, c->d_pos)) ||
        (rc = stage_pinned(c, nkv.data(), (size_t)B * 4, c->d_nkv)) || (rc = stage_pinned(c, fe.P.data(), (size_t)G * 4, bm.P)) ||
        (rc = stage_pinned(c, zero.data(), (size_t)G * 4, bm.n_fin)) || (rc = stage_pinned(c, zero.data(), (size_t)G * 4, bm.done)) ||
        (rc = stage_pinned(c, zero.data(), (size_t)G * 4, bm.t)) || (rc = stage_pinned(c, &eos, 4, bm.eos)))
        return rc;
    // step 0 from the prefill's logits; its fork copies [0, P) of row 0 to the other rows
    if ((rc = beam_step(c, G, (maxP + 7) / 8))) return rc;
    if ((rc = decode_graph(c, B, false, maxP)) || (rc = probe_arm(c, max_tokens - 1))) return rc;
    RoctxRange dec_range("qasr.decode");
    int steps = 0;   // decode steps run: steps + 1 beam steps
    std::vector<int> done(G, 0);
    auto all_done = [&]() -> int {
        if (ignore_eos) return 0;   // (nothing finishes)
        if (hipMemcpyAsync(done.data(), bm.done, (size_t)G * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return -1;
        return std::count(done.begin(), done.end(), 0) == 0 ? 1 : 0;
    };
    int st = 0;
    while (steps + 1 < max_tokens && (st = all_done()) == 0) {   // the done flags every 8 steps, as greedy_loop reads its history
        const int todo = std::min(8, max_tokens - 1 - steps);
        for (int k = 0; k < todo; k++)
            if ((rc = launch_step(c, B, steps + k))) return rc;
        steps += todo;
    }
    if (st < 0) return fail(QASR_ERR_DEVICE, "device copy failed in the beam loop");
    HIPCHK(hipEventRecord(c->ev[EV_END], s));
    HIPCHK(hipEventSynchronize(c->ev[EV_END]));
    if ((rc = check_dev_err(c))) return rc;
    if ((rc = probe_collect(c, B, steps))) return rc;
    // the state back: history slots 0 .. steps, the finished tables, the live rows' sums
    const int T = steps + 1, MB = c->max_batch;
    std::vector<int> h_par((size_t)T * MB), fin_row(B), fin_t(B), n_fin(G);
    std::vector<int32_t> h_id((size_t)T * MB);
    std::vector<float> h_lp((size_t)T * MB), fin_sum(B), fin_lp(B);
    HIPCHK(hipMemcpyAsync(h_par.data(), bm.h_par, h_par.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_id.data(), bm.h_id, h_id.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_lp.data(), bm.h_lp, h_lp.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(fin_row.data(), bm.fin_row, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(fin_t.data(), bm.fin_t, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(fin_sum.data(), bm.fin_sum, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(fin_lp.data(), bm.fin_lp, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_fin.data(), bm.n_fin, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(done.data(), bm.done, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cum.data(), bm.cum, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    c->beam_res.resize(G);
    for (int g = 0; g < G; g++) {
        BeamGroup bg;
        bg.W = W; bg.row0 = g * W; bg.stride = MB;
        // a group frozen before the run's end took its last beam step at done - 1
        bg.T = done[g] ? std::min(done[g], T) : T;
        bg.h_par = h_par.data(); bg.h_id = h_id.data(); bg.h_lp = h_lp.data(); bg.cum = cum.data();
        bg.fin_row = fin_row.data(); bg.fin_t = fin_t.data(); bg.fin_sum = fin_sum.data(); bg.fin_lp = fin_lp.data();
        bg.n_fin = n_fin[g]; bg.done = done[g];
        c->beam_res[g] = beam_hypotheses(bg);
        const BeamHyp &best = c->beam_res[g][0];
        n_tokens[g] = (int)best.tokens.size();
        std::copy(best.tokens.begin(), best.tokens.end(), tokens + (size_t)g * max_tokens);
    }
    return run_timings(c, steps, t);
}

// (a count on success, so errors are minus the code, as qasr_align_json)
extern "C" int qasr_get_beams(qasr_ctx *c, int clip, int32_t *tokens, float *logprobs, int *n_tokens, float *sum_logprob,
                              int *finished, int cap_hyp, int max_tokens) {
    if (!c || !tokens || !n_tokens || !sum_logprob || !finished || cap_hyp <= 0 || max_tokens <= 0)
        return -fail(QASR_ERR_ARG, "bad arguments");
    if (!c->last_run_beam || c->beam_res.empty()) return -fail(QASR_ERR_STATE, "no beam run has finished (option beam_width >= 2)");
    if (clip < 0 || clip >= (int)c->beam_res.size()) return -fail(QASR_ERR_ARG, "clip index outside the last beam run");
    const std::vector<BeamHyp> &hs = c->beam_res[clip];
    if ((int)hs.size() > cap_hyp) return -fail(QASR_ERR_ARG, "buffers hold fewer hypotheses than the clip has");
    for (const BeamHyp &h : hs)
        if ((int)h.tokens.size() > max_tokens) return -fail(QASR_ERR_ARG, "buffer rows shorter than the hypotheses");
    for (size_t i = 0; i < hs.size(); i++) {
        const BeamHyp &h = hs[i];
        std::copy(h.tokens.begin(), h.tokens.end(), tokens + i * max_tokens);
        if (logprobs) std::copy(h.logprobs.begin(), h.logprobs.end(), logprobs + i * max_tokens);
        n_tokens[i] = (int)h.tokens.size();
        sum_logprob[i] = h.sum;
        finished[i] = h.finished;
    }
    return (int)hs.size();
}
