// engine_score.hip -- teacher-forced scoring (DESIGN.md "Teacher-forced scoring"): the score head
// (score_head.hip) over rows of the prefill's final hidden states, and its two entry points --
// qasr_prefill_score at the stage level and qasr_score over the staged pool, which prefills a clip's
// prompt once, forks its KV rows to the clip's hypotheses and runs every hypothesis as one chunk.
// Nothing here is captured or touches a step graph.
#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

namespace {

constexpr int kScoreBlock = 4096;   // rows a score-head launch: bounds its scratch (two 4096 x N / 128 tables)

// rows.row[i] of c->px (the final hidden rows prefill_layers left) against rows.target[i]; the three
// results to entry rows.out[i] of the host arrays.  The same hidden row may appear several times.
int run_score_rows(qasr_ctx *c, const ScoreRows &rows, float *lp, int32_t *gid, float *glp) {
    const int R = (int)rows.size();
    if (R == 0) return 0;
    const Hparams &hp = c->m->hp;
    const int H = hp.hidden, blk = std::min(R, kScoreBlock);
    hipStream_t s = c->st;
    int rc;
    std::vector<int> tab(rows.row);
    tab.insert(tab.end(), rows.target.begin(), rows.target.end());
    if ((rc = upload(c, c->sc_tab, tab)) || (rc = ensure(c, c->sc_rows, (size_t)blk * H * 2)) ||
        (rc = ensure(c, c->sc_out, (size_t)R * 3 * 4)) || (rc = ensure(c, c->sc_scratch, score_head_scratch(blk, hp.vocab))))
        return rc;
    const int *d_row = c->sc_tab.as<int>();
    const int32_t *d_tg = (const int32_t *)(d_row + R);
    float *d_lp = c->sc_out.as<float>(), *d_glp = d_lp + R;
    int32_t *d_gid = (int32_t *)(d_lp + 2 * (size_t)R);
    for (int r0 = 0; r0 < R; r0 += kScoreBlock) {
        const int n = std::min(kScoreBlock, R - r0);
        launch_rmsnorm_f16(c->px.as<float>(), H, d_row + r0, n, H, c->m->out_norm, hp.rms_eps, c->sc_rows.as<uint16_t>(), s);
        ScoreHeadArgs a{};
        a.A = c->sc_rows.as<uint16_t>(); a.lda = H;
        a.W = c->m->embd; a.ldw = H;
        a.R = n; a.N = hp.vocab; a.K = H;
        a.target = d_tg + r0;
        a.lp = d_lp + r0; a.gid = d_gid + r0; a.glp = d_glp + r0;
        a.scratch = c->sc_scratch.p;
        if (!launch_score_head(a, s))
            return fail(QASR_ERR_STATE, "the score head has no kernel for " + std::to_string(n) + " x " + std::to_string(hp.vocab) + " x " +
                                            std::to_string(H) + " (kernels.h)");
    }
    HIPCHK(hipGetLastError());
    std::vector<float> h((size_t)R * 3);
    HIPCHK(hipMemcpyAsync(h.data(), d_lp, h.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < R; i++) {
        lp[rows.out[i]] = h[i];
        glp[rows.out[i]] = h[(size_t)R + i];
        memcpy(&gid[rows.out[i]], &h[2 * (size_t)R + i], 4);
    }
    return declined_check("score head");
}

int score_model_check(const qasr_ctx *c) {
    if (c->m->hp.aligner) return fail(QASR_ERR_STATE, "scoring needs an ASR model (this is a ForcedAligner file)");
    return 0;
}

}  // namespace

static int prefill_score(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, const float *feats, const int *audio_pos,
                         const int *N, const int *slots, int B, const int32_t *targets, float *logprobs, int32_t *greedy_ids,
                         float *greedy_logprobs, int cap, int *count) {
    if (!c || !ids || !P || B <= 0 || !targets || cap < 0) return fail(QASR_ERR_ARG, "bad arguments");
    if (int rc = score_model_check(c)) return rc;
    ScoreRows rows;
    long nid = 0;
    for (int b = 0; b < B; b++) {
        if (P[b] < 0) return fail(QASR_ERR_ARG, "negative P / n_past / N");
        nid += P[b];
    }
    for (long t = 0; t < nid; t++) {
        if (targets[t] < 0) continue;
        if (targets[t] >= c->m->hp.vocab) return fail(QASR_ERR_ARG, "target id out of range");
        rows.out.push_back((int)rows.row.size());
        rows.row.push_back((int)t);
        rows.target.push_back(targets[t]);
    }
    const int R = (int)rows.size();
    if (R > cap) return fail(QASR_ERR_ARG, "buffers hold fewer entries than the scored rows");
    if (R && (!logprobs || !greedy_ids || !greedy_logprobs)) return fail(QASR_ERR_ARG, "bad arguments");
    int rc;
    if ((rc = prefill_chunk_common(c, ids, P, n_past, feats, audio_pos, N, B, nullptr, nullptr, slots))) return rc;
    if ((rc = run_score_rows(c, rows, logprobs, greedy_ids, greedy_logprobs))) return rc;
    *count = R;
    return 0;
}

static int score(qasr_ctx *c, const int *clips, const int32_t *tokens, const int *n_tokens, int S, int include_eos, float *logprobs,
                 int32_t *greedy_ids, float *greedy_logprobs, float *sum_logprob, qasr_timings *t, int *count) {
    if (!c || !clips || !n_tokens || S <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    if (int rc = score_model_check(c)) return rc;
    if (c->staged_n.empty()) return fail(QASR_ERR_STATE, "no staged audio");
    if (!c->fuse.fa_exact_prefill)
        return fail(QASR_ERR_STATE, "qasr_score runs the hypotheses as chunks after the cached prompt: option fa_exact_prefill must be 1");
    const Hparams &hp = c->m->hp;
    ScorePlan plan;
    std::string err;
    if (!score_plan(clips, n_tokens, S, include_eos, (int)c->staged_n.size(), c->max_batch, plan, err)) return fail(QASR_ERR_ARG, err);
    const int n_out = (int)plan.out_off[S];
    long n_tok = 0;
    for (int s = 0; s < S; s++) n_tok += n_tokens[s];
    if ((n_tok && !tokens) || (n_out && (!logprobs || !greedy_ids || !greedy_logprobs))) return fail(QASR_ERR_ARG, "bad arguments");
    for (long i = 0; i < n_tok; i++)
        if (tokens[i] < 0 || tokens[i] >= hp.vocab) return fail(QASR_ERR_ARG, "token id out of range");
    if (n_out == 0) {   // (empty hypotheses without the EOS: valid, nothing to run)
        *count = 0;
        return 0;
    }
    // (the prompt length from the clip's samples, as qasr_run_stream's estimate: checked before any work)
    for (int s = 0; s < S; s++) {
        const int P = qasr_prompt_len(encoder_frames(mel_frames(std::max(c->staged_n[clips[s]], 0)))) + (int)c->sys_ids.size();
        if (P + n_tokens[s] + 1 > c->max_ctx) return fail(QASR_ERR_ARG, "Context length exceeded (prompt + n_tokens + 1 > max_ctx)");
    }
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    hipStream_t st = c->st;
    int rc;
    // mel + encoder + prompt prefill of the D distinct clips, clip d's prompt into slot d * G
    std::vector<int> n(plan.D), slots(plan.D);
    std::vector<long> off(plan.D);
    for (int d = 0; d < plan.D; d++) {
        n[d] = c->staged_n[plan.clip[d]];
        off[d] = c->staged_off[plan.clip[d]];
        slots[d] = d * plan.G;
    }
    FrontEnd fe;
    std::swap(n, c->staged_n);
    std::swap(off, c->staged_off);
    rc = front_end_staged(c, 1, &slots, fe);
    std::swap(n, c->staged_n);   // the staged pool stays
    std::swap(off, c->staged_off);
    if (rc) return rc;
    for (int s = 0; s < S; s++)
        if (fe.P[plan.group[s]] + n_tokens[s] + 1 > c->max_ctx) return fail(QASR_ERR_STATE, "prompt length differs from its estimate");
    // pass 1: every hypothesis's first token from its clip's last prompt row
    if ((rc = run_score_rows(c, score_rows_prompt(plan, fe.P.data(), tokens, n_tokens, hp.eos_id), logprobs, greedy_ids, greedy_logprobs)))
        return rc;
    // pass 2: the prompts' KV rows to the hypotheses' slots, then every hypothesis's tokens as one chunk
    const ScoreChunk ch = score_chunk(plan, fe.P.data(), tokens, n_tokens, hp.eos_id);
    if (!ch.len.empty()) {
        std::vector<int> parent, from, to, tab;
        score_fork(plan, fe.P.data(), parent, from, to);
        const int B = plan.D * plan.G, hi = *std::max_element(to.begin(), to.end());
        if (hi > 0) {
            tab = parent;
            tab.insert(tab.end(), from.begin(), from.end());
            tab.insert(tab.end(), to.begin(), to.end());
            if ((rc = upload(c, c->fork_args, tab))) return rc;
            const int *d = c->fork_args.as<int>();
            if (!launch_kv_fork(fork_args(c, d, d + B, d + 2 * B, B, plan.G, (hi + 7) / 8), st))
                return fail(QASR_ERR_STATE, "qasr_score: the KV fork declined its shape");
        }
        const std::vector<int> none((size_t)ch.len.size(), -1), zero((size_t)ch.len.size(), 0);
        if ((rc = prefill_layers(c, ch.ids, ch.len, nullptr, none, zero, &ch.slot, &ch.pos0))) return rc;
        if ((rc = reset_granules(c))) return rc;
        if ((rc = run_score_rows(c, ch.rows, logprobs, greedy_ids, greedy_logprobs))) return rc;
    }
    HIPCHK(hipEventRecord(c->ev[EV_END], st));
    HIPCHK(hipEventSynchronize(c->ev[EV_END]));
    if ((rc = check_dev_err(c))) return rc;
    if (sum_logprob)
        for (int s = 0; s < S; s++) {
            float sum = 0.f;
            for (long k = plan.out_off[s]; k < plan.out_off[s + 1]; k++) sum += logprobs[k];
            sum_logprob[s] = sum;
        }
    c->lp_step_B = c->tk_step_B = 0;   // (the prompts' prefill is not a step the caller asked for)
    if ((rc = run_timings(c, 0, t))) return rc;
    *count = n_out;
    return 0;
}

// (a count on success, so errors are minus the code, as qasr_get_beams)
extern "C" int qasr_prefill_score(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, const float *feats,
                                  const int *audio_pos, const int *N, const int *slots, int B, const int32_t *targets,
                                  float *logprobs, int32_t *greedy_ids, float *greedy_logprobs, int cap) {
    int count = 0;
    const int rc = prefill_score(c, ids, P, n_past, feats, audio_pos, N, slots, B, targets, logprobs, greedy_ids, greedy_logprobs, cap, &count);
    return rc ? -rc : count;
}

extern "C" int qasr_score(qasr_ctx *c, const int *clips, const int32_t *tokens, const int *n_tokens, int S, int include_eos,
                          float *logprobs, int32_t *greedy_ids, float *greedy_logprobs, float *sum_logprob, qasr_timings *t) {
    int count = 0;
    const int rc = score(c, clips, tokens, n_tokens, S, include_eos, logprobs, greedy_ids, greedy_logprobs, sum_logprob, t, &count);
    return rc ? -rc : count;
}
