// engine_constrain.hip -- decoding constraints: qasr_constraints_validate, qasr_set_constraints /
// qasr_get_constraints and the constraint stage that follows the bookkeeping of a prefill or decode step while
// constraints are on (constrain.hip: the edits of the fp32 logits, then the constrained token into d_tok and the
// history slot the bookkeeping just wrote).
#include "engine_impl.h"

#include <set>

using namespace qasr;
using namespace qasr::eng;

static_assert(QASR_NGRAM_MAX == kConstrainNgramMax && QASR_BIAS_MAX == kConstrainBiasMax, "the header's limits are the kernels'");

// ------------------------------------------------------------------ ranges
extern "C" int qasr_constraints_validate(const qasr_constraints *k, int vocab) {
    if (!k) return fail(QASR_ERR_ARG, "constraints: null");
    if (k->no_repeat_ngram < 0 || k->no_repeat_ngram > QASR_NGRAM_MAX) return fail(QASR_ERR_ARG, "constraints: no_repeat_ngram must be in 0..8");
    if (!(k->repetition_penalty > 0.f && k->repetition_penalty <= 10.f))
        return fail(QASR_ERR_ARG, "constraints: repetition_penalty must be in (0, 10]");
    if (k->penalty_last_n < 0) return fail(QASR_ERR_ARG, "constraints: penalty_last_n must be >= 0");
    if (k->n_bias < 0 || k->n_bias > QASR_BIAS_MAX) return fail(QASR_ERR_ARG, "constraints: n_bias must be in 0..1024");
    if (k->n_bias > 0 && (!k->bias_ids || !k->bias)) return fail(QASR_ERR_ARG, "constraints: n_bias > 0 without bias_ids and bias");
    std::set<int32_t> seen;
    for (int i = 0; i < k->n_bias; i++) {
        const int32_t v = k->bias_ids[i];
        if (v < 0 || (vocab > 0 && v >= vocab)) return fail(QASR_ERR_ARG, "constraints: bias id " + std::to_string(v) + " outside the vocabulary");
        if (!seen.insert(v).second) return fail(QASR_ERR_ARG, "constraints: bias id " + std::to_string(v) + " listed twice");
        const float b = k->bias[i];
        if (std::isnan(b) || b == INFINITY) return fail(QASR_ERR_ARG, "constraints: a bias must be finite or -inf");
    }
    return 0;
}

// ------------------------------------------------------------------ state
static int ensure_constrain(qasr_ctx *c) {
    if (c->cd.gtok) return 0;   // (the last one allocated below)
    const size_t rows = (size_t)c->max_batch;
    qasr_ctx::ConstrainDev d;
    int rc;
    if ((rc = dev_alloc(c, (void **)&d.prm, sizeof(ConstrainParams))) || (rc = dev_alloc(c, (void **)&d.ids, (size_t)QASR_BIAS_MAX * 4)) ||
        (rc = dev_alloc(c, (void **)&d.bias, (size_t)QASR_BIAS_MAX * 4)) || (rc = dev_alloc(c, (void **)&d.skey, rows * 8)) ||
        (rc = dev_alloc(c, (void **)&d.flag, rows * 4)) || (rc = dev_alloc(c, (void **)&d.gtok, rows * 4)))
        return rc;
    HIPCHK(hipMemset(d.ids, 0, (size_t)QASR_BIAS_MAX * 4));
    HIPCHK(hipMemset(d.bias, 0, (size_t)QASR_BIAS_MAX * 4));
    HIPCHK(hipMemset(d.skey, 0, rows * 8));
    HIPCHK(hipMemset(d.flag, 0, rows * 4));
    HIPCHK(hipMemset(d.gtok, 0, rows * 4));
    c->cd = d;
    return 0;
}

extern "C" int qasr_set_constraints(qasr_ctx *c, const qasr_constraints *k) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    if (!k) {   // off: no kernel, graph or result of the other paths changes
        c->con = qasr_ctx::ConstrainState();
        return 0;
    }
    if (int rc = qasr_constraints_validate(k, c->m->hp.vocab)) return rc;
    if (k->no_repeat_ngram == 0 && k->repetition_penalty == 1.f && k->n_bias == 0) {
        c->con = qasr_ctx::ConstrainState();
        return 0;
    }
    if (c->m->hp.vocab > kConstrainVocabMax) return fail(QASR_ERR_STATE, "constraints: the model's vocabulary exceeds 2^20");
    HIPCHK(hipSetDevice(c->m->device));
    if (int rc = ensure_constrain(c)) return rc;
    ConstrainParams prm;
    prm.ngram = k->no_repeat_ngram;
    prm.p = k->repetition_penalty;
    prm.inv_p = 1.0f / k->repetition_penalty;
    prm.last_n = k->penalty_last_n;
    prm.n_bias = k->n_bias;
    // (device memory: a captured step serves any values)
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipMemcpy(c->cd.prm, &prm, sizeof prm, hipMemcpyHostToDevice));
    if (k->n_bias) {
        HIPCHK(hipMemcpy(c->cd.ids, k->bias_ids, (size_t)k->n_bias * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->cd.bias, k->bias, (size_t)k->n_bias * 4, hipMemcpyHostToDevice));
    }
    // (zero at rest whatever an earlier failed call left)
    HIPCHK(hipMemset(c->cd.skey, 0, (size_t)c->max_batch * 8));
    HIPCHK(hipMemset(c->cd.flag, 0, (size_t)c->max_batch * 4));
    c->con.on = true;
    c->con.ngram = k->no_repeat_ngram;
    c->con.p = k->repetition_penalty;
    c->con.last_n = k->penalty_last_n;
    c->con.ids.assign(k->bias_ids, k->bias_ids + k->n_bias);
    c->con.bias.assign(k->bias, k->bias + k->n_bias);
    return 0;
}

extern "C" int qasr_get_constraints(const qasr_ctx *c, qasr_constraints *out, int32_t *ids, float *bias, int cap) {
    if (!c || !out || cap < 0) return fail(QASR_ERR_ARG, "bad arguments");
    const int nb = (int)c->con.ids.size();
    if ((ids || bias) && cap < nb) return fail(QASR_ERR_ARG, "buffers hold fewer entries than the bias list");
    out->no_repeat_ngram = c->con.ngram;
    out->repetition_penalty = c->con.p;
    out->penalty_last_n = c->con.last_n;
    out->n_bias = nb;
    out->bias_ids = ids;
    out->bias = bias;
    if (ids) std::copy(c->con.ids.begin(), c->con.ids.end(), ids);
    if (bias) std::copy(c->con.bias.begin(), c->con.bias.end(), bias);
    return 0;
}

// --------------------------------------------------------- constraint stage
int qasr::eng::constrain_step(qasr_ctx *c, int B, int src_div) {
    const int V = c->m->hp.vocab;
    if (B > c->max_batch) return fail(QASR_ERR_ARG, "constraints: rows exceed the context's max_batch");
    ConstrainArgs a{};
    a.logits = c->d_logits; a.ld = V; a.n_valid = V;
    a.greedy = c->d_tok;
    a.hist_in = c->d_hist; a.hist_stride = c->hist_cap; a.step = c->d_step;
    a.prm = c->cd.prm; a.bias_ids = c->cd.ids; a.bias = c->cd.bias;
    a.skey = c->cd.skey; a.flag = c->cd.flag;
    a.tok = c->d_tok; a.hist = c->d_hist; a.gtok = c->cd.gtok;
    a.R = B; a.src_div = src_div;
    if (!launch_constrain(a, 0, c->st)) return fail(QASR_ERR_STATE, "constraints: the launcher declined " + std::to_string(B) + " rows");
    return 0;
}
