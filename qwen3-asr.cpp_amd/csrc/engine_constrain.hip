// engine_constrain.hip -- decoding constraints: qasr_constraints_validate, qasr_set_constraints /
// qasr_get_constraints and the constraint stage that follows the bookkeeping of a prefill or decode step while
// constraints are on (constrain.hip: the edits of the fp32 logits, then the constrained token into d_tok and the
// history slot the bookkeeping just wrote).  Hotword boosting is part of the same stage:
// qasr_phrases_validate, qasr_set_phrases / qasr_get_phrases, qasr_phrase_tokenize.
#include "engine_impl.h"
#include "phrase_host.h"

#include <set>

using namespace qasr;
using namespace qasr::eng;

static_assert(QASR_NGRAM_MAX == kConstrainNgramMax && QASR_BIAS_MAX == kConstrainBiasMax, "the header's limits are the kernels'");
static_assert(QASR_PHRASE_MAX == kPhraseMax && QASR_PHRASE_LEN_MAX == kPhraseLenMax && kPhraseWalkMax == kPhraseLenMax - 1,
              "the header's limits are the compiler's and the kernel's");

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
    if ((rc = dev_alloc(c, (void **)&d.ph, sizeof(PhraseTrie)))) return rc;
    HIPCHK(hipMemset(d.ph, 0, sizeof(PhraseTrie)));
    if ((rc = dev_alloc(c, (void **)&d.prm, sizeof(ConstrainParams))) || (rc = dev_alloc(c, (void **)&d.ids, (size_t)QASR_BIAS_MAX * 4)) ||
        (rc = dev_alloc(c, (void **)&d.bias, (size_t)QASR_BIAS_MAX * 4)) || (rc = dev_alloc(c, (void **)&d.skey, rows * 8)) ||
        (rc = dev_alloc(c, (void **)&d.flag, rows * 4)) || (rc = dev_alloc(c, (void **)&d.gtok, rows * 4)))
        return rc;
    HIPCHK(hipMemset(d.ids, 0, (size_t)QASR_BIAS_MAX * 4));
    HIPCHK(hipMemset(d.bias, 0, (size_t)QASR_BIAS_MAX * 4));
    HIPCHK(hipMemset(d.skey, 0, rows * 8));
    HIPCHK(hipMemset(d.flag, 0, rows * 4));
    HIPCHK(hipMemset(d.gtok, 0, rows * 4));
    const ConstrainParams neutral{0, 1.f, 1.f, 0, 0};
    HIPCHK(hipMemcpy(d.prm, &neutral, sizeof neutral, hipMemcpyHostToDevice));
    c->cd = d;
    return 0;
}

// constraints off: the parameters a stage that phrases keep on reads become the neutral ones
static int constraints_off(qasr_ctx *c) {
    const bool was_on = c->con.on;
    c->con = qasr_ctx::ConstrainState();
    if (!was_on || !c->cd.prm) return 0;   // (already off: the device holds the neutral parameters)
    const ConstrainParams neutral{0, 1.f, 1.f, 0, 0};
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipMemcpy(c->cd.prm, &neutral, sizeof neutral, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int qasr_set_constraints(qasr_ctx *c, const qasr_constraints *k) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    if (!k) return constraints_off(c);   // off: no kernel, graph or result of the other paths changes
    if (int rc = qasr_constraints_validate(k, c->m->hp.vocab)) return rc;
    if (k->no_repeat_ngram == 0 && k->repetition_penalty == 1.f && k->n_bias == 0) return constraints_off(c);
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
    c->con.on = true;   // (from here the device's parameters are no longer the neutral ones)
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

// ------------------------------------------------------------------ phrases
extern "C" int qasr_phrases_validate(const qasr_phrases *p, int vocab) {
    if (!p) return fail(QASR_ERR_ARG, "phrases: null");
    const std::string err = phrase_check(p->n_phrases, p->ids, p->len, p->boost, vocab);
    return err.empty() ? 0 : fail(QASR_ERR_ARG, err);
}

extern "C" int qasr_set_phrases(qasr_ctx *c, const qasr_phrases *p) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    PhraseTrieHost tr;
    if (p) {
        if (int rc = qasr_phrases_validate(p, c->m->hp.vocab)) return rc;
        const std::string err = phrase_compile(p->n_phrases, p->ids, p->len, p->boost, tr);
        if (!err.empty()) return fail(QASR_ERR_ARG, err);
    }
    if (!p || p->n_phrases == 0) {   // off: the header a captured step reads says "no phrases"
        const bool was_on = c->phr.on;
        c->phr = qasr_ctx::PhraseState();
        if (!was_on || !c->cd.ph) return 0;   // (already off: the header says so)
        HIPCHK(hipSetDevice(c->m->device));
        HIPCHK(hipStreamSynchronize(c->st));
        HIPCHK(hipMemset(c->cd.ph, 0, sizeof(int)));   // (n_nodes, the first member)
        return 0;
    }
    if (c->m->hp.vocab > kConstrainVocabMax) return fail(QASR_ERR_STATE, "phrases: the model's vocabulary exceeds 2^20");
    HIPCHK(hipSetDevice(c->m->device));
    if (int rc = ensure_constrain(c)) return rc;
    if (!c->cd.ph_bonus) {   // (the last one allocated below)
        qasr_ctx::ConstrainDev d = c->cd;
        int rc;
        if ((rc = dev_alloc(c, (void **)&d.ph_off, (size_t)(kPhraseNodeMax + 1) * 4)) || (rc = dev_alloc(c, (void **)&d.ph_tok, (size_t)kPhraseEdgeMax * 4)) ||
            (rc = dev_alloc(c, (void **)&d.ph_dst, (size_t)kPhraseEdgeMax * 4)) || (rc = dev_alloc(c, (void **)&d.ph_bonus, (size_t)kPhraseEdgeMax * 4)))
            return rc;
        c->cd = d;
    }
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipMemcpy(c->cd.ph_off, tr.child_off.data(), tr.child_off.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->cd.ph_tok, tr.tok.data(), tr.tok.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->cd.ph_dst, tr.dst.data(), tr.dst.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->cd.ph_bonus, tr.bonus.data(), tr.bonus.size() * 4, hipMemcpyHostToDevice));
    const PhraseTrie hd{tr.nodes(), c->cd.ph_off, c->cd.ph_tok, c->cd.ph_dst, c->cd.ph_bonus};
    c->phr.on = true;   // (from here the header names a list)
    HIPCHK(hipMemcpy(c->cd.ph, &hd, sizeof hd, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->cd.skey, 0, (size_t)c->max_batch * 8));
    HIPCHK(hipMemset(c->cd.flag, 0, (size_t)c->max_batch * 4));
    size_t total = 0;
    for (int k = 0; k < p->n_phrases; k++) total += (size_t)p->len[k];
    c->phr.on = true;
    c->phr.ids.assign(p->ids, p->ids + total);
    c->phr.len.assign(p->len, p->len + p->n_phrases);
    c->phr.boost.assign(p->boost, p->boost + p->n_phrases);
    return 0;
}

extern "C" int qasr_get_phrases(const qasr_ctx *c, qasr_phrases *out, int32_t *ids, int32_t *len, float *boost, int cap_ids, int cap_phrases) {
    if (!c || !out || cap_ids < 0 || cap_phrases < 0) return fail(QASR_ERR_ARG, "bad arguments");
    const int n = (int)c->phr.len.size();
    if (ids && cap_ids < (int)c->phr.ids.size()) return fail(QASR_ERR_ARG, "ids holds fewer entries than the phrases' tokens");
    if ((len || boost) && cap_phrases < n) return fail(QASR_ERR_ARG, "len / boost hold fewer entries than the phrase list");
    out->n_phrases = n;
    out->ids = ids;
    out->len = len;
    out->boost = boost;
    if (ids) std::copy(c->phr.ids.begin(), c->phr.ids.end(), ids);
    if (len) std::copy(c->phr.len.begin(), c->phr.len.end(), len);
    if (boost) std::copy(c->phr.boost.begin(), c->phr.boost.end(), boost);
    return 0;
}

extern "C" int qasr_phrase_tokenize(const qasr_model *m, const char *text, int32_t *ids, int32_t *len, int cap_ids) {
    if (!m || !text || !ids || !len || cap_ids < 0) return -fail(QASR_ERR_ARG, "bad arguments");
    std::string s(text);
    const char *ws = " \t\r\n\f\v";
    const size_t b = s.find_first_not_of(ws);
    if (b == std::string::npos) return -fail(QASR_ERR_ARG, "phrases: an empty hotword");
    s = s.substr(b, s.find_last_not_of(ws) - b + 1);
    std::vector<int32_t> v[2] = {m->tok.encode(s), m->tok.encode(s, true)};   // (the second: " " + text)
    const int n = v[0] == v[1] ? 1 : 2;
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        if (v[i].empty()) return -fail(QASR_ERR_ARG, "phrases: an empty hotword");
        if ((int)v[i].size() > QASR_PHRASE_LEN_MAX)
            return -fail(QASR_ERR_ARG, "phrases: hotword \"" + s + "\" takes " + std::to_string(v[i].size()) + " tokens, a phrase holds 1..16");
        if (at + v[i].size() > (size_t)cap_ids) return -fail(QASR_ERR_ARG, "phrases: ids holds fewer entries than the hotword's tokens");
        std::copy(v[i].begin(), v[i].end(), ids + at);
        at += v[i].size();
        len[i] = (int32_t)v[i].size();
    }
    return n;
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
    a.ph = c->cd.ph;
    if (!launch_constrain(a, 0, c->st)) return fail(QASR_ERR_STATE, "constraints: the launcher declined " + std::to_string(B) + " rows");
    return 0;
}
