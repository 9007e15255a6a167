// engine_align.hip -- the forced aligner on the prefill stage of
// engine_stages.hip, and the CLI's JSON documents built from its classes.
#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

// ------------------------------------------------------------ forced aligner
// ForcedAligner::align (src/forced_aligner.cpp:1636-1720), device part: mel ->
// aligner encoder (padded chunks, 104-frame windows) -> <|audio_start|> pad x n
// <|audio_end|> text prompt (n from HF _get_feat_extract_output_lengths, the
// encoder rows spliced from index 1) -> one causal prefill -> at every
// timestamp-token row: RMSNorm -> classify head -> argmax (strict '>', :1280-1306).
// B clips at once (configs[4]'s aligner leg over a rank's transcripts): the
// mel and the windowed encoder of all clips in one pass, one prefill of the B
// prompts (prefill_layers' sequences), one classify GEMM over every timestamp
// row of every clip.  Rows are independent in each of them, so a clip's
// classes are the same alone or in a batch (tests/test_gpu_aligner.py).
static int align_classes(qasr_ctx *c, const float *const *pcm, const int *n, const std::vector<std::vector<int32_t>> &text_ids,
                         std::vector<std::vector<int32_t>> &classes, qasr_timings *t) {
    qasr_model *m = c->m;
    const Hparams &hp = m->hp;
    const int B = (int)text_ids.size();
    if (!hp.aligner || !m->cls_w) return fail(QASR_ERR_STATE, "not a ForcedAligner model");
    if (B <= 0 || B > c->max_batch) return fail(QASR_ERR_ARG, "aligner batch exceeds the context's max_batch");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    hipStream_t s = c->st;
    int rc;
    std::vector<long> off;
    std::vector<int> nv(n, n + B);
    for (int b = 0; b < B; b++)
        if (n[b] <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    if ((rc = pack_pcm(c, pcm, n, B, off))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_START], s));
    std::vector<long> mo;
    std::vector<int> T, Nb;
    if ((rc = run_mel(c, off, nv, mo, T))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_MEL], s));
    if ((rc = run_encoder(c, c->mel.as<float>(), mo, T, false, Nb))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_ENC], s));
    std::vector<int32_t> ids;
    std::vector<int> P(B), ap(B, 1), rows, nrows(B, 0);
    for (int b = 0; b < B; b++) {
        const std::vector<int32_t> ib = build_align_tokens(hp, text_ids[b], feat_extract_output_lengths(T[b]));
        P[b] = (int)ib.size();
        if (P[b] > c->max_ctx) return fail(QASR_ERR_ARG, "Context length exceeded (aligner prompt > max_ctx)");
        for (int i = 0; i < P[b]; i++)
            if (ib[i] == hp.timestamp_id) {
                rows.push_back((int)ids.size() + i);   // the row in the prefill's concatenated rows
                nrows[b]++;
            }
        ids.insert(ids.end(), ib.begin(), ib.end());
    }
    if ((rc = prefill_layers(c, ids, P, c->feats.as<float>(), ap, Nb, nullptr))) return rc;
    const int NT = (int)rows.size(), H = hp.hidden;
    std::vector<unsigned long long> keys(NT);
    if (NT > 0) {
        if ((rc = upload(c, c->ats, rows)) || (rc = ensure(c, c->atx, (size_t)NT * H * 2)) || (rc = ensure(c, c->aam, (size_t)NT * 8)))
            return rc;
        HIPCHK(hipMemsetAsync(c->aam.p, 0, (size_t)NT * 8, s));
        launch_rmsnorm_f16(c->px.as<float>(), H, c->ats.as<int>(), NT, H, m->out_norm, hp.rms_eps, c->atx.as<uint16_t>(), s);
        GemmArgs g{};
        g.A = c->atx.as<uint16_t>(); g.lda = H; g.W = m->cls_w; g.ldw = H; g.M = NT; g.N = m->cls_rows; g.K = H;
        g.amax = c->aam.as<unsigned long long>(); g.n_valid = hp.classify_num;
        launch_gemm_c(c, AM_DENSE, EPI_ARGMAX, g, s);
        HIPCHK(hipGetLastError());
        if ((rc = declined_check("aligner head"))) return rc;
        HIPCHK(hipMemcpyAsync(keys.data(), c->aam.p, (size_t)NT * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipEventRecord(c->ev[EV_PREFILL], s));
    HIPCHK(hipEventSynchronize(c->ev[EV_PREFILL]));
    classes.assign(B, {});
    for (int b = 0, k = 0; b < B; b++)
        for (int i = 0; i < nrows[b]; i++, k++) classes[b].push_back((int32_t)(0xffffffffu - (uint32_t)(keys[k] & 0xffffffffu)));
    if (t) {
        float a = 0, bb = 0, d = 0, tt = 0;
        HIPCHK(hipEventElapsedTime(&a, c->ev[EV_START], c->ev[EV_MEL]));
        HIPCHK(hipEventElapsedTime(&bb, c->ev[EV_MEL], c->ev[EV_ENC]));
        HIPCHK(hipEventElapsedTime(&d, c->ev[EV_ENC], c->ev[EV_PREFILL]));
        HIPCHK(hipEventElapsedTime(&tt, c->ev[EV_START], c->ev[EV_PREFILL]));
        *t = qasr_timings{a, bb, d, 0.0, tt, 0};
    }
    return 0;
}
static int align_classes(qasr_ctx *c, const float *pcm, int n, const std::vector<int32_t> &text_ids, std::vector<int32_t> &classes,
                         qasr_timings *t) {
    std::vector<std::vector<int32_t>> cls;
    const int rc = align_classes(c, &pcm, &n, {text_ids}, cls, t);
    if (!rc) classes = cls[0];
    return rc;
}

extern "C" int qasr_align(qasr_ctx *c, const float *pcm, int n, const int32_t *text_ids, int n_text, int32_t *classes,
                          int cap, int *n_ts, qasr_timings *t) {
    if (!c || !pcm || n <= 0 || n_text < 0 || (n_text && !text_ids) || !n_ts) return fail(QASR_ERR_ARG, "bad arguments");
    std::vector<int32_t> cls;
    int rc = align_classes(c, pcm, n, std::vector<int32_t>(text_ids, text_ids + n_text), cls, t);
    if (rc) return rc;
    *n_ts = (int)cls.size();
    if (classes) for (int i = 0; i < (int)cls.size() && i < cap; i++) classes[i] = cls[i];
    return 0;
}

// ForcedAligner::tokenize_with_timestamps (src/forced_aligner.cpp:1564-1609)
static std::vector<int32_t> align_tokens(const qasr_model *m, const std::string &text, const std::string &lang,
                                         std::vector<std::string> &words) {
    words = (lang == "korean" && !m->ko_dict.empty()) ? tokenize_korean(text, m->ko_dict) : split_words(text);
    std::vector<int32_t> ids;
    for (const std::string &w : words) {
        std::vector<int32_t> t = m->tok.encode_word(w);
        ids.insert(ids.end(), t.begin(), t.end());
        ids.push_back(m->hp.timestamp_id);
        ids.push_back(m->hp.timestamp_id);
    }
    return ids;
}

extern "C" int qasr_align_tokenize(const qasr_model *m, const char *text, const char *language, int32_t *ids, int cap,
                                   int *n_words) {
    if (!m || !text) return fail(QASR_ERR_ARG, "bad arguments");
    std::vector<std::string> words;
    std::vector<int32_t> v = align_tokens(m, text, language ? language : "", words);
    if (ids) for (int i = 0; i < (int)v.size() && i < cap; i++) ids[i] = v[i];
    if (n_words) *n_words = (int)words.size();
    return (int)v.size();
}

extern "C" int qasr_align_words(const qasr_model *m, const char *text, const char *language, char *out, int cap) {
    if (!m || !text) return -fail(QASR_ERR_ARG, "bad arguments");
    std::vector<std::string> words;
    align_tokens(m, text, language ? language : "", words);
    std::string j;
    for (size_t i = 0; i < words.size(); i++) { if (i) j += '\n'; j += words[i]; }
    if (out && cap > 0) {
        const size_t k = std::min(j.size(), (size_t)cap - 1);
        memcpy(out, j.data(), k);
        out[k] = 0;
    }
    return (int)j.size();
}

extern "C" int qasr_fix_timestamps(const int32_t *classes, int n, int32_t *out) {
    if (n < 0 || (n && (!classes || !out))) return fail(QASR_ERR_ARG, "bad arguments");
    std::vector<int32_t> r = fix_timestamp_classes(std::vector<int32_t>(classes, classes + n));
    if (n) memcpy(out, r.data(), (size_t)n * 4);
    return 0;
}

static std::string json_escape(const std::string &s) {   // src/main.cpp:230-254
    std::string r;
    for (char ch : s) {
        switch (ch) {
            case '"': r += "\\\""; break;
            case '\\': r += "\\\\"; break;
            case '\b': r += "\\b"; break;
            case '\f': r += "\\f"; break;
            case '\n': r += "\\n"; break;
            case '\r': r += "\\r"; break;
            case '\t': r += "\\t"; break;
            default:
                if ((unsigned char)ch < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", (unsigned char)ch); r += b; }
                else r += ch;
        }
    }
    return r;
}

// whole alignment -> the CLI's JSON document (src/main.cpp:257-276); returns
// the JSON length (excluding NUL) or minus the error code; writes at most
// cap-1 bytes + NUL
static std::string align_doc(const qasr_model *m, const std::vector<std::string> &words, const std::vector<int32_t> &cls, int n);
static int put_str(const std::string &js, char *out, int cap) {
    if (out && cap > 0) {
        const size_t k = std::min(js.size(), (size_t)cap - 1);
        memcpy(out, js.data(), k);
        out[k] = 0;
    }
    return (int)js.size();
}
extern "C" int qasr_align_json(qasr_ctx *c, const float *pcm, int n, const char *text, const char *language, char *out,
                               int cap, qasr_timings *t) {
    if (!c || !pcm || n <= 0 || !text) return -fail(QASR_ERR_ARG, "bad arguments");
    const qasr_model *m = c->m;
    std::vector<std::string> words;
    const std::vector<int32_t> ids = align_tokens(m, text, language ? language : "", words);
    std::vector<int32_t> cls;
    int rc = align_classes(c, pcm, n, ids, cls, t);
    if (rc) return -rc;
    return put_str(align_doc(m, words, cls, n), out, cap);
}

// B clips in one aligner pass (align_classes' batch form): the documents as
// one JSON array, in input order; returns its length or minus the error code
extern "C" int qasr_align_json_batch(qasr_ctx *c, const float *const *pcm, const int *n, const char *const *text, int B,
                                     const char *language, char *out, int cap, qasr_timings *t) {
    if (!c || !pcm || !n || !text || B <= 0) return -fail(QASR_ERR_ARG, "bad arguments");
    const qasr_model *m = c->m;
    std::vector<std::vector<std::string>> words(B);
    std::vector<std::vector<int32_t>> ids(B), cls;
    for (int b = 0; b < B; b++) {
        if (!pcm[b] || n[b] <= 0 || !text[b]) return -fail(QASR_ERR_ARG, "bad arguments");
        ids[b] = align_tokens(m, text[b], language ? language : "", words[b]);
    }
    int rc = align_classes(c, pcm, n, ids, cls, t);
    if (rc) return -rc;
    std::string js = "[";
    for (int b = 0; b < B; b++) js += (b ? ",\n" : "") + align_doc(m, words[b], cls[b], n[b]);
    return put_str(js + "]", out, cap);
}

// the CLI's document for one clip (src/main.cpp:257-276)
static std::string align_doc(const qasr_model *m, const std::vector<std::string> &words, const std::vector<int32_t> &cls, int n) {
    const std::vector<int32_t> fixed = fix_timestamp_classes(cls);
    const float dur = (float)n / 16000.0f, seg = m->hp.ts_segment_ms / 1000.0f;
    std::vector<float> ts(fixed.size());
    for (size_t i = 0; i < fixed.size(); i++) ts[i] = std::min(fixed[i] * seg, dur);
    std::string js = "{\n  \"words\": [\n";
    for (size_t i = 0; i < words.size(); i++) {
        const float st = 2 * i < ts.size() ? ts[2 * i] : 0.0f, en = 2 * i + 1 < ts.size() ? ts[2 * i + 1] : dur;
        char b[64];
        js += "    {\"word\": \"" + json_escape(words[i]) + "\", ";
        snprintf(b, sizeof b, "\"start\": %.3f, \"end\": %.3f}", st, en);
        js += b;
        if (i + 1 < words.size()) js += ",";
        js += "\n";
    }
    js += "  ]\n}";
    return js;
}
