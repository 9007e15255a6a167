// engine.hip -- C-ABI implementation (include/qasr_capi.h), restating
// Qwen3ASR::transcribe_internal (src/qwen3_asr.cpp:81-149) on HIP:
//   PCM -> mel -> conv front-end -> encoder -> prompt + splice -> prefill ->
//   greedy decode (HIP-graph replayed step) -> token ids
// This unit: the last-error string, the option table, context creation and
// its buffers, the fused launches' counters and device lock, profile report.
// engine_impl.h maps the other engine_*.hip units.
#include <memory>

#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

// ----------------------------------------------------------------- errors
static thread_local std::string g_err;

int qasr::eng::fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// a GEMM / GEMV launch that found no kernel for its (mode, epilogue) pair
// (gemm.hip note_declined) fails the stage that issued it
int qasr::eng::declined_check(const char *stage) {
    std::string msg;
    if (qasr::take_declined(&msg)) return fail(QASR_ERR_STATE, std::string(stage) + ": " + msg);
    return 0;
}

// ---------------------------------------------------------------- options
// per-context options of the fused batch-1 launches: name (qasr_ctx_set_option),
// environment default, field
struct FuseOption {
    const char *name, *env;
    int FuseCfg::*field;
};
static const std::vector<FuseOption> &fuse_options() {
    static const std::vector<FuseOption> v = {
        {"fuse_ffn", "QASR_FUSE_FFN", &FuseCfg::ffn},          {"fuse_qkv", "QASR_FUSE_QKV", &FuseCfg::qkv},
        {"fuse_o", "QASR_FUSE_O", &FuseCfg::o},
        {"ffn_delay", "QASR_FFN_DELAY", &FuseCfg::ffn_delay},
        {"ffn_wdelay", "QASR_FFN_WDELAY", &FuseCfg::ffn_wdelay}, {"qkv_delay", "QASR_FUSE_DELAY", &FuseCfg::qkv_delay},
        {"o_delay", "QASR_FUSE_ODELAY", &FuseCfg::o_delay},    {"att_spl1", "QASR_ATT_SPL1", &FuseCfg::spl1},
        {"poll_limit", "QASR_POLL_LIMIT", &FuseCfg::poll_limit}, {"handoff_fence", "QASR_HANDOFF_FENCE", &FuseCfg::fence},
        {"fa_exact_prefill", "QASR_FA_EXACT_PREFILL", &FuseCfg::fa_exact_prefill},
        {"enc_attn_f32", "QASR_ENC_ATTN_F32", &FuseCfg::enc_attn_f32},
        {"gemm_regs", "QASR_GEMM_REGS", &FuseCfg::gemm_regs},
        {"gran", "QASR_GRAN", &FuseCfg::gran},
        {"fa_exact_decode", "QASR_FA_EXACT_DECODE", &FuseCfg::fa_exact_decode},
        {"fx_vpf", "QASR_FX_VPF", &FuseCfg::fx_vpf},
        {"kvw_delay", "QASR_KVW_DELAY", &FuseCfg::kvw_delay},
        {"k_stagger", "QASR_K_STAGGER", &FuseCfg::k_stagger},
        {"vt_stagger", "QASR_VT_STAGGER", &FuseCfg::vt_stagger},
        {"att_stream", "QASR_ATT_STREAM", &FuseCfg::att_stream},
        {"skinny", "QASR_SKINNY", &FuseCfg::skinny},
        {"att_spl", "QASR_ATT_SPL", &FuseCfg::att_spl},
        {"kv_nt", "QASR_KV_NT", &FuseCfg::kv_nt},
        {"lmh", "QASR_LMH", &FuseCfg::lmh},
        {"fx_seq", "QASR_FX_SEQ", &FuseCfg::fx_seq},
        {"skinny_inf", "QASR_SKINNY_INF", &FuseCfg::skinny_inf},
        {"skinny_wdef", "QASR_SKINNY_WDEF", &FuseCfg::skinny_wdef},
        {"refill_group", "QASR_REFILL_GROUP", &FuseCfg::refill_group},
        {"live_prefix", "QASR_LIVE_PREFIX", &FuseCfg::live_prefix},
        {"staged_wrap", "QASR_STAGED_WRAP", &FuseCfg::staged_wrap},
        {"poison_scratch", "QASR_POISON_SCRATCH", &FuseCfg::poison},
        {"token_logprobs", "QASR_TOKEN_LOGPROBS", &FuseCfg::token_logprobs},
        {"top_k", "QASR_TOP_K", &FuseCfg::top_k},
        {"lmh_topk", "QASR_LMH_TOPK", &FuseCfg::lmh_topk},
        {"beam_width", "QASR_BEAM_WIDTH", &FuseCfg::beam_width},
        {"sample_slices", "QASR_SAMPLE_SLICES", &FuseCfg::sample_slices},
    };
    return v;
}

// ------------------------------------------- fused-launch counters and lock
// every arrival counter of the fused launches back to rest (zero), on the
// context stream: after an option change and after a wait that gave up
int qasr::eng::reset_counters(qasr_ctx *c) {
    HIPCHK(hipMemsetAsync(c->d_ffncnt, 0, c->ffncnt_bytes(), c->st));
    HIPCHK(hipMemsetAsync(c->d_qcnt, 0, c->qcnt_bytes(), c->st));
    HIPCHK(hipMemsetAsync(c->d_attdone, 0, c->attdone_bytes(), c->st));
    HIPCHK(hipMemsetAsync(c->d_counter, 0, c->counter_bytes(), c->st));
    HIPCHK(hipMemsetAsync(c->d_done, 0, qasr_ctx::kDoneBytes, c->st));
    HIPCHK(hipMemsetAsync(c->d_amax, 0, c->amax_bytes(), c->st));
    return 0;
}

// the QKV and score granules back to zero (no valid tag), on the context stream: tags
// repeat across runs at the same positions
int qasr::eng::reset_granules(qasr_ctx *c) {
    HIPCHK(hipMemsetAsync(c->d_gran, 0, c->gran_bytes(), c->st));
    HIPCHK(hipMemsetAsync(c->d_sgran, 0, c->sgran_bytes(), c->st));
    return 0;
}

// the fused launches' sticky device error word: read (and cleared) after every
// call that ran decode steps; a bounded wait that ran out is a device error
int qasr::eng::check_dev_err(qasr_ctx *c) {
    unsigned e = 0;
    HIPCHK(hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (!e) return 0;
    // a wait that gave up can leave late arrivals in the counters: back to rest
    HIPCHK(hipMemsetAsync(c->d_err, 0, 4, c->st));
    const int rc = reset_counters(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    std::string what;
    if (e & DEVERR_QKV_WAIT) what += " attention<-QKV";
    if (e & DEVERR_O_WAIT) what += " o-proj<-attention";
    if (e & DEVERR_FFN_WAIT) what += " down<-gate/up";
    if (e & DEVERR_SCORE_WAIT) what += " chain<-scores";
    return fail(QASR_ERR_DEVICE, "fused decode launch: an in-launch wait timed out (" + what.substr(1) +
                                     "); outputs of this call are invalid (another process or context sharing the GPU?)");
}

// The batch-1 fused launches assume the whole GPU is theirs (every workgroup
// of a launch co-resident: a role waits on another role in-launch).  Calls
// that can take them hold their device's lock, so contexts driven from
// several host threads on one GPU run those calls one at a time instead of
// sharing the CUs (a GPU shared with another PROCESS is not covered: a wait
// that runs out then fails the call with QASR_ERR_DEVICE; QASR_FUSE_*=0 or
// qasr_ctx_set_option turns the fused launches off).
std::mutex &qasr::eng::device_lock(int device) {
    static std::mutex m[64];
    return m[(unsigned)device % 64];
}

// ---------------------------------------------------------------- buffers
int qasr::eng::dev_alloc(qasr_ctx *c, void **p, size_t bytes) {
    HIPCHK(hipMalloc(p, bytes ? bytes : 256));
    c->owned.push_back({*p, bytes});
    return 0;
}

// grow a scratch buffer (contents are not preserved)
int qasr::eng::ensure(qasr_ctx *c, DevBuf &b, size_t bytes) {
    if (b.n >= bytes && b.p) return 0;
    if (b.p) {
        HIPCHK(hipStreamSynchronize(c->st));
        for (auto it = c->owned.begin(); it != c->owned.end(); ++it)
            if (it->p == b.p) { c->owned.erase(it); break; }
        HIPCHK(hipFree(b.p));
        b.p = nullptr;
    }
    size_t n = std::max<size_t>(bytes + bytes / 4, 4096);
    HIPCHK(hipMalloc(&b.p, n));
    b.n = n;
    c->owned.push_back({b.p, n});
    if (c->fuse.poison) HIPCHK(hipMemsetAsync(b.p, 0xFF, n, c->st));
    return 0;
}

// option top_k: its device buffers, sized for QASR_TOPK_MAX, the first time the option is non-zero
static_assert(QASR_TOPK_MAX == qasr::TOPK_MAX, "the C-ABI's largest K is the row kernel's");
int qasr::eng::ensure_topk(qasr_ctx *c) {
    if (c->d_tkpart) return 0;   // (the last of the five: set only once all are)
    const size_t step = (size_t)c->max_batch * QASR_TOPK_MAX * 4, hist = step * c->hist_cap;
    int32_t *id = nullptr, *hid = nullptr;
    float *lp = nullptr, *hlp = nullptr;
    unsigned long long *part = nullptr;
    int rc;
    if ((rc = dev_alloc(c, (void **)&id, step)) || (rc = dev_alloc(c, (void **)&lp, step)) ||
        (rc = dev_alloc(c, (void **)&hid, hist)) || (rc = dev_alloc(c, (void **)&hlp, hist)) ||
        (rc = dev_alloc(c, (void **)&part, (size_t)lmhead_grid() * 128 * QASR_TOPK_MAX * 8)))
        return rc;   // (what was allocated stays owned by the context and is freed with it)
    c->d_tkid = id; c->d_tklp = lp; c->d_tkhid = hid; c->d_tkhlp = hlp; c->d_tkpart = part;
    return 0;
}

static_assert(QASR_BEAM_MAX == qasr::TOPK_MAX, "a beam step ranks the row kernel's K = W alternatives");
// option beam_width: the beam state (qasr_ctx::BeamDev) and the top-K buffers its steps read, the first time it is >= 2
int qasr::eng::ensure_beam(qasr_ctx *c) {
    if (c->bm.h_lp) return ensure_topk(c);   // (the last one allocated below)
    const size_t rows = (size_t)c->max_batch * 4, hist = rows * c->hist_cap;
    qasr_ctx::BeamDev b;
    int rc;
    if ((rc = ensure_topk(c)) || (rc = dev_alloc(c, (void **)&b.cum, rows)) || (rc = dev_alloc(c, (void **)&b.fin_sum, rows)) ||
        (rc = dev_alloc(c, (void **)&b.fin_lp, rows)) || (rc = dev_alloc(c, (void **)&b.fin_row, rows)) ||
        (rc = dev_alloc(c, (void **)&b.fin_t, rows)) || (rc = dev_alloc(c, (void **)&b.n_fin, rows)) ||
        (rc = dev_alloc(c, (void **)&b.done, rows)) || (rc = dev_alloc(c, (void **)&b.t, rows)) ||
        (rc = dev_alloc(c, (void **)&b.P, rows)) || (rc = dev_alloc(c, (void **)&b.eos, 4)) || (rc = dev_alloc(c, (void **)&b.parent, rows)) ||
        (rc = dev_alloc(c, (void **)&b.from, rows)) || (rc = dev_alloc(c, (void **)&b.to, rows)) ||
        (rc = dev_alloc(c, (void **)&b.h_par, hist)) || (rc = dev_alloc(c, (void **)&b.h_id, hist)) ||
        (rc = dev_alloc(c, (void **)&b.h_lp, hist)))
        return rc;
    c->bm = b;
    return 0;
}

int qasr::eng::topk_step(qasr_ctx *c, int B) {
    const int K = step_k(c);
    if (K <= 0) return 0;
    if (!launch_topk_rows(c->d_logits, c->m->hp.vocab, B, 0, K, c->d_step, c->d_tkid, c->d_tklp, c->d_tkhid, c->d_tkhlp,
                          c->hist_cap, c->st))
        return fail(QASR_ERR_STATE, "option top_k: the row kernel declined K = " + std::to_string(K));
    return 0;
}

// host bytes -> dst on the context stream through the pinned staging area (upload)
int qasr::eng::stage_pinned(qasr_ctx *c, const void *src, size_t bytes, void *dst) {
    const size_t need = (bytes + 255) / 256 * 256;
    if (c->pin_used + need > c->pin_cap) {
        HIPCHK(hipStreamSynchronize(c->st));   // every earlier staged copy has landed
        c->pin_used = 0;
        if (need > c->pin_cap) {
            if (c->pin) HIPCHK(hipHostFree(c->pin));
            c->pin_cap = std::max<size_t>(need * 2, 1 << 20);
            HIPCHK(hipHostMalloc((void **)&c->pin, c->pin_cap, hipHostMallocDefault));
        }
    }
    char *h = c->pin + c->pin_used;
    c->pin_used += need;
    memcpy(h, src, bytes);
    HIPCHK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, c->st));
    return 0;
}

// ---------------------------------------------------- version and device

extern "C" const char *qasr_last_error(void) { return g_err.c_str(); }
extern "C" const char *qasr_version(void) { return "qasr-mi355x 0.1.0 (gfx950)"; }
extern "C" int qasr_device_count(int *n) {
    int k = 0;
    if (hipGetDeviceCount(&k) != hipSuccess) k = 0;
    if (n) *n = k;
    return 0;
}

extern "C" int qasr_check_expf_nonpos(int device, uint64_t *mismatches) {
    if (!mismatches) return fail(QASR_ERR_ARG, "bad arguments");
    int nd = 0, cur = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return fail(QASR_ERR_DEVICE, "no such HIP device");
    (void)hipGetDevice(&cur);
    if (hipSetDevice(device) != hipSuccess) return fail(QASR_ERR_DEVICE, "hipSetDevice failed");
    unsigned long long bad = ~0ull;
    const hipError_t e = check_expf_nonpos(&bad);
    (void)hipSetDevice(cur);
    if (e != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("expf check: ") + hipGetErrorString(e));
    *mismatches = bad;
    return 0;
}

// --------------------------------------------------------------- context
extern "C" int qasr_ctx_create(qasr_model *m, int max_batch, int max_ctx, qasr_ctx **out) {
    if (!m || !out || max_batch <= 0 || max_ctx <= 0) return fail(QASR_ERR_ARG, "bad context arguments");
    if (!m->arena) return fail(QASR_ERR_STATE, "model was loaded host-only (device QASR_HOST_ONLY)");
    *out = nullptr;
    HIPCHK(hipSetDevice(m->device));
    std::unique_ptr<qasr_ctx> c(new qasr_ctx());
    c->m = m;
    c->max_batch = max_batch;
    c->max_ctx = max_ctx;
    HIPCHK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    for (auto &e : c->ev) HIPCHK(hipEventCreate(&e));
    const Hparams &hp = m->hp;
    // + padding rows: fa_exact.hip's chains read V a few batches past the context
    const size_t kv = (size_t)hp.dec_layers * max_batch * hp.n_kv_head * max_ctx * 128 + kKvPadRows * 128;
    int rc = 0;
    if ((rc = dev_alloc(c.get(), (void **)&c->kc, kv * 2)) || (rc = dev_alloc(c.get(), (void **)&c->vc, kv * 2))) return rc;
    const size_t vt = (size_t)hp.dec_layers * layer_vt(c.get());
    if ((rc = dev_alloc(c.get(), (void **)&c->vt, vt * 2))) return rc;
    HIPCHK(hipMemset(c->vt, 0, vt * 2));
    std::vector<float> rope;
    rope_table(rope, max_ctx, 128, hp.rope_theta);
    if ((rc = dev_alloc(c.get(), (void **)&c->rope, rope.size() * 4))) return rc;
    HIPCHK(hipMemcpy(c->rope, rope.data(), rope.size() * 4, hipMemcpyHostToDevice));
    const int B = max_batch, QD = hp.n_head * 128, KD = hp.n_kv_head * 128;
    c->max_splits = (max_ctx + decode_split_len() - 1) / decode_split_len();
    if (c->max_splits > decode_max_splits())
        return fail(QASR_ERR_ARG, "max_ctx exceeds " + std::to_string(decode_max_splits() * decode_split_len()));
    const char *ng = getenv("QASR_NO_GRAPH");
    c->eager = ng && ng[0] == '1';
#ifdef QASR_DIAG_SKIP   // diagnostic builds only (tools/): drops decode kernels to price them -- wrong tokens
    if (const char *ds = getenv("QASR_DEV_SKIP")) c->dev_skip = atoi(ds);
#endif
    // fused-launch options: environment defaults, per-context overrides via qasr_ctx_set_option
    for (const auto &o : fuse_options()) {
        if (const char *e = getenv(o.env)) c->fuse.*(o.field) = atoi(e);
    }
    if (c->fuse.top_k < 0 || c->fuse.top_k > QASR_TOPK_MAX) return fail(QASR_ERR_ARG, "QASR_TOP_K out of range (0..8)");
    fused_slots(c->fuse);   // co-residency on this context's device
    if (const char *tp = getenv("QASR_DEV_TRACE")) {
        c->trace_path = tp;
        if (const char *tl = getenv("QASR_DEV_TRACE_LAYER")) c->trace_layer = atoi(tl);
        if ((rc = dev_alloc(c.get(), (void **)&c->d_trace, qasr_ctx::kTraceBytes))) return rc;
        HIPCHK(hipMemset(c->d_trace, 0, qasr_ctx::kTraceBytes));
    }
    c->hist_cap = max_ctx;
    // Nothing reads this buffer (it was once a fp16 Q row per sequence), but its place in the allocation
    // order is load-bearing: without it every later fixed buffer moves, and the batch-1 decode step
    // measured 0.9 % slower (profiles/engine_split/bench_ab.txt).  Freed with the context (c->owned).
    void *unread_pad = nullptr;
    if ((rc = dev_alloc(c.get(), (void **)&c->d_tok, B * 4)) || (rc = dev_alloc(c.get(), (void **)&c->d_hist, (size_t)B * max_ctx * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_pos, B * 4)) || (rc = dev_alloc(c.get(), (void **)&c->d_nkv, B * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_slot, B * 4)) || (rc = dev_alloc(c.get(), (void **)&c->d_step, 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_x, (size_t)B * hp.hidden * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_xh, (size_t)B * hp.hidden * 2)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_qkv, (size_t)B * (QD + 2 * KD) * 4)) ||
        (rc = dev_alloc(c.get(), &unread_pad, (size_t)B * QD * 2)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_att, (size_t)B * QD * 2)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_act, (size_t)B * hp.dec_ffn * 2)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_att32, (size_t)B * QD * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_act32, (size_t)B * hp.dec_ffn * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_q8a, (size_t)B * std::max(QD, std::max(hp.hidden, hp.dec_ffn)))) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_q8d, (size_t)B * std::max(QD, std::max(hp.hidden, hp.dec_ffn)) / 32 * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_x32, (size_t)B * std::max(QD, std::max(hp.hidden, hp.dec_ffn)) * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_q8n, (size_t)B * hp.hidden)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_q8nd, (size_t)B * hp.hidden / 32 * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_part, (size_t)B * hp.n_kv_head * c->max_splits * 2 * 132 * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_counter, c->counter_bytes())) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_scores, (size_t)B * hp.n_head * max_ctx * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_qcnt, c->qcnt_bytes())) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_attdone, c->attdone_bytes())) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_gran, c->gran_bytes())) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_sgran, c->sgran_bytes())) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_ffncnt, c->ffncnt_bytes())) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_done, qasr_ctx::kDoneBytes)) || (rc = dev_alloc(c.get(), (void **)&c->d_err, 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_pstamp, (size_t)max_ctx * kStampRec * 8)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_logits, (size_t)B * hp.vocab * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_amax, c->amax_bytes())) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_lp, (size_t)B * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_lphist, (size_t)B * max_ctx * 4)) ||
        (rc = dev_alloc(c.get(), (void **)&c->d_lppart, (size_t)lmhead_grid() * 128 * 8)))
        return rc;
    if (c->fuse.beam_width < 0 || c->fuse.beam_width > QASR_BEAM_MAX) return fail(QASR_ERR_ARG, "QASR_BEAM_WIDTH out of range (0..8)");
    if (c->fuse.top_k && (rc = ensure_topk(c.get()))) return rc;
    if (c->fuse.beam_width >= 2 && (rc = ensure_beam(c.get()))) return rc;
    std::vector<int> slots(B);
    for (int b = 0; b < B; b++) slots[b] = b;
    HIPCHK(hipMemcpy(c->d_slot, slots.data(), B * 4, hipMemcpyHostToDevice));
    // counters and granules start at rest: the same two resets every later call uses
    if ((rc = reset_counters(c.get())) || (rc = reset_granules(c.get()))) return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipMemset(c->d_err, 0, 4));
    c->fuse.err = c->d_err;
    HIPCHK(hipMemset(c->kc, 0, kv * 2));   // decode attention reads whole splits and masks: keep every row finite
    HIPCHK(hipMemset(c->vc, 0, kv * 2));
    *out = c.release();
    return 0;
}

extern "C" void qasr_ctx_free(qasr_ctx *c) { delete c; }

extern "C" int qasr_ctx_set_option(qasr_ctx *c, const char *name, int value) {
    if (!c || !name) return fail(QASR_ERR_ARG, "bad arguments");
    const std::string n = name;
    if (n == "probe_layer") {
        if (value < 0 || value >= c->m->hp.dec_layers) return fail(QASR_ERR_ARG, "probe_layer out of range");
        c->probe_layer = value;
        c->drop_graphs();
        c->graph_probe_group = -1;
        return 0;
    }
    if (n == "probe_stride") {
        if (value < 1) return fail(QASR_ERR_ARG, "probe_stride must be >= 1");
        c->probe_stride = value;
        return 0;
    }
    if (n == "dec_layers") {
        if (value < 0 || value > c->m->hp.dec_layers) return fail(QASR_ERR_ARG, "dec_layers out of range");
        c->dbg_layers = value;
        c->drop_graphs();
        return 0;
    }
    for (const auto &o : fuse_options())
        if (n == o.name) {
            if (n == "poll_limit" && value <= 0) return fail(QASR_ERR_ARG, "poll_limit must be positive");
            if (n == "top_k" && (value < 0 || value > QASR_TOPK_MAX)) return fail(QASR_ERR_ARG, "top_k out of range (0..8)");
            if (n == "beam_width" && (value < 0 || value > QASR_BEAM_MAX)) return fail(QASR_ERR_ARG, "beam_width out of range (0..8)");
            if (n == "sample_slices" && value < 0) return fail(QASR_ERR_ARG, "sample_slices must be >= 0");
            if (n == "beam_width" && value >= 2) {
                HIPCHK(hipSetDevice(c->m->device));
                if (const int rc = ensure_beam(c)) return rc;
            }
            if (n == "top_k" && value > 0) {
                HIPCHK(hipSetDevice(c->m->device));
                if (const int rc = ensure_topk(c)) return rc;
            }
            c->fuse.*(o.field) = value;
            c->drop_graphs();   // captured steps hold the old launch configuration
            if (o.field == &FuseCfg::token_logprobs) {   // nothing has run under the new setting
                c->lp_step_B = c->lp_run_B = c->lp_run_T = 0;
                c->lp_run.clear();
                c->lp_run_n.clear();
            }
            if (o.field == &FuseCfg::beam_width) {
                c->last_run_beam = false;
                c->beam_res.clear();
            }
            if (o.field == &FuseCfg::top_k) {
                c->tk_step_B = c->tk_run_B = c->tk_run_T = 0;
                c->tk_run_id.clear();
                c->tk_run_lp.clear();
                c->tk_run_n.clear();
            }
            HIPCHK(hipSetDevice(c->m->device));   // arrival counters back to rest
            const int rc = reset_counters(c);
            if (rc) return rc;
            HIPCHK(hipStreamSynchronize(c->st));
            return 0;
        }
    return fail(QASR_ERR_ARG, "unknown option '" + n + "'");
}

extern "C" int qasr_ctx_get_option(const qasr_ctx *c, const char *name, int *value) {
    if (!c || !name || !value) return fail(QASR_ERR_ARG, "bad arguments");
    const std::string n = name;
    if (n == "dec_layers") { *value = c->dbg_layers; return 0; }
    if (n == "probe_layer") { *value = c->probe_layer; return 0; }
    if (n == "probe_stride") { *value = c->probe_stride; return 0; }
    if (n == "slots_ffn") { *value = c->fuse.slots_ffn; return 0; }
    if (n == "fused_mode") { *value = c->last_fmode; return 0; }
    if (n == "fused_exact") { *value = c->last_fx; return 0; }
    if (n == "attn_path") { *value = c->last_attn; return 0; }
    if (n == "graph_captures") { *value = (int)c->n_captures; return 0; }
    if (n == "slots_qkv") { *value = std::min(c->fuse.slots_qkv64, c->fuse.slots_qkv128); return 0; }
    for (const auto &o : fuse_options())
        if (n == o.name) { *value = c->fuse.*(o.field); return 0; }
    return fail(QASR_ERR_ARG, "unknown option '" + n + "'");
}

extern "C" int qasr_debug_read(qasr_ctx *c, const char *buffer, void *dst, int64_t bytes) {
    if (!c || !buffer || !dst || bytes < 0) return fail(QASR_ERR_ARG, "bad arguments");
    const Hparams &hp = c->m->hp;
    const int64_t B = c->max_batch, QD = hp.n_head * 128, KD = hp.n_kv_head * 128;
    const std::string n = buffer;
    const void *src = nullptr;
    int64_t cap = 0;
    if (n == "x") { src = c->d_x; cap = B * hp.hidden * 4; }
    else if (n == "act") { src = c->d_act; cap = B * hp.dec_ffn * 2; }
    else if (n == "qkv") { src = c->d_qkv; cap = B * (QD + 2 * KD) * 4; }
    else if (n == "att") { src = c->d_att; cap = B * QD * 2; }
    else return fail(QASR_ERR_ARG, "unknown buffer '" + n + "'");
    if (bytes > cap) return fail(QASR_ERR_ARG, "read past the buffer");
    HIPCHK(hipSetDevice(c->m->device));
    if (n == "qkv" && c->qkv_in_gran) {   // the last layer's QKV went out as {value, tag} granules (batch 1)
        std::vector<unsigned long long> g(c->gran_bytes() / 8);   // one per QKV output: QD + 2 * KD
        HIPCHK(hipMemcpyAsync(g.data(), c->d_gran, c->gran_bytes(), hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        std::vector<uint32_t> v(B * (QD + 2 * KD), 0u);
        for (size_t i = 0; i < g.size(); i++) v[i] = (uint32_t)g[i];
        memcpy(dst, v.data(), bytes);
        return 0;
    }
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// ------------------------------------------------------------ size helpers
extern "C" int qasr_mel_frames(int n) { return mel_frames(n); }
extern "C" int qasr_encoder_frames(int T) { return encoder_frames(T); }
extern "C" int qasr_prompt_len(int n) { return n + 15; }
extern "C" int qasr_align_prompt_len(int n_samples, int n_text) {
    return n_text + 2 + feat_extract_output_lengths(mel_frames(n_samples));
}
extern "C" int qasr_build_prompt(const qasr_model *m, int n_audio, int32_t *ids, int *audio_pos) {
    Hparams hp = m ? m->hp : Hparams();
    std::vector<int32_t> p = build_prompt(hp, n_audio, {}, audio_pos);
    if (ids) memcpy(ids, p.data(), p.size() * 4);
    return (int)p.size();
}

// ---------------------------------------------------------------- profile
extern "C" int qasr_set_profile(qasr_ctx *c, int on) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    c->profile_on = on != 0;
    c->prof.clear();
    return 0;
}

// QWEN3_TIMER_REPORT's table (src/timing.h:32-48) over the sections recorded since qasr_set_profile
extern "C" int qasr_profile_report(qasr_ctx *c, char *out, int cap) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    std::string r = "\n================================================================================\n"
                    "                         TIMING PROFILE REPORT\n"
                    "================================================================================\n";
    char line[160];
    snprintf(line, sizeof line, "%-45s %12s %8s %12s\n", "Section", "Total (ms)", "Calls", "Avg (ms)");
    r += line;
    r += "--------------------------------------------------------------------------------\n";
    for (const auto &kv : c->prof) {
        snprintf(line, sizeof line, "%-45s %12.2f %8ld %12.2f\n", kv.first.c_str(), kv.second.first, kv.second.second,
                 kv.second.second ? kv.second.first / kv.second.second : 0.0);
        r += line;
    }
    r += "================================================================================\n";
    if (out && cap > 0) {
        const size_t n = std::min(r.size(), (size_t)cap - 1);
        memcpy(out, r.data(), n);
        out[n] = 0;
    }
    return (int)r.size();
}
