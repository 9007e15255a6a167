// engine_impl.h -- internal to the engine*.hip units (the C-ABI implementation,
// include/qasr_capi.h): the model and context structs and the helpers the units
// share.  The host side by unit:
//   engine.hip         errors, context create / free / options, buffers, counters, profile report
//   engine_model.hip   GGUF load into the device arena, tokenizer, WAV / synthetic-GGUF utilities
//   engine_stages.hip  mel, encoder, prefill (run_* and their qasr_* entry points), Q8_0 GEMM helpers
//   engine_decode.hip  the decode-step emitter, graph capture, kernel probes, qasr_decode_step
//   engine_run.hip     qasr_run, the continuous-batching stream, their log-probability readers
//   engine_beam.hip    beam search: the KV-cache fork entry, the beam loop, the hypothesis reader
//   engine_sample.hip  temperature sampling: qasr_set_sampling, the sampler step, the n_best run, the sample reader
//   engine_constrain.hip  decoding constraints: qasr_set_constraints, the constraint stage of a prefill or decode step
//   engine_score.hip   teacher-forced scoring: the score head over prefill rows, qasr_prefill_score, qasr_score
//   engine_align.hip   the forced aligner and its JSON output
//   engine_resample.hip  audio at other rates: the host-only resampler entries, the tap-table cache, the resample stage
//   engine_segment.hip  long recordings: the host-only segmentation entries, the segment stage, qasr_stage_long
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/qasr_capi.h"
#include "../host/gguf.h"
#include "../host/qasr_host.h"
#include "beam_host.h"
#include "score_host.h"
#include "resample_host.h"
#include "segment_host.h"
#include "dev_common.h"
#include "kernels.h"

// (hidden visibility: the shared helpers stay out of libqasr.so's dynamic symbols, as when they were static)
namespace qasr {
namespace eng __attribute__((visibility("hidden"))) {
// the calling thread's last error (qasr_last_error): one definition, engine.hip
int fail(int code, const std::string &msg);
}  // namespace eng
}  // namespace qasr

#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) return ::qasr::eng::fail(QASR_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------ model
// Linear weights are fp16 [N][K] (F16 files) or int8 [N][K] quants with fp16
// block scales *_d [N][K/32] (Q8_0 files: block_q8_0 split in two arrays).
struct EncLayer {
    uint16_t *wqkv, *wo, *w1, *w2;
    uint16_t *wqkv_d = nullptr, *wo_d = nullptr, *w1_d = nullptr, *w2_d = nullptr;
    float *bqkv, *bo, *b1, *b2, *ln1_w, *ln1_b, *ln2_w, *ln2_b;
};
struct DecLayer {
    float *attn_norm, *q_norm, *k_norm, *ffn_norm;
    uint16_t *wqkv, *wo, *wgu, *wd;
    uint16_t *wqkv_d = nullptr, *wo_d = nullptr, *wgu_d = nullptr, *wd_d = nullptr;
};

struct qasr_model {
    qasr::Hparams hp;
    int device = 0;
    qasr::Tokenizer tok;
    char *arena = nullptr;
    size_t arena_bytes = 0;
    uint16_t *conv1_w, *conv2_w, *conv3_w, *conv_out_w, *proj1_w, *proj2_w, *embd;
    uint16_t *conv_out_d = nullptr, *proj1_d = nullptr, *proj2_d = nullptr;
    bool q8 = false;   // linear weights are Q8_0 (scripts/convert_hf_to_gguf.py:230-308)
    uint16_t *cls_w = nullptr;   // aligner: classify head [cls_rows][hidden] fp16, rows >= classify_num zero
    int cls_rows = 0;
    std::unordered_map<std::string, int> ko_dict;   // aligner: Korean word list (src/forced_aligner.cpp:1543-1562)
    float *conv1_b, *conv2_b, *conv3_b, *ln_post_w, *ln_post_b, *proj1_b, *proj2_b, *out_norm;
    std::vector<EncLayer> enc;
    std::vector<DecLayer> dec;
    uint16_t *gelu;
    float *pe, *filters;
    double2 *tw;
    double *hann;
    ~qasr_model() {
        if (arena && device >= 0) {
            (void)hipSetDevice(device);
            (void)hipFree(arena);
        }
    }
};

// --------------------------------------------------------------- context
// qasr_ctx::ev: the stage boundaries of a run on the context stream
enum CtxEvent {
    EV_START,       // before the mel
    EV_MEL,         // mel | encoder
    EV_ENC,         // encoder | prefill
    EV_PREFILL,     // prefill | decode (aligner: after the classify head)
    EV_END,         // after the last decode step
    EV_ENC_CONV,    // inside run_encoder, profile only: conv front-end | transformer
    EV_COUNT
};

struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    template <class T> T *as() const { return (T *)p; }
};

// the resampler's plan of a rate and its table on the device (kernels.h ResampleClip's layout; null for the copy)
struct ResampleTab {
    qasr::ResamplePlan pl;
    float *d_taps = nullptr;
};

struct qasr_ctx {
    qasr_model *m = nullptr;
    int max_batch = 0, max_ctx = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[EV_COUNT] = {};
    uint16_t *kc = nullptr, *vc = nullptr;
    uint16_t *vt = nullptr;        // V^T cache (kernels.h vt_ctx): the exact decode attention's V
    float *rope = nullptr;
    std::vector<DevBuf> owned;     // everything hipMalloc'ed by the context
    // grow-on-demand scratch
    DevBuf pcm, spcm, mel, meltmp, melmax, melclips, melblocks;   // (spcm: qasr_run_stream's host clips)
    DevBuf chunks, rs1, rs2, rs3, pepos, act1, act2, act3;
    DevBuf pebig;                  // encode_no_chunk: sinusoidal PE over a whole clip's frames
    int pebig_rows = 0;
    DevBuf ex, exh, eqkv, eatt, eff, feats, segs;
    DevBuf px, pxh, pqkv, pq, patt, pact, prow, plast, pids;
    DevBuf pq32, pk32;             // ForcedAligner prefill: fp32 Q / K rows
    DevBuf ats, atx, aam;          // aligner: timestamp-row indices, their normed rows, argmax keys
    DevBuf exp_, gidx;             // aligner batches: conv_out over every padded chunk row, the valid rows' indices
    DevBuf q8a, q8d, x32;          // Q8_0 models: quantised activations (int8 + scales), fp32 layer inputs
    float *d_att32 = nullptr, *d_act32 = nullptr;   // Q8_0 decode: fp32 attention output / SwiGLU output
    int8_t *d_q8a = nullptr; float *d_q8d = nullptr, *d_x32 = nullptr;   // Q8_0 batched (B > 8) decode, graph-fixed
    int8_t *d_q8n = nullptr; float *d_q8nd = nullptr;   // ... the RMS-normed layer inputs (QKV, gate/up), quantised
    // fixed decode state (sized by max_batch)
    int32_t *d_tok = nullptr, *d_hist = nullptr;
    int *d_pos = nullptr, *d_nkv = nullptr, *d_slot = nullptr, *d_step = nullptr;
    float *d_x = nullptr, *d_qkv = nullptr, *d_part = nullptr, *d_logits = nullptr;
    float *d_scores = nullptr;     // exact decode attention: [B][n_head][max_ctx] scaled scores
    unsigned int *d_counter = nullptr, *d_done = nullptr;
    unsigned int *d_qcnt = nullptr;   // fused batch-1 QKV + attention: QKV-block arrivals per kv group
    unsigned long long *d_gran = nullptr;   // ... or its outputs as tagged granules (zeroed by every prefill)
    unsigned long long *d_sgran = nullptr;  // ... exact attention: the splits' scores as granules [n_head][max_ctx] (zeroed likewise)
    bool qkv_in_gran = false;               // the captured step's last layer hands its QKV over in granules
    unsigned int *d_attdone = nullptr;   // fused batch-1 o-proj: combiner arrivals, [layer][8 replicas][16]
    unsigned int *d_ffncnt = nullptr;    // fused batch-1 FFN: [layer][gate/up arrivals, o-proj arrivals][32 shards][16]
    uint16_t *d_att = nullptr, *d_act = nullptr, *d_xh = nullptr;
    unsigned long long *d_amax = nullptr;
    int max_splits = 0, hist_cap = 0;
    // byte sizes of the fixed buffers the host zeroes again after allocating them: the allocation
    // and every memset take them from here
    size_t gran_bytes() const { return (size_t)(m->hp.n_head + 2 * m->hp.n_kv_head) * 128 * 8; }
    size_t sgran_bytes() const { return (size_t)m->hp.n_head * qasr::sgran_ld(max_ctx) * 8; }
    size_t ffncnt_bytes() const { return (size_t)m->hp.dec_layers * 1024 * 4; }
    size_t qcnt_bytes() const { return (size_t)m->hp.n_kv_head * 8 * 16 * 4; }
    size_t attdone_bytes() const { return (size_t)m->hp.dec_layers * 128 * 4; }
    size_t counter_bytes() const { return (size_t)max_batch * m->hp.n_kv_head * 4; }
    size_t amax_bytes() const { return (size_t)max_batch * 8; }
    static constexpr size_t kDoneBytes = 4;
    // option token_logprobs: the last step's log-probabilities [B], their history parallel to d_hist
    // (stride hist_cap, the index of the token they belong to), the one-launch LM head's per-workgroup
    // (m, s) partials [lmhead_grid()][128]
    float *d_lp = nullptr, *d_lphist = nullptr;
    unsigned long long *d_lppart = nullptr;
    int lp_step_B = 0;             // rows of the last qasr_prefill* / qasr_decode_step with the option on (0: none)
    std::vector<float> lp_run;     // the last qasr_run's values [lp_run_B][lp_run_T], aligned with its tokens
    std::vector<int> lp_run_n;     // ... and how many per row
    int lp_run_B = 0, lp_run_T = 0;
    const std::vector<float> *lp_sink = nullptr;   // inside a qasr_sink_fn call: the delivered clip's values
    // option top_k (K = fuse.top_k): the last step's K alternatives per row [max_batch][K] as ids and
    // log-probabilities, and their histories parallel to d_hist ([max_batch][hist_cap][K]); allocated for
    // K = QASR_TOPK_MAX the first time the option is non-zero (ensure_topk), null until then
    int32_t *d_tkid = nullptr, *d_tkhid = nullptr;
    float *d_tklp = nullptr, *d_tkhlp = nullptr;
    unsigned long long *d_tkpart = nullptr;   // the one-launch LM head's per-workgroup keys [lmhead_grid()][128][QASR_TOPK_MAX]
    int tk_step_B = 0;                 // rows of the last qasr_prefill* / qasr_decode_step with the option on (0: none)
    std::vector<int32_t> tk_run_id;    // the last qasr_run's alternatives [tk_run_B][tk_run_T][K], aligned with its tokens
    std::vector<float> tk_run_lp;
    std::vector<int> tk_run_n;         // ... and how many tokens per row
    int tk_run_B = 0, tk_run_T = 0;
    const std::vector<int32_t> *tk_sink_id = nullptr;   // inside a qasr_sink_fn call: the delivered clip's alternatives
    const std::vector<float> *tk_sink_lp = nullptr;
    // option beam_width (W = fuse.beam_width >= 2): beam search in qasr_run (engine_beam.hip).  Clip g owns rows
    // g * W .. g * W + W - 1.  The device state is allocated the first time the option is >= 2 (ensure_beam):
    // per row the summed log-probability, the fork arguments and the group's finished table at g * W; per group
    // n_fin / done / t / P; the back-pointer history [hist_cap][max_batch] of (parent row, token, logprob)
    struct BeamDev {
        float *cum = nullptr, *fin_sum = nullptr, *fin_lp = nullptr, *h_lp = nullptr;
        int *fin_row = nullptr, *fin_t = nullptr, *n_fin = nullptr, *done = nullptr, *t = nullptr, *P = nullptr;
        int32_t *eos = nullptr;        // [1] the run's EOS id, -1 with ignore_eos (read by the captured beam step)
        int *parent = nullptr, *from = nullptr, *to = nullptr, *h_par = nullptr;
        int32_t *h_id = nullptr;
    } bm;
    int beam_W = 0;                    // inside a beam run: its width (the decode step then ends with the beam step and
                                       // the fork, and its top-K runs with K = W); else 0
    bool last_run_beam = false;        // the last qasr_run was a beam run (qasr_get_logprobs / qasr_get_topk refuse)
    std::vector<std::vector<qasr::BeamHyp>> beam_res;   // its hypotheses per clip, best first
    // temperature sampling (engine_sample.hip): off while samp.temperature <= 0.  The device state is
    // allocated the first time it is turned on (ensure_sample): the scalars a captured step reads, per row the draw's
    // identity (clip, sample, t) and the key the slices fold into (zero at rest)
    qasr_sampling samp = {0.f, 0.f, 0, 1};
    struct SampleDev {
        qasr::SampleScalars *sc = nullptr;
        int *clip = nullptr, *sample = nullptr, *t = nullptr;
        unsigned long long *skey = nullptr;
    } sd;
    int samp_run_N = 0;                // inside a sampling qasr_run: its n_best (the prefill then draws n_best rows a clip); else 0
    std::vector<int> run_clip_ids;     // qasr_run_staged: the pool indices of the subset (the draws' clip identities)
    bool last_run_sampled = false;     // the last qasr_run drew its tokens (qasr_get_samples reads samp_res)
    int last_run_nbest = 0;            // ... with this n_best
    struct SampleHyp { std::vector<int32_t> tokens; std::vector<float> logprobs; float sum = 0.f; };
    std::vector<std::vector<SampleHyp>> samp_res;   // its hypotheses per clip, in sample order
    // decoding constraints (engine_constrain.hip): off until qasr_set_constraints turns them on.  The
    // device state is allocated the first time (ensure_constrain): the parameters and the bias list a captured step
    // reads, per logits row the key the scan folds into and its flag (both zero at rest) and the constrained token
    struct ConstrainState {
        bool on = false;
        int ngram = 0;
        float p = 1.f;
        int last_n = 0;
        std::vector<int32_t> ids;
        std::vector<float> bias;
    } con;
    struct ConstrainDev {
        qasr::ConstrainParams *prm = nullptr;
        int32_t *ids = nullptr;
        float *bias = nullptr;
        unsigned long long *skey = nullptr;
        int *flag = nullptr;
        int32_t *gtok = nullptr;
        // hotword boosting: the trie's header lives with the state above (0 nodes until a list is
        // set), so a step captured before the first qasr_set_phrases serves the lists that follow; the arrays it
        // points to have a fixed capacity and are allocated by the first qasr_set_phrases
        qasr::PhraseTrie *ph = nullptr;
        int32_t *ph_off = nullptr, *ph_tok = nullptr, *ph_dst = nullptr;
        float *ph_bonus = nullptr;
    } cd;
    struct PhraseState {
        bool on = false;
        std::vector<int32_t> ids, len;
        std::vector<float> boost;
    } phr;
    int stage_t = 0;                   // constraints on: the history length of the rows of qasr_prefill* / qasr_decode_step
    long n_captures = 0;               // step graphs captured so far (option "graph_captures", read-only)
    DevBuf fork_args;                  // qasr_kv_fork: the caller's parent | from | to on the device
    // teacher-forced scoring (engine_score.hip): the gathered normed rows (fp16), row indices | targets, the three
    // outputs of a block of rows, the score head's scratch
    DevBuf sc_rows, sc_tab, sc_out, sc_scratch;
    // resampler to 16 kHz (engine_resample.hip): the raw clips of a call, its clip and block lists,
    // and the tap tables by rate, each built the first time a clip at that rate arrives
    DevBuf rsin, rsclips, rsblocks;
    std::map<int, ResampleTab> rs_tabs;
    bool rs_timed = false;
    hipEvent_t rs_ev[2] = {};          // around qasr_resample's launch (qasr_resample_last_us), created by its first call
    // pause segmentation of long recordings (engine_segment.hip): the recording and block lists of a
    // call, e / s, the cut kernel's outputs (peak | peak_rec | cuts | n_seg in one buffer, one copy back), and the
    // table of the last qasr_stage_long (seg_valid: the pool is that table's; any qasr_stage_audio* clears it)
    DevBuf sgrecs, sgblocks, sg_e, sg_s, sg_out;
    bool sg_timed = false;
    hipEvent_t sg_ev[3] = {};          // before, between and after qasr_segment's two launches, created by its first call
    bool seg_valid = false;
    std::vector<int> seg_first;        // per recording: its first pool entry; one more entry: the pool size
    std::vector<long> seg_rec_off;     // per recording: its first sample in c->pcm
    std::vector<double> seg_peak;      // per pool entry
    std::vector<int> seg_silent;
    // pinned host staging for small per-call tables (reset at each top-level call)
    char *pin = nullptr;
    size_t pin_cap = 0, pin_used = 0;
    std::vector<int32_t> sys_ids;
    // staged audio
    std::vector<int> staged_n;
    std::vector<long> staged_off;
    bool eager = false;            // QASR_NO_GRAPH=1: launch the decode step eagerly (profilers)
    int dev_skip = 0;              // QASR_DEV_SKIP bitmask (-DQASR_DIAG_SKIP builds only): omits decode kernels
    qasr::FuseCfg fuse;                 // batch-1 fused launches: switches, delays, co-residency of this device
    unsigned int *d_err = nullptr; // sticky device error word of the fused launches (DevErr bits)
    int dbg_layers = 0;            // diagnostic: decode steps run only the first n decoder layers (0 = all)
    // --profile (src/timing.h QWEN3_TIMER sections): per-section device time from
    // HIP events, accumulated over calls until qasr_set_profile resets it
    bool profile_on = false;
    std::map<std::string, std::pair<double, long>> prof;   // section -> (total ms, calls)
    std::vector<hipEvent_t> step_ev;                       // per decode step, profile only
    // per-token callback (src/qwen3_asr.cpp:264-291): called synchronously
    // after every greedy step of qasr_run, in order, for every live sequence
    void (*tok_cb)(void *user, int seq, int n_generated, int32_t token) = nullptr;
    void *tok_cb_user = nullptr;
    // QASR_DEV_TRACE=<file>: per-block timestamps of one decode layer's kernels
    // (layer QASR_DEV_TRACE_LAYER, default 10) of the last step, dumped by qasr_run
    std::string trace_path;
    int trace_layer = 10;
    unsigned long long *d_trace = nullptr;   // [6 kernels][4096 blocks][8]
    static constexpr size_t kTraceBytes = (size_t)6 * 4096 * 8 * 8;
    // kernel probe: HIP-event timing of one decode-step kernel inside qasr_run
    int probe = 0;                 // 0 off, 1 LM head, 2 layer QKV + attention, 3 layer FFN
    int probe_layer = 14;          // decoder layer whose groups probes 2 / 3 time
    int probe_stride = 1;          // probe decode steps k with k % probe_stride == 0 (the others replay the whole-step
                                   // graph: the probed step's split graphs and eager group cost ~3 % of a step)
    bool probe_o_fused = false;    // the probed layer's o-projection runs inside the QKV launch
    int last_fmode = 0, last_fx = 0;   // the last emitted decode step, layer 0: fused launch mode (0 separate, 1 QKV +
                                       // attention, 2 + o-proj) and whether its attention was the chain role (options
                                       // "fused_mode" / "fused_exact", read-only)
    int last_attn = 0;             // the same step's decode attention launches (option "attn_path", read-only): 0 split-K
                                   // fp32, 1 chain role of the fused launch, 2 scores + chain in one launch per sequence
                                   // (decode_attn_seq_kernel), 3 separate scores and chain kernels
    double probe_ms = 0.0, probe_bytes = 0.0, probe_dev_ms = 0.0;
    long probe_dev_n = 0;
    unsigned long long *d_pstamp = nullptr;   // per decode step: [32 min-starts | 32 max-ends] of the probed launches
    unsigned long long *cur_stamp = nullptr;  // record of the group being emitted (probe only)
    long probe_n = 0;
    std::vector<int> run_P;        // prompt lengths of the current qasr_run (decode step k: n_kv = P_b + k + 1)
    std::vector<hipEvent_t> pev;
    // decode graphs, one set per attention split-grid bucket (the grid must
    // cover the longest sequence's context: it grows by 64 keys per split)
    struct StepGraphs { hipGraphExec_t full = nullptr, pre = nullptr, post = nullptr; };
    std::map<std::tuple<int, int, int>, StepGraphs> graphs;   // key: (step_mode: beam_W, sampling and n_best; batch; split bucket)
    int graph_B = -1;
    bool graph_logits = false;
    int graph_base = 0;            // max prompt length of the current run: step k feeds position base + k
    int graph_probe_group = -1;    // launch group timed between events (pre/post graphs split around it)
    void drop_graphs() {
        for (auto &kv : graphs) {
            if (kv.second.full) (void)hipGraphExecDestroy(kv.second.full);
            if (kv.second.pre) (void)hipGraphExecDestroy(kv.second.pre);
            if (kv.second.post) (void)hipGraphExecDestroy(kv.second.post);
        }
        graphs.clear();
    }
    ~qasr_ctx() {
        (void)hipSetDevice(m->device);
        drop_graphs();
        for (auto &e : pev) (void)hipEventDestroy(e);
        for (auto &e : step_ev) (void)hipEventDestroy(e);
        for (auto &b : owned) (void)hipFree(b.p);
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : rs_ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : sg_ev) if (e) (void)hipEventDestroy(e);
        if (pin) (void)hipHostFree(pin);
        if (st) (void)hipStreamDestroy(st);
    }
};

// ------------------------------------------------ helpers the units share
namespace qasr {
namespace eng __attribute__((visibility("hidden"))) {
constexpr int kStampRec = 2 * STAMP_ENDS;   // u64 per probed launch record (dev_common.h stamp_start/end)

// engine.hip
int declined_check(const char *stage);
int reset_counters(qasr_ctx *c);
int reset_granules(qasr_ctx *c);
int check_dev_err(qasr_ctx *c);
std::mutex &device_lock(int device);
int ensure(qasr_ctx *c, DevBuf &b, size_t bytes);
int stage_pinned(qasr_ctx *c, const void *src, size_t bytes, void *dst);
// option top_k after the greedy bookkeeping of a prefill or decode step (d_step names the slot of the
// token just written to d_hist): the step's alternatives from the fp32 logits in d_logits
int topk_step(qasr_ctx *c, int B);
// K of the step's top-K: the beam width inside a beam run, else option top_k
inline int step_k(const qasr_ctx *c) { return c->beam_W >= 2 ? c->beam_W : c->fuse.top_k; }
int ensure_topk(qasr_ctx *c);
int ensure_beam(qasr_ctx *c);
// sampling: on for this context's decoding (aligner models ignore it); the rows a prefill draws per sequence; the
// graph key's first entry (a beam run's width, or 16 x the rows per clip of a sampling step)
inline bool sampling_on(const qasr_ctx *c) { return c->samp.temperature > 0.f && !c->m->hp.aligner; }
inline int sample_mul(const qasr_ctx *c) { return std::max(1, c->samp_run_N); }
// decoding constraints or phrases: the constraint stage is on for this context's decoding (aligner models ignore them)
inline bool constraints_on(const qasr_ctx *c) { return (c->con.on || c->phr.on) && !c->m->hp.aligner; }
// (constraints on: 1024 on top, a key of its own beside every other mode's)
inline int step_mode(const qasr_ctx *c) {
    return (c->beam_W >= 2 ? c->beam_W : sampling_on(c) ? 16 * sample_mul(c) : 0) + (constraints_on(c) ? 1024 : 0);
}
int dev_alloc(qasr_ctx *c, void **p, size_t bytes);

// V^T cache elements of one layer
inline size_t layer_vt(const qasr_ctx *c) {
    return (size_t)c->max_batch * c->m->hp.n_kv_head * 128 * vt_ctx(c->max_ctx);
}
inline bool takes_fused(const qasr_ctx *c, int B) {
    return B == 1 && !c->m->q8 && (c->fuse.ffn || c->fuse.qkv);
}
// Small per-call tables go through a pinned staging area so the async copy
// never reads a host vector that has gone out of scope.
template <class T>
int upload(qasr_ctx *c, DevBuf &b, const std::vector<T> &v) {
    const size_t bytes = v.size() * sizeof(T);
    const int rc = ensure(c, b, bytes);
    if (rc || !bytes) return rc;
    return stage_pinned(c, v.data(), bytes, b.p);
}

// engine_stages.hip
void launch_gemm_c(qasr_ctx *c, int amode, int epi, GemmArgs g, hipStream_t s);
void gemm_q8(qasr_ctx *c, int epi, GemmArgs g, const float *a32, const uint16_t *a16, int lda, int gather_C, const uint16_t *W,
             const uint16_t *Wd, hipStream_t s, int8_t *qa = nullptr, float *qd = nullptr, bool decode = false);
void gemm_q8_pre(qasr_ctx *c, int epi, GemmArgs g, const uint16_t *W, const uint16_t *Wd, hipStream_t s,
                 const int8_t *qa = nullptr, const float *qd = nullptr);
bool gemm_q8_pre_swiglu_q8(qasr_ctx *c, GemmArgs g, const uint16_t *W, const uint16_t *Wd, hipStream_t s, const int8_t *qa,
                           const float *qd, int8_t *q, float *d);
int pack_pcm(qasr_ctx *c, const float *const *pcm, const int *n, int B, std::vector<long> &off);
int run_mel(qasr_ctx *c, const std::vector<long> &off, const std::vector<int> &n, std::vector<long> &mel_off, std::vector<int> &T,
            const float *d_pcm = nullptr);
int run_encoder(qasr_ctx *c, const float *d_mel, const std::vector<long> &mel_off, const std::vector<int> &T, bool conv_only,
                std::vector<int> &Nb, bool no_chunk = false);
int prefill_layers(qasr_ctx *c, const std::vector<int32_t> &ids, const std::vector<int> &P, const float *d_feats,
                   const std::vector<int> &audio_pos, const std::vector<int> &N, const std::vector<int> *slots,
                   const std::vector<int> *pos0 = nullptr);
int run_prefill(qasr_ctx *c, const std::vector<int32_t> &ids, const std::vector<int> &P, const float *d_feats,
                const std::vector<int> &audio_pos, const std::vector<int> &N, bool want_logits,
                const std::vector<int> *slots = nullptr, const std::vector<int> *pos0 = nullptr);
// the body of qasr_prefill / _chunk / _chunk_audio / _slots (n_past, feats, slots: null as there)
int prefill_chunk_common(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, const float *feats, const int *audio_pos,
                         const int *N, int B, float *logits_last, int32_t *argmax, const int *slots = nullptr);

// a roctx range for the lifetime of the object (rocprofv3 --marker-trace); engine_run.hip
struct RoctxRange {
    explicit RoctxRange(const char *name);
    ~RoctxRange();
    RoctxRange(const RoctxRange &) = delete;
    RoctxRange &operator=(const RoctxRange &) = delete;
};

// engine_run.hip
struct FrontEnd {
    std::vector<int> P, audio_pos, Nb;   // per clip: prompt length, first audio row, encoder frames
};
int front_end_staged(qasr_ctx *c, int max_tokens, const std::vector<int> *slots, FrontEnd &fe);
int run_timings(qasr_ctx *c, int steps, qasr_timings *t);

// engine_beam.hip
KvForkArgs fork_args(qasr_ctx *c, const int *parent, const int *from, const int *to, int B, int group, int blocks);
int beam_run(qasr_ctx *c, int max_tokens, int ignore_eos, int32_t *tokens, int *n_tokens, qasr_timings *t);
// the beam step and the fork that end a decode step of a beam run (blocks: 8-key blocks the fork's grid covers)
int beam_step(qasr_ctx *c, int G, int blocks);

// engine_sample.hip
// the draw that ends a sampling prefill or decode step: B rows, row r from logits row r / src_div; then the drawn
// tokens' log-probabilities at T = 1 into d_lp / d_lphist
int sample_step(qasr_ctx *c, int B, int src_div);
int sample_set_streams(qasr_ctx *c, const std::vector<int> &clip, const std::vector<int> &sample, const std::vector<int> &t);
int sample_run(qasr_ctx *c, int max_tokens, int ignore_eos, int32_t *tokens, int *n_tokens, qasr_timings *t);
// the hypotheses of a sampling run from its token history (rows g * N + i) and d_lphist -> c->samp_res
int sample_collect(qasr_ctx *c, int G, int N, const std::vector<int32_t> &hist, int steps, int max_tokens, int ignore_eos);

// engine_constrain.hip
// the constraint stage after the bookkeeping of a prefill or decode step: B token rows, row r from logits row
// r / src_div; d_logits becomes the edited rows, d_tok and the history slot the constrained tokens
int constrain_step(qasr_ctx *c, int B, int src_div);

// engine_run.hip
int greedy_loop(qasr_ctx *c, int B, int max_tokens, int ignore_eos, std::vector<int32_t> &hist, int &steps);
int run_results(qasr_ctx *c, int B, int max_tokens, int ignore_eos, const std::vector<int32_t> &hist, int steps, int32_t *tokens,
                int *n_tokens, qasr_timings *t);

// engine_resample.hip
struct ResampleLayout {
    std::vector<long> in_off, out_off;   // per clip: first raw sample, first resampled sample
    std::vector<int> n_in, n_out, rate;
    long in_tot = 0, out_tot = 0;
};
int resample_table(qasr_ctx *c, int rate, ResampleTab &out);
int resample_layout(const int *n, const int *rate, int B, ResampleLayout &o);
int run_resample(qasr_ctx *c, const ResampleLayout &o, const float *d_in, float *d_out, bool timed = false);

// engine_segment.hip
// the segment tables of B recordings already on the device (d_pcm + off[b], n[b] samples at 16 kHz), on the context
// stream; synchronises.  want_e: e is kept in c->sg_e beside s in c->sg_s (frame_off: each recording's first row)
struct SegmentRun {
    std::vector<qasr::SegmentTable> tab;
    std::vector<long> frame_off;
    long frames = 0;
};
int run_segment(qasr_ctx *c, const float *d_pcm, const std::vector<long> &off, const std::vector<int> &n,
                const qasr::SegmentParams &p, bool want_e, bool timed, SegmentRun &out);

// engine_decode.hip
int split_bucket(qasr_ctx *c, int pos);
int decode_graph(qasr_ctx *c, int B, bool want_logits, int base);
int launch_whole_step(qasr_ctx *c, int B, int splits);
int launch_step(qasr_ctx *c, int B, int k);
int probe_arm(qasr_ctx *c, int nsteps);
int probe_collect(qasr_ctx *c, int B, int nsteps);
}  // namespace eng
}  // namespace qasr
