// engine_decode.hip -- one greedy decode step: the kernel emitter, its capture
// into HIP graphs per (batch, split bucket), the kernel probes, and
// qasr_decode_step.
#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

// ------------------------------------------------------- the step emitter
// decode attention with ggml's fp16 V accumulation (fa_exact.hip)?
static bool exact_decode(const qasr_ctx *c) {
    return c->fuse.fa_exact_decode != 0;
}

// decode-batch projections: the weight-streaming skinny GEMM where it takes
// the shape, the tiled GEMM otherwise (f16 weights; only this path sets g.wdef,
// the Q8_0 helpers of engine_stages.hip leave it 0)
static void dec_gemm(qasr_ctx *c, int epi, GemmArgs g, hipStream_t s) {
    g.no_skinny = !c->fuse.skinny;
    g.skinny_inflight = c->fuse.skinny_inf;
    g.wdef = c->fuse.skinny_wdef;
    if (launch_gemm_skinny(epi, g, s)) return;
    launch_gemm(AM_DENSE, epi, g, s);
}

// Launch groups of one decode step, in stream order (decoder cut at nl layers):
//   0          embedding gather (batches; batch <= 8 fuses it into layer 0)
//   1 + 2l     layer l: QKV projection + attention (+ o-projection when fused)
//   2 + 2l     layer l: o-projection (when separate) + FFN
//   1 + 2nl    final norm + LM head + argmax (+ bookkeeping at batch <= 8)
//   2 + 2nl    bookkeeping (batches)
// A step is emitted as the groups in [lo, hi): whole (graph replay), or split
// around one probed group that runs between HIP events.
struct StepRange {
    int lo, hi;
    bool in(int g) const { return g >= lo && g < hi; }
};
static constexpr StepRange kWholeStep{0, 1 << 30};
// option lmh_topk = 1: the fused top-K variant of the one-launch LM head up to this K (profiles/topk/topk_cost.txt: at 64
// rows it beats the row kernel's path at K = 1 and 2 and loses from K = 4 on, its LDS insertion chain growing with K)
static constexpr int kLmhTopkAutoMax = 2;
static int step_layers(const qasr_ctx *c) { return c->dbg_layers > 0 ? c->dbg_layers : c->m->hp.dec_layers; }

// one decode step for B sequences: token d_tok at position d_pos;
// splits: attention grid (64-key splits) covering the longest context of the step
// returns 0, or an error (a launch that declined its shape: nothing runs silently short)
static int decode_step_kernels(qasr_ctx *c, int B, bool want_logits, StepRange r, int splits) {
    qasr_model *m = c->m;
    const Hparams &hp = m->hp;
    const int H = hp.hidden, QD = hp.n_head * 128, KD = hp.n_kv_head * 128, F = hp.dec_ffn;
    hipStream_t s = c->st;
    float *x = c->d_x;
    const bool skinny = B <= 8;
    // decode batches: the LM head as one launch (lmhead.hip's shape conditions)
    const bool lmh_one = !skinny && B <= 128 && c->fuse.lmh && H == 1024 && hp.vocab % 16 == 0;
    // option token_logprobs: inside the one-launch LM head, else from the fp32 logits after the bookkeeping
    const bool lp = c->fuse.token_logprobs != 0;
    if (lp && !lmh_one) want_logits = true;
    // option top_k: inside the one-launch LM head at 9 .. 64 rows where that measured faster (lmhead.hip TK; FuseCfg::lmh_topk);
    // every other path writes its logits, then the row kernel after the bookkeeping (the one-launch heads write them too)
    // (a beam run: K = its width, whatever option top_k says)
    const int K = step_k(c);
    const bool tk = K > 0;
    // decoding constraints: the stage edits the fp32 logits after the bookkeeping and chooses again; the log-probability
    // and the alternatives are the edited row's, so neither comes from the one-launch heads' fused groups (the raw row's)
    const bool con = constraints_on(c);
    const bool tk_fused = tk && !con && lmh_one && B <= 64 && (c->fuse.lmh_topk >= 2 || (c->fuse.lmh_topk == 1 && K <= kLmhTopkAutoMax));
    if (tk && !tk_fused) want_logits = true;
    if (con) want_logits = true;
    // sampling: the draw reads the fp32 logits after the bookkeeping, and the drawn token's log-probability comes from
    // them too (the fused LSE's value would be the argmax's)
    const bool smp = sampling_on(c);
    if (smp) want_logits = true;
    int rc;
    const size_t layer_kv = (size_t)c->max_batch * hp.n_kv_head * c->max_ctx * 128;
    const int nl = step_layers(c);   // diagnostic layer cap
    // probed group (emitted alone): every launch in it folds its block times into one record
    unsigned long long *stamp = r.hi - r.lo == 1 ? c->cur_stamp : nullptr;
    if (r.in(0) && !skinny) launch_embed(c->d_tok, B, m->embd, H, nullptr, nullptr, x, s);
    const int skip = c->dev_skip;   // 0 unless built with -DQASR_DIAG_SKIP (QASR_DEV_SKIP): drop kernels to price them
    if (c->d_trace && r.in(0)) (void)hipMemsetAsync(c->d_trace, 0, qasr_ctx::kTraceBytes, s);
    for (int l = 0; l < nl; l++) {
        const bool ga = r.in(1 + 2 * l), gb = r.in(2 + 2 * l);
        if (!ga && !gb) continue;
        const DecLayer &L = m->dec[l];
        auto tr = [&](int k) -> unsigned long long * {
            return c->d_trace && l == c->trace_layer ? c->d_trace + (size_t)k * 4096 * 8 : nullptr;
        };
        const bool q8 = m->q8;
        DecodeAttnArgs da{};
        da.qkv = c->d_qkv; da.q_norm = L.q_norm; da.k_norm = L.k_norm; da.eps = hp.rms_eps; da.rope = c->rope;
        da.pos = c->d_pos; da.kc = c->kc + l * layer_kv; da.vc = c->vc + l * layer_kv; da.seq_slot = c->d_slot; da.B = B;
        da.vt = c->vt + l * layer_vt(c);
        da.n_head = hp.n_head; da.n_kv_head = hp.n_kv_head; da.max_ctx = c->max_ctx; da.max_splits = c->max_splits; da.grid_splits = splits;
        da.scale = 1.0f / sqrtf(128.0f); da.part = c->d_part; da.counter = c->d_counter; da.out = c->d_att;
        da.out32 = q8 && skinny ? c->d_att32 : nullptr;
        if (q8 && !skinny) { da.outq = c->d_q8a; da.outd = c->d_q8d; }
        da.trace = tr(1);
        da.qcnt = c->d_qcnt;
        da.spl1 = c->fuse.spl1;
        da.stream_blocks = !skinny && c->fuse.att_stream ? c->fuse.slots_stream : 0;
        da.spl_batch = c->fuse.att_spl;
        da.kv_nt = c->fuse.kv_nt;
        da.stamp = stamp;
        GemvArgs o{};
        if (skinny) {
            if (q8) { o.x = c->d_att32; o.ldx = QD; o.Wd = L.wo_d; }
            else { o.xh = c->d_att; o.ldxh = QD; }
            o.trace = tr(2);
            o.W = L.wo; o.K = QD; o.N = H; o.M = B; o.res = x; o.ldr = H; o.out_f32 = x; o.ldo = H;
            o.stamp = stamp;
        }
        GemvArgs q1{};   // batch-1 QKV projection, launched together with the attention when fusable
        if (skinny) {
            q1.x = x; q1.ldx = H; q1.norm_w = L.attn_norm; q1.eps = hp.rms_eps; q1.W = L.wqkv; q1.Wd = L.wqkv_d; q1.K = H;
            q1.N = QD + 2 * KD; q1.M = B; q1.out_f32 = c->d_qkv; q1.ldo = QD + 2 * KD;
            if (l == 0) { q1.embd_ids = c->d_tok; q1.embd = m->embd; q1.x_store = x; }   // fused embedding gather
            q1.trace = tr(0);
            q1.stamp = stamp;
        }
        GemvArgs gu{}, dn{};   // batch <= 8 FFN
        if (skinny) {
            gu.x = x; gu.ldx = H; gu.norm_w = L.ffn_norm; gu.eps = hp.rms_eps; gu.W = L.wgu; gu.Wd = L.wgu_d; gu.K = H; gu.N = F; gu.M = B;
            if (q8) { gu.out_f32 = c->d_act32; gu.ldo = F; }
            else { gu.out_f16 = c->d_act; gu.ldo16 = F; }
            gu.trace = tr(3);
            gu.stamp = stamp;
            if (q8) { dn.x = c->d_act32; dn.ldx = F; dn.Wd = L.wd_d; }
            else { dn.xh = c->d_act; dn.ldxh = F; }
            dn.W = L.wd; dn.K = F; dn.N = H; dn.M = B; dn.res = x; dn.ldr = H; dn.out_f32 = x; dn.ldo = H;
            dn.trace = tr(4);
            dn.stamp = stamp;
        }
        const bool exact = exact_decode(c);
        const bool fusable = skinny && B == 1 && !q8 && !skip;
        unsigned int *att_done = c->d_attdone + (size_t)l * 128;   // this layer's replicas
        if (fusable) da.att_done = att_done;
        if (fusable && exact && c->fuse.gran) {   // ggml's attention numerics as the fused launch's chain role
            da.fx = 1;
            da.sgran = c->d_sgran;
            da.gran = c->d_gran;   // (the fused decision needs the granule hand-off)
            da.layer = l;
        }
        unsigned int *fcnt = c->d_ffncnt + (size_t)l * 1024, *fcnt_next = c->d_ffncnt + (size_t)((l + 1) % nl) * 1024;
        // 0 = separate launches, 1 = QKV + attention in one launch, 2 = + o-projection.  ggml's numerics
        // in the fused launch need the granule hand-off (the chain role reads the new v from its granule):
        // without it the exact attention runs as separate launches, never as the fused fp32 split-K form
        const int fmode = fusable && (!exact || c->fuse.gran) ? launch_qkv_attention1(q1, da, &o, c->fuse, s, true) : 0;
        const bool o_fused = fmode >= 2;
        if (l == std::min(c->probe_layer, nl - 1)) c->probe_o_fused = o_fused;
        if (l == 0) {
            c->last_fmode = fmode;
            c->last_fx = fmode && da.fx;
            c->last_attn = fmode ? (da.fx ? 1 : 0) : -1;   // -1: set below by the separate path
        }
        if (ga) {
            if (l == nl - 1) c->qkv_in_gran = false;
            if (fmode) {
                if (c->fuse.gran) { da.gran = c->d_gran; da.layer = l; }
                if (l == nl - 1) c->qkv_in_gran = c->fuse.gran != 0;
                (void)launch_qkv_attention1(q1, da, &o, c->fuse, s, false);
            } else {
                if (skinny) {
                    if (!(skip & 1)) launch_gemv(EPI_F32, q1, s);
                } else {
                    GemmArgs q{};
                    q.M = B; q.N = QD + 2 * KD; q.K = H; q.out_f32 = c->d_qkv; q.ldo = QD + 2 * KD;
                    if (q8) {
                        launch_rmsnorm_q8(x, H, B, H, L.attn_norm, hp.rms_eps, c->d_q8n, c->d_q8nd, s);
                        gemm_q8_pre(c, EPI_F32, q, L.wqkv, L.wqkv_d, s, c->d_q8n, c->d_q8nd);
                    } else {
                        launch_rmsnorm_f16(x, H, nullptr, B, H, L.attn_norm, hp.rms_eps, c->d_xh, s);
                        q.A = c->d_xh; q.lda = H; q.W = L.wqkv; q.ldw = H; dec_gemm(c, EPI_F32, q, s);
                    }
                }
                da.att_done = nullptr;
                if (skip & 2) {
                } else if (exact) {   // ggml CPU FA numerics: scores by the splits, then the in-order chain
                    da.scores = c->d_scores;
                    da.fx_seq = c->fuse.fx_seq;
                    const bool one = launch_decode_attention_exact_seq(da, s);
                    if (!one) {
                        launch_decode_attention(da, s);
                        launch_decode_attention_exact(da, s);
                    }
                    if (l == 0) c->last_attn = one ? 2 : 3;
                } else {
                    launch_decode_attention(da, s);
                    if (l == 0) c->last_attn = 0;
                }
            }
        }
        if (!gb) continue;
        if (skinny) {
            if (!o_fused && !(skip & 4)) launch_gemv(EPI_F32, o, s);
            if (o_fused) dn.zero8 = att_done;   // re-arm the fused o-proj's arrival counters
            if (skip & 24 || nl < 2 || !launch_ffn1(gu, dn, fcnt, fcnt_next, c->fuse, s)) {
                if (!(skip & 8)) launch_gemv(q8 ? EPI_SWIGLU_F32 : EPI_SWIGLU_F16, gu, s);
                if (!(skip & 16)) launch_gemv(EPI_F32, dn, s);
                else if (o_fused) (void)hipMemsetAsync(att_done, 0, 8 * 16 * 4, s);   // the skipped down-proj re-arms these
            }
        } else if (q8) {
            GemmArgs ob{};
            ob.M = B; ob.N = H; ob.K = QD; ob.res = x; ob.ldr = H; ob.out_f32 = x; ob.ldo = H;
            gemm_q8_pre(c, EPI_F32, ob, L.wo, L.wo_d, s);
            launch_rmsnorm_q8(x, H, B, H, L.ffn_norm, hp.rms_eps, c->d_q8n, c->d_q8nd, s);
            GemmArgs gu{};
            gu.M = B; gu.N = 2 * F; gu.K = H; gu.out_f32 = c->d_x32; gu.ldo = F;
            GemmArgs dn{};
            dn.M = B; dn.N = H; dn.K = F; dn.res = x; dn.ldr = H; dn.out_f32 = x; dn.ldo = H;
            // the down projection's Q8_0 input quantised in the gate/up epilogue (one launch
            // fewer a layer, the same bits); the two-launch form where the skinny GEMM declines
            if (gemm_q8_pre_swiglu_q8(c, gu, L.wgu, L.wgu_d, s, c->d_q8n, c->d_q8nd, c->d_q8a, c->d_q8d)) {
                gemm_q8_pre(c, EPI_F32, dn, L.wd, L.wd_d, s, c->d_q8a, c->d_q8d);
            } else {
                gemm_q8_pre(c, EPI_SWIGLU_F32, gu, L.wgu, L.wgu_d, s, c->d_q8n, c->d_q8nd);
                gemm_q8(c, EPI_F32, dn, c->d_x32, nullptr, F, 0, L.wd, L.wd_d, s, c->d_q8a, c->d_q8d, true);
            }
        } else {
            GemmArgs ob{};
            ob.A = c->d_att; ob.lda = QD; ob.W = L.wo; ob.ldw = QD; ob.M = B; ob.N = H; ob.K = QD; ob.res = x; ob.ldr = H; ob.out_f32 = x; ob.ldo = H;
            dec_gemm(c, EPI_F32, ob, s);
            launch_rmsnorm_f16(x, H, nullptr, B, H, L.ffn_norm, hp.rms_eps, c->d_xh, s);
            GemmArgs gu{};
            gu.A = c->d_xh; gu.lda = H; gu.W = L.wgu; gu.ldw = H; gu.M = B; gu.N = 2 * F; gu.K = H; gu.out_f16 = c->d_act; gu.ldo16 = F;
            dec_gemm(c, EPI_SWIGLU_F16, gu, s);
            GemmArgs dn{};
            dn.A = c->d_act; dn.lda = F; dn.W = L.wd; dn.ldw = F; dn.M = B; dn.N = H; dn.K = F; dn.res = x; dn.ldr = H; dn.out_f32 = x; dn.ldo = H;
            dec_gemm(c, EPI_F32, dn, s);
        }
    }
    if (r.in(1 + 2 * nl)) {
        if (skinny || lmh_one) {   // the LM head as one launch: the batch <= 8 GEMV, or lmhead.hip at decode batches
            GemvArgs lm{};
            lm.x = x; lm.ldx = H; lm.norm_w = m->out_norm; lm.eps = hp.rms_eps; lm.W = m->embd; lm.K = H; lm.N = hp.vocab; lm.M = B;
            lm.out_f32 = want_logits ? c->d_logits : nullptr; lm.ldo = hp.vocab; lm.amax = c->d_amax;
            lm.done = c->d_done; lm.tok_out = c->d_tok; lm.hist = c->d_hist; lm.hist_stride = c->hist_cap; lm.step = c->d_step;
            lm.pos = c->d_pos;
            lm.stamp = stamp;
            if (skinny) {   // amax / done are zero at rest: the LM head's last workgroup re-arms them
                launch_gemv(EPI_ARGMAX, lm, s);
                if (con && (rc = constrain_step(c, B, 1))) return rc;
                if (lp && !smp) launch_token_logprob(c->d_logits, hp.vocab, B, 0, c->d_tok, c->d_step, c->d_lp, c->d_lphist, c->hist_cap, s);
                if (tk && (rc = topk_step(c, B))) return rc;
            } else {   // norm + GEMM + argmax + bookkeeping in one launch (lmhead.hip)
                lm.nkv = c->d_nkv;
                // (the top-K variant carries the log-sum-exp code: d_lp / d_lphist are written with either option)
                if ((lp && !smp && !con) || tk_fused) { lm.lp_part = c->d_lppart; lm.lp_out = c->d_lp; lm.lp_hist = c->d_lphist; }
                if (tk_fused) {
                    lm.tk_part = c->d_tkpart; lm.tk_out = c->d_tkid; lm.tk_lp = c->d_tklp; lm.tk_hist = c->d_tkhid;
                    lm.tk_lphist = c->d_tkhlp; lm.tk_k = K;
                }
                if (!launch_lmhead_batch(lm, s))   // (lmh_one mirrors its shape conditions: never expected)
                    return fail(QASR_ERR_STATE, "decode step: the batched LM head declined B = " + std::to_string(B));
                if (con) {
                    if ((rc = constrain_step(c, B, 1))) return rc;
                    if (lp && !smp) launch_token_logprob(c->d_logits, hp.vocab, B, 0, c->d_tok, c->d_step, c->d_lp, c->d_lphist, c->hist_cap, s);
                }
                if (tk && !tk_fused && (rc = topk_step(c, B))) return rc;
            }
        } else {
            launch_fill_u64(c->d_amax, B, 0ull, s);
            launch_rmsnorm_f16(x, H, nullptr, B, H, m->out_norm, hp.rms_eps, c->d_xh, s);
            GemmArgs lm{};
            lm.A = c->d_xh; lm.lda = H; lm.W = m->embd; lm.ldw = H; lm.M = B; lm.N = hp.vocab; lm.K = H;
            lm.out_f32 = want_logits ? c->d_logits : nullptr; lm.ldo = hp.vocab; lm.amax = c->d_amax;
            dec_gemm(c, EPI_ARGMAX, lm, s);
        }
    }
    if (r.in(2 + 2 * nl) && !skinny && !lmh_one) {   // bookkeeping (fused into the LM-head GEMV at batch <= 8)
        launch_step_advance(c->d_pos, c->d_nkv, c->d_step, B, s);
        launch_argmax_finish(c->d_amax, B, c->d_tok, c->d_hist, c->hist_cap, c->d_step, s);
        if (con && (rc = constrain_step(c, B, 1))) return rc;
        if (lp && !smp) launch_token_logprob(c->d_logits, hp.vocab, B, 0, c->d_tok, c->d_step, c->d_lp, c->d_lphist, c->hist_cap, s);
        if (tk && (rc = topk_step(c, B))) return rc;
        launch_fill_u64(c->d_amax, B, 0ull, s);   // re-arm (zero at rest)
    }
    // sampling: the draw replaces the greedy choice in d_tok and in the history slot the bookkeeping just wrote
    if (smp && r.in(skinny || lmh_one ? 1 + 2 * nl : 2 + 2 * nl) && (rc = sample_step(c, B, 1))) return rc;
    // a beam run: the beam step replaces the greedy choice in d_tok, then the fork (the grid covers the bucket's keys)
    if (c->beam_W >= 2 && r.in(skinny || lmh_one ? 1 + 2 * nl : 2 + 2 * nl) &&
        (rc = beam_step(c, B / c->beam_W, (std::min(c->max_ctx, splits * decode_split_len()) + 7) / 8)))
        return rc;
    return declined_check("decode step");
}

// ----------------------------------------------------------------- probes
// Kernel probes (qasr_set_probe): HIP events on the context stream around one
// launch group of every decode step of qasr_run; the rest of the step replays
// as two graphs around it.
//   1 = LM head + argmax (group 1 + 2nl)
//   2 = layer probe_layer's QKV + attention (+ o-projection): at batch 1 the
//       fused qkv_attn1_kernel, the dominant kernel of the headline decode
//   3 = layer probe_layer's o-projection (if separate) + FFN: at batch 1 the
//       fused ffn1_kernel
//   4 = decode batches (9..128 rows): layer probe_layer's attention launch
//       alone (decode_attn_seq_kernel: the only launch of group 2's set that
//       records device stamps at these batches; its bytes are the K / V^T rows
//       of every sequence plus its q / output rows -- the utterance set's
//       dominant decode kernel, bench.py utterance_set.roofline)
static int probe_group(const qasr_ctx *c) {
    const int nl = step_layers(c), pl = std::min(c->probe_layer, nl - 1);
    return c->probe == 1 ? 1 + 2 * nl : (c->probe == 2 || c->probe == 4) ? 1 + 2 * pl : 2 + 2 * pl;
}

// algorithmic HBM bytes of one launch of the probed group at decode step k
// (SURVEY.md §8(d)): weights streamed once for the batch + each sequence's
// K/V rows of the layer (fp16, n_kv = P_b + k + 1 keys) + activations
static double probe_bytes(const qasr_ctx *c, int B, int k) {
    const Hparams &hp = c->m->hp;
    const double H = hp.hidden, QD = hp.n_head * 128.0, KD = hp.n_kv_head * 128.0, F = hp.dec_ffn;
    const double wb = c->m->q8 ? 34.0 / 32.0 : 2.0;   // bytes per linear weight (Q8_0 block: 34 B / 32)
    if (c->probe == 1) return (double)hp.vocab * H * 2 + B * H * 4 + B * 8.0;
    if (c->probe == 4) {   // the attention launch: K and V^T rows (fp16) + q / k / v rows (fp32) in + output (fp16) out
        double kv = 0;
        for (int b = 0; b < B; b++) kv += (double)(c->run_P[b] + k + 1) * KD * 2 * 2;
        return kv + B * (QD + 2 * KD) * 4 + B * QD * 2;
    }
    if (c->probe == 2) {
        double kv = 0;
        for (int b = 0; b < B; b++) kv += (double)(c->run_P[b] + k + 1) * KD * 2 * 2;
        const bool o_in = c->probe_o_fused;
        return (QD + 2 * KD) * H * wb + B * H * 4 + (o_in ? H * QD * wb + B * H * 8 : 0.0) + kv + B * (QD + 2 * KD) * 4;
    }
    return 3 * F * H * wb + (c->probe_o_fused ? 0.0 : H * QD * wb) + B * H * 4 * 3;
}

// ------------------------------------------------------------ step graphs
static int capture(qasr_ctx *c, int B, bool want_logits, StepRange r, int splits, hipGraphExec_t *out) {
    hipGraph_t gr;
    HIPCHK(hipStreamBeginCapture(c->st, hipStreamCaptureModeThreadLocal));
    const int rc = decode_step_kernels(c, B, want_logits, r, splits);
    HIPCHK(hipStreamEndCapture(c->st, &gr));
    if (rc) {
        (void)hipGraphDestroy(gr);
        return rc;
    }
    HIPCHK(hipGraphInstantiate(out, gr, nullptr, nullptr, 0));
    HIPCHK(hipGraphDestroy(gr));
    c->n_captures++;
    return 0;
}

// split-grid bucket for a step whose longest sequence feeds position `pos`
// (rounded up to 4 splits = 256 keys, so a run re-captures every 256 steps)
int qasr::eng::split_bucket(qasr_ctx *c, int pos) {
    const int need = (pos + 1 + decode_split_len() - 1) / decode_split_len();
    return std::min(c->max_splits, (need + 3) / 4 * 4);
}

// prepare decode graphs for batch B; base = longest prompt (step k feeds base + k)
int qasr::eng::decode_graph(qasr_ctx *c, int B, bool want_logits, int base) {
    const int pg = c->probe ? probe_group(c) : -1;
    // (graphs are kept per (batch, split bucket): a stream's decode chunks switch between live-prefix batches)
    if (c->graph_logits != want_logits || c->graph_probe_group != pg) c->drop_graphs();
    c->graph_B = B;
    c->graph_logits = want_logits;
    c->graph_base = base;
    c->graph_probe_group = pg;
    return 0;
}

static int step_graphs(qasr_ctx *c, int splits, qasr_ctx::StepGraphs **out) {
    const int B = c->graph_B;
    auto &gs = c->graphs[std::make_tuple(step_mode(c), B, splits)];   // (a beam run's and a sampling run's steps are graphs of their own)
    int rc;
    if (!gs.full && (rc = capture(c, B, c->graph_logits, kWholeStep, splits, &gs.full))) return rc;
    if (c->probe && !gs.pre) {
        const int g = c->graph_probe_group;
        if ((rc = capture(c, B, c->graph_logits, StepRange{0, g}, splits, &gs.pre)) ||
            (rc = capture(c, B, c->graph_logits, StepRange{g + 1, 1 << 30}, splits, &gs.post)))
            return rc;
    }
    *out = &gs;
    return 0;
}

// a whole decode step of the batch decode_graph prepared (B): the kernels
// themselves where the context runs eagerly, else the (batch, splits) graph
int qasr::eng::launch_whole_step(qasr_ctx *c, int B, int splits) {
    if (c->eager) return decode_step_kernels(c, B, c->graph_logits, kWholeStep, splits);
    qasr_ctx::StepGraphs *gs = nullptr;
    if (int rc = step_graphs(c, splits, &gs)) return rc;
    HIPCHK(hipGraphLaunch(gs->full, c->st));
    return 0;
}

// one greedy step (k = 0-based step of the run); under a probe the probed
// group runs eagerly between HIP events
int qasr::eng::launch_step(qasr_ctx *c, int B, int k) {
    const int splits = split_bucket(c, c->graph_base + k);
    if (!c->probe || k % c->probe_stride != 0) return launch_whole_step(c, B, splits);
    qasr_ctx::StepGraphs *gs = nullptr;
    int rc;
    if (!c->eager && (rc = step_graphs(c, splits, &gs))) return rc;
    while ((int)c->pev.size() < 2 * (k + 1)) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        c->pev.push_back(e);
    }
    const int g = c->graph_probe_group;
    if (c->eager) {
        if ((rc = decode_step_kernels(c, B, c->graph_logits, StepRange{0, g}, splits))) return rc;
    } else {
        HIPCHK(hipGraphLaunch(gs->pre, c->st));
    }
    HIPCHK(hipEventRecord(c->pev[2 * k], c->st));
    c->cur_stamp = k < c->max_ctx ? c->d_pstamp + (size_t)k * kStampRec : nullptr;
    rc = decode_step_kernels(c, B, c->graph_logits, StepRange{g, g + 1}, splits);
    c->cur_stamp = nullptr;
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->pev[2 * k + 1], c->st));
    if (c->eager) {
        if ((rc = decode_step_kernels(c, B, c->graph_logits, StepRange{g + 1, 1 << 30}, splits))) return rc;
    } else {
        HIPCHK(hipGraphLaunch(gs->post, c->st));
    }
    return 0;
}

// arm the device-clock records of a run's probed launches (qasr_run): per
// step kStampRec u64, starts (~0) then ends (0), one 256-B line per shard
int qasr::eng::probe_arm(qasr_ctx *c, int nsteps) {
    if (!c->probe || nsteps <= 0) return 0;
    const int n = std::min(nsteps, c->max_ctx);
    launch_fill_u64(c->d_pstamp, n * kStampRec, ~0ull, c->st);
    HIPCHK(hipMemset2DAsync(c->d_pstamp + STAMP_ENDS, kStampRec * 8, 0, STAMP_ENDS * 8, n, c->st));
    return 0;
}

int qasr::eng::probe_collect(qasr_ctx *c, int B, int nsteps) {
    if (!c->probe) return 0;
    const int n = std::min(nsteps, c->max_ctx);
    // the first word of every shard line: [step][64]
    std::vector<unsigned long long> st((size_t)n * 64);
    if (n > 0)
        HIPCHK(hipMemcpy2D(st.data(), 8, c->d_pstamp, 32 * 8, 8, (size_t)n * 64, hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++) {   // first block start -> last block end, 100 MHz clock
        unsigned long long t0 = ~0ull, t1 = 0;
        for (int i = 0; i < 32; i++) { t0 = std::min(t0, st[(size_t)k * 64 + i]); t1 = std::max(t1, st[(size_t)k * 64 + 32 + i]); }
        if (t0 == ~0ull || t1 <= t0) continue;   // launches without records (batch > 8 groups)
        c->probe_dev_ms += (double)(t1 - t0) * 1e-5;
        c->probe_dev_n++;
    }
    for (int k = 0; k < nsteps; k += c->probe_stride) {   // (steps between strides left no records)
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->pev[2 * k], c->pev[2 * k + 1]));
        c->probe_ms += ms;
        c->probe_n++;
        c->probe_bytes += probe_bytes(c, B, k);
    }
    return 0;
}

extern "C" int qasr_set_probe(qasr_ctx *c, int kernel) {
    if (!c || kernel < 0 || kernel > 4) return fail(QASR_ERR_ARG, "bad probe id");
    c->probe = kernel;
    c->probe_ms = 0.0;
    c->probe_n = 0;
    c->probe_bytes = 0.0;
    c->probe_dev_ms = 0.0;
    c->probe_dev_n = 0;
    return 0;
}

extern "C" int qasr_get_probe_device(qasr_ctx *c, double *total_ms, int64_t *launches) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    if (total_ms) *total_ms = c->probe_dev_ms;
    if (launches) *launches = c->probe_dev_n;
    return 0;
}

extern "C" int qasr_get_probe(qasr_ctx *c, double *total_ms, int64_t *launches, double *bytes_per_launch) {
    if (!c) return fail(QASR_ERR_ARG, "null context");
    if (total_ms) *total_ms = c->probe_ms;
    if (launches) *launches = c->probe_n;
    if (bytes_per_launch) *bytes_per_launch = c->probe_n ? c->probe_bytes / c->probe_n : 0.0;
    return 0;
}

// ------------------------------------------------------- single-step entry
extern "C" int qasr_decode_step(qasr_ctx *c, const int32_t *tok, const int *n_past, int B, float *logits, int32_t *argmax) {
    if (!c || !tok || !n_past || B <= 0 || B > c->max_batch) return fail(QASR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->m->device));
    // a caller may repeat a position (same tag): no granule of an earlier call may match
    if (int rc = reset_granules(c)) return rc;
    std::vector<int> pos(B), nkv(B);
    for (int b = 0; b < B; b++) {
        if (n_past[b] < 0 || n_past[b] + 1 > c->max_ctx) return fail(QASR_ERR_ARG, "Context length exceeded");
        if (tok[b] < 0 || tok[b] >= c->m->hp.vocab) return fail(QASR_ERR_ARG, "token id out of range");
        pos[b] = n_past[b];
        nkv[b] = n_past[b] + 1;
    }
    std::unique_lock<std::mutex> dev_lk;
    if (takes_fused(c, B)) {
        dev_lk = std::unique_lock<std::mutex>(device_lock(c->m->device));
        if (int rc = reset_counters(c)) return rc;   // zero at rest whatever the previous call's launch modes were
    }
    HIPCHK(hipMemcpyAsync(c->d_tok, tok, B * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->d_pos, pos.data(), B * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->d_nkv, nkv.data(), B * 4, hipMemcpyHostToDevice, c->st));
    // constraints on: the rows' history goes on from the last prefill (the step writes slot stage_t + 1); else slot 1 of a
    // history nothing reads
    const bool con = constraints_on(c);
    if (con && c->stage_t + 2 > c->hist_cap) return fail(QASR_ERR_STATE, "constraints: the history holds max_ctx tokens (prefill again)");
    if (con) HIPCHK(hipMemcpyAsync(c->d_step, &c->stage_t, 4, hipMemcpyHostToDevice, c->st));
    else HIPCHK(hipMemsetAsync(c->d_step, 0, 4, c->st));
    if (int rc = decode_step_kernels(c, B, logits != nullptr, kWholeStep, split_bucket(c, *std::max_element(pos.begin(), pos.end()))))
        return rc;
    HIPCHK(hipGetLastError());
    if (logits) HIPCHK(hipMemcpyAsync(logits, c->d_logits, (size_t)B * c->m->hp.vocab * 4, hipMemcpyDeviceToHost, c->st));
    if (argmax) HIPCHK(hipMemcpyAsync(argmax, c->d_tok, B * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->lp_step_B = c->fuse.token_logprobs ? B : 0;
    c->tk_step_B = c->fuse.top_k ? B : 0;
    if (con) c->stage_t++;
    return check_dev_err(c);
}

extern "C" int qasr_get_step_logprobs(qasr_ctx *c, float *out, int B) {
    if (!c || !out || B <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    if (!c->fuse.token_logprobs) return fail(QASR_ERR_STATE, "option token_logprobs is off");
    if (!c->lp_step_B) return fail(QASR_ERR_STATE, "no prefill or decode step has run with option token_logprobs on");
    if (B < c->lp_step_B) return fail(QASR_ERR_ARG, "buffer shorter than the last step's batch");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipMemcpyAsync(out, c->d_lp, (size_t)c->lp_step_B * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

extern "C" int qasr_get_step_topk(qasr_ctx *c, int32_t *ids, float *logprobs, int B, int K) {
    if (!c || !ids || !logprobs || B <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    if (!c->fuse.top_k) return fail(QASR_ERR_STATE, "option top_k is off");
    if (K != c->fuse.top_k) return fail(QASR_ERR_ARG, "K differs from option top_k");
    if (!c->tk_step_B) return fail(QASR_ERR_STATE, "no prefill or decode step has run with option top_k on");
    if (B < c->tk_step_B) return fail(QASR_ERR_ARG, "buffer shorter than the last step's batch");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipMemcpyAsync(ids, c->d_tkid, (size_t)c->tk_step_B * K * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(logprobs, c->d_tklp, (size_t)c->tk_step_B * K * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}
