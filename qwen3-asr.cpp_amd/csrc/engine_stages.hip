// engine_stages.hip -- the stages before the decode loop (mel, encoder,
// prefill) with their stand-alone qasr_* entry points, and the linear-layer
// helpers (F16 / Q8_0) that the decode step shares.
#include <memory>

#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

// --------------------------------------------------------- linear layers
// encoder / prefill GEMMs with the context's tile option
void qasr::eng::launch_gemm_c(qasr_ctx *c, int amode, int epi, GemmArgs g, hipStream_t s) {
    g.regs_staged = c->fuse.gemm_regs;
    launch_gemm(amode, epi, g, s);
}

// operands of a Q8_0 GEMM: quantised activation rows (qa, qd) against the weight (W, Wd), both K wide
// (g.wdef stays 0: only the f16 dec_gemm takes option skinny_wdef)
static void q8_operands(const qasr_ctx *c, GemmArgs &g, const int8_t *qa, const float *qd, const uint16_t *W, const uint16_t *Wd) {
    g.Aq = qa; g.lda = g.K; g.Ad = qd; g.ldad = g.K / 32;
    g.Wq = (const int8_t *)W; g.ldw = g.K; g.Wd = Wd;
    g.no_skinny = !c->fuse.skinny;
    g.skinny_inflight = c->fuse.skinny_inf;
}

// A Q8_0 linear layer: quantise the activation rows (fp32 a32 or fp16 a16,
// optional conv_out gather) into c->q8a / c->q8d, then the int8 block GEMM.
// g carries M, N, K and the epilogue.
void qasr::eng::gemm_q8(qasr_ctx *c, int epi, GemmArgs g, const float *a32, const uint16_t *a16, int lda, int gather_C,
                        const uint16_t *W, const uint16_t *Wd, hipStream_t s, int8_t *qa, float *qd, bool decode) {
    if (!qa) { qa = c->q8a.as<int8_t>(); qd = c->q8d.as<float>(); }
    launch_quantize_q8(a32, a16, lda, g.M, g.K, gather_C, qa, qd, s);
    q8_operands(c, g, qa, qd, W, Wd);
    if (decode && launch_gemm_skinny_q8(epi, g, s)) return;
    launch_gemm_q8(epi, g, s);
}

// decode batches: activations already quantised into d_q8a / d_q8d by the
// producing kernel (rmsnorm_q8, the attention combiner)
void qasr::eng::gemm_q8_pre(qasr_ctx *c, int epi, GemmArgs g, const uint16_t *W, const uint16_t *Wd, hipStream_t s,
                            const int8_t *qa, const float *qd) {
    q8_operands(c, g, qa ? qa : c->d_q8a, qa ? qd : c->d_q8d, W, Wd);
    if (launch_gemm_skinny_q8(epi, g, s)) return;
    launch_gemm_q8(epi, g, s);
}

// decode batches: SwiGLU gate/up with the output quantised to Q8_0 (q / d, row
// length N / 2) in the skinny GEMM's epilogue; false (nothing launched) where
// the skinny GEMM declines the shape or is switched off
bool qasr::eng::gemm_q8_pre_swiglu_q8(qasr_ctx *c, GemmArgs g, const uint16_t *W, const uint16_t *Wd, hipStream_t s,
                                      const int8_t *qa, const float *qd, int8_t *q, float *d) {
    q8_operands(c, g, qa, qd, W, Wd);
    g.out_q = q; g.out_d = d; g.ldoq = g.N / 2;
    return launch_gemm_skinny_q8(EPI_SWIGLU_Q8, g, s);
}

// y = act W^T with the model's weight type: F16 takes the fp16 activation
// (a16), Q8_0 quantises the fp32 (a32) where given, else the fp16 one
static void linear(qasr_ctx *c, int epi, GemmArgs g, const float *a32, const uint16_t *a16, int lda, const uint16_t *W,
                   const uint16_t *Wd, hipStream_t s) {
    if (c->m->q8) { gemm_q8(c, epi, g, a32, a32 ? nullptr : a16, lda, 0, W, Wd, s); return; }
    g.A = a16; g.lda = lda; g.W = W; g.ldw = g.K;
    launch_gemm_c(c, AM_DENSE, epi, g, s);
}

static int ensure_q8(qasr_ctx *c, size_t rows, size_t kmax, size_t x32_cols) {
    int rc;
    if ((rc = ensure(c, c->q8a, rows * kmax)) || (rc = ensure(c, c->q8d, rows * (kmax / 32) * 4)) ||
        (rc = ensure(c, c->x32, rows * x32_cols * 4)))
        return rc;
    return 0;
}

// =================================================================== stages
// B host clips (n[b] >= 0 samples, checked by the caller) back to back into
// c->pcm, copies on the context stream; off[b] = clip b's first sample
int qasr::eng::pack_pcm(qasr_ctx *c, const float *const *pcm, const int *n, int B, std::vector<long> &off) {
    off.resize(B);
    long tot = 0;
    for (int b = 0; b < B; b++) { off[b] = tot; tot += n[b]; }
    const int rc = ensure(c, c->pcm, std::max<long>(tot, 1) * 4);
    if (rc) return rc;
    for (int b = 0; b < B; b++)
        if (n[b]) HIPCHK(hipMemcpyAsync(c->pcm.as<float>() + off[b], pcm[b], (size_t)n[b] * 4, hipMemcpyHostToDevice, c->st));
    return 0;
}

// mel for B clips whose PCM is already in c->pcm (offsets/lengths given);
// result in c->mel as B blocks [128][T_b].
int qasr::eng::run_mel(qasr_ctx *c, const std::vector<long> &off, const std::vector<int> &n, std::vector<long> &mel_off,
                       std::vector<int> &T, const float *d_pcm) {
    qasr_model *m = c->m;
    const int B = (int)n.size();
    std::vector<MelClip> clips(B);
    std::vector<int2> blocks;
    long tmp_total = 0, out_total = 0;
    T.resize(B);
    mel_off.resize(B);
    const int fpb = mel_frames_per_block();
    for (int b = 0; b < B; b++) {
        const int TF = n[b] / 160 + 1;
        clips[b] = MelClip{off[b], n[b], TF, tmp_total, out_total};
        T[b] = TF - 1;
        mel_off[b] = out_total;
        tmp_total += 128L * TF;
        out_total += 128L * (TF - 1);
        for (int f = 0; f < TF; f += fpb) blocks.push_back(make_int2(b, f));
    }
    int rc;
    if ((rc = upload(c, c->melclips, clips)) || (rc = upload(c, c->melblocks, blocks)) ||
        (rc = ensure(c, c->meltmp, tmp_total * 8)) || (rc = ensure(c, c->mel, std::max<long>(out_total, 1) * 4)) ||
        (rc = ensure(c, c->melmax, B * 8)))
        return rc;
    HIPCHK(hipMemsetAsync(c->melmax.p, 0, B * 8, c->st));
    launch_mel(d_pcm ? d_pcm : c->pcm.as<float>(), c->melclips.as<MelClip>(), B, blocks.empty() ? nullptr : c->melblocks.as<int2>(),
               (int)blocks.size(), m->tw, m->hann, m->filters, c->meltmp.as<double>(), c->melmax.as<unsigned long long>(),
               c->mel.as<float>(), c->st);
    HIPCHK(hipGetLastError());
    return 0;
}

// encoder over B clips whose mel sits at d_mel + mel_off[b] ([128][T_b]).
// conv_only: stop after conv_out + PE (output [sum N][d_model] in c->ex).
// no_chunk: AudioEncoder::encode_no_chunk (src/audio_encoder.cpp:603-852): the
// conv stack over each clip's frames as one chunk, PE positions 0 .. N-1 (ASR)
int qasr::eng::run_encoder(qasr_ctx *c, const float *d_mel, const std::vector<long> &mel_off, const std::vector<int> &T,
                           bool conv_only, std::vector<int> &Nb, bool no_chunk) {
    qasr_model *m = c->m;
    const Hparams &hp = m->hp;
    const int B = (int)T.size(), C = hp.conv_ch, D = hp.d_model, FF = hp.enc_ffn;
    std::vector<ChunkDesc> ch;
    std::vector<int> s1, s2, s3, pepos;
    int r1 = 0, r2 = 0, r3 = 0, er = 0;
    Nb.assign(B, 0);
    // ASR: each chunk on its own length (src/audio_encoder.cpp:331-409).  Aligner:
    // every chunk zero-padded to 100 frames, the valid frames of the (short)
    // last one kept (src/forced_aligner.cpp:601-735).  One clip: the valid
    // conv_out rows are the leading rows.  Several clips: a clip's short last
    // chunk leaves padded rows before the next clip's, so conv_out runs over
    // every padded row (PE position = row within its chunk, as for the valid
    // ones) and the valid rows are gathered after it.
    const bool al = hp.aligner;
    if (no_chunk && al) return fail(QASR_ERR_ARG, "encode_no_chunk: ASR models only");
    const bool al_gather = al && B > 1;
    std::vector<int> pepos_pad, gidx;
    for (int b = 0; b < B; b++) {
        const int CH = no_chunk ? std::max(T[b], 1) : 100;
        for (int s = 0; s < T[b]; s += CH) {
            ChunkDesc d;
            d.mel_off = mel_off[b] + s;
            d.T = T[b];
            d.Lv = std::min(CH, T[b] - s);
            d.L = al ? 100 : d.Lv;
            d.W1 = (d.L - 1) / 2 + 1;
            d.W2 = (d.W1 - 1) / 2 + 1;
            d.W3 = (d.W2 - 1) / 2 + 1;
            d.row1 = r1; d.row2 = r2; d.row3 = r3; d.enc_row = er;
            s1.push_back(r1); s2.push_back(r2); s3.push_back(r3);
            const int valid = chunk_out_len(d.Lv);
            if (al_gather) {
                for (int w = 0; w < d.W3; w++) pepos_pad.push_back(w);
                for (int w = 0; w < valid; w++) gidx.push_back(r3 / 16 + w);
            }
            r1 += 64 * d.W1; r2 += 32 * d.W2; r3 += 16 * d.W3; er += valid;
            for (int w = 0; w < valid; w++) pepos.push_back(w);
            Nb[b] += valid;
            ch.push_back(d);
        }
    }
    const int NC = (int)ch.size(), N = er;
    if (N == 0) return 0;
    int rc;
    const float *pe_tab = m->pe;   // 13 positions: a 100-frame chunk's
    if (no_chunk) {
        int npos = 0;
        for (int v : Nb) npos = std::max(npos, v);
        if (npos > c->pebig_rows) {
            std::vector<float> pe;
            sinusoidal_pe(pe, npos, D);
            if ((rc = ensure(c, c->pebig, pe.size() * 4))) return rc;
            HIPCHK(hipMemcpy(c->pebig.p, pe.data(), pe.size() * 4, hipMemcpyHostToDevice));
            c->pebig_rows = npos;
        }
        pe_tab = c->pebig.as<float>();
    }
    const int NP = r3 / 16;   // conv_out rows over every (padded) chunk row
    if (al_gather && ((rc = upload(c, c->gidx, gidx)) || (rc = ensure(c, c->exp_, (size_t)NP * D * 4)))) return rc;
    if ((rc = upload(c, c->chunks, ch)) || (rc = upload(c, c->rs1, s1)) || (rc = upload(c, c->rs2, s2)) ||
        (rc = upload(c, c->rs3, s3)) || (rc = upload(c, c->pepos, al_gather ? pepos_pad : pepos)) ||
        (rc = ensure(c, c->act1, (size_t)r1 * C * 2)) || (rc = ensure(c, c->act2, (size_t)r2 * C * 2)) ||
        (rc = ensure(c, c->act3, (size_t)r3 * C * 2)) || (rc = ensure(c, c->ex, (size_t)N * D * 4)) ||
        (rc = ensure(c, c->exh, (size_t)N * std::max(D, FF) * 2)) || (rc = ensure(c, c->eqkv, (size_t)N * 3 * D * 4)) ||
        (rc = ensure(c, c->eatt, (size_t)N * D * 2)) || (rc = ensure(c, c->eff, (size_t)N * FF * 2)) ||
        (rc = ensure(c, c->feats, (size_t)N * hp.hidden * 4)))
        return rc;
    hipStream_t s = c->st;
    int max_w1 = 0;
    for (const ChunkDesc &d : ch) max_w1 = std::max(max_w1, d.W1);
    launch_conv1(d_mel, c->chunks.as<ChunkDesc>(), c->rs1.as<int>(), NC, r1, m->conv1_w, m->conv1_b, m->gelu, C,
                 c->act1.as<uint16_t>(), s, max_w1);
    GemmArgs g{};
    g.chunks = c->chunks.as<ChunkDesc>();
    g.n_chunks = NC;
    g.C = C;
    g.gelu = m->gelu;
    // conv2: act1 (NHWC, H=64) -> act2 (NHWC, H=32)
    g.A = c->act1.as<uint16_t>(); g.W = m->conv2_w; g.ldw = conv_kpad(C); g.M = r2; g.N = C; g.K = 9 * C;
    g.row_start = c->rs2.as<int>(); g.bias = m->conv2_b; g.out_f16 = c->act2.as<uint16_t>(); g.ldo16 = C;
    launch_gemm_c(c, AM_CONV2, EPI_GELU_F16, g, s);
    // conv3: act2 -> act3 rows ordered (chunk, w, h) so conv_out's A is dense
    g.A = c->act2.as<uint16_t>(); g.W = m->conv3_w; g.M = r3; g.row_start = c->rs3.as<int>(); g.bias = m->conv3_b;
    g.out_f16 = c->act3.as<uint16_t>();
    launch_gemm_c(c, AM_CONV3, EPI_GELU_F16, g, s);
    const bool q8 = m->q8;
    const int MO = al_gather ? NP : N;
    if (q8 && (rc = ensure_q8(c, MO, std::max(16 * C, std::max(D, FF)), D))) return rc;
    // conv_out (no bias) + per-chunk sinusoidal PE (src/audio_encoder.cpp:147-149, :400-404)
    GemmArgs o{};
    o.M = MO; o.N = D; o.K = 16 * C;
    o.out_f32 = al_gather ? c->exp_.as<float>() : c->ex.as<float>(); o.ldo = D; o.pe = pe_tab; o.pe_pos = c->pepos.as<int>();
    if (q8) {
        gemm_q8(c, EPI_F32, o, nullptr, c->act3.as<uint16_t>(), 16 * C, C, m->conv_out_w, m->conv_out_d, s);
    } else {
        o.A = c->act3.as<uint16_t>(); o.lda = 16 * C; o.W = m->conv_out_w; o.ldw = 16 * C;
        launch_gemm_c(c, AM_DENSE, EPI_F32, o, s);
    }
    if (al_gather) launch_gather_rows(c->exp_.as<float>(), c->gidx.as<int>(), N, D, c->ex.as<float>(), s);
    HIPCHK(hipGetLastError());
    if (c->profile_on) HIPCHK(hipEventRecord(c->ev[EV_ENC_CONV], s));   // conv front-end | transformer
    if (conv_only) return 0;

    // attention segments: whole clips (ASR: full attention, src/audio_encoder.cpp:466-486)
    // or the aligner's block-diagonal windows of 13 * (800 / 100) = 104 frames
    // (src/forced_aligner.cpp:737-766)
    std::vector<int> sst, sln;
    int acc = 0, maxn = 0;
    for (int b = 0; b < B; b++) {
        const int win = al ? 104 : std::max(Nb[b], 1);
        for (int o = 0; o < Nb[b]; o += win) {
            sst.push_back(acc + o);
            sln.push_back(std::min(win, Nb[b] - o));
            maxn = std::max(maxn, sln.back());
        }
        acc += Nb[b];
    }
    const int NS = (int)sst.size();
    std::vector<int> segs(sst);
    segs.insert(segs.end(), sln.begin(), sln.end());
    if ((rc = upload(c, c->segs, segs))) return rc;
    float *x = c->ex.as<float>();
    uint16_t *xh = c->exh.as<uint16_t>();
    float *x32 = q8 ? c->x32.as<float>() : nullptr;
    for (int l = 0; l < hp.enc_layers; l++) {
        const EncLayer &L = m->enc[l];
        launch_layernorm_f16(x, N, D, L.ln1_w, L.ln1_b, hp.enc_eps, xh, s, x32);
        GemmArgs q{};
        q.M = N; q.N = 3 * D; q.K = D; q.bias = L.bqkv; q.out_f32 = c->eqkv.as<float>(); q.ldo = 3 * D;
        linear(c, EPI_F32, q, x32, xh, D, L.wqkv, L.wqkv_d, s);
        launch_enc_attention(c->eqkv.as<float>(), c->segs.as<int>(), c->segs.as<int>() + NS, NS, maxn, D, hp.enc_heads,
                             c->eatt.as<uint16_t>(), s, x32, c->fuse.enc_attn_f32 != 0);
        GemmArgs op{};
        op.M = N; op.N = D; op.K = D; op.bias = L.bo; op.res = x; op.ldr = D; op.out_f32 = x; op.ldo = D;
        linear(c, EPI_F32, op, x32, c->eatt.as<uint16_t>(), D, L.wo, L.wo_d, s);
        launch_layernorm_f16(x, N, D, L.ln2_w, L.ln2_b, hp.enc_eps, xh, s, x32);
        GemmArgs f1{};
        f1.M = N; f1.N = FF; f1.K = D; f1.bias = L.b1; f1.gelu = m->gelu; f1.out_f16 = c->eff.as<uint16_t>(); f1.ldo16 = FF;
        linear(c, EPI_GELU_F16, f1, x32, xh, D, L.w1, L.w1_d, s);
        GemmArgs f2{};   // GELU output is fp16-exact (LUT): the Q8_0 path quantises it as is
        f2.M = N; f2.N = D; f2.K = FF; f2.bias = L.b2; f2.res = x; f2.ldr = D; f2.out_f32 = x; f2.ldo = D;
        linear(c, EPI_F32, f2, nullptr, c->eff.as<uint16_t>(), FF, L.w2, L.w2_d, s);
    }
    launch_layernorm_f16(x, N, D, m->ln_post_w, m->ln_post_b, hp.enc_eps, xh, s, x32);
    GemmArgs p1{};
    p1.M = N; p1.N = D; p1.K = D; p1.bias = m->proj1_b; p1.gelu = m->gelu; p1.out_f16 = c->eatt.as<uint16_t>(); p1.ldo16 = D;
    linear(c, EPI_GELU_F16, p1, x32, xh, D, m->proj1_w, m->proj1_d, s);
    GemmArgs p2{};
    p2.M = N; p2.N = hp.hidden; p2.K = D; p2.bias = m->proj2_b; p2.out_f32 = c->feats.as<float>(); p2.ldo = hp.hidden;
    linear(c, EPI_F32, p2, nullptr, c->eatt.as<uint16_t>(), D, m->proj2_w, m->proj2_d, s);
    HIPCHK(hipGetLastError());
    return declined_check("encoder");
}

// embedding gather + audio splice + decoder layer stack over the prompt rows of
// B sequences (positions 0..P_b-1, KV cache of sequence b reset); leaves the
// final hidden rows in c->px.  Row tables live in c->prow:
// [row_seq | row_pos | row_audio] (3*rows ints) + [seq_row0 | seq_len | seq_slot].
int qasr::eng::prefill_layers(qasr_ctx *c, const std::vector<int32_t> &ids, const std::vector<int> &P, const float *d_feats,
                              const std::vector<int> &audio_pos, const std::vector<int> &N, const std::vector<int> *slots,
                              const std::vector<int> *pos0) {
    qasr_model *m = c->m;
    const Hparams &hp = m->hp;
    const int B = (int)P.size(), H = hp.hidden, QD = hp.n_head * 128, KD = hp.n_kv_head * 128, F = hp.dec_ffn;
    if (B > c->max_batch) return fail(QASR_ERR_ARG, "batch exceeds context max_batch");
    if (slots)
        for (int v : *slots)
            if (v < 0 || v >= c->max_batch) return fail(QASR_ERR_ARG, "KV-cache slot out of range");
    int rows = 0, maxp = 0;
    auto p0 = [&](int b) { return pos0 ? (*pos0)[b] : 0; };   // a chunk after p0(b) cached tokens
    for (int b = 0; b < B; b++) {
        if (P[b] <= 0) return fail(QASR_ERR_ARG, "empty prompt");
        if (p0(b) < 0 || p0(b) + P[b] > c->max_ctx) return fail(QASR_ERR_ARG, "Context length exceeded");
        rows += P[b];
        maxp = std::max(maxp, P[b]);
    }
    if (pos0 && (m->hp.aligner || !c->fuse.fa_exact_prefill))   // (the chunk form is built on the exact kernel)
        for (int b = 0; b < B; b++)
            if (p0(b)) return fail(QASR_ERR_ARG, "a chunk after cached tokens needs the exact prefill attention (ASR model)");
    std::vector<int> tab(3 * rows + 4 * B), lastrow(B);
    int r = 0, fr = 0;
    for (int b = 0; b < B; b++) {
        const bool splice = d_feats && N[b] > 0 && audio_pos[b] >= 0 && audio_pos[b] + N[b] <= P[b];
        for (int t = 0; t < P[b]; t++, r++) {
            tab[r] = slots ? (*slots)[b] : b;   // the KV-cache slot the row writes
            tab[rows + r] = p0(b) + t;
            tab[2 * rows + r] = (splice && t >= audio_pos[b] && t < audio_pos[b] + N[b]) ? fr + (t - audio_pos[b]) : -1;
        }
        fr += N[b];
        lastrow[b] = r - 1;
    }
    int acc = 0;
    for (int b = 0; b < B; b++) {   // seq_row0 | seq_len | seq_slot | seq_pos0
        tab[3 * rows + b] = acc;
        tab[3 * rows + B + b] = P[b];
        tab[3 * rows + 2 * B + b] = slots ? (*slots)[b] : b;
        tab[3 * rows + 3 * B + b] = p0(b);
        acc += P[b];
    }
    int rc;
    if ((rc = upload(c, c->prow, tab)) || (rc = upload(c, c->plast, lastrow)) || (rc = upload(c, c->pids, ids)) ||
        (rc = ensure(c, c->px, (size_t)rows * H * 4)) || (rc = ensure(c, c->pxh, (size_t)rows * std::max(H, F) * 2)) ||
        (rc = ensure(c, c->pqkv, (size_t)rows * (QD + 2 * KD) * 4)) || (rc = ensure(c, c->pq, (size_t)rows * QD * 2)) ||
        (rc = ensure(c, c->patt, (size_t)rows * QD * 2)) || (rc = ensure(c, c->pact, (size_t)rows * F * 2)))
        return rc;
    const bool al = hp.aligner;   // fp32 Q / K scores (src/forced_aligner.cpp:1041-1046)
    if (al && ((rc = ensure(c, c->pq32, (size_t)rows * QD * 4)) || (rc = ensure(c, c->pk32, (size_t)rows * KD * 4)))) return rc;
    hipStream_t s = c->st;
    const int *d_seq = c->prow.as<int>(), *d_pos = d_seq + rows, *d_aud = d_seq + 2 * rows;
    const int *d_srow0 = d_seq + 3 * rows, *d_slen = d_srow0 + B, *d_sslot = d_slen + B, *d_spos0 = d_sslot + B;
    float *x = c->px.as<float>();
    uint16_t *xh = c->pxh.as<uint16_t>();
    const bool q8 = m->q8;
    if (q8 && (rc = ensure_q8(c, rows, std::max(H, std::max(QD, F)), std::max(H, std::max(QD, F))))) return rc;
    float *x32 = q8 ? c->x32.as<float>() : nullptr;
    launch_embed(c->pids.as<int32_t>(), rows, m->embd, H, d_feats, d_aud, x, s);
    const size_t layer_kv = (size_t)c->max_batch * hp.n_kv_head * c->max_ctx * 128;
    for (int l = 0; l < hp.dec_layers; l++) {
        const DecLayer &L = m->dec[l];
        launch_rmsnorm_f16(x, H, nullptr, rows, H, L.attn_norm, hp.rms_eps, xh, s, x32);
        GemmArgs q{};
        q.M = rows; q.N = QD + 2 * KD; q.K = H; q.out_f32 = c->pqkv.as<float>(); q.ldo = QD + 2 * KD;
        linear(c, EPI_F32, q, x32, xh, H, L.wqkv, L.wqkv_d, s);
        QkvPostArgs qa{};
        qa.qkv = c->pqkv.as<float>(); qa.rows = rows; qa.row_seq = d_seq; qa.row_pos = d_pos;
        qa.q_norm = L.q_norm; qa.k_norm = L.k_norm; qa.eps = hp.rms_eps; qa.rope = c->rope;
        qa.n_head = hp.n_head; qa.n_kv_head = hp.n_kv_head; qa.q_out = c->pq.as<uint16_t>();
        qa.kc = c->kc + l * layer_kv; qa.vc = c->vc + l * layer_kv; qa.max_ctx = c->max_ctx;
        qa.vt = c->vt + l * layer_vt(c);
        if (al) { qa.q32 = c->pq32.as<float>(); qa.k32 = c->pk32.as<float>(); }
        launch_qkv_post(qa, s);
        PrefillAttnArgs pa{};
        pa.q = c->pq.as<uint16_t>(); pa.kc = qa.kc; pa.vc = qa.vc; pa.seq_row0 = d_srow0; pa.seq_len = d_slen;
        pa.seq_slot = d_sslot; pa.n_seq = B; pa.max_len = maxp; pa.n_head = hp.n_head; pa.n_kv_head = hp.n_kv_head;
        pa.max_ctx = c->max_ctx; pa.scale = 1.0f / sqrtf(128.0f); pa.out = c->patt.as<uint16_t>(); pa.out32 = x32;
        if (al) { pa.q32 = qa.q32; pa.k32 = qa.k32; }
        if (pos0) pa.seq_pos0 = d_spos0;
        if (c->fuse.fa_exact_prefill || al) launch_prefill_attention_exact(pa, s);   // ggml CPU FA numerics
        else launch_prefill_attention(pa, s);
        GemmArgs o{};
        o.M = rows; o.N = H; o.K = QD; o.res = x; o.ldr = H; o.out_f32 = x; o.ldo = H;
        linear(c, EPI_F32, o, x32, c->patt.as<uint16_t>(), QD, L.wo, L.wo_d, s);
        launch_rmsnorm_f16(x, H, nullptr, rows, H, L.ffn_norm, hp.rms_eps, xh, s, x32);
        GemmArgs gu{};
        gu.M = rows; gu.N = 2 * F; gu.K = H;
        // Q8_0: SwiGLU in fp32 (the down projection quantises it); x32 is free once quantised
        if (q8) { gu.out_f32 = x32; gu.ldo = F; }
        else { gu.out_f16 = c->pact.as<uint16_t>(); gu.ldo16 = F; }
        linear(c, q8 ? EPI_SWIGLU_F32 : EPI_SWIGLU_F16, gu, x32, xh, H, L.wgu, L.wgu_d, s);
        GemmArgs dn{};
        dn.M = rows; dn.N = H; dn.K = F; dn.res = x; dn.ldr = H; dn.out_f32 = x; dn.ldo = H;
        linear(c, EPI_F32, dn, x32, c->pact.as<uint16_t>(), F, L.wd, L.wd_d, s);
    }
    return declined_check("prefill");
}

// prefill (src/text_decoder.cpp:588-684): layers, then the LAST row of each
// sequence -> RMSNorm -> tied LM head + argmax (:564-572)
// slots: the KV-cache slot of each sequence (nullptr: sequence b -> slot b);
// the decode state (d_tok / d_pos / d_nkv) is written for entries 0..B-1
int qasr::eng::run_prefill(qasr_ctx *c, const std::vector<int32_t> &ids, const std::vector<int> &P, const float *d_feats,
                           const std::vector<int> &audio_pos, const std::vector<int> &N, bool want_logits,
                           const std::vector<int> *slots, const std::vector<int> *pos0) {
    int rc;
    if ((rc = prefill_layers(c, ids, P, d_feats, audio_pos, N, slots, pos0))) return rc;
    // granule tags repeat across runs at the same positions: back to zero (no valid tag)
    if ((rc = reset_granules(c))) return rc;
    qasr_model *m = c->m;
    const Hparams &hp = m->hp;
    const int B = (int)P.size(), H = hp.hidden;
    hipStream_t s = c->st;
    float *x = c->px.as<float>();
    uint16_t *xl = c->d_xh;
    launch_rmsnorm_f16(x, H, c->plast.as<int>(), B, H, m->out_norm, hp.rms_eps, xl, s);
    launch_fill_u64(c->d_amax, B, 0ull, s);
    const bool lp = c->fuse.token_logprobs != 0;   // the log-probabilities come from the fp32 logits
    const bool smp = sampling_on(c);   // sampling: the draw and its log-probability read them too
    const bool con = constraints_on(c);   // decoding constraints: the stage edits them and chooses again
    want_logits = want_logits || lp || step_k(c) > 0 || smp || con;   // (option top_k or a beam run: the alternatives likewise)
    if (B <= 8) {
        GemvArgs gv{};
        gv.xh = xl; gv.ldxh = H; gv.W = m->embd; gv.K = H; gv.N = hp.vocab; gv.M = B;
        gv.out_f32 = want_logits ? c->d_logits : nullptr; gv.ldo = hp.vocab; gv.amax = c->d_amax;
        launch_gemv(EPI_ARGMAX, gv, s);
    } else {
        GemmArgs lm{};
        lm.A = xl; lm.lda = H; lm.W = m->embd; lm.ldw = H; lm.M = B; lm.N = hp.vocab; lm.K = H;
        lm.out_f32 = want_logits ? c->d_logits : nullptr; lm.ldo = hp.vocab; lm.amax = c->d_amax;
        launch_gemm_c(c, AM_DENSE, EPI_ARGMAX, lm, s);
    }
    HIPCHK(hipMemsetAsync(c->d_step, 0, 4, s));
    launch_argmax_finish(c->d_amax, B, c->d_tok, c->d_hist, c->hist_cap, c->d_step, s);
    // constraints: token 0 from the edited rows (an empty history: the bias list alone can act), before anything reads them
    c->stage_t = 0;
    if (con && (rc = constrain_step(c, B * sample_mul(c), sample_mul(c)))) return rc;
    if (lp && !smp) launch_token_logprob(c->d_logits, hp.vocab, B, 0, c->d_tok, c->d_step, c->d_lp, c->d_lphist, c->hist_cap, s);
    if ((rc = topk_step(c, B))) return rc;
    launch_fill_u64(c->d_amax, B, 0ull, s);   // zero at rest for the decode graph
    // sampling: token t = 0 of every hypothesis from the prefill's logits (an n_best run: n_best rows a clip from its one row)
    if (smp && (rc = sample_step(c, B * sample_mul(c), sample_mul(c)))) return rc;
    // decode state: next position = P_b, n_kv = P_b + 1 (the fed token's own key included)
    std::vector<int> pos(B), nkv(B);
    for (int b = 0; b < B; b++) {
        pos[b] = (pos0 ? (*pos0)[b] : 0) + P[b];
        nkv[b] = pos[b] + 1;
    }
    HIPCHK(hipMemcpyAsync(c->d_pos, pos.data(), B * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_nkv, nkv.data(), B * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // pos/nkv host vectors go out of scope
    HIPCHK(hipGetLastError());
    return declined_check("prefill LM head");
}

// ====================================================== stage entry points
extern "C" int qasr_mel(qasr_ctx *c, const float *const *pcm, const int *n, int B, float *mel_out) {
    if (!c || !pcm || !n || B <= 0 || !mel_out) return fail(QASR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    std::vector<long> off;
    std::vector<int> nn(n, n + B);
    for (int b = 0; b < B; b++)
        if (n[b] < 0) return fail(QASR_ERR_ARG, "negative length");
    int rc = pack_pcm(c, pcm, n, B, off);
    if (rc) return rc;
    std::vector<long> mo;
    std::vector<int> T;
    if ((rc = run_mel(c, off, nn, mo, T))) return rc;
    long total = 0;
    for (int b = 0; b < B; b++) total += 128L * T[b];
    if (total) HIPCHK(hipMemcpyAsync(mel_out, c->mel.p, total * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// ---------------------------------------------------- standalone log-mel
// log_mel_spectrogram of the component API (include/mel_spectrogram.h,
// src/mel_spectrogram.h:53-55) takes no model: an engine holds the DFT /
// window tables and a filterbank on one device and runs the same mel kernels
// as a context (launch_mel, csrc/mel.hip).
struct qasr_mel_engine {
    int device = 0;
    hipStream_t st = nullptr;
    double2 *tw = nullptr;
    double *hann = nullptr;
    float *filt = nullptr;        // [128][201], the last filterbank run with
    std::vector<float> filt_host; // ... its host copy (re-uploaded when a call brings other values)
    float *pcm = nullptr, *out = nullptr;
    double *tmp = nullptr;
    unsigned long long *cmax = nullptr;
    MelClip *clip = nullptr;
    int2 *blocks = nullptr;
    size_t pcm_cap = 0, out_cap = 0, tmp_cap = 0, blk_cap = 0;
    ~qasr_mel_engine() {
        (void)hipSetDevice(device);
        for (void *p : {(void *)tw, (void *)hann, (void *)filt, (void *)pcm, (void *)out, (void *)tmp, (void *)cmax, (void *)clip,
                        (void *)blocks})
            if (p) (void)hipFree(p);
        if (st) (void)hipStreamDestroy(st);
    }
};

static int grow(void **p, size_t &cap, size_t bytes) {
    if (bytes <= cap && *p) return 0;
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
    cap = std::max<size_t>(bytes + bytes / 4, 4096);
    HIPCHK(hipMalloc(p, cap));
    return 0;
}

extern "C" int qasr_mel_filters(float *out) {
    if (!out) return fail(QASR_ERR_ARG, "bad arguments");
    std::vector<float> f;
    mel_filters(f);
    memcpy(out, f.data(), f.size() * 4);
    return 0;
}

extern "C" int qasr_mel_engine_create(int device, qasr_mel_engine **out) {
    if (!out) return fail(QASR_ERR_ARG, "bad arguments");
    *out = nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return fail(QASR_ERR_DEVICE, "no such HIP device");
    std::unique_ptr<qasr_mel_engine> e(new qasr_mel_engine());
    e->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking));
    std::vector<double> tw, hn;
    dft_twiddles(tw);
    hann_window(hn);
    mel_filters(e->filt_host);
    HIPCHK(hipMalloc((void **)&e->tw, tw.size() * 8));
    HIPCHK(hipMalloc((void **)&e->hann, hn.size() * 8));
    HIPCHK(hipMalloc((void **)&e->filt, e->filt_host.size() * 4));
    HIPCHK(hipMalloc((void **)&e->cmax, 8));
    HIPCHK(hipMalloc((void **)&e->clip, sizeof(MelClip)));
    HIPCHK(hipMemcpy(e->tw, tw.data(), tw.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->hann, hn.data(), hn.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->filt, e->filt_host.data(), e->filt_host.size() * 4, hipMemcpyHostToDevice));
    *out = e.release();
    return 0;
}

extern "C" void qasr_mel_engine_free(qasr_mel_engine *e) { delete e; }

extern "C" int qasr_mel_engine_run(qasr_mel_engine *e, const float *pcm, int n, const float *filters, float *mel_out) {
    if (!e || n < 0 || (n > 0 && !pcm) || (mel_frames(n) > 0 && !mel_out)) return fail(QASR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(e->device));
    const int TF = n / 160 + 1, T = TF - 1;
    if (filters && memcmp(filters, e->filt_host.data(), e->filt_host.size() * 4) != 0) {
        memcpy(e->filt_host.data(), filters, e->filt_host.size() * 4);
        HIPCHK(hipMemcpyAsync(e->filt, e->filt_host.data(), e->filt_host.size() * 4, hipMemcpyHostToDevice, e->st));
    }
    std::vector<int2> blocks;
    for (int f = 0; f < TF; f += mel_frames_per_block()) blocks.push_back(make_int2(0, f));
    const MelClip clip{0, n, TF, 0, 0};
    int rc;
    if ((rc = grow((void **)&e->pcm, e->pcm_cap, std::max<size_t>((size_t)n, 1) * 4)) ||
        (rc = grow((void **)&e->tmp, e->tmp_cap, (size_t)128 * TF * 8)) ||
        (rc = grow((void **)&e->out, e->out_cap, std::max<size_t>((size_t)128 * T, 1) * 4)) ||
        (rc = grow((void **)&e->blocks, e->blk_cap, blocks.size() * sizeof(int2))))
        return rc;
    if (n) HIPCHK(hipMemcpyAsync(e->pcm, pcm, (size_t)n * 4, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->clip, &clip, sizeof clip, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->blocks, blocks.data(), blocks.size() * sizeof(int2), hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(e->cmax, 0, 8, e->st));
    launch_mel(e->pcm, e->clip, 1, e->blocks, (int)blocks.size(), e->tw, e->hann, e->filt, e->tmp, e->cmax, e->out, e->st);
    HIPCHK(hipGetLastError());
    if (T > 0) HIPCHK(hipMemcpyAsync(mel_out, e->out, (size_t)128 * T * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));   // (the host vectors above go out of scope)
    return 0;
}

static int encode_common(qasr_ctx *c, const float *mel, const int *T, int B, float *outp, bool conv_only, bool no_chunk = false) {
    if (!c || !mel || !T || B <= 0 || !outp) return fail(QASR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    std::vector<int> Tv(T, T + B);
    std::vector<long> mo(B);
    long tot = 0;
    for (int b = 0; b < B; b++) { if (T[b] < 0) return fail(QASR_ERR_ARG, "negative length"); mo[b] = tot; tot += 128L * T[b]; }
    int rc = ensure(c, c->mel, std::max<long>(tot, 1) * 4);
    if (rc) return rc;
    if (tot) HIPCHK(hipMemcpyAsync(c->mel.p, mel, tot * 4, hipMemcpyHostToDevice, c->st));
    std::vector<int> Nb;
    if ((rc = run_encoder(c, c->mel.as<float>(), mo, Tv, conv_only, Nb, no_chunk))) return rc;
    long N = 0;
    for (int v : Nb) N += v;
    const int width = conv_only ? c->m->hp.d_model : c->m->hp.hidden;
    if (N) HIPCHK(hipMemcpyAsync(outp, conv_only ? c->ex.p : c->feats.p, (size_t)N * width * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

extern "C" int qasr_encode(qasr_ctx *c, const float *mel, const int *T, int B, float *feats) {
    return encode_common(c, mel, T, B, feats, false);
}
extern "C" int qasr_encode_conv(qasr_ctx *c, const float *mel, const int *T, int B, float *out) {
    return encode_common(c, mel, T, B, out, true);
}
extern "C" int qasr_encode_no_chunk(qasr_ctx *c, const float *mel, const int *T, int B, float *feats) {
    return encode_common(c, mel, T, B, feats, false, true);
}
extern "C" int qasr_encoder_frames_no_chunk(int n_mel_frames) {
    int L = n_mel_frames;
    if (L <= 0) return 0;
    for (int i = 0; i < 3; i++) L = (L - 1) / 2 + 1;   // src/audio_encoder.cpp:304-310 over the whole length
    return L;
}

// TextDecoder::forward with n_tokens > 1 at n_past > 0 (src/text_decoder.cpp:
// 392-581 builds one graph for the chunk): the chunk's rows through the
// prefill layers at positions n_past[b] .. n_past[b] + P[b] - 1, causal
// attention over the cached keys and the chunk's own; logits of each chunk's
// last row.  n_past[b] = 0 is the plain prefill.  With feats: forward_with_audio
// at any n_past (src/text_decoder.cpp:588-644, the splice of :431-459) -- rows
// [audio_pos[b], audio_pos[b] + N[b]) of the chunk take the audio embeddings
// when they fit inside it, as the reference's condition.
// n_past == nullptr is qasr_prefill: every sequence from position 0, with the
// plain prefill's attention arguments (no seq_pos0) and its laxer argument rules.
// slots (qasr_prefill_slots): sequence b's KV-cache slot; nullptr = slot b
int qasr::eng::prefill_chunk_common(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, const float *feats,
                                    const int *audio_pos, const int *N, int B, float *logits_last, int32_t *argmax,
                                    const int *slots) {
    if (!c || !ids || !P || B <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    if (n_past) {
        if (feats && (!N || !audio_pos)) return fail(QASR_ERR_ARG, "audio features need N and audio_pos");
        for (int b = 0; b < B; b++)
            if (P[b] < 0 || n_past[b] < 0 || (feats && N[b] < 0)) return fail(QASR_ERR_ARG, "negative P / n_past / N");
    }
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    const int H = c->m->hp.hidden;
    std::vector<int> Pv(P, P + B), Nv(B, 0), ap(B, -1), p0;
    if (n_past) p0.assign(n_past, n_past + B);
    long nid = 0, nf = 0;
    for (int b = 0; b < B; b++) {
        nid += P[b];
        if (feats && N) { Nv[b] = N[b]; nf += N[b]; }
        if (audio_pos) ap[b] = audio_pos[b];
    }
    for (long i = 0; i < nid; i++)
        if (ids[i] < 0 || ids[i] >= c->m->hp.vocab) return fail(QASR_ERR_ARG, "token id out of range");
    std::vector<int32_t> idv(ids, ids + nid);
    std::vector<int> sl;
    if (slots) sl.assign(slots, slots + B);   // (prefill_layers checks their range)
    int rc;
    if (nf) {
        if ((rc = ensure(c, c->feats, (size_t)nf * H * 4))) return rc;
        HIPCHK(hipMemcpyAsync(c->feats.p, feats, (size_t)nf * H * 4, hipMemcpyHostToDevice, c->st));
    }
    if ((rc = run_prefill(c, idv, Pv, nf ? c->feats.as<float>() : nullptr, ap, Nv, logits_last != nullptr, slots ? &sl : nullptr,
                          n_past ? &p0 : nullptr)))
        return rc;
    if (logits_last) HIPCHK(hipMemcpyAsync(logits_last, c->d_logits, (size_t)B * c->m->hp.vocab * 4, hipMemcpyDeviceToHost, c->st));
    if (argmax) HIPCHK(hipMemcpyAsync(argmax, c->d_tok, B * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->lp_step_B = c->fuse.token_logprobs ? B : 0;
    c->tk_step_B = c->fuse.top_k ? B : 0;
    return 0;
}

extern "C" int qasr_prefill(qasr_ctx *c, const int32_t *ids, const int *P, const float *feats, const int *audio_pos,
                            const int *N, int B, float *logits_last, int32_t *argmax) {
    return prefill_chunk_common(c, ids, P, nullptr, feats, audio_pos, N, B, logits_last, argmax);
}

extern "C" int qasr_prefill_slots(qasr_ctx *c, const int32_t *ids, const int *P, const float *feats, const int *audio_pos,
                                  const int *N, const int *slots, int B, float *logits_last, int32_t *argmax) {
    if (!slots) return fail(QASR_ERR_ARG, "bad arguments");
    return prefill_chunk_common(c, ids, P, nullptr, feats, audio_pos, N, B, logits_last, argmax, slots);
}

extern "C" int qasr_prefill_chunk(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, int B, float *logits_last,
                                  int32_t *argmax) {
    if (!n_past) return fail(QASR_ERR_ARG, "bad arguments");
    return prefill_chunk_common(c, ids, P, n_past, nullptr, nullptr, nullptr, B, logits_last, argmax);
}

extern "C" int qasr_prefill_chunk_audio(qasr_ctx *c, const int32_t *ids, const int *P, const int *n_past, const float *feats,
                                        const int *audio_pos, const int *N, int B, float *logits_last, int32_t *argmax) {
    if (!n_past) return fail(QASR_ERR_ARG, "bad arguments");
    return prefill_chunk_common(c, ids, P, n_past, feats, audio_pos, N, B, logits_last, argmax);
}
