// kernel_harness.hip -- test-only C entry points (include/qasr_capi.h, "test
// only"): one GEMM / GEMV / quantisation launcher of kernels.h on arrays the
// caller supplies, so tests/test_gpu_kernels.py can hold every tile, tiling and
// epilogue to a float64 reference without a model; likewise the norm, RoPE and
// prefill / encoder attention launchers for tests/test_gpu_attn_kernels.py, and
// the decode attention launchers that do not wait in-launch for
// tests/test_gpu_decode_attn_kernels.py, and the conv front end (launch_conv1,
// launch_gemm in AM_CONV2 / AM_CONV3) for tests/test_gpu_conv_kernels.py.
//
// What a kernel may not touch is made visible: inputs carry `guard` rows of
// 0xFF bytes (NaN) after their last row (0x7F for int8 quants; the conv entry's
// input: before its first row too, where a mis-bounded tap lands), outputs are
// allocated with `guard` rows on both sides and every byte 0xFF before the
// launch, and come back whole.  A launcher that takes no kernel is reported
// as declined, never as success.
#include "engine_impl.h"
#include "phrase_host.h"

using namespace qasr;
using qasr::eng::fail;

namespace {

struct KtBuf {
    char *d = nullptr;
    size_t bytes = 0, off = 0;   // off: byte offset of the first real row
    ~KtBuf() {
        if (d) (void)hipFree(d);
    }
    template <class T>
    T *ptr() const { return d ? (T *)(d + off) : nullptr; }
};

// input: rows x ld elements of esz bytes from host, then guard rows of `fill` bytes
int put_in(KtBuf &b, const void *host, long rows, long ld, int esz, int guard, int fill) {
    if (!host) return 0;
    const size_t real = (size_t)rows * ld * esz;
    b.bytes = real + (size_t)guard * ld * esz + 256;
    HIPCHK(hipMalloc((void **)&b.d, b.bytes));
    HIPCHK(hipMemset(b.d, fill, b.bytes));
    if (real) HIPCHK(hipMemcpy(b.d, host, real, hipMemcpyHostToDevice));
    return 0;
}

// output: guard + rows + guard rows of ld elements, every byte 0xFF
int put_out(KtBuf &b, const void *host, long rows, long ld, int esz, int guard) {
    if (!host) return 0;
    b.bytes = (size_t)(rows + 2 * guard) * ld * esz;
    b.off = (size_t)guard * ld * esz;
    HIPCHK(hipMalloc((void **)&b.d, b.bytes));
    HIPCHK(hipMemset(b.d, 0xFF, b.bytes));
    return 0;
}

// in / out state (no guards): host -> device
int put_state(KtBuf &b, const void *host, size_t bytes) {
    if (!host) return 0;
    b.bytes = bytes;
    HIPCHK(hipMalloc((void **)&b.d, bytes));
    HIPCHK(hipMemcpy(b.d, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

int get(const KtBuf &b, void *host) {
    if (b.d && host) HIPCHK(hipMemcpy(host, b.d, b.bytes, hipMemcpyDeviceToHost));
    return 0;
}

void copy_str(char *dst, size_t cap, const std::string &s) {
    const size_t n = std::min(cap - 1, s.size());
    memcpy(dst, s.data(), n);
    dst[n] = 0;
}

// after the launch(es): synchronise, collect the tag and any declined message
template <class Args>
int finish(Args *a, bool ran) {
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipDeviceSynchronize();
    std::string msg, tag;
    const bool declined = take_declined(&msg);
    const bool tagged = take_kernel(&tag);
    if (le != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(le));
    if (se != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("kernel run: ") + hipGetErrorString(se));
    a->declined = declined || !ran;
    if (a->declined && msg.empty()) msg = "the launcher returned false";
    if (!a->declined && !tagged) return fail(QASR_ERR_STATE, "the launcher recorded no kernel tag");
    copy_str(a->tag, sizeof a->tag, a->declined ? std::string() : tag);
    copy_str(a->msg, sizeof a->msg, msg);
    return 0;
}

int use_device(int device) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return fail(QASR_ERR_DEVICE, "no such HIP device");
    HIPCHK(hipSetDevice(device));
    (void)take_declined(nullptr);
    (void)take_kernel(nullptr);
    return 0;
}

}  // namespace

extern "C" int qasr_kt_gemm(int device, qasr_kt_gemm_args *a) {
    if (!a || a->M <= 0 || a->N <= 0 || a->K <= 0 || a->guard < 0 || a->launcher < 0 || a->launcher > 3)
        return fail(QASR_ERR_ARG, "bad arguments");
    const bool q8 = a->launcher == 1 || a->launcher == 3;
    if (q8 ? !(a->Aq && a->Ad && a->Wq && a->Wd) : !(a->A && a->W)) return fail(QASR_ERR_ARG, "operands missing");
    if (a->lda < a->K || a->ldw < a->K || (q8 && a->ldad < a->K / 32) || (a->pe && (!a->pe_pos || a->pe_rows <= 0)))
        return fail(QASR_ERR_ARG, "leading dimensions smaller than the rows");
    int rc = use_device(device);
    if (rc) return rc;
    const int M = a->M, N = a->N, K = a->K, G = a->guard;
    KtBuf A, W, Aq, Ad, Wq, Wd, bias, res, pe, pe_pos, gelu, o32, o16, oq, od, amax;
    if ((rc = put_in(A, a->A, M, a->lda, 2, G, 0xFF)) || (rc = put_in(W, a->W, N, a->ldw, 2, G, 0xFF)) ||
        (rc = put_in(Aq, a->Aq, M, a->lda, 1, G, 0x7F)) || (rc = put_in(Ad, a->Ad, M, a->ldad, 4, G, 0xFF)) ||
        (rc = put_in(Wq, a->Wq, N, a->ldw, 1, G, 0x7F)) || (rc = put_in(Wd, a->Wd, N, K / 32, 2, G, 0xFF)) ||
        (rc = put_in(bias, a->bias, 1, N, 4, 1, 0xFF)) || (rc = put_in(res, a->res, M, a->ldr, 4, G, 0xFF)) ||
        (rc = put_in(pe, a->pe, a->pe_rows, N, 4, 1, 0xFF)) || (rc = put_in(pe_pos, a->pe_pos, 1, M, 4, 0, 0)) ||
        (rc = put_out(o32, a->out_f32, M, a->ldo, 4, G)) || (rc = put_out(o16, a->out_f16, M, a->ldo16, 2, G)) ||
        (rc = put_out(oq, a->out_q, M, a->ldoq, 1, G)) || (rc = put_out(od, a->out_d, M, a->ldoq / 32, 4, G)) ||
        (rc = put_out(amax, a->amax, M, 1, 8, G)))
        return rc;
    if (amax.d) HIPCHK(hipMemset(amax.ptr<char>(), 0, (size_t)M * 8));
    std::vector<uint16_t> lut;
    gelu_table(lut);
    if ((rc = put_in(gelu, lut.data(), 1, 65536, 2, 0, 0))) return rc;
    if (a->gelu_out) memcpy(a->gelu_out, lut.data(), 65536 * 2);

    GemmArgs g{};
    g.A = A.ptr<uint16_t>(); g.lda = a->lda;
    g.W = W.ptr<uint16_t>(); g.ldw = a->ldw;
    g.M = M; g.N = N; g.K = K;
    g.bias = bias.ptr<float>();
    g.res = res.ptr<float>(); g.ldr = a->ldr;
    g.out_f32 = o32.ptr<float>(); g.ldo = a->ldo;
    g.out_f16 = o16.ptr<uint16_t>(); g.ldo16 = a->ldo16;
    g.gelu = gelu.ptr<uint16_t>();
    g.pe = pe.ptr<float>(); g.pe_pos = pe_pos.ptr<int>();
    g.amax = amax.ptr<unsigned long long>();
    g.n_valid = a->n_valid;
    g.Aq = Aq.ptr<int8_t>(); g.Ad = Ad.ptr<float>(); g.ldad = a->ldad;
    g.Wq = Wq.ptr<int8_t>(); g.Wd = Wd.ptr<uint16_t>();
    g.regs_staged = a->regs_staged;
    g.skinny_inflight = a->skinny_inflight;
    g.out_q = oq.ptr<int8_t>(); g.out_d = od.ptr<float>(); g.ldoq = a->ldoq;
    g.wdef = a->wdef;

    bool ran = true;
    switch (a->launcher) {
        case 0: launch_gemm(AM_DENSE, a->epi, g, nullptr); break;
        case 1: launch_gemm_q8(a->epi, g, nullptr); break;
        case 2: ran = launch_gemm_skinny(a->epi, g, nullptr); break;
        default: ran = launch_gemm_skinny_q8(a->epi, g, nullptr); break;
    }
    if ((rc = finish(a, ran))) return rc;
    if ((rc = get(o32, a->out_f32)) || (rc = get(o16, a->out_f16)) || (rc = get(oq, a->out_q)) || (rc = get(od, a->out_d)) ||
        (rc = get(amax, a->amax)))
        return rc;
    return 0;
}

extern "C" int qasr_kt_gemv(int device, qasr_kt_gemv_args *a) {
    if (!a || a->M <= 0 || a->N <= 0 || a->K <= 0 || a->guard < 0 || a->launches < 1 || a->wrows < a->N)
        return fail(QASR_ERR_ARG, "bad arguments");
    if (!(a->Wq ? a->Wd != nullptr : a->W != nullptr) || !(a->x || a->xh || (a->embd_ids && a->embd)))
        return fail(QASR_ERR_ARG, "operands missing");
    const bool book = a->done || a->tok_out || a->hist || a->step || a->pos;
    if (book && !(a->done && a->tok_out && a->hist && a->step && a->pos && a->amax && a->hist_stride > 0))
        return fail(QASR_ERR_ARG, "the bookkeeping group is all or none");
    int rc = use_device(device);
    if (rc) return rc;
    const int M = a->M, N = a->N, K = a->K, G = a->guard;
    KtBuf x, xh, nw, W, Wq, Wd, bias, res, ids, embd, xs, o32, o16, amax, done, tok, hist, step, pos;
    if ((rc = put_in(x, a->x, M, a->ldx, 4, G, 0xFF)) || (rc = put_in(xh, a->xh, M, a->ldxh, 2, G, 0xFF)) ||
        (rc = put_in(nw, a->norm_w, 1, K, 4, 1, 0xFF)) || (rc = put_in(W, a->W, a->wrows, K, 2, G, 0xFF)) ||
        (rc = put_in(Wq, a->Wq, a->wrows, K, 1, G, 0x7F)) || (rc = put_in(Wd, a->Wd, a->wrows, K / 32, 2, G, 0xFF)) ||
        (rc = put_in(bias, a->bias, 1, N, 4, 1, 0xFF)) || (rc = put_in(res, a->res, M, a->ldr, 4, G, 0xFF)) ||
        (rc = put_in(ids, a->embd_ids, 1, M, 4, 0, 0)) || (rc = put_in(embd, a->embd, a->embd_rows, K, 2, G, 0xFF)) ||
        (rc = put_out(xs, a->x_store, M, a->ldx, 4, G)) || (rc = put_out(o32, a->out_f32, M, a->ldo, 4, G)) ||
        (rc = put_out(o16, a->out_f16, M, a->ldo16, 2, G)) || (rc = put_state(amax, a->amax, 8 * 8)) ||
        (rc = put_state(done, a->done, 4)) || (rc = put_state(tok, a->tok_out, 8 * 4)) ||
        (rc = put_state(hist, a->hist, (size_t)M * a->hist_stride * 4)) || (rc = put_state(step, a->step, 4)) ||
        (rc = put_state(pos, a->pos, 8 * 4)))
        return rc;

    GemvArgs g{};
    g.x = x.ptr<float>(); g.ldx = a->ldx;
    g.xh = xh.ptr<uint16_t>(); g.ldxh = a->ldxh;
    g.norm_w = nw.ptr<float>(); g.eps = a->eps;
    g.W = a->Wq ? (const uint16_t *)Wq.ptr<int8_t>() : W.ptr<uint16_t>();
    g.K = K; g.N = N; g.M = M;
    g.Wd = Wd.ptr<uint16_t>();
    g.bias = bias.ptr<float>();
    g.res = res.ptr<float>(); g.ldr = a->ldr;
    g.out_f32 = o32.ptr<float>(); g.ldo = a->ldo;
    g.out_f16 = o16.ptr<uint16_t>(); g.ldo16 = a->ldo16;
    g.amax = amax.ptr<unsigned long long>();
    g.embd_ids = ids.ptr<int32_t>(); g.embd = embd.ptr<uint16_t>(); g.x_store = xs.ptr<float>();
    g.done = done.ptr<unsigned int>(); g.tok_out = tok.ptr<int32_t>(); g.hist = hist.ptr<int32_t>();
    g.hist_stride = a->hist_stride; g.step = step.ptr<int>(); g.pos = pos.ptr<int>();

    for (int i = 0; i < a->launches; i++) {
        launch_gemv(a->epi, g, nullptr);
        if (i + 1 < a->launches) HIPCHK(hipDeviceSynchronize());
    }
    if ((rc = finish(a, true))) return rc;
    if ((rc = get(xs, a->x_store)) || (rc = get(o32, a->out_f32)) || (rc = get(o16, a->out_f16)) || (rc = get(amax, a->amax)) ||
        (rc = get(done, a->done)) || (rc = get(tok, a->tok_out)) || (rc = get(hist, a->hist)) || (rc = get(step, a->step)) ||
        (rc = get(pos, a->pos)))
        return rc;
    return 0;
}

extern "C" int qasr_kt_quantize_q8(int device, qasr_kt_quant_args *a) {
    if (!a || a->M <= 0 || a->K <= 0 || a->K % 32 != 0 || a->guard < 0 || !a->q || !a->d || !a->x32 == !a->x16 || a->gather_C < 0)
        return fail(QASR_ERR_ARG, "bad arguments");
    // the widest column a row reads: K - 1, or (15, K / 16 - 1) of the gathered [h][c] order
    const long last = a->gather_C > 0 ? 15L * a->gather_C + (a->K / 16 - 1) : a->K - 1;
    if (a->ldx <= last) return fail(QASR_ERR_ARG, "ldx smaller than the rows read");
    int rc = use_device(device);
    if (rc) return rc;
    KtBuf x32, x16, q, d;
    if ((rc = put_in(x32, a->x32, a->M, a->ldx, 4, a->guard, 0xFF)) || (rc = put_in(x16, a->x16, a->M, a->ldx, 2, a->guard, 0xFF)) ||
        (rc = put_out(q, a->q, a->M, a->K, 1, a->guard)) || (rc = put_out(d, a->d, a->M, a->K / 32, 4, a->guard)))
        return rc;
    launch_quantize_q8(x32.ptr<float>(), x16.ptr<uint16_t>(), a->ldx, a->M, a->K, a->gather_C, q.ptr<int8_t>(), d.ptr<float>(), nullptr);
    const hipError_t le = hipGetLastError(), se = hipDeviceSynchronize();
    if (le != hipSuccess || se != hipSuccess)
        return fail(QASR_ERR_DEVICE, std::string("launch_quantize_q8: ") + hipGetErrorString(le != hipSuccess ? le : se));
    if ((rc = get(q, a->q)) || (rc = get(d, a->d))) return rc;
    return 0;
}

// ------------------------------------------------------------- beam search
namespace {
// an in / out array between two 4 KiB fences of 0xFF bytes the launch must leave alone
struct KtFenced {
    static constexpr size_t kFence = 4096;
    KtBuf b;
    size_t bytes = 0;
    int put(const void *host, size_t n) {
        bytes = n;
        b.bytes = n + 2 * kFence;
        b.off = kFence;
        HIPCHK(hipMalloc((void **)&b.d, b.bytes));
        HIPCHK(hipMemset(b.d, 0xFF, b.bytes));
        HIPCHK(hipMemcpy(b.d + kFence, host, n, hipMemcpyHostToDevice));
        return 0;
    }
    int take(void *host, const char *name) {
        std::vector<unsigned char> all(b.bytes);
        HIPCHK(hipMemcpy(all.data(), b.d, b.bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kFence; i++)
            if (all[i] != 0xFF || all[kFence + bytes + i] != 0xFF) return fail(QASR_ERR_STATE, std::string("a write outside ") + name);
        memcpy(host, all.data() + kFence, bytes);
        return 0;
    }
};

int finish_plain(int32_t *declined, bool ran) {
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipDeviceSynchronize();
    if (le != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(le));
    if (se != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("kernel run: ") + hipGetErrorString(se));
    *declined = ran ? 0 : 1;
    return 0;
}
}  // namespace

extern "C" int qasr_kt_kv_fork(int device, qasr_kt_kv_fork_args *a) {
    if (!a || !a->kc || !a->vc || !a->vt || !a->parent || !a->from || !a->to || a->layers <= 0 || a->n_kv_head <= 0 || a->max_ctx <= 0 ||
        a->slots <= 0 || a->guard < 0 || a->B <= 0 || a->B > a->slots || a->blocks < 0)
        return fail(QASR_ERR_ARG, "bad arguments");
    // (the kernel clamps ranges to [0, max_ctx] and follows no parent outside a row's group; B <= slots keeps every row inside)
    int rc = use_device(device);
    if (rc) return rc;
    const size_t S = (size_t)a->slots + a->guard;
    const size_t kv = (size_t)a->layers * S * a->n_kv_head * a->max_ctx * 128 * 2, vt = (size_t)a->layers * S * a->n_kv_head * 128 * vt_ctx(a->max_ctx) * 2;
    KtFenced kc, vc, vtb;
    KtBuf par, frm, to;
    if ((rc = kc.put(a->kc, kv)) || (rc = vc.put(a->vc, kv)) || (rc = vtb.put(a->vt, vt)) || (rc = put_state(par, a->parent, (size_t)a->B * 4)) ||
        (rc = put_state(frm, a->from, (size_t)a->B * 4)) || (rc = put_state(to, a->to, (size_t)a->B * 4)))
        return rc;
    KvForkArgs f{};
    f.kc = kc.b.ptr<uint16_t>(); f.vc = vc.b.ptr<uint16_t>(); f.vt = vtb.b.ptr<uint16_t>();
    f.layers = a->layers; f.n_kv_head = a->n_kv_head; f.max_ctx = a->max_ctx; f.slots = (int)S;
    f.parent = par.ptr<int>(); f.from = frm.ptr<int>(); f.to = to.ptr<int>();
    f.B = a->B; f.group = a->group; f.blocks = a->blocks ? a->blocks : (a->max_ctx + 7) / 8;
    const bool ran = launch_kv_fork(f, nullptr);
    if ((rc = finish_plain(&a->declined, ran))) return rc;
    if ((rc = kc.take(a->kc, "kc")) || (rc = vc.take(a->vc, "vc")) || (rc = vtb.take(a->vt, "vt"))) return rc;
    return 0;
}

extern "C" int qasr_kt_beam_select(int device, qasr_kt_beam_select_args *a) {
    if (!a || a->W < 2 || a->W > QASR_BEAM_MAX || a->G <= 0 || a->t < 0 || a->guard < 0 || !a->ids || !a->lps || !a->P || !a->cum ||
        !a->fin_row || !a->fin_t || !a->fin_sum || !a->fin_lp || !a->n_fin || !a->done || !a->t_out || !a->tok || !a->parent ||
        !a->from || !a->to || !a->h_par || !a->h_id || !a->h_lp)
        return fail(QASR_ERR_ARG, "bad arguments");
    int rc = use_device(device);
    if (rc) return rc;
    const int R = a->G * a->W, G = a->G;
    std::vector<int> tv(G, a->t);
    KtBuf ids, lps, P, cum, fr, ft, fs, fl, nf, dn, t, tok, par, frm, to, hp, hi, hl, eos;
    if ((rc = put_in(ids, a->ids, R, a->W, 4, a->guard, 0xFF)) || (rc = put_in(lps, a->lps, R, a->W, 4, a->guard, 0xFF)) ||
        (rc = put_state(P, a->P, (size_t)G * 4)) || (rc = put_state(cum, a->cum, (size_t)R * 4)) ||
        (rc = put_state(fr, a->fin_row, (size_t)R * 4)) || (rc = put_state(ft, a->fin_t, (size_t)R * 4)) ||
        (rc = put_state(fs, a->fin_sum, (size_t)R * 4)) || (rc = put_state(fl, a->fin_lp, (size_t)R * 4)) ||
        (rc = put_state(nf, a->n_fin, (size_t)G * 4)) || (rc = put_state(dn, a->done, (size_t)G * 4)) ||
        (rc = put_state(t, tv.data(), (size_t)G * 4)) || (rc = put_state(eos, &a->eos, 4)) || (rc = put_out(tok, a->tok, 1, R, 4, a->guard)) ||
        (rc = put_out(par, a->parent, 1, R, 4, a->guard)) || (rc = put_out(frm, a->from, 1, R, 4, a->guard)) ||
        (rc = put_out(to, a->to, 1, R, 4, a->guard)) || (rc = put_out(hp, a->h_par, 1, R, 4, a->guard)) ||
        (rc = put_out(hi, a->h_id, 1, R, 4, a->guard)) || (rc = put_out(hl, a->h_lp, 1, R, 4, a->guard)))
        return rc;
    BeamSelectArgs s{};
    s.tk_id = ids.ptr<int32_t>(); s.tk_lp = lps.ptr<float>();
    s.cum = cum.ptr<float>(); s.fin_row = fr.ptr<int>(); s.fin_t = ft.ptr<int>(); s.fin_sum = fs.ptr<float>(); s.fin_lp = fl.ptr<float>();
    s.n_fin = nf.ptr<int>(); s.done = dn.ptr<int>(); s.t = t.ptr<int>(); s.P = P.ptr<int>();
    s.tok = tok.ptr<int32_t>(); s.parent = par.ptr<int>(); s.from = frm.ptr<int>(); s.to = to.ptr<int>();
    s.h_par = hp.ptr<int>(); s.h_id = hi.ptr<int32_t>(); s.h_lp = hl.ptr<float>();
    s.hist_stride = R; s.hist_base = a->t;   // the one history slot the buffers hold
    s.W = a->W; s.G = G; s.eos = eos.ptr<int32_t>();
    const bool ran = launch_beam_select(s, nullptr);
    if ((rc = finish_plain(&a->declined, ran))) return rc;
    if ((rc = get(cum, a->cum)) || (rc = get(fr, a->fin_row)) || (rc = get(ft, a->fin_t)) || (rc = get(fs, a->fin_sum)) ||
        (rc = get(fl, a->fin_lp)) || (rc = get(nf, a->n_fin)) || (rc = get(dn, a->done)) || (rc = get(t, a->t_out)) ||
        (rc = get(tok, a->tok)) || (rc = get(par, a->parent)) || (rc = get(frm, a->from)) || (rc = get(to, a->to)) ||
        (rc = get(hp, a->h_par)) || (rc = get(hi, a->h_id)) || (rc = get(hl, a->h_lp)))
        return rc;
    return 0;
}

// --------------------------------------------------------------- score head
extern "C" int qasr_kt_score_head(int device, qasr_kt_score_args *a) {
    if (!a || a->R <= 0 || a->N <= 0 || a->K <= 0 || a->guard < 0 || a->launches < 1 || !a->A || !a->W || !a->target || !a->lp ||
        !a->gid || !a->glp)
        return fail(QASR_ERR_ARG, "bad arguments");
    if (a->lda < a->K || a->ldw < a->K) return fail(QASR_ERR_ARG, "leading dimensions smaller than the rows");
    int rc = use_device(device);
    if (rc) return rc;
    const int R = a->R, G = a->guard;
    KtBuf A, W, tg, lp, gid, glp, scr;
    if ((rc = put_in(A, a->A, R, a->lda, 2, G, 0xFF)) || (rc = put_in(W, a->W, a->N, a->ldw, 2, G, 0xFF)) ||
        (rc = put_in(tg, a->target, R, 1, 4, G, 0xFF)) || (rc = put_out(lp, a->lp, R, 1, 4, G)) ||
        (rc = put_out(gid, a->gid, R, 1, 4, G)) || (rc = put_out(glp, a->glp, R, 1, 4, G)))
        return rc;
    scr.bytes = std::max<size_t>(score_head_scratch(R, a->N), 256);
    HIPCHK(hipMalloc((void **)&scr.d, scr.bytes));
    HIPCHK(hipMemset(scr.d, 0xFF, scr.bytes));
    ScoreHeadArgs s{};
    s.A = A.ptr<uint16_t>(); s.lda = a->lda;
    s.W = W.ptr<uint16_t>(); s.ldw = a->ldw;
    s.R = R; s.N = a->N; s.K = a->K; s.n_valid = a->n_valid;
    s.target = tg.ptr<int32_t>();
    s.lp = lp.ptr<float>(); s.gid = gid.ptr<int32_t>(); s.glp = glp.ptr<float>();
    s.scratch = scr.d;
    s.cols_fast = a->cols_fast;
    bool ran = true;
    for (int i = 0; i < a->launches && ran; i++) {
        ran = launch_score_head(s, nullptr);
        if (ran && i + 1 < a->launches) HIPCHK(hipDeviceSynchronize());
    }
    if ((rc = finish(a, ran))) return rc;
    if ((rc = get(lp, a->lp)) || (rc = get(gid, a->gid)) || (rc = get(glp, a->glp))) return rc;
    return 0;
}

// ------------------------------------------------------------------ sampling
extern "C" int qasr_kt_sample(int device, qasr_kt_sample_args *a) {
    if (!a) return fail(QASR_ERR_ARG, "bad arguments");
    int rc;
    if (a->dump_n > 0) {   // G(u_n) over a range of n
        if (!a->dump || (uint64_t)a->dump_n0 + a->dump_n > (1ull << 23)) return fail(QASR_ERR_ARG, "dump range outside [0, 2^23)");
        if ((rc = use_device(device))) return rc;
        KtBuf d;
        d.bytes = (size_t)a->dump_n * 4;
        HIPCHK(hipMalloc((void **)&d.d, d.bytes));
        HIPCHK(hipMemset(d.d, 0xFF, d.bytes));
        launch_sample_gumbel_dump(a->dump_n0, a->dump_n, d.ptr<float>(), nullptr);
        if ((rc = finish_plain(&a->declined, true))) return rc;
        return get(d, a->dump);
    }
    if (a->R <= 0 || a->ld <= 0 || a->n_valid <= 0 || a->n_valid > a->ld || a->src_div < 1 || a->R % a->src_div != 0 || a->slices < 0 ||
        a->guard < 0 || a->launches < 1 || !a->logits || !a->greedy || !a->clip || !a->sample || !a->t || !a->tok || !a->key || !a->hist ||
        !a->t_out || !a->skey_out)
        return fail(QASR_ERR_ARG, "bad arguments");
    const int R = a->R, RS = R / a->src_div, G = a->guard;
    for (int r = 0; r < RS; r++)
        if (a->greedy[r] < 0 || a->greedy[r] >= a->n_valid) return fail(QASR_ERR_ARG, "greedy id outside [0, n_valid)");
    if ((rc = use_device(device))) return rc;
    KtBuf lg, gr, cl, sm, t, sc, step, tok, key, hist;
    KtFenced skey;
    const SampleScalars scal{a->inv_T, a->cut, (uint32_t)(a->seed & 0xffffffffull), (uint32_t)(a->seed >> 32)};
    const int zero = 0;
    std::vector<unsigned long long> rest(R, 0ull);
    if ((rc = put_in(lg, a->logits, RS, a->ld, 4, G, 0xFF)) || (rc = put_state(gr, a->greedy, (size_t)RS * 4)) ||
        (rc = put_state(cl, a->clip, (size_t)R * 4)) || (rc = put_state(sm, a->sample, (size_t)R * 4)) ||
        (rc = put_state(t, a->t, (size_t)R * 4)) || (rc = put_state(sc, &scal, sizeof scal)) || (rc = put_state(step, &zero, 4)) ||
        (rc = put_out(tok, a->tok, R, 1, 4, G)) || (rc = put_out(key, a->key, R, 1, 4, G)) || (rc = put_out(hist, a->hist, R, 1, 4, G)) ||
        (rc = skey.put(rest.data(), (size_t)R * 8)))
        return rc;
    SampleArgs s{};
    s.logits = lg.ptr<float>(); s.ld = a->ld; s.n_valid = a->n_valid;
    s.greedy = gr.ptr<int32_t>();
    s.clip = cl.ptr<int>(); s.sample = sm.ptr<int>(); s.t = t.ptr<int>();
    s.sc = sc.ptr<SampleScalars>(); s.skey = skey.b.ptr<unsigned long long>();
    s.tok = tok.ptr<int32_t>(); s.hist = hist.ptr<int32_t>(); s.hist_stride = 1; s.step = step.ptr<int>();
    s.key_out = key.ptr<float>();
    s.R = R; s.src_div = a->src_div;
    bool ran = true;
    for (int i = 0; i < a->launches && ran; i++) {
        if (i) HIPCHK(hipMemcpy(t.d, a->t, (size_t)R * 4, hipMemcpyHostToDevice));   // (the same draw again)
        ran = launch_sample(s, a->slices, nullptr);
        if (ran && i + 1 < a->launches) HIPCHK(hipDeviceSynchronize());
    }
    if ((rc = finish(a, ran))) return rc;
    if ((rc = get(tok, a->tok)) || (rc = get(key, a->key)) || (rc = get(hist, a->hist)) || (rc = get(t, a->t_out)) ||
        (rc = skey.take(a->skey_out, "the key scratch")))
        return rc;
    return 0;
}

// ------------------------------------------------------- decoding constraints
// qasr_kt_constrain and qasr_kt_phrases: the same call, the second with a phrase list (compiled here) and the
// per-row record of which path chose the token
namespace {
template <class Args>
int kt_constrain_run(int device, Args *a, const qasr_phrases *ph, int32_t *scanned_out) {
    if (!a) return fail(QASR_ERR_ARG, "bad arguments");
    if (a->R <= 0 || a->ld <= 0 || a->n_valid <= 0 || a->n_valid > a->ld || a->src_div < 1 || a->R % a->src_div != 0 || a->slices < 0 ||
        a->guard < 0 || a->launches < 1 || a->hist_stride < 1 || a->t < 0 || a->t >= a->hist_stride || !a->logits || !a->greedy || !a->hist ||
        !a->tok || !a->hist_slot || !a->logits_out || !a->skey_out || !a->flag_out)
        return fail(QASR_ERR_ARG, "bad arguments");
    const qasr_constraints k{a->no_repeat_ngram, a->repetition_penalty, a->penalty_last_n, a->n_bias, a->bias_ids, a->bias};
    int rc;
    if ((rc = qasr_constraints_validate(&k, a->n_valid))) return rc;
    PhraseTrieHost tr;
    if (ph) {
        if (!scanned_out) return fail(QASR_ERR_ARG, "bad arguments");
        if ((rc = qasr_phrases_validate(ph, a->n_valid))) return rc;
        const std::string err = phrase_compile(ph->n_phrases, ph->ids, ph->len, ph->boost, tr);
        if (!err.empty()) return fail(QASR_ERR_ARG, err);
    }
    const int R = a->R, RS = R / a->src_div, G = a->guard, HS = a->hist_stride;
    for (int r = 0; r < RS; r++)
        if (a->greedy[r] < 0 || a->greedy[r] >= a->n_valid) return fail(QASR_ERR_ARG, "greedy id outside [0, n_valid)");
    for (size_t i = 0; i < (size_t)R * HS; i++)
        if (a->hist[i] < 0 || a->hist[i] >= a->n_valid) return fail(QASR_ERR_ARG, "history id outside [0, n_valid)");
    if ((rc = use_device(device))) return rc;
    KtBuf lg, gr, hs, prm, ids, bias, step, tok, p_hd, p_off, p_tok, p_dst, p_bonus, scanned;
    KtFenced skey, flag;
    const ConstrainParams cp{a->no_repeat_ngram, a->repetition_penalty, 1.0f / a->repetition_penalty, a->penalty_last_n, a->n_bias};
    std::vector<int32_t> idv(QASR_BIAS_MAX, 0);
    std::vector<float> bv(QASR_BIAS_MAX, 0.f);
    std::copy(a->bias_ids, a->bias_ids + a->n_bias, idv.begin());
    std::copy(a->bias, a->bias + a->n_bias, bv.begin());
    const std::vector<unsigned long long> rest(RS, 0ull);
    const std::vector<int> rest_flag(RS, 0);
    const size_t row_bytes = (size_t)a->ld * 4, hist_bytes = (size_t)R * HS * 4;
    if ((rc = put_out(lg, a->logits_out, RS, a->ld, 4, G)) || (rc = put_state(gr, a->greedy, (size_t)RS * 4)) ||
        (rc = put_out(hs, a->hist, R, HS, 4, G)) || (rc = put_state(prm, &cp, sizeof cp)) ||
        (rc = put_state(ids, idv.data(), idv.size() * 4)) || (rc = put_state(bias, bv.data(), bv.size() * 4)) ||
        (rc = put_state(step, &a->t, 4)) || (rc = put_out(tok, a->tok, R, 1, 4, G)) || (rc = skey.put(rest.data(), (size_t)RS * 8)) ||
        (rc = flag.put(rest_flag.data(), (size_t)RS * 4)))
        return rc;
    ConstrainArgs s{};
    if (ph) {   // (an empty list: a header of 0 nodes, the arrays one unused entry each)
        const std::vector<int32_t> none(1, 0);
        const std::vector<int32_t> &off = tr.nodes() ? tr.child_off : none, &tk = tr.edges() ? tr.tok : none, &ds = tr.edges() ? tr.dst : none;
        const std::vector<float> nob(1, 0.f);
        const std::vector<float> &bo = tr.edges() ? tr.bonus : nob;
        const std::vector<int32_t> unset(RS, -1);
        if ((rc = put_state(p_off, off.data(), off.size() * 4)) || (rc = put_state(p_tok, tk.data(), tk.size() * 4)) ||
            (rc = put_state(p_dst, ds.data(), ds.size() * 4)) || (rc = put_state(p_bonus, bo.data(), bo.size() * 4)) ||
            (rc = put_state(scanned, unset.data(), (size_t)RS * 4)))
            return rc;
        const PhraseTrie hd{tr.nodes(), p_off.ptr<int32_t>(), p_tok.ptr<int32_t>(), p_dst.ptr<int32_t>(), p_bonus.ptr<float>()};
        if ((rc = put_state(p_hd, &hd, sizeof hd))) return rc;
        s.ph = p_hd.ptr<PhraseTrie>();
        s.scanned = scanned.ptr<int>();
    }
    s.logits = lg.ptr<float>(); s.ld = a->ld; s.n_valid = a->n_valid;
    s.greedy = gr.ptr<int32_t>();
    s.hist_in = hs.ptr<int32_t>(); s.hist_stride = HS; s.step = step.ptr<int>();
    s.prm = prm.ptr<ConstrainParams>(); s.bias_ids = ids.ptr<int32_t>(); s.bias = bias.ptr<float>();
    s.skey = skey.b.ptr<unsigned long long>(); s.flag = flag.b.ptr<int>();
    s.tok = tok.ptr<int32_t>(); s.hist = hs.ptr<int32_t>();
    s.R = R; s.src_div = a->src_div;
    bool ran = true;
    for (int i = 0; i < a->launches && ran; i++) {   // (the same device state before every launch)
        HIPCHK(hipMemcpy(lg.ptr<char>(), a->logits, (size_t)RS * row_bytes, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(hs.ptr<char>(), a->hist, hist_bytes, hipMemcpyHostToDevice));
        ran = launch_constrain(s, a->slices, nullptr);
        if (ran && i + 1 < a->launches) HIPCHK(hipDeviceSynchronize());
    }
    if ((rc = finish(a, ran))) return rc;
    // the history: slot t of every row out; every other entry and the guard rows as they were
    std::vector<int32_t> hall(hs.bytes / 4);
    if ((rc = get(hs, hall.data()))) return rc;
    for (int i = 0; i < R + 2 * G; i++) a->hist_slot[i] = -1;
    for (size_t i = 0; i < hall.size(); i++) {
        const long row = (long)(i / HS) - G, col = (long)(i % HS);
        const bool real = row >= 0 && row < R;
        if (real && col == a->t) a->hist_slot[G + row] = hall[i];
        else if (hall[i] != (real ? a->hist[(size_t)row * HS + col] : -1)) return fail(QASR_ERR_STATE, "a write outside the history slot");
    }
    if ((rc = get(tok, a->tok)) || (rc = get(lg, a->logits_out)) || (rc = skey.take(a->skey_out, "the key scratch")) ||
        (rc = flag.take(a->flag_out, "the flag scratch")) || (rc = get(scanned, scanned_out)))
        return rc;
    return 0;
}
}  // namespace

extern "C" int qasr_kt_constrain(int device, qasr_kt_constrain_args *a) { return kt_constrain_run(device, a, nullptr, nullptr); }

extern "C" int qasr_kt_phrases(int device, qasr_kt_phrases_args *a) {
    if (!a) return fail(QASR_ERR_ARG, "bad arguments");
    const qasr_phrases ph{a->n_phrases, a->ph_ids, a->ph_len, a->ph_boost};
    return kt_constrain_run(device, a, &ph, a->scanned_out);
}

// the resampler (csrc/resample.hip) on B packed clips at mixed rates, with the library's tap tables.  The packed
// input is followed by `guard` floats of 0xFF bytes; every clip's output has `guard` floats of 0xFF before and after
// it, and the whole buffer ([sum n_out + 2 * guard * B]) comes back.  launches == 2: a second launch on the same
// inputs, clip list and tables into out2, laid out the same.
extern "C" int qasr_kt_resample(int device, qasr_kt_resample_args *a) {
    if (!a || a->B <= 0 || a->guard < 0 || !a->n_in || !a->rate || !a->out || a->launches < 1 || a->launches > 2 ||
        (a->launches == 2 && !a->out2))
        return fail(QASR_ERR_ARG, "bad arguments");
    int rc = use_device(device);
    if (rc) return rc;
    const int B = a->B, G = a->guard;
    eng::ResampleLayout o;
    if ((rc = eng::resample_layout(a->n_in, a->rate, B, o))) return rc;
    if (o.in_tot > 0 && !a->pcm) return fail(QASR_ERR_ARG, "bad arguments");
    std::vector<KtBuf> tabs(B);
    std::vector<ResampleClip> clips(B);
    std::vector<int2> blocks;
    for (int b = 0; b < B; b++) {
        ResamplePlan pl;
        (void)resample_plan(o.rate[b], pl);   // (resample_layout refused the unsupported ones)
        if (!resample_fits(pl.L, pl.M, pl.H)) return fail(QASR_ERR_STATE, "the kernel's window does not hold this rate");
        if (!pl.copy()) {
            std::vector<float> h, dev;
            resample_taps(o.rate[b], pl, h);
            resample_taps_device(pl, h, dev);
            if ((rc = put_in(tabs[b], dev.data(), 1, (long)dev.size(), 4, 0, 0xFF))) return rc;
        }
        clips[b] = ResampleClip{o.in_off[b], o.out_off[b] + (long)G * (2 * b + 1), o.n_in[b], o.n_out[b], pl.L, pl.M, pl.H,
                                tabs[b].ptr<float>()};
        for (long f = 0; f < o.n_out[b]; f += resample_tile()) blocks.push_back(make_int2(b, (int)f));
    }
    const long out_len = o.out_tot + 2L * G * B;
    // the packed input with `guard` floats of 0xFF after it
    KtBuf in, dclips, dblocks, out, out2;
    in.bytes = (size_t)(o.in_tot + G) * 4 + 256;
    HIPCHK(hipMalloc((void **)&in.d, in.bytes));
    HIPCHK(hipMemset(in.d, 0xFF, in.bytes));
    if (o.in_tot) HIPCHK(hipMemcpy(in.d, a->pcm, (size_t)o.in_tot * 4, hipMemcpyHostToDevice));
    const int2 none = make_int2(0, 0);
    if ((rc = put_state(dclips, clips.data(), clips.size() * sizeof(ResampleClip))) ||
        (rc = put_state(dblocks, blocks.empty() ? &none : blocks.data(), std::max<size_t>(blocks.size(), 1) * sizeof(int2))) ||
        (rc = put_out(out, a->out, out_len, 1, 4, 0)) || (rc = put_out(out2, a->launches == 2 ? a->out2 : nullptr, out_len, 1, 4, 0)))
        return rc;
    const float *d_in = in.ptr<float>();
    launch_resample(d_in, dclips.ptr<ResampleClip>(), dblocks.ptr<int2>(), (int)blocks.size(), out.ptr<float>(), nullptr);
    if (a->launches == 2)
        launch_resample(d_in, dclips.ptr<ResampleClip>(), dblocks.ptr<int2>(), (int)blocks.size(), out2.ptr<float>(), nullptr);
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipDeviceSynchronize();
    if (le != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(le));
    if (se != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("kernel run: ") + hipGetErrorString(se));
    a->tile = resample_tile();
    if ((rc = get(out, a->out)) || (rc = get(out2, a->out2))) return rc;
    return 0;
}

// the segmentation kernels (csrc/segment.hip) on B packed recordings.  The packed input is followed by `guard`
// floats of 0xFF bytes; every output has `guard` elements of 0xFF bytes before and after it and comes back whole.
// launches == 2: a second pair of launches on the same inputs and lists into the *2 outputs, laid out the same.
extern "C" int qasr_kt_segment(int device, qasr_kt_segment_args *a) {
    if (!a || a->B <= 0 || a->guard < 0 || a->cap < 1 || !a->n || !a->e || !a->s || !a->peak || !a->peak_rec || !a->cuts || !a->n_seg ||
        a->launches < 1 || a->launches > 2 ||
        (a->launches == 2 && !(a->e2 && a->s2 && a->peak2 && a->peak_rec2 && a->cuts2 && a->n_seg2)))
        return fail(QASR_ERR_ARG, "bad arguments");
    SegmentParams prm;
    prm.max_frames = a->prm.max_frames; prm.min_frames = a->prm.min_frames; prm.smooth_half = a->prm.smooth_half;
    prm.skip_ratio = a->prm.skip_ratio;
    const std::string err = segment_validate(prm);
    if (!err.empty()) return fail(QASR_ERR_ARG, err);
    int rc = use_device(device);
    if (rc) return rc;
    const int B = a->B, G = a->guard, cap = a->cap;
    std::vector<SegmentRec> recs(B);
    std::vector<int2> blocks;
    long tot = 0, frames = 0;
    for (int b = 0; b < B; b++) {
        if (a->n[b] < 0) return fail(QASR_ERR_ARG, "negative length");
        const int F = (int)segment_frames(a->n[b]);
        if (segment_cap(a->n[b], prm) > cap) return fail(QASR_ERR_ARG, "cap below F / min_frames + 1");
        recs[b] = SegmentRec{tot, frames, (long)b * cap, F, cap};
        for (int f = 0; f < F; f += segment_tile()) blocks.push_back(make_int2(b, f));
        tot += a->n[b];
        frames += F;
    }
    if (tot > 0 && !a->pcm) return fail(QASR_ERR_ARG, "bad arguments");
    KtBuf in, drecs, dblocks, e[2], s[2], peak[2], prec[2], cuts[2], nseg[2];
    in.bytes = (size_t)(tot + G) * 4 + 256;
    HIPCHK(hipMalloc((void **)&in.d, in.bytes));
    HIPCHK(hipMemset(in.d, 0xFF, in.bytes));
    if (tot) HIPCHK(hipMemcpy(in.d, a->pcm, (size_t)tot * 4, hipMemcpyHostToDevice));
    const int2 none = make_int2(0, 0);
    if ((rc = put_state(drecs, recs.data(), recs.size() * sizeof(SegmentRec))) ||
        (rc = put_state(dblocks, blocks.empty() ? &none : blocks.data(), std::max<size_t>(blocks.size(), 1) * sizeof(int2))))
        return rc;
    double *he[2] = {a->e, a->e2}, *hs[2] = {a->s, a->s2}, *hpk[2] = {a->peak, a->peak2}, *hpr[2] = {a->peak_rec, a->peak_rec2};
    int32_t *hc[2] = {a->cuts, a->cuts2}, *hn[2] = {a->n_seg, a->n_seg2};
    for (int l = 0; l < a->launches; l++)
        if ((rc = put_out(e[l], he[l], frames, 1, 8, G)) || (rc = put_out(s[l], hs[l], frames, 1, 8, G)) ||
            (rc = put_out(peak[l], hpk[l], (long)B * cap, 1, 8, G)) || (rc = put_out(prec[l], hpr[l], B, 1, 8, G)) ||
            (rc = put_out(cuts[l], hc[l], (long)B * cap, 1, 4, G)) || (rc = put_out(nseg[l], hn[l], B, 1, 4, G)))
            return rc;
    for (int l = 0; l < a->launches; l++)
        launch_segment(in.ptr<float>(), drecs.ptr<SegmentRec>(), B, dblocks.ptr<int2>(), (int)blocks.size(), prm.max_frames,
                       prm.min_frames, prm.smooth_half, e[l].ptr<double>(), s[l].ptr<double>(), cuts[l].ptr<int>(), peak[l].ptr<double>(),
                       nseg[l].ptr<int>(), prec[l].ptr<double>(), nullptr);
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipDeviceSynchronize();
    if (le != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(le));
    if (se != hipSuccess) return fail(QASR_ERR_DEVICE, std::string("kernel run: ") + hipGetErrorString(se));
    a->tile = segment_tile();
    for (int l = 0; l < a->launches; l++)
        if ((rc = get(e[l], he[l])) || (rc = get(s[l], hs[l])) || (rc = get(peak[l], hpk[l])) || (rc = get(prec[l], hpr[l])) ||
            (rc = get(cuts[l], hc[l])) || (rc = get(nseg[l], hn[l])))
            return rc;
    return 0;
}

// ------------------------------------------- norms, RoPE, prefill / encoder attention
// (tests/test_gpu_attn_kernels.py; the launchers return nothing, so "declined" is take_declined's word)
namespace {
template <class Args>
int finish_declinable(Args *a) {
    std::string msg;
    const bool declined = take_declined(&msg);
    const int rc = finish_plain(&a->declined, !declined);
    copy_str(a->msg, sizeof a->msg, msg);
    return rc;
}
}  // namespace

extern "C" int qasr_kt_norm(int device, qasr_kt_norm_args *a) {
    if (!a || a->kind < 0 || a->kind > 2 || a->M <= 0 || a->D <= 0 || a->guard < 0 || !a->x || a->xrows < a->M || a->ldx < a->D)
        return fail(QASR_ERR_ARG, "bad arguments");
    if (a->kind == 0 ? (a->ldx != a->D || a->row_idx || !a->y == !a->y32 || a->yq || a->yd)
                     : (!a->w || (a->kind == 1 ? (!a->y == !a->y32 || a->yq || a->yd)
                                               : (a->row_idx || a->y || a->y32 || !a->yq || !a->yd || a->D % 32 != 0))))
        return fail(QASR_ERR_ARG, "operands missing or not this launcher's");
    if (a->row_idx)
        for (int i = 0; i < a->M; i++)
            if (a->row_idx[i] < 0 || a->row_idx[i] >= a->xrows) return fail(QASR_ERR_ARG, "row_idx outside [0, xrows)");
    int rc = use_device(device);
    if (rc) return rc;
    const int M = a->M, D = a->D, G = a->guard;
    KtBuf x, idx, w, b, y, y32, yq, yd;
    if ((rc = put_in(x, a->x, a->xrows, a->ldx, 4, G, 0xFF)) || (rc = put_in(idx, a->row_idx, 1, M, 4, 0, 0)) ||
        (rc = put_in(w, a->w, 1, D, 4, 1, 0xFF)) || (rc = put_in(b, a->b, 1, D, 4, 1, 0xFF)) || (rc = put_out(y, a->y, M, D, 2, G)) ||
        (rc = put_out(y32, a->y32, M, D, 4, G)) || (rc = put_out(yq, a->yq, M, D, 1, G)) || (rc = put_out(yd, a->yd, M, D / 32, 4, G)))
        return rc;
    switch (a->kind) {
        case 0: launch_layernorm_f16(x.ptr<float>(), M, D, w.ptr<float>(), b.ptr<float>(), a->eps, y.ptr<uint16_t>(), nullptr, y32.ptr<float>()); break;
        case 1:
            launch_rmsnorm_f16(x.ptr<float>(), a->ldx, idx.ptr<int>(), M, D, w.ptr<float>(), a->eps, y.ptr<uint16_t>(), nullptr,
                               y32.ptr<float>());
            break;
        default: launch_rmsnorm_q8(x.ptr<float>(), a->ldx, M, D, w.ptr<float>(), a->eps, yq.ptr<int8_t>(), yd.ptr<float>(), nullptr); break;
    }
    if ((rc = finish_declinable(a))) return rc;
    if ((rc = get(y, a->y)) || (rc = get(y32, a->y32)) || (rc = get(yq, a->yq)) || (rc = get(yd, a->yd))) return rc;
    return 0;
}

extern "C" int qasr_kt_qkv_post(int device, qasr_kt_qkv_post_args *a) {
    if (!a || a->rows <= 0 || a->n_head <= 0 || a->n_kv_head <= 0 || a->max_ctx <= 0 || a->slots <= 0 || a->max_pos <= 0 || a->guard < 0 ||
        !a->qkv || !a->row_seq || !a->row_pos || !a->q_norm || !a->k_norm || !a->rope || !a->q_out || !a->kc || !a->vc || !a->vt ||
        !a->q32 != !a->k32)
        return fail(QASR_ERR_ARG, "bad arguments");
    for (int r = 0; r < a->rows; r++)
        if (a->row_seq[r] < 0 || a->row_seq[r] >= a->slots || a->row_pos[r] < 0 || a->row_pos[r] >= std::min(a->max_ctx, a->max_pos))
            return fail(QASR_ERR_ARG, "row_seq / row_pos outside the caches or the rope table");
    int rc = use_device(device);
    if (rc) return rc;
    const int R = a->rows, G = a->guard, QD = a->n_head * 128, KD = a->n_kv_head * 128;
    const size_t kv = (size_t)a->slots * a->n_kv_head * a->max_ctx * 128 * 2, vt = (size_t)a->slots * a->n_kv_head * 128 * vt_ctx(a->max_ctx) * 2;
    KtBuf qkv, seq, pos, qn, kn, rope, qo, q32, k32;
    KtFenced kc, vc, vtb;
    if ((rc = put_in(qkv, a->qkv, R, QD + 2 * KD, 4, G, 0xFF)) || (rc = put_in(seq, a->row_seq, 1, R, 4, 0, 0)) ||
        (rc = put_in(pos, a->row_pos, 1, R, 4, 0, 0)) || (rc = put_in(qn, a->q_norm, 1, 128, 4, 1, 0xFF)) ||
        (rc = put_in(kn, a->k_norm, 1, 128, 4, 1, 0xFF)) || (rc = put_in(rope, a->rope, a->max_pos, 128, 4, G, 0xFF)) ||
        (rc = put_out(qo, a->q_out, R, QD, 2, G)) || (rc = put_out(q32, a->q32, R, QD, 4, G)) || (rc = put_out(k32, a->k32, R, KD, 4, G)) ||
        (rc = kc.put(a->kc, kv)) || (rc = vc.put(a->vc, kv)) || (rc = vtb.put(a->vt, vt)))
        return rc;
    QkvPostArgs p{};
    p.qkv = qkv.ptr<float>(); p.rows = R;
    p.row_seq = seq.ptr<int>(); p.row_pos = pos.ptr<int>();
    p.q_norm = qn.ptr<float>(); p.k_norm = kn.ptr<float>(); p.eps = a->eps;
    p.rope = rope.ptr<float>();
    p.n_head = a->n_head; p.n_kv_head = a->n_kv_head;
    p.q_out = qo.ptr<uint16_t>();
    p.kc = kc.b.ptr<uint16_t>(); p.vc = vc.b.ptr<uint16_t>(); p.vt = vtb.b.ptr<uint16_t>();
    p.max_ctx = a->max_ctx;
    p.q32 = q32.ptr<float>(); p.k32 = k32.ptr<float>();
    launch_qkv_post(p, nullptr);
    if ((rc = finish_declinable(a))) return rc;
    if ((rc = get(qo, a->q_out)) || (rc = get(q32, a->q32)) || (rc = get(k32, a->k32)) || (rc = kc.take(a->kc, "kc")) ||
        (rc = vc.take(a->vc, "vc")) || (rc = vtb.take(a->vt, "vt")))
        return rc;
    return 0;
}

extern "C" int qasr_kt_enc_attention(int device, qasr_kt_enc_attention_args *a) {
    if (!a || a->rows <= 0 || a->D <= 0 || a->H <= 0 || a->n_seg <= 0 || a->max_len <= 0 || a->guard < 0 || !a->qkv || !a->seg_start ||
        !a->seg_len || !a->out == !a->out32)
        return fail(QASR_ERR_ARG, "bad arguments");
    if (a->D != 64 * a->H) return fail(QASR_ERR_ARG, "encoder attention: D must be 64 H");   // (the launcher throws)
    for (int i = 0; i < a->n_seg; i++)
        if (a->seg_start[i] < 0 || a->seg_len[i] < 1 || a->seg_len[i] > a->max_len || a->seg_start[i] > a->rows - a->seg_len[i])
            return fail(QASR_ERR_ARG, "a segment outside the rows or longer than max_len");
    int rc = use_device(device);
    if (rc) return rc;
    KtBuf qkv, st, ln, out, out32;
    if ((rc = put_in(qkv, a->qkv, a->rows, 3 * a->D, 4, a->guard, 0xFF)) || (rc = put_in(st, a->seg_start, 1, a->n_seg, 4, 0, 0)) ||
        (rc = put_in(ln, a->seg_len, 1, a->n_seg, 4, 0, 0)) || (rc = put_out(out, a->out, a->rows, a->D, 2, a->guard)) ||
        (rc = put_out(out32, a->out32, a->rows, a->D, 4, a->guard)))
        return rc;
    try {
        launch_enc_attention(qkv.ptr<float>(), st.ptr<int>(), ln.ptr<int>(), a->n_seg, a->max_len, a->D, a->H, out.ptr<uint16_t>(), nullptr,
                             out32.ptr<float>(), a->f32_mfma != 0);
    } catch (const std::exception &e) {
        return fail(QASR_ERR_ARG, e.what());
    }
    if ((rc = finish_declinable(a))) return rc;
    if ((rc = get(out, a->out)) || (rc = get(out32, a->out32))) return rc;
    return 0;
}

extern "C" int qasr_kt_prefill_attention(int device, qasr_kt_prefill_attention_args *a) {
    if (!a || a->rows <= 0 || a->n_head <= 0 || a->n_kv_head <= 0 || a->n_head % a->n_kv_head != 0 || a->max_ctx <= 0 || a->slots <= 0 ||
        a->n_seq <= 0 || a->max_len <= 0 || a->guard < 0 || !a->q || !a->kc || !a->vc || !a->seq_row0 || !a->seq_len || !a->seq_slot ||
        !a->out == !a->out32 || !a->q32 != !a->k32 || (a->q32 && (!a->exact || a->seq_pos0)))
        return fail(QASR_ERR_ARG, "bad arguments");
    for (int s = 0; s < a->n_seq; s++) {
        const int L = a->seq_len[s], P0 = a->seq_pos0 ? a->seq_pos0[s] : 0;
        if (L < 1 || L > a->max_len || a->seq_row0[s] < 0 || a->seq_row0[s] > a->rows - L || a->seq_slot[s] < 0 || a->seq_slot[s] >= a->slots ||
            P0 < 0 || P0 > a->max_ctx - L)
            return fail(QASR_ERR_ARG, "a sequence outside the rows, the slots or the context");
    }
    int rc = use_device(device);
    if (rc) return rc;
    const int G = a->guard, QD = a->n_head * 128, KD = a->n_kv_head * 128;
    // the caches as a context holds them: the regions, then kKvPadRows rows the exact kernel may stage (NaN here)
    const size_t kv = (size_t)a->slots * a->n_kv_head * a->max_ctx * 128 * 2, padded = kv + (size_t)kKvPadRows * 128 * 2;
    std::vector<unsigned char> hk(padded, 0xFF), hv(padded, 0xFF), bk(padded), bv(padded);
    memcpy(hk.data(), a->kc, kv);
    memcpy(hv.data(), a->vc, kv);
    KtBuf q, r0, ln, sl, p0, q32, k32, out, out32;
    KtFenced kc, vc;
    if ((rc = put_in(q, a->q, a->rows, QD, 2, G, 0xFF)) || (rc = put_in(r0, a->seq_row0, 1, a->n_seq, 4, 0, 0)) ||
        (rc = put_in(ln, a->seq_len, 1, a->n_seq, 4, 0, 0)) || (rc = put_in(sl, a->seq_slot, 1, a->n_seq, 4, 0, 0)) ||
        (rc = put_in(p0, a->seq_pos0, 1, a->n_seq, 4, 0, 0)) || (rc = put_in(q32, a->q32, a->rows, QD, 4, G, 0xFF)) ||
        (rc = put_in(k32, a->k32, a->rows, KD, 4, G, 0xFF)) || (rc = put_out(out, a->out, a->rows, QD, 2, G)) ||
        (rc = put_out(out32, a->out32, a->rows, QD, 4, G)) || (rc = kc.put(hk.data(), padded)) || (rc = vc.put(hv.data(), padded)))
        return rc;
    PrefillAttnArgs p{};
    p.q = q.ptr<uint16_t>();
    p.kc = kc.b.ptr<uint16_t>(); p.vc = vc.b.ptr<uint16_t>();
    p.seq_row0 = r0.ptr<int>(); p.seq_len = ln.ptr<int>(); p.seq_slot = sl.ptr<int>(); p.n_seq = a->n_seq; p.max_len = a->max_len;
    p.n_head = a->n_head; p.n_kv_head = a->n_kv_head; p.max_ctx = a->max_ctx;
    p.scale = a->scale;
    p.out = out.ptr<uint16_t>(); p.out32 = out32.ptr<float>();
    p.q32 = q32.ptr<float>(); p.k32 = k32.ptr<float>();
    p.seq_pos0 = p0.ptr<int>();
    if (a->exact) launch_prefill_attention_exact(p, nullptr);
    else launch_prefill_attention(p, nullptr);
    if ((rc = finish_declinable(a))) return rc;
    if ((rc = kc.take(bk.data(), "kc")) || (rc = vc.take(bv.data(), "vc"))) return rc;
    if (bk != hk || bv != hv) return fail(QASR_ERR_STATE, "a write into the K / V cache");
    if ((rc = get(out, a->out)) || (rc = get(out32, a->out32))) return rc;
    return 0;
}

// ------------------------------------------------------------ decode attention
// (tests/test_gpu_decode_attn_kernels.py) the launchers that do not wait in-launch: the fused batch-1 launch's
// counters, granules, trace, stamp and error word are always null here
extern "C" int qasr_kt_decode_attention(int device, qasr_kt_decode_attention_args *a) {
    if (!a || a->mode < 0 || a->mode > 4 || a->B <= 0 || a->n_head <= 0 || a->n_kv_head <= 0 || a->max_ctx <= 0 || a->max_pos <= 0 ||
        a->guard < 0 || a->repeat < 1 || a->repeat > 2 || !a->pos || !a->vt)
        return fail(QASR_ERR_ARG, "bad arguments");
    const int mode = a->mode, B = a->B, G = a->guard, nh = a->n_head, nkv = a->n_kv_head;
    const bool chain_only = mode == 4, two = a->repeat == 2;
    if (chain_only ? !a->scores_in : !(a->qkv && a->q_norm && a->k_norm && a->rope && a->kc && a->vc))
        return fail(QASR_ERR_ARG, "operands missing");
    if (two && (mode == 1 || mode == 4)) return fail(QASR_ERR_ARG, "repeat 2 is for modes 0, 2 and 3");
    const int kinds = (a->out != nullptr) + (a->out32 != nullptr) + (a->outq != nullptr);
    if (!a->outq != !a->outd || (mode == 1 ? (kinds != 0 || !a->scores) : (kinds != 1 || a->scores)))
        return fail(QASR_ERR_ARG, "exactly one output kind");
    if (two && (!a->out != !a->out_b || !a->out32 != !a->out32_b || !a->outq != !a->outq_b || !a->outd != !a->outd_b))
        return fail(QASR_ERR_ARG, "repeat 2 needs the second output of the same kind");
    int top = 0;
    for (int b = 0; b < B; b++) {
        if (a->pos[b] < 0 || a->pos[b] >= std::min(a->max_ctx, a->max_pos)) return fail(QASR_ERR_ARG, "pos outside the caches or the rope table");
        top = std::max(top, a->pos[b]);
    }
    if (!chain_only) {
        if (a->grid_splits <= 0 || (long)a->grid_splits * decode_split_len() <= top)
            return fail(QASR_ERR_ARG, "grid_splits does not cover the longest sequence");
        DecodeAttnArgs probe{};
        probe.B = B; probe.n_head = nh; probe.n_kv_head = nkv; probe.grid_splits = a->grid_splits; probe.spl1 = a->spl1;
        probe.spl_batch = a->spl_batch; probe.stream_blocks = a->stream_blocks;
        if (decode_split_count(probe) > decode_max_splits()) return fail(QASR_ERR_ARG, "more splits than decode_max_splits()");
    }
    int rc = use_device(device);
    if (rc) return rc;
    const int QD = nh * 128, KD = nkv * 128, MS = decode_max_splits();
    const size_t kv = (size_t)B * nkv * a->max_ctx * 128 * 2, padded = kv + (size_t)kKvPadRows * 128 * 2;
    const size_t vtb = (size_t)B * nkv * 128 * vt_ctx(a->max_ctx) * 2;
    const size_t part_bytes = (size_t)B * nkv * MS * 2 * 132 * 4, cnt_bytes = (size_t)B * nkv * 4;
    std::vector<unsigned char> hk(padded, 0xFF), hv(padded, 0xFF), k1, v1, t1, k2(padded), v2(padded), hpart(part_bytes, 0xFF),
        hcnt(cnt_bytes, 0);
    if (!chain_only) {
        memcpy(hk.data(), a->kc, kv);
        memcpy(hv.data(), a->vc, kv);
    }
    KtBuf qkv, pos, qn, kn, rope, sc_in, sc_mid, sc_out, o16[2], o32[2], oq[2], od[2];
    KtFenced kc, vc, vt, part, cnt;
    uint16_t *h16[2] = {a->out, a->out_b};
    float *h32[2] = {a->out32, a->out32_b}, *hd[2] = {a->outd, a->outd_b};
    int8_t *hq[2] = {a->outq, a->outq_b};
    if ((rc = put_in(qkv, a->qkv, B, QD + 2 * KD, 4, G, 0xFF)) || (rc = put_in(pos, a->pos, 1, B, 4, 0, 0)) ||
        (rc = put_in(qn, a->q_norm, 1, 128, 4, 1, 0xFF)) || (rc = put_in(kn, a->k_norm, 1, 128, 4, 1, 0xFF)) ||
        (rc = put_in(rope, a->rope, a->max_pos, 128, 4, G, 0xFF)) || (rc = put_in(sc_in, a->scores_in, (long)B * nh, a->max_ctx, 4, G, 0xFF)) ||
        (rc = put_out(sc_out, a->scores, (long)B * nh, a->max_ctx, 4, G)) ||
        // (mode 2's scores stay on the device: allocated like an output, never copied back)
        (rc = put_out(sc_mid, mode == 2 ? (const void *)a : nullptr, (long)B * nh, a->max_ctx, 4, G)) || (rc = kc.put(hk.data(), padded)) ||
        (rc = vc.put(hv.data(), padded)) || (rc = vt.put(a->vt, vtb)) || (rc = part.put(hpart.data(), part_bytes)) ||
        (rc = cnt.put(hcnt.data(), cnt_bytes)))
        return rc;
    for (int r = 0; r < a->repeat; r++)
        if ((rc = put_out(o16[r], h16[r], B, QD, 2, G)) || (rc = put_out(o32[r], h32[r], B, QD, 4, G)) ||
            (rc = put_out(oq[r], hq[r], B, QD, 1, G)) || (rc = put_out(od[r], hd[r], B, QD / 32, 4, G)))
            return rc;
    DecodeAttnArgs d{};
    d.qkv = qkv.ptr<float>(); d.q_norm = qn.ptr<float>(); d.k_norm = kn.ptr<float>(); d.eps = a->eps;
    d.rope = rope.ptr<float>(); d.pos = pos.ptr<int>();
    d.kc = kc.b.ptr<uint16_t>(); d.vc = vc.b.ptr<uint16_t>(); d.vt = vt.b.ptr<uint16_t>();
    d.B = B; d.n_head = nh; d.n_kv_head = nkv; d.max_ctx = a->max_ctx; d.max_splits = MS; d.grid_splits = a->grid_splits;
    d.scale = a->scale;
    d.part = part.b.ptr<float>(); d.counter = cnt.b.ptr<unsigned int>();
    d.spl1 = a->spl1; d.spl_batch = a->spl_batch; d.stream_blocks = a->stream_blocks; d.kv_nt = a->kv_nt; d.fx_seq = a->fx_seq;
    std::string tags, msg;
    bool declined = false;
    // one launcher call: its tag or its declined message
    auto after = [&](bool ran) {
        std::string t, m;
        const bool dec = take_declined(&m) || !ran;
        const bool tagged = take_kernel(&t);
        if (dec) {
            declined = true;
            msg = m.empty() ? "the launcher returned false" : m;
            return 0;
        }
        if (!tagged) return fail(QASR_ERR_STATE, "the launcher recorded no kernel tag");
        tags += (tags.empty() ? "" : "+") + t;
        return 0;
    };
    for (int r = 0; r < a->repeat && !declined; r++) {
        if (r) {   // the caches as the caller gave them; part and counter as the first launch left them
            k1.resize(padded); v1.resize(padded); t1.resize(vtb);
            if ((rc = kc.take(k1.data(), "kc")) || (rc = vc.take(v1.data(), "vc")) || (rc = vt.take(t1.data(), "vt"))) return rc;
            HIPCHK(hipMemcpy(kc.b.ptr<char>(), hk.data(), padded, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(vc.b.ptr<char>(), hv.data(), padded, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(vt.b.ptr<char>(), a->vt, vtb, hipMemcpyHostToDevice));
            tags.clear();
        }
        d.out = o16[r].ptr<uint16_t>(); d.out32 = o32[r].ptr<float>(); d.outq = oq[r].ptr<int8_t>(); d.outd = od[r].ptr<float>();
        d.scores = nullptr;
        switch (mode) {
            case 0: launch_decode_attention(d, nullptr); rc = after(true); break;
            case 1: d.scores = sc_out.ptr<float>(); launch_decode_attention(d, nullptr); rc = after(true); break;
            case 2:
                d.scores = sc_mid.ptr<float>();
                launch_decode_attention(d, nullptr);
                if ((rc = after(true)) || declined) break;
                launch_decode_attention_exact(d, nullptr);
                rc = after(true);
                break;
            case 3: rc = after(launch_decode_attention_exact_seq(d, nullptr)); break;
            default: d.scores = sc_in.ptr<float>(); launch_decode_attention_exact(d, nullptr); rc = after(true); break;
        }
        if (rc) return rc;
        int32_t unused = 0;
        if ((rc = finish_plain(&unused, true))) return rc;
        std::vector<unsigned char> c(cnt_bytes);
        if ((rc = cnt.take(c.data(), "the split counters"))) return rc;
        if (c != hcnt) return fail(QASR_ERR_STATE, "a split counter is not zero after the launch");
    }
    a->declined = declined;
    copy_str(a->tag, sizeof a->tag, declined ? std::string() : tags);
    copy_str(a->msg, sizeof a->msg, msg);
    if ((rc = part.take(hpart.data(), "part")) || (rc = kc.take(k2.data(), "kc")) || (rc = vc.take(v2.data(), "vc")) ||
        (rc = vt.take(a->vt, "vt")))
        return rc;
    if (memcmp(k2.data() + kv, hk.data() + kv, padded - kv) || memcmp(v2.data() + kv, hv.data() + kv, padded - kv))
        return fail(QASR_ERR_STATE, "a write into the rows after the last K / V region");
    if (two && !declined && (k1 != k2 || v1 != v2 || memcmp(t1.data(), a->vt, vtb)))
        return fail(QASR_ERR_STATE, "the two launches left different caches");
    if (!chain_only) {
        memcpy(a->kc, k2.data(), kv);
        memcpy(a->vc, v2.data(), kv);
    }
    if ((rc = get(sc_out, a->scores))) return rc;
    for (int r = 0; r < a->repeat; r++)
        if ((rc = get(o16[r], h16[r])) || (rc = get(o32[r], h32[r])) || (rc = get(oq[r], hq[r])) || (rc = get(od[r], hd[r]))) return rc;
    return 0;
}

// ------------------------------------------------------------- conv front end
// (tests/test_gpu_conv_kernels.py) launch_conv1 and launch_gemm's AM_CONV2 / AM_CONV3 on a caller-supplied chunk
// table.  The input sits between guard_in elements of 0xFF bytes on both sides: the NHWC layout puts a neighbour's
// valid data where a mis-bounded padding tap lands, and at the first and last chunk that neighbour is NaN here.
static_assert(sizeof(qasr_kt_chunk) == sizeof(ChunkDesc) && offsetof(qasr_kt_chunk, T) == offsetof(ChunkDesc, T) &&
                  offsetof(qasr_kt_chunk, row1) == offsetof(ChunkDesc, row1) && offsetof(qasr_kt_chunk, enc_row) == offsetof(ChunkDesc, enc_row),
              "qasr_kt_chunk mirrors ChunkDesc");

extern "C" int qasr_kt_conv(int device, qasr_kt_conv_args *a) {
    if (!a || a->layer < 1 || a->layer > 3 || a->C <= 0 || a->n_chunks <= 0 || a->in_len <= 0 || a->out_rows <= 0 || a->guard < 0 ||
        a->guard_in < 0 || !a->chunks || !a->W || !a->bias || !a->out || (a->layer == 1 ? !a->mel || a->max_w1 < 1 : !a->act))
        return fail(QASR_ERR_ARG, "bad arguments");
    const int layer = a->layer, C = a->C, NC = a->n_chunks, G = a->guard;
    // every address a chunk's in-bounds taps and its output rows can form lies inside the arrays; the output rows
    // of the chunks are consecutive from 0 (find_chunk) and out_rows is their sum
    std::vector<int> starts(NC);
    long next = 0;
    for (int c = 0; c < NC; c++) {
        const qasr_kt_chunk &d = a->chunks[c];
        if (d.W1 < 1 || d.W2 < 1 || d.W3 < 1 || d.T < 1 || d.L < 1 || d.Lv < 0 || d.Lv > d.L) return fail(QASR_ERR_ARG, "a chunk's widths");
        const long rin = layer == 2 ? d.row1 : d.row2, nin = layer == 2 ? 64L * d.W1 : 32L * d.W2;
        const long rout = layer == 1 ? d.row1 : layer == 2 ? d.row2 : d.row3;
        const long nout = layer == 1 ? 64L * d.W1 : layer == 2 ? 32L * d.W2 : 16L * d.W3;
        if (layer == 1 ? (d.mel_off < 0 || d.Lv > d.T || d.mel_off + 127L * d.T + d.Lv > a->in_len) : (rin < 0 || rin + nin > a->in_len))
            return fail(QASR_ERR_ARG, "a chunk reads outside the input");
        if (rout != next) return fail(QASR_ERR_ARG, "the chunks' output rows are not consecutive from 0");
        starts[c] = (int)rout;
        next += nout;
    }
    if (next != a->out_rows) return fail(QASR_ERR_ARG, "out_rows is not the sum of the chunks' rows");
    int rc = use_device(device);
    if (rc) return rc;
    const int KP = layer == 1 ? 9 : conv_kpad(C);
    // the input between two guards
    const int esz = layer == 1 ? 4 : 2;
    const size_t unit = (size_t)(layer == 1 ? 1 : C) * esz, lead = (size_t)a->guard_in * unit, real = (size_t)a->in_len * unit;
    KtBuf in, W, bias, chunks, rs, gelu, out;
    in.bytes = real + 2 * lead + 256;
    in.off = lead;
    HIPCHK(hipMalloc((void **)&in.d, in.bytes));
    HIPCHK(hipMemset(in.d, 0xFF, in.bytes));
    HIPCHK(hipMemcpy(in.d + lead, layer == 1 ? (const void *)a->mel : (const void *)a->act, real, hipMemcpyHostToDevice));
    if ((rc = put_in(W, a->W, C, KP, 2, G, 0xFF)) || (rc = put_in(bias, a->bias, 1, C, 4, 1, 0xFF)) ||
        (rc = put_state(chunks, a->chunks, (size_t)NC * sizeof(ChunkDesc))) || (rc = put_state(rs, starts.data(), (size_t)NC * 4)) ||
        (rc = put_out(out, a->out, a->out_rows, C, 2, G)))
        return rc;
    std::vector<uint16_t> lut;
    gelu_table(lut);
    if ((rc = put_in(gelu, lut.data(), 1, 65536, 2, 0, 0))) return rc;
    if (a->gelu_out) memcpy(a->gelu_out, lut.data(), 65536 * 2);
    if (layer == 1) {
        launch_conv1(in.ptr<float>(), chunks.ptr<ChunkDesc>(), rs.ptr<int>(), NC, a->out_rows, W.ptr<uint16_t>(), bias.ptr<float>(),
                     gelu.ptr<uint16_t>(), C, out.ptr<uint16_t>(), nullptr, a->max_w1);
    } else {
        GemmArgs g{};
        g.A = in.ptr<uint16_t>();
        g.W = W.ptr<uint16_t>(); g.ldw = KP;
        g.M = a->out_rows; g.N = C; g.K = 9 * C;
        g.chunks = chunks.ptr<ChunkDesc>(); g.row_start = rs.ptr<int>(); g.n_chunks = NC; g.C = C;
        g.bias = bias.ptr<float>();
        g.out_f16 = out.ptr<uint16_t>(); g.ldo16 = C;
        g.gelu = gelu.ptr<uint16_t>();
        g.regs_staged = a->regs_staged;
        launch_gemm(layer == 2 ? AM_CONV2 : AM_CONV3, EPI_GELU_F16, g, nullptr);
    }
    if ((rc = finish(a, true))) return rc;
    return get(out, a->out);
}
