// engine_model.hip -- the model side of the C-ABI (include/qasr_capi.h): GGUF
// tensors into one device arena, the tokenizer's text entry points, and the
// WAV / synthetic-PCM / synthetic-GGUF utilities.
#include <functional>
#include <memory>

#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

// -------------------------------------------------------------- loading
namespace {
struct Up {
    std::string name;
    size_t bytes;
    void **dst;
    std::function<void(uint8_t *)> fill;
};
}  // namespace

static bool check_shape(const gguf_tensor *t, std::vector<int64_t> ne, uint32_t want_type, std::string &err) {
    if (!t) { err = "missing tensor"; return false; }
    int64_t n = 1, m = 1;
    for (auto v : ne) n *= v;
    for (auto v : t->ne) m *= v;
    if (n != m) {
        err = "tensor " + t->name + ": expected " + std::to_string(n) + " elements, file has " + std::to_string(m);
        return false;
    }
    if (t->type != want_type) {
        err = "tensor " + t->name + ": unsupported ggml type " + std::to_string(t->type) +
              (want_type == DT_F32 ? " (expected F32)" : want_type == DT_Q8_0 ? " (expected Q8_0 like the other linear weights)"
                                                                              : " (expected F16)");
        return false;
    }
    return true;
}

extern "C" int qasr_model_load(const char *path, int device, qasr_model **out) {
    if (!path || !out) return fail(QASR_ERR_ARG, "null argument");
    *out = nullptr;
    const bool host_only = device == QASR_HOST_ONLY;
    if (!host_only) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(QASR_ERR_DEVICE, "no HIP device available");
        if (device < 0 || device >= ndev) return fail(QASR_ERR_ARG, "bad device index");
        HIPCHK(hipSetDevice(device));
    }
    GGUFFile f;
    if (!f.open(path)) return fail(QASR_ERR_IO, f.error());
    std::unique_ptr<qasr_model> m(new qasr_model());
    m->device = device;
    m->hp = read_hparams(f);
    const Hparams &hp = m->hp;
    std::string err;
    if (!m->tok.load(f, err)) return fail(QASR_ERR_FORMAT, err);
    if (hp.d_model / hp.enc_heads != 64 || hp.d_model % hp.enc_heads)
        return fail(QASR_ERR_FORMAT, "encoder head_dim must be 64");
    if (hp.head_dim != 128 || hp.n_head != 2 * hp.n_kv_head)
        return fail(QASR_ERR_FORMAT, "decoder must have head_dim 128 and GQA ratio 2");
    if (hp.n_mel != 128) return fail(QASR_ERR_FORMAT, "n_mel must be 128");
    if (!conv_width_ok(hp.conv_ch) || hp.dec_ffn % 16) return fail(QASR_ERR_FORMAT, "unsupported conv/ffn width");

    const int C = hp.conv_ch, D = hp.d_model, FF = hp.enc_ffn, H = hp.hidden, V = hp.vocab;
    const int QD = hp.n_head * 128, KD = hp.n_kv_head * 128, F = hp.dec_ffn;
    m->enc.resize(hp.enc_layers);
    m->dec.resize(hp.dec_layers);
    std::vector<Up> ups;
    auto T = [&](const std::string &n) { return f.tensor(n); };
    auto need = [&](const std::string &n, std::vector<int64_t> ne, uint32_t ty) -> const gguf_tensor * {
        const gguf_tensor *t = T(n);
        std::string e;
        if (!t) { if (err.empty()) err = "missing tensor: " + n; return nullptr; }
        if (!check_shape(t, ne, ty, e)) { if (err.empty()) err = e; return nullptr; }
        return t;
    };
    auto copy_f32 = [&](const std::string &n, int64_t len, float **dst) {
        const gguf_tensor *t = need(n, {len}, DT_F32);
        if (!t) return;
        ups.push_back({n, (size_t)len * 4, (void **)dst, [t, len](uint8_t *o) { memcpy(o, t->data, (size_t)len * 4); }});
    };
    auto copy_f16 = [&](const std::string &n, std::vector<int64_t> ne, uint16_t **dst) {
        const gguf_tensor *t = need(n, ne, DT_F16);
        if (!t) return;
        size_t bytes = t->nbytes;
        ups.push_back({n, bytes, (void **)dst, [t, bytes](uint8_t *o) { memcpy(o, t->data, bytes); }});
    };
    // conv kernels: [oc][ic][kh][kw] -> [oc][kh][kw][ic] (im2col K order of the implicit GEMM),
    // rows zero-padded to conv_kpad(IC) (the 8-phase tile's K % 128; gemm8p.h)
    auto conv_w = [&](const std::string &n, int IC, uint16_t **dst) {
        const gguf_tensor *t = need(n, {3, 3, IC, C}, DT_F16);
        if (!t) return;
        const int KP = conv_kpad(IC);
        ups.push_back({n, (size_t)C * KP * 2, (void **)dst, [t, IC, C, KP](uint8_t *o) {
                           const uint16_t *s = (const uint16_t *)t->data;
                           uint16_t *d = (uint16_t *)o;
                           memset(d, 0, (size_t)C * KP * 2);
                           for (int oc = 0; oc < C; oc++)
                               for (int ic = 0; ic < IC; ic++)
                                   for (int k = 0; k < 9; k++) d[(size_t)oc * KP + (size_t)k * IC + ic] = s[((size_t)oc * IC + ic) * 9 + k];
                       }});
    };
    copy_f16("audio.encoder.conv1.weight", {3, 3, 1, C}, &m->conv1_w);
    copy_f32("audio.encoder.conv1.bias", C, &m->conv1_b);
    conv_w("audio.encoder.conv2.weight", C, &m->conv2_w);
    copy_f32("audio.encoder.conv2.bias", C, &m->conv2_b);
    conv_w("audio.encoder.conv3.weight", C, &m->conv3_w);
    copy_f32("audio.encoder.conv3.bias", C, &m->conv3_b);
    // linear weights: every non-conv matrix except token_embd shares one type
    const gguf_tensor *probe = T("blk.0.attn_q.weight");
    const uint32_t LT = probe && probe->type == DT_Q8_0 ? DT_Q8_0 : DT_F16;
    m->q8 = LT == DT_Q8_0;
    // a linear weight [N][K] stacked from source tensors; rmap(r) -> {tensor, source row}
    auto lin = [&](const std::string &key, std::vector<const gguf_tensor *> src, int K, int N,
                   std::function<std::pair<int, int>(int)> rmap, uint16_t **dst, uint16_t **dst_d) {
        for (auto *t : src) if (!t) return;
        if (LT == DT_F16) {
            ups.push_back({key, (size_t)N * K * 2, (void **)dst, [src, K, N, rmap](uint8_t *o) {
                               for (int r = 0; r < N; r++) {
                                   const auto sr = rmap(r);
                                   memcpy(o + (size_t)r * K * 2, (const uint8_t *)src[sr.first]->data + (size_t)sr.second * K * 2,
                                          (size_t)K * 2);
                               }
                           }});
        } else {
            if (K % 32) { if (err.empty()) err = key + ": Q8_0 row length must be a multiple of 32"; return; }
            const int nb = K / 32;
            auto blocks = [src, nb, rmap](int r) {
                const auto sr = rmap(r);
                return (const uint8_t *)src[sr.first]->data + (size_t)sr.second * nb * 34;
            };
            ups.push_back({key, (size_t)N * K, (void **)dst, [blocks, K, N, nb](uint8_t *o) {
                               for (int r = 0; r < N; r++) {
                                   const uint8_t *b = blocks(r);
                                   for (int j = 0; j < nb; j++) memcpy(o + (size_t)r * K + 32 * j, b + 34 * j + 2, 32);
                               }
                           }});
            ups.push_back({key + ".d", (size_t)N * nb * 2, (void **)dst_d, [blocks, N, nb](uint8_t *o) {
                               for (int r = 0; r < N; r++) {
                                   const uint8_t *b = blocks(r);
                                   for (int j = 0; j < nb; j++) memcpy(o + ((size_t)r * nb + j) * 2, b + 34 * j, 2);
                               }
                           }});
        }
    };
    auto ident = [](int r) { return std::make_pair(0, r); };
    auto one = [&](const std::string &n, int K, int N, uint16_t **dst, uint16_t **dst_d) {
        lin(n, {need(n, {K, N}, LT)}, K, N, ident, dst, dst_d);
    };
    {   // conv_out: input feature c*16+h (src/audio_encoder.cpp:133-142).  F16: permuted
        // to h*C + c at load so the GEMM's A is conv3's [h][c] rows; Q8_0 keeps the
        // file order (blocks run along it) and the activation quantiser gathers.
        const gguf_tensor *t = need("audio.encoder.conv_out.weight", {(int64_t)C * 16, D}, LT);
        if (t && LT == DT_F16)
            ups.push_back({t->name, (size_t)D * C * 16 * 2, (void **)&m->conv_out_w, [t, C, D](uint8_t *o) {
                               const uint16_t *s = (const uint16_t *)t->data;
                               uint16_t *d = (uint16_t *)o;
                               for (int n = 0; n < D; n++)
                                   for (int c = 0; c < C; c++)
                                       for (int h = 0; h < 16; h++) d[(size_t)n * C * 16 + h * C + c] = s[(size_t)n * C * 16 + c * 16 + h];
                           }});
        else if (t)
            lin(t->name, {t}, 16 * C, D, ident, &m->conv_out_w, &m->conv_out_d);
    }
    for (int l = 0; l < hp.enc_layers; l++) {
        const std::string p = "audio.encoder.blk." + std::to_string(l) + ".";
        EncLayer &L = m->enc[l];
        const gguf_tensor *q = need(p + "attn_q.weight", {D, D}, LT), *k = need(p + "attn_k.weight", {D, D}, LT),
                          *v = need(p + "attn_v.weight", {D, D}, LT);
        const gguf_tensor *qb = need(p + "attn_q.bias", {D}, DT_F32), *kb = need(p + "attn_k.bias", {D}, DT_F32),
                          *vb = need(p + "attn_v.bias", {D}, DT_F32);
        lin(p + "qkv", {q, k, v}, D, 3 * D, [D](int r) { return std::make_pair(r / D, r % D); }, &L.wqkv, &L.wqkv_d);
        if (qb && kb && vb) {
            const size_t bb = (size_t)D * 4;
            ups.push_back({p + "bqkv", 3 * bb, (void **)&L.bqkv, [qb, kb, vb, bb](uint8_t *o) {
                               memcpy(o, qb->data, bb); memcpy(o + bb, kb->data, bb); memcpy(o + 2 * bb, vb->data, bb); }});
        }
        one(p + "attn_out.weight", D, D, &L.wo, &L.wo_d);
        copy_f32(p + "attn_out.bias", D, &L.bo);
        copy_f32(p + "attn_norm.weight", D, &L.ln1_w);
        copy_f32(p + "attn_norm.bias", D, &L.ln1_b);
        one(p + "ffn_up.weight", D, FF, &L.w1, &L.w1_d);
        copy_f32(p + "ffn_up.bias", FF, &L.b1);
        one(p + "ffn_down.weight", FF, D, &L.w2, &L.w2_d);
        copy_f32(p + "ffn_down.bias", D, &L.b2);
        copy_f32(p + "ffn_norm.weight", D, &L.ln2_w);
        copy_f32(p + "ffn_norm.bias", D, &L.ln2_b);
    }
    copy_f32("audio.encoder.ln_post.weight", D, &m->ln_post_w);
    copy_f32("audio.encoder.ln_post.bias", D, &m->ln_post_b);
    one("audio.encoder.proj1.weight", D, D, &m->proj1_w, &m->proj1_d);
    copy_f32("audio.encoder.proj1.bias", D, &m->proj1_b);
    one("audio.encoder.proj2.weight", D, H, &m->proj2_w, &m->proj2_d);
    copy_f32("audio.encoder.proj2.bias", H, &m->proj2_b);
    copy_f16("token_embd.weight", {H, V}, &m->embd);   // tied LM head (src/text_decoder.cpp:264-265), F16 in both file types
    if (hp.aligner) {   // classify head: output.weight as [hidden][classify_num] (src/forced_aligner.cpp:274-277, 1073)
        const gguf_tensor *t = T("output.weight");
        const int NC = hp.classify_num;
        if (!t || t->type != DT_F16 || t->ne.size() != 2 || t->ne[0] != H || t->ne[1] < NC || NC <= 0) {
            if (err.empty()) err = "aligner: output.weight must be F16 [hidden][>= classify_num]";
        } else {
            m->cls_rows = (NC + 63) / 64 * 64;   // the GEMM tiles 64 columns; padded rows never win the argmax
            const size_t bytes = (size_t)m->cls_rows * H * 2;
            ups.push_back({"output.weight", bytes, (void **)&m->cls_w, [t, NC, H, bytes](uint8_t *o) {
                               memset(o, 0, bytes);
                               memcpy(o, t->data, (size_t)NC * H * 2);
                           }});
        }
    }
    copy_f32("output_norm.weight", H, &m->out_norm);
    for (int l = 0; l < hp.dec_layers; l++) {
        const std::string p = "blk." + std::to_string(l) + ".";
        DecLayer &L = m->dec[l];
        copy_f32(p + "attn_norm.weight", H, &L.attn_norm);
        copy_f32(p + "attn_q_norm.weight", 128, &L.q_norm);
        copy_f32(p + "attn_k_norm.weight", 128, &L.k_norm);
        copy_f32(p + "ffn_norm.weight", H, &L.ffn_norm);
        const gguf_tensor *q = need(p + "attn_q.weight", {H, QD}, LT), *k = need(p + "attn_k.weight", {H, KD}, LT),
                          *v = need(p + "attn_v.weight", {H, KD}, LT);
        lin(p + "qkv", {q, k, v}, H, QD + 2 * KD,
            [QD, KD](int r) { return r < QD ? std::make_pair(0, r) : r < QD + KD ? std::make_pair(1, r - QD) : std::make_pair(2, r - QD - KD); },
            &L.wqkv, &L.wqkv_d);
        one(p + "attn_output.weight", QD, H, &L.wo, &L.wo_d);
        const gguf_tensor *gt = need(p + "ffn_gate.weight", {H, F}, LT), *ut = need(p + "ffn_up.weight", {H, F}, LT);
        // interleave 16-row blocks: [gate 16q..16q+15 | up 16q..16q+15] -> SwiGLU in one epilogue
        lin(p + "gu", {gt, ut}, H, 2 * F, [](int r) { return std::make_pair((r % 32) < 16 ? 0 : 1, 16 * (r / 32) + (r % 16)); },
            &L.wgu, &L.wgu_d);
        one(p + "ffn_down.weight", F, H, &L.wd, &L.wd_d);
    }
    if (!err.empty()) return fail(QASR_ERR_FORMAT, err);
    // constant tables
    std::vector<uint16_t> lut;
    gelu_table(lut);
    ups.push_back({"gelu", lut.size() * 2, (void **)&m->gelu, [lut](uint8_t *o) { memcpy(o, lut.data(), lut.size() * 2); }});
    std::vector<float> pe;
    sinusoidal_pe(pe, 13, D);   // a 100-frame chunk yields at most 13 frames
    ups.push_back({"pe", pe.size() * 4, (void **)&m->pe, [pe](uint8_t *o) { memcpy(o, pe.data(), pe.size() * 4); }});
    std::vector<float> fl;
    mel_filters(fl);
    ups.push_back({"filters", fl.size() * 4, (void **)&m->filters, [fl](uint8_t *o) { memcpy(o, fl.data(), fl.size() * 4); }});
    std::vector<double> tw, hn;
    dft_twiddles(tw);
    hann_window(hn);
    ups.push_back({"tw", tw.size() * 8, (void **)&m->tw, [tw](uint8_t *o) { memcpy(o, tw.data(), tw.size() * 8); }});
    ups.push_back({"hann", hn.size() * 8, (void **)&m->hann, [hn](uint8_t *o) { memcpy(o, hn.data(), hn.size() * 8); }});

    if (host_only) {   // hparams + tokenizer only: text helpers, validation, tests without a GPU
        *out = m.release();
        return 0;
    }
    size_t total = 0;
    std::vector<size_t> offs(ups.size());
    for (size_t i = 0; i < ups.size(); i++) {
        offs[i] = total;
        total += (ups[i].bytes + 255) / 256 * 256;
    }
    HIPCHK(hipMalloc((void **)&m->arena, total));
    m->arena_bytes = total;
    std::vector<uint8_t> host;
    for (size_t i = 0; i < ups.size(); i++) {
        host.resize(ups[i].bytes);
        ups[i].fill(host.data());
        HIPCHK(hipMemcpy(m->arena + offs[i], host.data(), ups[i].bytes, hipMemcpyHostToDevice));
        *ups[i].dst = m->arena + offs[i];
    }
    *out = m.release();
    return 0;
}

extern "C" void qasr_model_free(qasr_model *m) { delete m; }

extern "C" int qasr_model_hparams(const qasr_model *m, qasr_hparams *o) {
    if (!m || !o) return fail(QASR_ERR_ARG, "null argument");
    const Hparams &h = m->hp;
    *o = qasr_hparams{h.enc_layers, h.d_model, h.enc_heads, h.enc_ffn, h.conv_ch, h.n_mel, h.enc_eps,
                      h.vocab, h.hidden, h.dec_layers, h.n_head, h.n_kv_head, h.head_dim, h.dec_ffn, h.rms_eps, h.rope_theta,
                      h.eos_id, h.pad_id, h.audio_start_id, h.audio_end_id, h.audio_pad_id, h.weight_type,
                      h.aligner ? h.classify_num : 0, h.timestamp_id};
    return 0;
}

extern "C" int64_t qasr_model_device_bytes(const qasr_model *m) { return m ? (int64_t)m->arena_bytes : 0; }

// ------------------------------------------------------------------- text
extern "C" int qasr_detokenize(const qasr_model *m, const int32_t *ids, int n, char *out, int cap) {
    if (!m || (!ids && n > 0)) return fail(QASR_ERR_ARG, "bad arguments");
    std::string s = m->tok.decode(std::vector<int32_t>(ids, ids + n));
    if (out && cap > 0) {
        const int k = std::min<int>((int)s.size(), cap - 1);
        memcpy(out, s.data(), k);
        out[k] = 0;
    }
    return (int)s.size();
}

extern "C" int qasr_tokenize(const qasr_model *m, const char *text, int32_t *ids, int cap) {
    if (!m || !text) return fail(QASR_ERR_ARG, "bad arguments");
    std::vector<int32_t> v = m->tok.encode(text);
    if (ids) for (int i = 0; i < (int)v.size() && i < cap; i++) ids[i] = v[i];
    return (int)v.size();
}

extern "C" int qasr_model_load_korean_dict(qasr_model *m, const char *path) {
    if (!m || !path) return fail(QASR_ERR_ARG, "bad arguments");
    if (!load_korean_dict(path, m->ko_dict)) return fail(QASR_ERR_IO, std::string("cannot read Korean dictionary: ") + path);
    return 0;
}

// --------------------------------------------------------- host utilities
extern "C" int qasr_load_wav(const char *path, float *out, int max_n, int *sample_rate) {
    std::vector<float> s;
    int sr = 0;
    std::string err;
    if (!path || !load_wav(path, s, sr, err)) return fail(-1, err.empty() ? "bad path" : err);
    if (sample_rate) *sample_rate = sr;
    if (out) memcpy(out, s.data(), (size_t)std::min<int>((int)s.size(), max_n) * 4);
    return (int)s.size();
}

extern "C" int qasr_write_wav(const char *path, const float *pcm, int n, int sample_rate) {
    if (!path || (!pcm && n > 0) || !write_wav(path, pcm, n, sample_rate)) return fail(QASR_ERR_IO, "cannot write wav");
    return 0;
}

extern "C" int qasr_synth_pcm(uint64_t seed, int n, float *out) {
    if (!out || n < 0) return fail(QASR_ERR_ARG, "bad arguments");
    synth_pcm(seed, n, out);
    return 0;
}

// bump with every change to host_util.cpp write_synthetic_gguf's output
extern "C" int qasr_synthetic_gguf_version(void) { return 5; }

extern "C" int qasr_write_synthetic_gguf(const char *path, const char *config, uint64_t seed, int wtype) {
    std::string err;
    if (!path || !config) return fail(QASR_ERR_ARG, "bad arguments");
    if (!write_synthetic_gguf(path, config, seed, wtype, err)) return fail(QASR_ERR_IO, err);
    return 0;
}
