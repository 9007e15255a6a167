// kv_fp8.hip -- the FP8 (E4M3) shadow of the K / V caches (option kv_fp8):
//   kv_fp8_convert_kernel       the shadow's one writer outside the attention: position ranges of cache slots
//                               re-derived from the fp16 caches by the rule of kv_fp8_host.h
//   decode_attn_seq_fp8_kernel  the per-sequence decode attention of 9 .. 128-row steps reading the shadow
// Both turn bytes into numbers with gfx950's packed conversions (v_cvt_pk_fp8_f32, v_cvt_scalef32_pk_f16_fp8,
// v_cvt_pk_f32_fp8); the rule, not the instruction, is normative (tests/test_gpu_kv_fp8_kernel.py compares them).
#include <algorithm>
#include <cmath>

#include "dev_common.h"
#include "kernels.h"
#include "kv_fp8_host.h"

namespace qasr {

// ------------------------------------------------------------------ the rule on the device
// clamp(x 2^s, -448, 448) in fp32 (the product is exact); NaN passes through (fminf / fmaxf would drop it)
__device__ __forceinline__ float kv8_pre(float x, float up) {
    const float y = x * up;
    const float c = fminf(fmaxf(y, -kE4m3Max), kE4m3Max);
    return y != y ? y : c;
}
// two values -> two E4M3 bytes (RNE) in the low half of the result
__device__ __forceinline__ uint32_t kv8_pack2(float a, float b, float up) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(kv8_pre(a, up), kv8_pre(b, up), 0, false) & 0xffffu;
}
// eight fp16 values (16 B) -> eight bytes
__device__ __forceinline__ uint2 kv8_pack8(half8 h, float up) {
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_pre((float)h[0], up), kv8_pre((float)h[1], up), 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_pre((float)h[2], up), kv8_pre((float)h[3], up), lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_pre((float)h[4], up), kv8_pre((float)h[5], up), 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_pre((float)h[6], up), kv8_pre((float)h[7], up), hi, true);
    return make_uint2((uint32_t)lo, (uint32_t)hi);
}

// ------------------------------------------------------------------ convert
// grid (ceil(span / 16), B, layers * n_kv_head), 256 threads: 16 positions x 16 threads, a thread one 16-B piece
// (8 dims) of the K row and of the V row -> two 8-B stores.  Row b's range comes from device memory.
__global__ __launch_bounds__(256) void kv_fp8_convert_kernel(KvFp8ConvertArgs a) {
    const int b = blockIdx.y, l = blockIdx.z / a.n_kv_head, h = blockIdx.z % a.n_kv_head;
    const int f = a.from ? a.from[b] : 0;
    const int e = a.to ? a.to[b] : f + (a.len ? a.len[b] : a.span);
    const int slot = a.slot ? a.slot[b] : b;
    const long p = (long)f + blockIdx.x * 16 + (threadIdx.x >> 4);
    if (slot < 0 || slot >= a.slots || p < 0 || p < f || p >= e || p >= a.max_ctx) return;
    const size_t at = ((((size_t)l * a.slots + slot) * a.n_kv_head + h) * a.max_ctx + (size_t)p) * 128 + (threadIdx.x & 15) * 8;
    const float up = ldexpf(1.0f, a.exp);
    const half8 k = *(const half8 *)(a.kc + at), v = *(const half8 *)(a.vc + at);
    *(uint2 *)(a.k8 + at) = kv8_pack8(k, up);
    *(uint2 *)(a.v8 + at) = kv8_pack8(v, up);
}

bool launch_kv_fp8_convert(const KvFp8ConvertArgs &a, hipStream_t s) {
    if (!a.kc || !a.vc || !a.k8 || !a.v8 || a.layers <= 0 || a.slots <= 0 || a.n_kv_head <= 0 || a.max_ctx <= 0 || a.B <= 0 ||
        a.B > 65535 || (long)a.layers * a.n_kv_head > 65535 || a.span < 0 || a.exp < kKvFp8ExpMin || a.exp > kKvFp8ExpMax)
        return false;
    const int span = std::min(a.span, a.max_ctx);
    if (span == 0) return true;   // every range empty
    kv_fp8_convert_kernel<<<dim3((span + 15) / 16, a.B, a.layers * a.n_kv_head), 256, 0, s>>>(a);
    return true;
}

// ------------------------------------------------------------------ attention
// One workgroup (4 waves) per (kv group g, sequence b), as decode_attn_seq_kernel, walking the sequence's own keys
// in 128-key chunks: wave w owns keys c0 + 32 w .. + 31 of a chunk, two 16-key MFMA tiles.  A 16-B load carries 16
// dimensions of one key, so a register set of the fp16 kernel's size (4 K + 4 V loads a lane) holds twice the keys;
// two sets, the other chunk's requested before this chunk's arithmetic: the same bytes in flight a workgroup.
//   K: lane (q4 = lane / 16, c16 = lane % 16), tile t, load j (0, 1): key 16 t + c16, dims 64 j + 16 q4 .. + 15.
//      Bytes 8 h .. 8 h + 7 (h = 0, 1) of that load become, through v_cvt_scalef32_pk_f16_fp8 with scale 2^-s, the
//      lane's eight B-operand halves of MFMA (j, h); the A operand of that MFMA is q's dims 64 j + 16 q4 + 8 h .. + 7
//      of head c16 (rows 2 .. 15 zero): the same permutation of the 128 products on both sides, no shuffle.
//   V: lane (r8 = lane / 8, d16 = 16 (lane % 8)), load i (0 .. 3): key 8 i + r8, dims d16 .. + 15, bytes to fp32 by
//      v_cvt_pk_f32_fp8; the lane keeps 16 dims x 2 heads of O in fp32, summed over r8 and the waves once at the end.
//      The 2^-s of V is applied once to the finished output (exact: a power of two).
// As the fp16 kernel: no barrier in the key loop, a per-wave online softmax (one rescale a chunk) merged once through
// LDS, only keys <= pos loaded.  Key pos: the new row's bytes by the rule, from LDS, replace the loaded ones.
struct Kv8Chunk {
    u32x4 k[2][2];   // [tile][load j]
    u32x4 v[4];
};

__device__ __forceinline__ u32x4 kv8_load(const uint8_t *p, int nt) {
    return nt ? __builtin_nontemporal_load((const u32x4 *)p) : *(const u32x4 *)p;
}

__device__ __forceinline__ void kv8_issue(const uint8_t *k8, const uint8_t *v8, int c0, int kcap, Kv8Chunk &r, int nt) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int q4 = lane >> 4, c16 = lane & 15, r8 = lane >> 3, d16 = (lane & 7) * 16;
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const long key = min(c0 + 32 * wid + 16 * t + c16, kcap);
#pragma unroll
        for (int j = 0; j < 2; j++) r.k[t][j] = kv8_load(k8 + key * 128 + 64 * j + 16 * q4, nt);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) r.v[i] = kv8_load(v8 + (long)min(c0 + 32 * wid + 8 * i + r8, kcap) * 128 + d16, nt);
}

// eight bytes (two dwords) -> the eight fp16 values float(q) 2^-s
__device__ __forceinline__ half8 kv8_half8(uint32_t lo, uint32_t hi, float down) {
    const half2v a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)lo, down, false);
    const half2v b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)lo, down, true);
    const half2v c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)hi, down, false);
    const half2v d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)hi, down, true);
    return half8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

struct Kv8St {
    float m0, m1, l0, l1;     // running max / sum per head (uniform in the wave)
    float o0[16], o1[16];     // this lane's partial O over its keys (8 i + r8), dims d16 .. + 15, in units of 2^s
};

// one 128-key chunk for this wave (keys c0 + 32 wid .. + 31)
__device__ __forceinline__ void kv8_step(const DecodeAttnArgs &a, const half8 (*qa)[2], const uint8_t *knew, const uint8_t *vnew,
                                         int c0, int pos, float down, const Kv8Chunk &r, Kv8St &st) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int q4 = lane >> 4, c16 = lane & 15, r8 = lane >> 3, d16 = (lane & 7) * 16;
    float s0[2], s1[2];
    bool ok[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int key = c0 + 32 * wid + 16 * t + c16;
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32x4 kb = key == pos ? *(const u32x4 *)&knew[64 * j + 16 * q4] : r.k[t][j];
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa[j][0], kv8_half8(kb[0], kb[1], down), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa[j][1], kv8_half8(kb[2], kb[3], down), acc, 0, 0, 0);
        }
        // lanes 0-15 (q4 = 0): S[head r][key c16 of tile t] in acc[r]
        ok[t] = q4 == 0 && key <= pos;
        s0[t] = ok[t] ? acc[0] * a.scale : -INFINITY;
        s1[t] = ok[t] ? acc[1] * a.scale : -INFINITY;
    }
    const float M0 = fmaxf(st.m0, wave_max(fmaxf(s0[0], s0[1]))), M1 = fmaxf(st.m1, wave_max(fmaxf(s1[0], s1[1])));
    const float r0 = M0 == -INFINITY ? 1.f : expf(st.m0 - M0), r1 = M1 == -INFINITY ? 1.f : expf(st.m1 - M1);
    float p0[2], p1[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        p0[t] = ok[t] ? expf(s0[t] - M0) : 0.f;
        p1[t] = ok[t] ? expf(s1[t] - M1) : 0.f;
    }
    st.l0 = st.l0 * r0 + wave_sum(p0[0] + p0[1]);
    st.l1 = st.l1 * r1 + wave_sum(p1[0] + p1[1]);
    st.m0 = M0;
    st.m1 = M1;
#pragma unroll
    for (int e = 0; e < 16; e++) { st.o0[e] *= r0; st.o1[e] *= r1; }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int kl = 8 * i + r8;   // this lane's key of load i: tile i / 2, whose lane kl % 16 holds its p
        const float w0 = __shfl(p0[i >> 1], kl & 15, 64), w1 = __shfl(p1[i >> 1], kl & 15, 64);
        const u32x4 vb = c0 + 32 * wid + kl == pos ? *(const u32x4 *)&vnew[d16] : r.v[i];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const floatx2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb[d], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb[d], true);
            const float v[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                st.o0[4 * d + e] = fmaf(v[e], w0, st.o0[4 * d + e]);
                st.o1[4 * d + e] = fmaf(v[e], w1, st.o1[4 * d + e]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void decode_attn_seq_fp8_kernel(DecodeAttnArgs a, uint8_t *k8l, uint8_t *v8l, int exp) {
    __shared__ __attribute__((aligned(16))) uint16_t qs[2][128];
    __shared__ __attribute__((aligned(16))) uint8_t knew[128];
    __shared__ __attribute__((aligned(16))) uint8_t vnew[128];
    __shared__ float wst[4][2][2];                                  // per wave: (m, l) per head
    __shared__ __attribute__((aligned(16))) float wo[4][2][128];   // per wave: O per head
    stamp_start(a.stamp);
    const int g = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int QD = a.n_head * 128, KD = a.n_kv_head * 128;
    const int q4 = lane >> 4, c16 = lane & 15, r8 = lane >> 3, d16 = (lane & 7) * 16;
    const long cbase = ((long)b * a.n_kv_head + g) * a.max_ctx;
    uint16_t *kc = a.kc + cbase * 128, *vc = a.vc + cbase * 128;
    uint8_t *k8 = k8l + cbase * 128, *v8 = v8l + cbase * 128;
    const int pos = min(max(a.pos[b], 0), a.max_ctx - 1), nkv = pos + 1;
    const float up = ldexpf(1.0f, exp), down = ldexpf(1.0f, -exp);
    Kv8Chunk A, B;
    kv8_issue(k8, v8, 0, pos, A, a.kv_nt);
    // ---- the token's q / k / v: rms norm * weight + NEOX RoPE (decode_attn_body), the new fp16 K / V / V^T rows as
    //      decode_attn_seq_kernel writes them; the shadow's rows at pos by the rule, to the shadow and to LDS
    {
        const float *raw = a.qkv + (long)b * (QD + 2 * KD);
        const float *src = wid < 2 ? raw + (2 * g + wid) * 128 : raw + QD + (wid - 2) * KD + g * 128;
        const float x0 = src[lane], x1 = src[lane + 64];
        const float *nw = wid < 2 ? a.q_norm : a.k_norm;
        const float2 cs = *(const float2 *)(a.rope + ((long)pos * 64 + lane) * 2);
        uint16_t r0, r1;
        if (wid < 3) {
            const double ss = wave_sum_d((double)(x0 * x0) + (double)(x1 * x1));
            const float scale = 1.0f / sqrtf((float)(ss / 128.0) + a.eps);
            const float y0 = fmul_rn(fmul_rn(x0, scale), nw[lane]), y1 = fmul_rn(fmul_rn(x1, scale), nw[lane + 64]);
            r0 = f_to_u16(y0 * cs.x - y1 * cs.y);
            r1 = f_to_u16(y0 * cs.y + y1 * cs.x);
        } else {
            r0 = f_to_u16(x0);
            r1 = f_to_u16(x1);
        }
        if (wid < 2) {
            qs[wid][lane] = r0;
            qs[wid][lane + 64] = r1;
        } else {
            uint16_t *c16p = wid == 2 ? kc : vc;
            c16p[(long)pos * 128 + lane] = r0;
            c16p[(long)pos * 128 + lane + 64] = r1;
            if (wid == 3) {
                uint16_t *t = a.vt + ((long)b * a.n_kv_head + g) * 128 * vt_ctx(a.max_ctx);
                t[vt_index(pos, lane)] = r0;
                t[vt_index(pos, lane + 64)] = r1;
            }
            const uint32_t q2 = kv8_pack2(u16_to_f(r0), u16_to_f(r1), up);
            uint8_t *c8 = wid == 2 ? k8 : v8, *n8 = wid == 2 ? knew : vnew;
            n8[lane] = (uint8_t)q2;
            n8[lane + 64] = (uint8_t)(q2 >> 8);
            c8[(long)pos * 128 + lane] = (uint8_t)q2;
            c8[(long)pos * 128 + lane + 64] = (uint8_t)(q2 >> 8);
        }
    }
    __syncthreads();
    half8 qa[2][2];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int h = 0; h < 2; h++)
            qa[j][h] = c16 < 2 ? *(const half8 *)&qs[c16][64 * j + 16 * q4 + 8 * h] : half8{0, 0, 0, 0, 0, 0, 0, 0};
    Kv8St st;
    st.m0 = st.m1 = -INFINITY;
    st.l0 = st.l1 = 0.f;
#pragma unroll
    for (int e = 0; e < 16; e++) { st.o0[e] = 0.f; st.o1[e] = 0.f; }
    for (int c0 = 0; c0 < nkv; c0 += 256) {   // two chunks a trip, each prefetching the other set
        if (c0 + 128 < nkv) kv8_issue(k8, v8, c0 + 128, pos, B, a.kv_nt);
        kv8_step(a, qa, knew, vnew, c0, pos, down, A, st);
        if (c0 + 128 >= nkv) break;
        if (c0 + 256 < nkv) kv8_issue(k8, v8, c0 + 256, pos, A, a.kv_nt);
        kv8_step(a, qa, knew, vnew, c0 + 128, pos, down, B, st);
    }
    // ---- merge: lanes of equal d16 hold partial O over their keys (r8 = 0 .. 7): sum over r8, then over waves
#pragma unroll
    for (int e = 0; e < 16; e++) {
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) {
            st.o0[e] += __shfl_xor(st.o0[e], o, 64);
            st.o1[e] += __shfl_xor(st.o1[e], o, 64);
        }
    }
    if (r8 == 0) {
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            *(floatx4 *)&wo[wid][0][d16 + e] = floatx4{st.o0[e], st.o0[e + 1], st.o0[e + 2], st.o0[e + 3]};
            *(floatx4 *)&wo[wid][1][d16 + e] = floatx4{st.o1[e], st.o1[e + 1], st.o1[e + 2], st.o1[e + 3]};
        }
    }
    if (lane == 0) {
        wst[wid][0][0] = st.m0; wst[wid][0][1] = st.l0;
        wst[wid][1][0] = st.m1; wst[wid][1][1] = st.l1;
    }
    __syncthreads();
    const int hh = tid >> 7, d = tid & 127;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; w++) M = fmaxf(M, wst[w][hh][0]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const float mw = wst[w][hh][0];
        const float f = mw == -INFINITY ? 0.f : expf(mw - M);
        L = fmaf(wst[w][hh][1], f, L);
        O = fmaf(wo[w][hh][d], f, O);
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const float v = (O * inv) * down;   // V's 2^-s
    const long e = (long)b * QD + (2 * g + hh) * 128 + d;
    if (a.outq) {   // quantised for the Q8_0 o-proj: a 32-block = 32 lanes of one wave
        float am = fabsf(v);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
        a.outq[e] = q8_quant(v, am);
        if ((d & 31) == 0) a.outd[e >> 5] = q8_scale(am);
    } else if (a.out32) a.out32[e] = v;
    else a.out[e] = f_to_u16(v);
    stamp_end(a.stamp);
}

bool decode_attention_fp8_covers(int n_head, int n_kv_head) { return n_kv_head > 0 && n_head == 2 * n_kv_head; }

bool launch_decode_attention_fp8(const DecodeAttnArgs &a, uint8_t *k8, uint8_t *v8, int exp, hipStream_t s) {
    if (!decode_attention_fp8_covers(a.n_head, a.n_kv_head) || a.B <= 0 || a.B > 65535 || a.max_ctx <= 0 || !k8 || !v8 ||
        exp < kKvFp8ExpMin || exp > kKvFp8ExpMax || (!a.out && !a.out32 && !(a.outq && a.outd))) {
        note_declined_shape("launch_decode_attention_fp8", a.n_head, a.n_kv_head, a.B);
        return false;
    }
    hipLaunchKernelGGL(decode_attn_seq_fp8_kernel, dim3(a.n_kv_head, a.B), dim3(256), 0, s, a, k8, v8, exp);
    note_kernel("decode_seq_fp8", 1, 128);
    return true;
}

}  // namespace qasr
