// act_prologue.h -- the activation prologue of the <= 8-row GEMVs (gemv_q8_kernel in gemm.hip, the rows kernels of
// gemv_rows.hip and gemv_rows_q8.hip; gemv_kernel states the same inline), so that all multiply the same values and scales.
// 256 threads prepare the rows: thread tid owns elements p * 1024 + 4 tid .. + 3 of every row.  Per row: float squares
// summed in double (the thread's in ascending k, then wave_sum_d, then the four waves' partials in wave order), scale =
// 1 / sqrtf((float)(tot / K) + eps), v = fmul_rn(fmul_rn(x, scale), norm_w) -- ggml's rms_norm + mul -- then a finish.
#pragma once

#include "dev_common.h"
#include "kernels.h"

namespace qasr {

// elements k .. k + 3 of row m: fp32 x, or the embedding row of the layer-0 gather (workgroup 0 keeps it in x_store)
__device__ __forceinline__ float4 xp_load(const GemvArgs &g, int m, int k) {
    if (g.embd_ids) {
        const uint2 hv = *(const uint2 *)(g.embd + (long)g.embd_ids[m] * g.K + k);
        const float4 v = make_float4(u16_to_f(hv.x & 0xffff), u16_to_f(hv.x >> 16), u16_to_f(hv.y & 0xffff), u16_to_f(hv.y >> 16));
        if (g.x_store && blockIdx.x == 0) *(float4 *)(g.x_store + (long)m * g.ldx + k) = v;
        return v;
    }
    return *(const float4 *)(g.x + (long)m * g.ldx + k);
}

__device__ __forceinline__ void xp_sq(double &ss, const float4 &v) {
    ss += (double)(v.x * v.x); ss += (double)(v.y * v.y);
    ss += (double)(v.z * v.z); ss += (double)(v.w * v.w);
}

// the row's RMS scale from the four waves' sums (1 without a norm)
__device__ __forceinline__ float xp_row_scale(const GemvArgs &g, double w0, double w1, double w2, double w3) {
    if (!g.norm_w) return 1.0f;
    const double tot = w0 + w1 + w2 + w3;
    return 1.0f / sqrtf((float)(tot / g.K) + g.eps);
}

// the f16 finish: norm the thread's four elements at k < K, round each once to fp16
__device__ __forceinline__ uint2 xp_f16x4(const GemvArgs &g, const float4 &x, int k, float scale) {
    float v[4] = {x.x, x.y, x.z, x.w};
    if (g.norm_w) {
        const float4 w = *(const float4 *)(g.norm_w + k);
        v[0] = fmul_rn(fmul_rn(v[0], scale), w.x); v[1] = fmul_rn(fmul_rn(v[1], scale), w.y);
        v[2] = fmul_rn(fmul_rn(v[2], scale), w.z); v[3] = fmul_rn(fmul_rn(v[3], scale), w.w);
    }
    return make_uint2(f_to_u16(v[0]) | ((uint32_t)f_to_u16(v[1]) << 16), f_to_u16(v[2]) | ((uint32_t)f_to_u16(v[3]) << 16));
}

// the Q8_0 finish (ggml's quantize_row_q8_0; a block of 32 is 8 lanes, amax by xor-shuffles: every lane of the wave calls
// it; live: row < M and k < K, else the elements count as zeros): the four quants packed, d = fp16(amax / 127)
__device__ __forceinline__ uint32_t q8p_quant(const GemvArgs &g, const float4 &x, int k, float scale, bool live, float &d) {
    float v[4] = {x.x, x.y, x.z, x.w}, amax = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (g.norm_w && k < g.K) v[e] = fmul_rn(fmul_rn(v[e], scale), g.norm_w[k + e]);
        if (!live) v[e] = 0.0f;
        amax = fmaxf(amax, fabsf(v[e]));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
    uint32_t u = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) u |= (uint32_t)(uint8_t)q8_quant(v[e], amax) << (8 * e);
    d = q8_scale(amax);
    return u;
}

// the register form (K <= 1024 KP): rows into xr (past M or K: zeros); with a norm, red[0 .. 3][m] behind a barrier
template <int MR, int KP, int RM>
__device__ __forceinline__ void xp_load_rows(const GemvArgs &g, double (&red)[4][RM], float4 (&xr)[MR][KP]) {
    const int tid = threadIdx.x;
    double ss[MR];
#pragma unroll
    for (int m = 0; m < MR; m++) {
        ss[m] = 0.0;
#pragma unroll
        for (int p = 0; p < KP; p++) {
            const int k = p * 1024 + tid * 4;
            xr[m][p] = m < g.M && k < g.K ? xp_load(g, m, k) : make_float4(0.f, 0.f, 0.f, 0.f);
            xp_sq(ss[m], xr[m][p]);
        }
    }
    if (!g.norm_w) return;
#pragma unroll
    for (int m = 0; m < MR; m++) {
        const double t = wave_sum_d(ss[m]);
        if ((tid & 63) == 0) red[tid >> 6][m] = t;
    }
    __syncthreads();
}

// The rows of the 2 .. 8-row f16 kernel: put(m, k, v, scale) finishes elements k .. k + 3 < K of row m < M.  (The Q8_0 rows
// kernel keeps its own copy of these two loops, on every lane: through this one it measured 1 .. 3 % slower)
template <class Put>
__device__ __forceinline__ void xp_rows(const GemvArgs &g, double (&red)[4][8], Put put) {
    const int tid = threadIdx.x, K = g.K, M = g.M, np = (K - tid * 4 + 1023) >> 10;
    if (K <= 2048) {   // the rows stay in registers between the sum and the finish (the hidden-2048 decoders)
        float4 xr[8][2];
        xp_load_rows(g, red, xr);
#pragma unroll
        for (int m = 0; m < 8; m++) {
            if (m >= M) break;
            const float scale = xp_row_scale(g, red[0][m], red[1][m], red[2][m], red[3][m]);
#pragma unroll
            for (int p = 0; p < 2; p++)
                if (p * 1024 + tid * 4 < K) put(m, p * 1024 + tid * 4, xr[m][p], scale);
        }
        return;
    }
    if (g.norm_w) {    // longer rows are read twice (the second time from the caches)
        for (int m = 0; m < M; m++) {
            double ss = 0.0;
            for (int k = tid * 4; k < K; k += 1024) xp_sq(ss, xp_load(g, m, k));
            ss = wave_sum_d(ss);
            if ((tid & 63) == 0) red[tid >> 6][m] = ss;
        }
        __syncthreads();
    }
    for (int m = 0; m < M; m++) {
        const float scale = xp_row_scale(g, red[0][m], red[1][m], red[2][m], red[3][m]);
        for (int p = 0; p < np; p++) put(m, p * 1024 + tid * 4, xp_load(g, m, p * 1024 + tid * 4), scale);
    }
}

}  // namespace qasr
