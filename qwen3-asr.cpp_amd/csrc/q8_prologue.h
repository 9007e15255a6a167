// q8_prologue.h -- the activation prologue of the <= 8-row Q8_0 GEMVs (gemv_q8_kernel in gemm.hip,
// gemv_rows_q8_kernel in gemv_rows_q8.hip), stated once so that both multiply the same quants and scales.
//
// A workgroup of 256 threads prepares the rows: thread tid owns elements p * 1024 + 4 tid .. + 3 of every row, a
// Q8_0 block of 32 is 8 consecutive lanes.  Per row: float squares summed in double (the thread's elements in
// ascending k, then wave_sum_d, then the four waves' partials added in wave order), scale = 1 / sqrtf((float)(tot / K)
// + eps), v = fmul_rn(fmul_rn(x, scale), norm_w), amax over the block's lanes, d = fp16(amax / 127),
// q = rint(v * (127 / amax)) -- ggml's rms_norm + mul + quantize_row_q8_0.
#pragma once

#include "dev_common.h"
#include "kernels.h"

namespace qasr {

// elements k .. k + 3 of row m: fp32 x, or the embedding row of the layer-0 gather (workgroup 0 keeps it in x_store)
__device__ __forceinline__ float4 q8p_load(const GemvArgs &g, int m, int k) {
    if (g.embd_ids) {
        const uint2 hv = *(const uint2 *)(g.embd + (long)g.embd_ids[m] * g.K + k);
        const float4 v = make_float4(u16_to_f(hv.x & 0xffff), u16_to_f(hv.x >> 16), u16_to_f(hv.y & 0xffff), u16_to_f(hv.y >> 16));
        if (g.x_store && blockIdx.x == 0) *(float4 *)(g.x_store + (long)m * g.ldx + k) = v;
        return v;
    }
    return *(const float4 *)(g.x + (long)m * g.ldx + k);
}

__device__ __forceinline__ void q8p_sq(double &ss, const float4 &v) {
    ss += (double)(v.x * v.x);
    ss += (double)(v.y * v.y);
    ss += (double)(v.z * v.z);
    ss += (double)(v.w * v.w);
}

// the row's RMS scale from the four waves' sums (1 without a norm)
__device__ __forceinline__ float q8p_row_scale(const GemvArgs &g, double w0, double w1, double w2, double w3) {
    if (!g.norm_w) return 1.0f;
    const double tot = w0 + w1 + w2 + w3;
    return 1.0f / sqrtf((float)(tot / g.K) + g.eps);
}

// norm and quantise the thread's four elements at k (live: the row is < M and k < K; else they count as zeros).
// Every lane of the wave calls it (the block's amax goes through xor-shuffles).  Returns the four quants packed,
// d = the block's scale.
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

}  // namespace qasr
