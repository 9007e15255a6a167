// sample.hip -- temperature sampling (kernels.h "sampling"): a seeded Gumbel-max draw
// from the fp32 logits a decode step or prefill wrote.
//   sample_keys_kernel    every candidate column's key l * inv_T + G(u), u from Philox4x32-10 keyed by the
//                         context seed and counted by (column group, t, clip, sample); the row's largest
//                         argmax_key folded into skey[row] by one 64-bit atomicMax a workgroup
//   sample_finish_kernel  the drawn token out of skey into d_tok / d_hist, t advanced, skey re-armed
// A draw depends on (seed, clip, sample, t) and the row's logits alone: the maximum of distinct keys does
// not depend on the grid or on the order the workgroups finish in.  The per-row identities and the scalars
// (inv_T, cut, seed) are read from device memory, so a captured step serves any of their values.
#include <algorithm>

#include "dev_common.h"
#include "kernels.h"

namespace qasr {

// ------------------------------------------------------------------ Philox
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// G(u), u = ((w >> 9) + 0.5) * 2^-23: (2 (w >> 9) + 1) is a 24-bit odd integer, exact in fp32, so u is
// exact, inside (0, 1) and never an end point; logf is the library's (not the hardware log2 path)
__device__ __forceinline__ float gumbel_of(uint32_t w) {
    const float u = (float)(2u * (w >> 9) + 1u) * 0x1p-24f;
    return -logf(-logf(u));
}

// ------------------------------------------------------------------ keys
// grid (slice, row), 256 threads.  A slice is `slice_groups` groups of 4 consecutive columns (so it starts
// on a multiple of 4); thread i takes groups i, i + 256, ... of its slice, one Philox call a group.
static constexpr int kSampleThreads = 256;

__global__ __launch_bounds__(kSampleThreads) void sample_keys_kernel(SampleArgs a, int slice_groups) {
    __shared__ unsigned long long s_best[kSampleThreads / 64];
    const int row = blockIdx.y, src = row / a.src_div, tid = threadIdx.x;
    const float *l = a.logits + (size_t)src * a.ld;
    const int gr = a.greedy[src], g = (unsigned)gr < (unsigned)a.n_valid ? gr : 0;   // (the row's argmax: always inside)
    const SampleScalars sc = *a.sc;
    // a candidate: l[j] >= l[g] + cut, one add and one compare (a NaN logit compares false); g always is one
    const float thr = l[g] + sc.cut;
    const uint32_t t = (uint32_t)a.t[row], clip = (uint32_t)a.clip[row], smp = (uint32_t)a.sample[row];
    const bool vec = (a.ld & 3) == 0;   // rows 16-byte aligned
    const int g0 = blockIdx.x * slice_groups, g1 = min(g0 + slice_groups, (a.n_valid + 3) >> 2);
    unsigned long long best = 0ull;
    for (int grp = g0 + tid; grp < g1; grp += kSampleThreads) {
        const int j0 = 4 * grp;
        float v[4];
        if (vec && j0 + 4 <= a.n_valid) {
            const float4 q = *(const float4 *)(l + j0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = j0 + i < a.n_valid ? l[j0 + i] : __builtin_nanf("");
        }
        bool cand[4], any = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            cand[i] = j0 + i < a.n_valid && (v[i] >= thr || j0 + i == g);
            any |= cand[i];
        }
        if (!any) continue;   // (min_p cuts most of a row: no Philox call for a group without a candidate)
        uint32_t w[4];
        philox4x32_10((uint32_t)grp, t, clip, smp, sc.seed_lo, sc.seed_hi, w);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!cand[i]) continue;
            const unsigned long long k = argmax_key(fmaf(v[i], sc.inv_T, gumbel_of(w[i])), j0 + i);
            best = k > best ? k : best;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_xor(best, o, 64);
        best = x > best ? x : best;
    }
    if ((tid & 63) == 0) s_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kSampleThreads / 64; w++) best = s_best[w] > best ? s_best[w] : best;
        if (best) atomicMax(a.skey + row, best);   // (no candidate in this slice: nothing to fold)
    }
}

// one thread a row
__global__ __launch_bounds__(256) void sample_finish_kernel(SampleArgs a) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= a.R) return;
    const unsigned long long k = a.skey[row];
    const int tok = argmax_key_idx(k);
    a.tok[row] = tok;
    if (a.hist) a.hist[(size_t)row * a.hist_stride + *a.step] = tok;
    if (a.key_out) a.key_out[row] = argmax_key_val(k);
    a.t[row] += 1;
    a.skey[row] = 0ull;   // zero at rest
}

int sample_slices(int R, int n_valid) {
    const int groups = (n_valid + 3) / 4;
    // groups a thread: 1 up to 4 rows (a batch-1 step spreads its row over ~150 workgroups), 2 up to 32, then 4
    // (the row's work is fixed, and from 64 rows on the grid fills the device either way)
    const int per = R <= 4 ? 1 : R <= 32 ? 2 : 4;
    return std::max(1, (groups + kSampleThreads * per - 1) / (kSampleThreads * per));
}

bool launch_sample(const SampleArgs &a, int slices, hipStream_t s) {
    if (a.R <= 0 || a.ld <= 0 || a.n_valid <= 0 || a.n_valid > a.ld || a.src_div < 1 || a.R % a.src_div != 0 || a.R > 65535 ||
        slices < 0 || !a.sc || !a.skey || !a.t || !a.clip || !a.sample || !a.tok || (a.hist && !a.step))
        return false;
    const int groups = (a.n_valid + 3) / 4;
    if (slices == 0) slices = sample_slices(a.R, a.n_valid);
    slices = std::min(slices, groups);
    const int slice_groups = (groups + slices - 1) / slices;
    hipLaunchKernelGGL(sample_keys_kernel, dim3((groups + slice_groups - 1) / slice_groups, a.R), dim3(kSampleThreads), 0, s, a,
                       slice_groups);
    hipLaunchKernelGGL(sample_finish_kernel, dim3((a.R + 255) / 256), dim3(256), 0, s, a);
    note_kernel("sample", 2, slices, slice_groups);
    return true;
}

// ------------------------------------------------------------------ test only
// out[i] = G(u_n), n = n0 + i: the device's value for every u the rule can produce (n < 2^23)
__global__ void sample_gumbel_dump_kernel(uint32_t n0, uint32_t n, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = gumbel_of((n0 + i) << 9);
}

void launch_sample_gumbel_dump(uint32_t n0, uint32_t n, float *out, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(sample_gumbel_dump_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n0, n, out);
}

}  // namespace qasr
