// lmhead.hip -- the decode-batch LM head in one launch (9 <= M <= 128 rows):
// final RMS norm + tied-embedding GEMM (151936 x 1024 f16) + first-index
// argmax + the greedy step's bookkeeping (src/text_decoder.cpp forward's last
// ggml_rms_norm / ggml_mul / ggml_mul_mat over model.output, then
// src/qwen3_asr.cpp:270-296's sample_greedy per sequence).
//
// The skinny GEMM (gemm_skinny.hip) took 140-150 us for these 311 MB: 2374
// workgroups each streamed 128 KB of weights but re-read the whole 64 x 1024
// activation (another 128 KB) through LDS-DMA, every 64-column tile folded its
// keys into the same 64 global argmax words (152k atomics on 64 addresses), and
// the norm, the key reset and the bookkeeping were five more launches.
//
// Here one persistent workgroup per CU normalises the rows once into LDS
// (rms_row's arithmetic: the values launch_rmsnorm_f16 writes), then each wave
// streams a contiguous run of 16-column units of the weight matrix through a
// D-deep ring of fragment registers (nontemporal buffer loads, out-of-range
// items read as zeros without a memory access), multiplies them against the
// LDS rows on v_mfma_f32_16x16x32_f16 (K ascending in 32-wide steps, fp32
// accumulation; even and odd chunks in two accumulators summed at the end, the
// order of gemm_skinny_kernel<4, 4, 2>'s two K waves, so the logits are
// bit-identical to the separate launches'), keeps a per-lane running best key per row across all its
// units, and reduces those once at the end: one atomicMax per row per
// workgroup, then the last workgroup decodes the tokens (tok, hist[step+1],
// pos += 1, n_kv += 1, step += 1) and re-arms amax / done (zero at rest).
//
// LSE = true (GemvArgs::lp_part set, option token_logprobs) adds the
// log-probability of each row's argmax to the same launch: beside its best key
// every lane keeps a running (m, s) of the log-sum-exp over the columns it
// owns (dev_common.h lse_add), reduced over the 16 column lanes by
// xor-shuffles and over the waves through LDS in wave order; each workgroup
// publishes one packed (m, s) per row to lp_part[workgroup][row] with an
// 8-byte agent-scope atomic store -- past the workgroup's XCD L2, complete
// before the s_waitcnt vmcnt(0) that precedes its `done` arrival -- and the
// last workgroup reads them with agent-scope atomic loads (as it reads amax),
// merges them per row in a fixed order (LPR lanes a row, each over the
// workgroups w = lane, lane + LPR, ... ascending in rounds of 16, then an
// xor-shuffle tree)
// and writes lp_out / lp_hist next to tok_out / hist.  No floating-point
// atomics: the value does not depend on arrival order.  LSE = false is the
// kernel as it was.
//
// TK = true (GemvArgs::tk_part set, option top_k; lmhead_batch_kernel only,
// implies LSE) adds the K largest keys of every row: each workgroup keeps a
// sorted K-list a row in LDS (tk_insert), publishes it beside its (m, s), and
// the last workgroup merges the lists behind the K largest slot-0 keys
// (tk_finish).  TK = false is the kernel as it was.
#include "dev_common.h"
#include "kernels.h"

namespace qasr {

namespace {

constexpr int LMH_K = 1024;   // hidden width this kernel is built for (host checks)
typedef __attribute__((address_space(3))) void lds_void_l;
typedef __attribute__((address_space(1))) void glb_void_l;

// LDS row layout: 128 chunks of 16 B per row, chunk ch stored at ch ^ (row & 15)
// so the 16 rows of a fragment read hit 16 distinct 16-B bank groups
__device__ __forceinline__ int lmh_off(int row, int k) {   // element offset of (row, k), k % 8 == 0 .. +7
    const int ch = k >> 3;
    return row * LMH_K + ((ch ^ (row & 15)) << 3) + (k & 7);
}

// last workgroup, every thread: row tid / LPR's (m, s) over the G workgroups' partials, 16 loads in
// flight a lane; then the log-probability of the row's argmax (the value in its amax key, still
// armed) to lp_out / lp_hist[row][st + 1]
// (ms_out non-null, the top-K variant: the row's (m, s) is left there too)
template <int LPR>
__device__ __forceinline__ void lse_finish(const GemvArgs &g, int M, int G, int st, float2 *ms_out = nullptr) {
    const int tid = threadIdx.x, row = tid / LPR, sub = tid % LPR;
    float m = -INFINITY, s = 0.f;
    if (row < M) {
        for (int w0 = sub; w0 < G; w0 += 16 * LPR) {
            unsigned long long p[16];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int w = w0 + u * LPR;
                p[u] = __hip_atomic_load(g.lp_part + (long)(w < G ? w : w0) * 128 + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // the round's pair: its largest m, then 16 independent terms (one dependent merge a round, not 16)
            float mr = -INFINITY, sr = 0.f;
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (w0 + u * LPR < G) mr = fmaxf(mr, lse_pack_m(p[u]));
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (w0 + u * LPR < G) {
                    const float mu = lse_pack_m(p[u]), su = lse_pack_s(p[u]);
                    sr += mu == mr ? su : su * lse_exp(mu - mr);
                }
            lse_merge(m, s, mr, sr);
        }
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    if (sub == 0 && row < M) {
        const unsigned long long k = __hip_atomic_load(g.amax + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float lp = lse_logprob(argmax_key_val(k), m, s);
        g.lp_out[row] = lp;
        g.lp_hist[(long)row * g.hist_stride + st + 1] = lp;
        if (ms_out) ms_out[row] = make_float2(m, s);
    }
}

// ---- top-K alternatives (TK = true, GemvArgs::tk_part set, option top_k) ----
// A sorted list of K distinct keys in LDS, slot 0 the largest, kept by a chain of
// 64-bit atomicMax: slot j keeps the larger of its key and the arriving one and
// the smaller carries on to slot j + 1.  Every key that ever reaches slot j but
// its final maximum leaves it exactly once, so slot j ends with the (j + 1)-th
// largest key inserted, whatever the order of arrival.
__device__ __forceinline__ void tk_insert(unsigned long long *list, unsigned long long k, int K) {
    for (int j = 0; j < K && k != 0ull; j++) {
        const unsigned long long old = atomicMax(list + j, k);
        k = old < k ? old : k;
    }
}
// the list's K-th key (0 while it is not full): no key below it can enter any more.  A stale read is lower, so conservative.
__device__ __forceinline__ unsigned long long tk_kth(const unsigned long long *list, int K) {
    return __hip_atomic_load(list + K - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
constexpr int TKS = 8;   // list stride (TOPK_MAX)

// last workgroup, every thread (row tid / LPR, lane sub of LPR >= K): the K largest of the row's G slot-0
// keys (lists are sorted: only the workgroups behind them can hold one of the row's K largest keys; a key's
// column names its workgroup), then the K largest of those <= K lists' keys, as ids and log-probabilities
// with the row's (m, s) from lse_finish.  l1 / l2: two zeroed LDS lists a row.
template <int LPR, int WPG>
__device__ __forceinline__ void tk_finish(const GemvArgs &g, int M, int G, int st, unsigned long long *l1, unsigned long long *l2,
                                          const float2 *ms) {
    const int tid = threadIdx.x, row = tid / LPR, sub = tid % LPR, K = g.tk_k;
    if (row < M) {
        for (int w = sub; w < G; w += LPR) {
            const unsigned long long k = __hip_atomic_load(g.tk_part + ((long)w * 128 + row) * TKS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k > tk_kth(l1 + row * TKS, K)) tk_insert(l1 + row * TKS, k, K);
        }
    }
    __syncthreads();
    if (row < M && sub < K) {
        const unsigned long long k0 = l1[row * TKS + sub];
        if (k0) {
            const long U = g.N >> 4, TW = (long)G * WPG, u = argmax_key_idx(k0) >> 4;
            const int w = (int)((((u + 1) * TW + U - 1) / U - 1) / WPG);   // the wave whose units [gw U / TW, (gw + 1) U / TW) hold u
            for (int j = 0; j < K; j++)
                tk_insert(l2 + row * TKS, __hip_atomic_load(g.tk_part + ((long)w * 128 + row) * TKS + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), K);
        }
    }
    __syncthreads();
    if (row < M && sub < K) {
        const unsigned long long k = l2[row * TKS + sub];
        const int id = k ? argmax_key_idx(k) : -1;
        const float lp = k ? lse_logprob(argmax_key_val(k), ms[row].x, ms[row].y) : -INFINITY;
        g.tk_out[(long)row * K + sub] = id;
        g.tk_lp[(long)row * K + sub] = lp;
        const long h = ((long)row * g.hist_stride + st + 1) * K + sub;
        g.tk_hist[h] = id;
        g.tk_lphist[h] = lp;
    }
}

template <int MT, int WPG, int D, bool LSE, bool TK>
__global__ __launch_bounds__(64 * WPG) void lmhead_batch_kernel(GemvArgs g) {
    static_assert(LSE || !TK, "the top-K variant carries the log-sum-exp code");
    extern __shared__ __attribute__((aligned(16))) uint16_t xs[];   // [MT*16][LMH_K] fp16, swizzled
    __shared__ unsigned long long bestk[WPG][MT * 16];
    __shared__ float2 lsek[LSE ? WPG : 1][LSE ? MT * 16 : 1];
    __shared__ unsigned long long tk[TK ? MT * 16 * TKS : 1], tk2[TK ? MT * 16 * TKS : 1];   // TK: the workgroup's K keys a row
    __shared__ int last_wg, st;
    stamp_start(g.stamp);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int q = lane >> 4, c16 = lane & 15;
    const int M = g.M;
    if constexpr (TK) {   // (visible after the prologue's barrier)
        for (int e = tid; e < MT * 16 * TKS; e += 64 * WPG) tk[e] = 0ull;
    }

    // ---- this wave's units (16 weight rows each) and items (unit, 128-wide K chunk)
    const int U = g.N >> 4, TW = gridDim.x * WPG, gw = blockIdx.x * WPG + wid;
    const int u0 = (int)((long)gw * U / TW), u1 = (int)((long)(gw + 1) * U / TW);
    const int n_items = (u1 - u0) * (LMH_K / 128);
    const uint32_t wbytes = (uint32_t)((long)g.N * LMH_K * 2);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc((void *)g.W, (short)0, (int)wbytes, 0x00020000);
    u32x4 wb[D][4];
    auto load = [&](int b, int j) {
        const int u = u0 + (j >> 3), c = j & 7;
        const uint32_t base = (uint32_t)(((long)(u * 16 + c16) * LMH_K + c * 128 + q * 8) * 2);
#pragma unroll
        for (int s = 0; s < 4; s++)
            wb[b][s] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wsrd, j < n_items ? base + 64 * s : wbytes, 0, 2));
    };
#pragma unroll
    for (int b = 0; b < D; b++) load(b, b);

    // ---- prologue: rows -> RMS norm (rms_row<1024> arithmetic) -> fp16 LDS;
    //      the wave's rows in batches of RB, every load of a batch in flight
    //      together (one row at a time left the weight ring idle for ~10 us at 64 rows)
    constexpr int R = MT * 16 / WPG, RB = R < 4 ? R : 4;
    static_assert(R * WPG == MT * 16, "rows split evenly over the waves");
    float4 wv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) wv[i] = *(const float4 *)(g.norm_w + 4 * lane + 256 * i);
#pragma unroll
    for (int r0 = 0; r0 < R; r0 += RB) {
        float4 v[RB][4];
#pragma unroll
        for (int r = 0; r < RB; r++) {
            const int m = wid + WPG * (r0 + r);
            const float *xr = g.x + (long)(m < M ? m : 0) * g.ldx;
#pragma unroll
            for (int i = 0; i < 4; i++) v[r][i] = *(const float4 *)(xr + 4 * lane + 256 * i);
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
            const int m = wid + WPG * (r0 + r);
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++)
                s += ((double)fmul_rn(v[r][i].x, v[r][i].x) + (double)fmul_rn(v[r][i].y, v[r][i].y)) +
                     ((double)fmul_rn(v[r][i].z, v[r][i].z) + (double)fmul_rn(v[r][i].w, v[r][i].w));
            s = wave_sum_d(s);
            const float mean = (float)(s / LMH_K);
            const float scale = 1.0f / sqrtf(mean + g.eps);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint32_t lo = f_to_u16(fmul_rn(fmul_rn(v[r][i].x, scale), wv[i].x)) |
                              ((uint32_t)f_to_u16(fmul_rn(fmul_rn(v[r][i].y, scale), wv[i].y)) << 16);
                uint32_t hi = f_to_u16(fmul_rn(fmul_rn(v[r][i].z, scale), wv[i].z)) |
                              ((uint32_t)f_to_u16(fmul_rn(fmul_rn(v[r][i].w, scale), wv[i].w)) << 16);
                if (m >= M) lo = hi = 0u;   // rows past M: zeros
                *(uint2 *)(xs + lmh_off(m, 4 * lane + 256 * i)) = make_uint2(lo, hi);
            }
        }
    }
    __syncthreads();

    // ---- stream: item j = (unit u0 + j / 8, K chunk j % 8), ring slot j % D
    unsigned long long best[MT][4];
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) best[i][r] = 0ull;
    float lm[LSE ? MT : 1][4], ls[LSE ? MT : 1][4];   // LSE: this lane's (m, s) per row over its columns
    if constexpr (LSE) {
#pragma unroll
        for (int i = 0; i < MT; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) { lm[i][r] = -INFINITY; ls[i][r] = 0.f; }
    }
    floatx4 acc[2][MT];   // even / odd K chunks: the skinny kernel's two K waves (bit-identical logits)
    const int nvalid = g.n_valid > 0 ? g.n_valid : g.N;
    for (int j0 = 0; j0 < n_items; j0 += D) {
#pragma unroll
        for (int b = 0; b < D; b++) {
            const int j = j0 + b;
            if (j >= n_items) break;
            const int c = j & 7;
            if (c == 0) {
#pragma unroll
                for (int i = 0; i < MT; i++) acc[0][i] = acc[1][i] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int s = 0; s < 4; s++) {
#pragma unroll
                for (int i = 0; i < MT; i++) {
                    const half8 a8 = *(const half8 *)(xs + lmh_off(i * 16 + c16, c * 128 + 32 * s + 8 * q));
                    acc[c & 1][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, __builtin_bit_cast(half8, wb[b][s]), acc[c & 1][i], 0, 0, 0);
                }
            }
            load(b, j + D);
            if (c == 7) {   // unit done: C layout, lane (q, c16) = rows 16i + 4q + r, column 16u + c16
                const int col = (u0 + (j >> 3)) * 16 + c16;
#pragma unroll
                for (int i = 0; i < MT; i++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int row = i * 16 + 4 * q + r;
                        const float v = acc[0][i][r] + acc[1][i][r];
                        if (g.out_f32 && row < M) g.out_f32[(long)row * g.ldo + col] = v;
                        const unsigned long long key = col < nvalid ? argmax_key(v, col) : 0ull;
                        best[i][r] = key > best[i][r] ? key : best[i][r];
                        if constexpr (LSE) {
                            if (col < nvalid) lse_add(lm[i][r], ls[i][r], v);
                        }
                        if constexpr (TK) {
                            // against the list's K-th key as it is now, not as of the last unit: the eight waves finish
                            // their units at different times, and the later ones find the list the earlier ones filled
                            // (a full-key compare: a key below the K-th can never enter, an equal value with a lower
                            // column is above it)
                            unsigned long long *list = tk + (row < M ? row : 0) * TKS;
                            if (col < nvalid && row < M && key > tk_kth(list, g.tk_k)) tk_insert(list, key, g.tk_k);
                        }
                    }
            }
        }
    }

    // ---- per-row best over the 16 columns lanes, the waves, then the workgroups
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            unsigned long long k = best[i][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const unsigned long long t = __shfl_xor(k, o, 64);
                k = t > k ? t : k;
            }
            if (c16 == 0) bestk[wid][i * 16 + 4 * q + r] = k;
            if constexpr (LSE) {
                float m = lm[i][r], s = ls[i][r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
                if (c16 == 0) lsek[wid][i * 16 + 4 * q + r] = make_float2(m, s);
            }
        }
    __syncthreads();
    if (tid < M) {
        unsigned long long b = bestk[0][tid];
#pragma unroll
        for (int w = 1; w < WPG; w++) b = bestk[w][tid] > b ? bestk[w][tid] : b;
        const unsigned long long old = atomicMax(g.amax + tid, b);
        asm volatile("" ::"v"(old));   // returned value used: the max has been performed at L2
        if constexpr (LSE) {   // this workgroup's (m, s) of the row, the waves in order
            float m = lsek[0][tid].x, s = lsek[0][tid].y;
#pragma unroll
            for (int w = 1; w < WPG; w++) lse_merge(m, s, lsek[w][tid].x, lsek[w][tid].y);
            __hip_atomic_store(g.lp_part + (long)blockIdx.x * 128 + tid, lse_pack(m, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (TK) {   // this workgroup's K keys a row (complete at the barrier above), published as lp_part is
        for (int e = tid; e < M * TKS; e += 64 * WPG)
            if ((e & (TKS - 1)) < g.tk_k)
                __hip_atomic_store(g.tk_part + (long)blockIdx.x * 128 * TKS + e, tk[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) last_wg = __hip_atomic_fetch_add(g.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    __syncthreads();
    if (last_wg) {
        if (tid == 0) st = *g.step;
        if constexpr (TK) {   // (every thread is past its publication: the lists are free)
            for (int e = tid; e < MT * 16 * TKS; e += 64 * WPG) tk[e] = tk2[e] = 0ull;
        }
        __syncthreads();
        if constexpr (LSE) {
            constexpr int LPR = MT == 1 ? 32 : MT == 2 ? 16 : 8;   // lanes a row: 64 WPG threads over MT * 16 rows
            static_assert(LPR * MT * 16 <= 64 * WPG, "a lane group for every row");
            lse_finish<LPR>(g, M, gridDim.x, st, TK ? &lsek[0][0] : nullptr);
            __syncthreads();   // amax read before it is re-armed below
            if constexpr (TK) {
                static_assert(LPR >= TKS, "a lane for each of a row's K keys");
                tk_finish<LPR, WPG>(g, M, gridDim.x, st, tk, tk2, &lsek[0][0]);
            }
        }
        if (tid < M) {
            const unsigned long long k = __hip_atomic_load(g.amax + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int id = argmax_key_idx(k);
            g.tok_out[tid] = id;
            if (g.hist) g.hist[(long)tid * g.hist_stride + st + 1] = id;
            g.pos[tid] += 1;
            if (g.nkv) g.nkv[tid] += 1;
            __hip_atomic_store(g.amax + tid, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0) {
            if (!g.keep_step) *g.step = st + 1;
            __hip_atomic_store(g.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    stamp_end(g.stamp);
}

// 8 waves a CU with a 4-deep ring (tools/micro/lmh_bench.hip, MI355X: 16 rows
// 60.8 us against 68.9 with 16 waves x 3; 64 rows: 6- and 8-deep rings and 4
// waves x 8 or 12 slower)
template <int MT, bool LSE, bool TK, int WPG = 8, int D = 4>
void run_lmhead_v(const GemvArgs &g, hipStream_t s) {
    static int ncu_dev[64];   // per device: CU count once the LDS attribute is set
    int dev = 0;
    (void)hipGetDevice(&dev);
    int &ncu = ncu_dev[dev & 63];
    if (!ncu) {
        int n = 0;
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        (void)hipFuncSetAttribute((const void *)lmhead_batch_kernel<MT, WPG, D, LSE, TK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  MT * 16 * LMH_K * 2);
        ncu = n > 0 ? n : 256;
    }
    hipLaunchKernelGGL((lmhead_batch_kernel<MT, WPG, D, LSE, TK>), dim3(ncu), dim3(64 * WPG), MT * 16 * LMH_K * 2, s, g);
}
template <int MT>
void run_lmhead(const GemvArgs &g, hipStream_t s) {
    if (g.tk_part) run_lmhead_v<MT, true, true>(g, s);
    else if (g.lp_part) run_lmhead_v<MT, true, false>(g, s);
    else run_lmhead_v<MT, false, false>(g, s);
}

// ---- 65..128 rows in one launch, the embedding read once (round 6).  The
// 128 normalised rows (256 KB fp16) do not fit the LDS, so they live in
// registers: wave w holds rows 16w .. 16w + 15 as its 32 MFMA A fragments of
// K (128 VGPRs a lane), staged through LDS 32 rows at a time with
// lmhead_batch_kernel's norm arithmetic.  The weight units (16 vocabulary rows
// x 1024, 32 KB) stream through an L128_R-slot LDS ring by LDS-DMA
// (nontemporal, 16-B chunks XOR-swizzled by row so the fragment reads of 16
// rows hit distinct banks), two units in flight behind the one being read,
// and every unit is read by all eight waves: one HBM read of the 311 MB
// embedding per step instead of one per 64-row half.  Per (row tile, unit)
// the MFMA order is lmhead_batch_kernel's -- K chunks ascending, even / odd
// chunks in two accumulators summed at the end -- so the logits, and the
// tokens, are bit-identical to the two-launch path (tools/micro/lmh128_bench).
// Each wave owns its rows outright: per row one atomicMax per workgroup, then
// the last workgroup decodes the tokens as lmhead_batch_kernel does.  (A
// 9-slot ring of half units, seven in flight, ran slower: 97 against 86 us,
// profiles/r6/lmhead128_r9ring_ab.txt -- twice the barriers.)
constexpr int L128_R = 4;                  // ring slots (32 KB each)
constexpr int L128_UNIT = 16 * LMH_K;      // halves per unit
constexpr int L128_LDS = L128_R * L128_UNIT * 2;

template <bool LSE>
__global__ __launch_bounds__(512) void lmhead128_kernel(GemvArgs g) {
    extern __shared__ __attribute__((aligned(16))) uint16_t ring[];   // [L128_R][16][LMH_K], swizzled
    __shared__ int last_wg, st;
    stamp_start(g.stamp);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, c16 = lane & 15;
    const int M = g.M;
    const int U = g.N >> 4;
    const int u0 = (int)((long)blockIdx.x * U / gridDim.x), u1 = (int)((long)(blockIdx.x + 1) * U / gridDim.x);
    const int nu = u1 - u0;
    // unit j of this workgroup -> ring slot j % R: 32 pieces of 1 KB (row r = piece / 2), four per wave
    auto issue = [&](int j) {
        const int u = u0 + j;
        uint16_t *dst = ring + (j % L128_R) * L128_UNIT;
#pragma unroll
        for (int ii = 0; ii < 4; ii++) {
            const int i = wid * 4 + ii, r = i >> 1, p = ((i & 1) << 6) + lane;
            const uint16_t *src = g.W + ((long)(u * 16 + r) * LMH_K + ((p ^ (r & 15)) << 3));
            __builtin_amdgcn_global_load_lds((glb_void_l *)src, (lds_void_l *)(dst + i * 512), 16, 0, 2);
        }
    };
    // units 0, 1 land while the rows are normalised (slots 2, 3 hold the staging rows meanwhile)
    if (nu > 0) issue(0);
    if (nu > 1) issue(1);

    // ---- prologue: rows 32p .. 32p + 31 -> RMS norm -> fp16 staging (slots 2-3), then the two
    //      waves owning them take their A fragments; wave w normalises rows 32p + w + 8i
    uint16_t *xs = ring + 2 * L128_UNIT;   // [32][LMH_K], lmh_off swizzle
    half8 af[32];                          // K step t: k = 32 t + 8 q .. + 8 of row 16 wid + c16
    float4 wv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) wv[i] = *(const float4 *)(g.norm_w + 4 * lane + 256 * i);
#pragma unroll
    for (int p = 0; p < 4; p++) {
        float4 v[4][4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = 32 * p + wid + 8 * r;
            const float *xr = g.x + (long)(m < M ? m : 0) * g.ldx;
#pragma unroll
            for (int i = 0; i < 4; i++) v[r][i] = *(const float4 *)(xr + 4 * lane + 256 * i);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = 32 * p + wid + 8 * r, lr = wid + 8 * r;
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++)
                s += ((double)fmul_rn(v[r][i].x, v[r][i].x) + (double)fmul_rn(v[r][i].y, v[r][i].y)) +
                     ((double)fmul_rn(v[r][i].z, v[r][i].z) + (double)fmul_rn(v[r][i].w, v[r][i].w));
            s = wave_sum_d(s);
            const float mean = (float)(s / LMH_K);
            const float scale = 1.0f / sqrtf(mean + g.eps);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint32_t lo = f_to_u16(fmul_rn(fmul_rn(v[r][i].x, scale), wv[i].x)) |
                              ((uint32_t)f_to_u16(fmul_rn(fmul_rn(v[r][i].y, scale), wv[i].y)) << 16);
                uint32_t hi = f_to_u16(fmul_rn(fmul_rn(v[r][i].z, scale), wv[i].z)) |
                              ((uint32_t)f_to_u16(fmul_rn(fmul_rn(v[r][i].w, scale), wv[i].w)) << 16);
                if (m >= M) lo = hi = 0u;   // rows past M: zeros
                *(uint2 *)(xs + lmh_off(lr, 4 * lane + 256 * i)) = make_uint2(lo, hi);
            }
        }
        __syncthreads();
        if ((wid >> 1) == p) {
            const int lr = 16 * (wid & 1) + c16;
#pragma unroll
            for (int t = 0; t < 32; t++) af[t] = *(const half8 *)(xs + lmh_off(lr, 32 * t + 8 * q));
        }
        __syncthreads();
    }
    if (nu > 2) issue(2);

    // ---- stream: unit j from slot j % R; unit j + R - 1 issued once every wave is past unit j - 1
    unsigned long long best[4] = {0ull, 0ull, 0ull, 0ull};
    float lm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, ls[4] = {0.f, 0.f, 0.f, 0.f};   // LSE: (m, s) per row
    const int nvalid = g.n_valid > 0 ? g.n_valid : g.N;
    for (int j = 0; j < nu; j++) {
        // this wave's pieces of unit j landed: the units after it still in flight (four pieces each)
        const int later = min(nu - 1 - j, L128_R - 2);
        if (later >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (later == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // every wave's pieces of unit j; every wave done with unit j - 1 (its slot is free)
        if (j + L128_R - 1 < nu) issue(j + L128_R - 1);
        const uint16_t *sl = ring + (j % L128_R) * L128_UNIT + c16 * LMH_K;
        floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int c = 0; c < 8; c++)
#pragma unroll
            for (int s4 = 0; s4 < 4; s4++) {
                const int ch = 16 * c + 4 * s4 + q;
                const half8 b8 = *(const half8 *)(sl + ((ch ^ c16) << 3));
                acc[c & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[4 * c + s4], b8, acc[c & 1], 0, 0, 0);
            }
        const int col = (u0 + j) * 16 + c16;
#pragma unroll
        for (int r = 0; r < 4; r++) {   // C layout: lane (q, c16) = rows 16 wid + 4q + r, column col
            const int row = 16 * wid + 4 * q + r;
            const float v = acc[0][r] + acc[1][r];
            if (g.out_f32 && row < M) g.out_f32[(long)row * g.ldo + col] = v;
            const unsigned long long key = col < nvalid ? argmax_key(v, col) : 0ull;
            best[r] = key > best[r] ? key : best[r];
            if constexpr (LSE) {
                if (col < nvalid) lse_add(lm[r], ls[r], v);
            }
        }
    }

    // ---- per-row best over the 16 column lanes; each row belongs to one wave
#pragma unroll
    for (int r = 0; r < 4; r++) {
        unsigned long long k = best[r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const unsigned long long t = __shfl_xor(k, o, 64);
            k = t > k ? t : k;
        }
        const int row = 16 * wid + 4 * q + r;
        if (c16 == 0 && row < M) {
            const unsigned long long old = atomicMax(g.amax + row, k);
            asm volatile("" ::"v"(old));   // returned value used: the max has been performed at L2
        }
        if constexpr (LSE) {
            float m = lm[r], s = ls[r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
            if (c16 == 0 && row < M)
                __hip_atomic_store(g.lp_part + (long)blockIdx.x * 128 + row, lse_pack(m, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) last_wg = __hip_atomic_fetch_add(g.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    __syncthreads();
    if (last_wg) {
        if (tid == 0) st = *g.step;
        __syncthreads();
        if constexpr (LSE) {
            lse_finish<4>(g, M, gridDim.x, st);   // 512 threads over 128 rows
            __syncthreads();   // amax read before it is re-armed below
        }
        if (tid < M) {
            const unsigned long long k = __hip_atomic_load(g.amax + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int id = argmax_key_idx(k);
            g.tok_out[tid] = id;
            if (g.hist) g.hist[(long)tid * g.hist_stride + st + 1] = id;
            g.pos[tid] += 1;
            if (g.nkv) g.nkv[tid] += 1;
            __hip_atomic_store(g.amax + tid, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0) {
            if (!g.keep_step) *g.step = st + 1;
            __hip_atomic_store(g.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    stamp_end(g.stamp);
}

template <bool LSE>
void run_lmhead128(const GemvArgs &g, hipStream_t s) {
    static int ncu_dev[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    int &ncu = ncu_dev[dev & 63];
    if (!ncu) {
        int n = 0;
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        (void)hipFuncSetAttribute((const void *)lmhead128_kernel<LSE>, hipFuncAttributeMaxDynamicSharedMemorySize, L128_LDS);
        ncu = n > 0 ? n : 256;
    }
    hipLaunchKernelGGL(lmhead128_kernel<LSE>, dim3(ncu), dim3(512), L128_LDS, s, g);
}

}  // namespace

int lmhead_grid() {   // (run_lmhead_v / run_lmhead128: one workgroup a CU, 256 where the query fails)
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
}

bool launch_lmhead_batch(const GemvArgs &g, hipStream_t s) {
    if (g.M < 1 || g.M > 128 || g.K != LMH_K || g.N % 16 != 0 || !g.x || !g.norm_w || !g.amax || !g.done || !g.tok_out ||
        !g.step || !g.pos || g.Wd)
        return false;
    if ((g.lp_part || g.lp_out || g.lp_hist) && !(g.lp_part && g.lp_out && g.lp_hist && g.hist_stride > 0)) return false;
    // top-K pointers: all or none, 9 .. 64 rows only (lmhead128_kernel has no such variant), on top of the lp_* group
    const bool tk_any = g.tk_part || g.tk_out || g.tk_lp || g.tk_hist || g.tk_lphist;
    if (tk_any && !(g.tk_part && g.tk_out && g.tk_lp && g.tk_hist && g.tk_lphist && g.lp_part && g.tk_k >= 1 && g.tk_k <= TKS &&
                    g.M <= 64))
        return false;
    if (g.M > 64) {   // 65..128 rows: the rows in registers, the embedding read once (round 6; until then one
                      // launch per 64-row half, each streaming all 311 MB: tools/micro/lmh128_bench)
        if (g.lp_part) run_lmhead128<true>(g, s);
        else run_lmhead128<false>(g, s);
        return true;
    }
    const int mt = (g.M + 15) / 16;
    if (mt == 1) run_lmhead<1>(g, s);
    else if (mt == 2) run_lmhead<2>(g, s);
    else if (mt == 3) run_lmhead<3>(g, s);
    else run_lmhead<4>(g, s);
    return true;
}

}  // namespace qasr
