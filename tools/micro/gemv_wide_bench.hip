// gemv_wide_bench.hip -- the K-split GEMV (csrc/gemv_wide.hip) at the hidden-2048 decoder's down projection:
// N = 2048, K = 6144, M = 1 / 2 / 4 / 8, weights cold in HBM.
//
// Times hipGraph-captured chains of dependent launches (x += W act, as the engine's down projection) over NL
// distinct weight sets (NL x 25 MB > the 256 MiB Infinity Cache, so every launch streams from HBM) and reports
// us per launch against the bytes floor N K 2 / (measured HBM read bandwidth):
//   wide    qasr::launch_gemv_wide (libqasr.so)
//   row1    M = 1 only: one wave per output row, gemv1_kernel's arithmetic at K = 6144 (twelve 16-byte loads a
//           row in every lane before the first fma) -- lives here only, the baseline the K split is measured against
//   read    a plain read of all NL weight sets (the bandwidth the floor uses)
// and checks wide against row1 (the same products, another summation order: a few fp32 ulps).
//
// build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
//        -I../../include -I../../qwen3-asr.cpp_amd/csrc gemv_wide_bench.hip -o gemv_wide_bench
//        -L../../qwen3-asr.cpp_amd -lqasr -Wl,-rpath,'$ORIGIN/../../qwen3-asr.cpp_amd'
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dev_common.h"
#include "kernels.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

constexpr int N = 2048, K = 6144, NL = 16, REPS = 20;

// gemv1_kernel<EPI_F32, 6144, 1> with the fp16 input and the residual of the down projection
__global__ __launch_bounds__(256) void row1_kernel(const uint16_t *W, const uint16_t *xh, const float *res, float *out) {
    constexpr int NT = K / 512;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    half8 wv[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) wv[t] = __builtin_nontemporal_load((const half8 *)(W + (long)min(row, N - 1) * K + t * 512 + lane * 8));
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const half8 h = *(const half8 *)(xh + t * 512 + lane * 8);
#pragma unroll
        for (int e = 0; e < 8; e++) acc = fmaf((float)wv[t][e], (float)h[e], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0 && row < N) out[row] = fadd_rn(acc, res[row]);
}

__global__ __launch_bounds__(256) void read_kernel(const u32x4 *p, long n, unsigned *sink) {
    unsigned a = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const u32x4 v = __builtin_nontemporal_load(p + i);
        a ^= v[0] ^ v[1] ^ v[2] ^ v[3];
    }
    if (a == 0x12345678u) *sink = a;   // (keeps the loads)
}

static std::vector<uint16_t *> g_w;
static uint16_t *g_xh;
static float *g_x;   // [8][N] residual stream, read and rewritten by every launch
static int g_m, g_variant;

static void body(hipStream_t s) {
    for (int l = 0; l < NL; l++) {
        if (g_variant == 1) {
            hipLaunchKernelGGL(row1_kernel, dim3(N / 4), dim3(256), 0, s, g_w[l], g_xh, g_x, g_x);
            continue;
        }
        qasr::GemvArgs g{};
        g.xh = g_xh; g.ldxh = K; g.W = g_w[l]; g.K = K; g.N = N; g.M = g_m;
        g.res = g_x; g.ldr = N; g.out_f32 = g_x; g.ldo = N;
        if (!qasr::launch_gemv_wide(qasr::EPI_F32, g, s)) { printf("launch_gemv_wide declined M = %d\n", g_m); exit(1); }
    }
}

// median us per launch over REPS timed replays of the captured chain (one warm-up replay first)
static float time_chain(hipStream_t s) {
    hipGraph_t gr;
    hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    body(s);
    CK(hipStreamEndCapture(s, &gr));
    CK(hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0));
    CK(hipGraphLaunch(ge, s));
    CK(hipStreamSynchronize(s));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::vector<float> us;
    for (int r = 0; r < REPS; r++) {
        CK(hipEventRecord(a, s));
        CK(hipGraphLaunch(ge, s));
        CK(hipEventRecord(b, s));
        CK(hipEventSynchronize(b));
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        us.push_back(ms * 1e3f / NL);
    }
    CK(hipGraphExecDestroy(ge));
    CK(hipGraphDestroy(gr));
    std::sort(us.begin(), us.end());
    printf("    (min %.2f  median %.2f  max %.2f us)\n", us.front(), us[REPS / 2], us.back());
    return us[REPS / 2];
}

int main() {
    hipStream_t s;
    CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const size_t wn = (size_t)N * K;
    std::vector<uint16_t> hw(wn), hx(8 * K);
    uint32_t r = 12345u;
    auto rnd = [&]() { r = r * 1664525u + 1013904223u; return (float)((r >> 8) & 0xffff) / 32768.f - 1.f; };   // [-1, 1)
    for (auto &v : hw) v = __builtin_bit_cast(uint16_t, (_Float16)(rnd() * 0.0128f));   // ~ 1 / sqrt(K)
    for (auto &v : hx) v = __builtin_bit_cast(uint16_t, (_Float16)rnd());
    uint16_t *all;
    CK(hipMalloc(&all, NL * wn * 2));
    for (int l = 0; l < NL; l++) {
        g_w.push_back(all + l * wn);
        CK(hipMemcpy(g_w[l], hw.data(), wn * 2, hipMemcpyHostToDevice));
    }
    CK(hipMalloc(&g_xh, hx.size() * 2));
    CK(hipMemcpy(g_xh, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
    CK(hipMalloc(&g_x, 8 * N * 4));
    unsigned *sink;
    CK(hipMalloc(&sink, 4));

    // HBM read bandwidth: all NL sets (403 MB) in one launch, median of REPS
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::vector<float> rd;
    for (int i = 0; i < REPS + 1; i++) {
        CK(hipEventRecord(a, s));
        hipLaunchKernelGGL(read_kernel, dim3(256 * 8), dim3(256), 0, s, (const u32x4 *)all, (long)(NL * wn / 8), sink);
        CK(hipEventRecord(b, s));
        CK(hipEventSynchronize(b));
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        if (i) rd.push_back(ms);
    }
    std::sort(rd.begin(), rd.end());
    const double bw = NL * wn * 2 / (rd[REPS / 2] * 1e-3);   // bytes / s
    const double floor_us = wn * 2 / bw * 1e6;
    printf("read   %.0f MB in %.3f ms (median of %d): %.0f GB/s; floor of one %d x %d f16 launch %.2f us\n", NL * wn * 2 / 1e6,
           rd[REPS / 2], REPS, bw / 1e9, N, K, floor_us);

    for (int m : {1, 2, 4, 8}) {
        g_m = m;
        g_variant = 0;
        CK(hipMemsetAsync(g_x, 0, 8 * N * 4, s));   // (outside the captured chain)
        printf("wide   M = %d\n", m);
        const float us = time_chain(s);
        printf("wide   M = %d: %.2f us / launch, %.0f GB/s, %.2f x the floor\n", m, us, wn * 2 / (us * 1e-6) / 1e9, us / floor_us);
    }
    g_m = 1;
    g_variant = 1;
    CK(hipMemsetAsync(g_x, 0, 8 * N * 4, s));
    printf("row1   M = 1\n");
    const float us1 = time_chain(s);
    printf("row1   M = 1: %.2f us / launch, %.0f GB/s, %.2f x the floor\n", us1, wn * 2 / (us1 * 1e-6) / 1e9, us1 / floor_us);

    // the two forms on the same operands: one launch each from a zero residual
    std::vector<float> o0(N), o1(N);
    for (int v = 0; v < 2; v++) {
        CK(hipMemsetAsync(g_x, 0, 8 * N * 4, s));   // (outside the captured chain)
        g_variant = v;
        CK(hipStreamSynchronize(s));
        if (v == 1) hipLaunchKernelGGL(row1_kernel, dim3(N / 4), dim3(256), 0, s, g_w[0], g_xh, g_x, g_x);
        else {
            qasr::GemvArgs g{};
            g.xh = g_xh; g.ldxh = K; g.W = g_w[0]; g.K = K; g.N = N; g.M = 1; g.res = g_x; g.ldr = N; g.out_f32 = g_x; g.ldo = N;
            (void)qasr::launch_gemv_wide(qasr::EPI_F32, g, s);
        }
        CK(hipStreamSynchronize(s));
        CK(hipMemcpy((v ? o1 : o0).data(), g_x, N * 4, hipMemcpyDeviceToHost));
    }
    double worst = 0, scale = 0;
    for (int i = 0; i < N; i++) { worst = std::max(worst, (double)fabsf(o0[i] - o1[i])); scale = std::max(scale, (double)fabsf(o1[i])); }
    printf("wide vs row1, M = 1: max |difference| %.3g at an output scale of %.3g\n", worst, scale);
    return 0;
}
