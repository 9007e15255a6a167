// gemv_rows_q8_bench.hip -- the int8-MFMA weight-streaming GEMV (csrc/gemv_rows_q8.hip) next to launch_gemv's
// gemv_q8_kernel at the four layer launches of a Q8_0 decoder, 1.7B shape (hidden 2048, FFN 6144) and 0.6B shape
// (hidden 1024, FFN 3072), M = 2 / 4 / 8, weights cold in HBM.
//
// Per shape: NL distinct weight sets (quants, then their scales), NL = 16 or as many as make NL x bytes exceed
// 512 MiB (twice the Infinity Cache), one hipGraph-captured chain of NL launches in stream order with the engine's
// operands (QKV and gate/up: fp32 x + norm_w; o and down: fp32 x, the residual stream read and rewritten in place),
// median of 20 replays, us per launch:
//   rows    qasr::launch_gemv_rows_q8
//   old     qasr::launch_gemv (Q8_0)
//   read    a plain nontemporal read of the same NL sets in one launch: the bytes floor
// and the largest difference of the two kernels' outputs on one set (the same products, another summation order).
//
// build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -I../../include -I../../qwen3-asr.cpp_amd/csrc
//        gemv_rows_q8_bench.hip -o gemv_rows_q8_bench -L../../qwen3-asr.cpp_amd -lqasr
//        -Wl,-rpath,'$ORIGIN/../../qwen3-asr.cpp_amd'
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dev_common.h"
#include "kernels.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

constexpr int REPS = 20, HMAX = 2048, FMAX = 6144;

struct Shape {
    const char *name;
    int epi, N, K, H;    // N output columns (SwiGLU: 2 N weight rows); H: the residual stream's width
    bool norm;           // fp32 x + norm_w into a buffer of its own (else the residual stream in place)
};
static const Shape kShapes[8] = {
    {"1.7B qkv", qasr::EPI_F32, 4096, 2048, 2048, true},        {"1.7B o", qasr::EPI_F32, 2048, 2048, 2048, false},
    {"1.7B gate/up", qasr::EPI_SWIGLU_F32, 6144, 2048, 2048, true}, {"1.7B down", qasr::EPI_F32, 2048, 6144, 2048, false},
    {"0.6B qkv", qasr::EPI_F32, 4096, 1024, 1024, true},        {"0.6B o", qasr::EPI_F32, 1024, 2048, 1024, false},
    {"0.6B gate/up", qasr::EPI_SWIGLU_F32, 3072, 1024, 1024, true}, {"0.6B down", qasr::EPI_F32, 1024, 3072, 1024, false}};

__global__ __launch_bounds__(256) void read_kernel(const u32x4 *p, long n, unsigned *sink) {
    unsigned a = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const u32x4 v = __builtin_nontemporal_load(p + i);
        a ^= v[0] ^ v[1] ^ v[2] ^ v[3];
    }
    if (a == 0x12345678u) *sink = a;   // (keeps the loads)
}

static float *g_x, *g_nw, *g_in, *g_o32;   // [8][H] residual stream, [H] norm weights, [8][F] input, [8][F] output

static qasr::GemvArgs args_of(const Shape &sh, const int8_t *W, int M) {
    qasr::GemvArgs g{};
    const size_t wn = (size_t)sh.N * (sh.epi == qasr::EPI_SWIGLU_F32 ? 2 : 1) * sh.K;
    g.W = (const uint16_t *)W; g.Wd = (const uint16_t *)(W + wn); g.K = sh.K; g.N = sh.N; g.M = M; g.eps = 1e-6f;
    if (sh.norm) { g.x = g_x; g.ldx = sh.H; g.norm_w = g_nw; g.out_f32 = g_o32; g.ldo = sh.N; }
    else { g.x = g_in; g.ldx = sh.K; g.res = g_x; g.ldr = sh.H; g.out_f32 = g_x; g.ldo = sh.H; }
    return g;
}

static void launch(const Shape &sh, const int8_t *W, int M, bool rows, hipStream_t s) {
    const qasr::GemvArgs g = args_of(sh, W, M);
    bool ok = true;
    if (rows) ok = qasr::launch_gemv_rows_q8(sh.epi, g, s);
    else qasr::launch_gemv(sh.epi, g, s);
    std::string msg;
    if (!ok || qasr::take_declined(&msg)) { printf("%s declined at M = %d: %s\n", sh.name, M, msg.c_str()); exit(1); }
}

// median us per launch over REPS timed replays of the captured chain (one warm-up replay first)
static float time_chain(const Shape &sh, const std::vector<int8_t *> &w, int M, bool rows, hipStream_t s) {
    hipGraph_t gr;
    hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int8_t *p : w) launch(sh, p, M, rows, s);
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
        us.push_back(ms * 1e3f / w.size());
    }
    CK(hipGraphExecDestroy(ge));
    CK(hipGraphDestroy(gr));
    std::sort(us.begin(), us.end());
    printf("    %-5s M = %d  min %.2f  median %.2f  max %.2f us\n", rows ? "rows" : "old", M, us.front(), us[REPS / 2], us.back());
    return us[REPS / 2];
}

int main() {
    hipStream_t s;
    CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    uint32_t r = 12345u;
    auto rnd = [&]() { r = r * 1664525u + 1013904223u; return (float)((r >> 8) & 0xffff) / 32768.f - 1.f; };   // [-1, 1)
    std::vector<float> hin(8 * FMAX), hnw(HMAX), hx0(8 * HMAX);
    for (auto &v : hin) v = rnd();
    for (auto &v : hnw) v = 1.f + 0.1f * rnd();
    for (auto &v : hx0) v = rnd();
    CK(hipMalloc(&g_in, hin.size() * 4));
    CK(hipMemcpy(g_in, hin.data(), hin.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&g_nw, HMAX * 4));
    CK(hipMemcpy(g_nw, hnw.data(), HMAX * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&g_x, 8 * HMAX * 4));
    CK(hipMalloc(&g_o32, 8 * FMAX * 4));
    unsigned *sink;
    CK(hipMalloc(&sink, 4));
    auto reset_x = [&]() { CK(hipMemcpy(g_x, hx0.data(), hx0.size() * 4, hipMemcpyHostToDevice)); };

    for (const Shape &sh : kShapes) {
        const size_t wn = (size_t)sh.N * (sh.epi == qasr::EPI_SWIGLU_F32 ? 2 : 1) * sh.K, set = wn + wn / 16;   // + fp16 scales
        const int NL = (int)std::max<size_t>(16, ((size_t)512 << 20) / set + 1);
        std::vector<int8_t> hw(set);
        for (size_t i = 0; i < wn; i++) hw[i] = (int8_t)(rnd() * 127.f);
        const float dscale = 1.7f / sqrtf((float)sh.K) / 127.f;
        for (size_t i = 0; i < wn / 32; i++) ((_Float16 *)(hw.data() + wn))[i] = (_Float16)((0.5f + 0.5f * fabsf(rnd())) * dscale);
        int8_t *all;
        CK(hipMalloc(&all, NL * set));
        std::vector<int8_t *> w;
        for (int l = 0; l < NL; l++) {
            w.push_back(all + l * set);
            CK(hipMemcpy(w[l], hw.data(), set, hipMemcpyHostToDevice));
        }
        hipEvent_t a, b;
        CK(hipEventCreate(&a));
        CK(hipEventCreate(&b));
        std::vector<float> rd;
        for (int i = 0; i < REPS + 1; i++) {
            CK(hipEventRecord(a, s));
            hipLaunchKernelGGL(read_kernel, dim3(256 * 8), dim3(256), 0, s, (const u32x4 *)all, (long)(NL * set / 16), sink);
            CK(hipEventRecord(b, s));
            CK(hipEventSynchronize(b));
            float ms;
            CK(hipEventElapsedTime(&ms, a, b));
            if (i) rd.push_back(ms);
        }
        std::sort(rd.begin(), rd.end());
        const double bw = (double)NL * set / (rd[REPS / 2] * 1e-3), floor_us = set / bw * 1e6;
        printf("%s  N %d K %d: %d weight sets of %.1f MB; read %.0f GB/s, bytes floor %.2f us a launch\n", sh.name, sh.N, sh.K, NL,
               set / 1e6, bw / 1e9, floor_us);
        for (int M : {2, 4, 8}) {
            reset_x();
            const float t_old = time_chain(sh, w, M, false, s);
            reset_x();
            const float t_new = time_chain(sh, w, M, true, s);
            printf("  %-12s M = %d: rows %.2f us (%.2f x floor)  old %.2f us (%.2f x floor)  rows / old %.3f\n", sh.name, M, t_new,
                   t_new / floor_us, t_old, t_old / floor_us, t_new / t_old);
        }
        // both kernels on one set from the same state
        const int on = sh.norm ? sh.N : sh.H;
        std::vector<float> o[2];
        for (int v = 0; v < 2; v++) {
            reset_x();
            launch(sh, w[0], 8, v == 1, s);
            CK(hipStreamSynchronize(s));
            o[v].resize(8 * on);
            CK(hipMemcpy(o[v].data(), sh.norm ? g_o32 : g_x, o[v].size() * 4, hipMemcpyDeviceToHost));
        }
        double worst = 0, scale = 0;
        for (size_t i = 0; i < o[0].size(); i++) {
            worst = std::max(worst, (double)fabsf(o[0][i] - o[1][i]));
            scale = std::max(scale, (double)fabsf(o[0][i]));
        }
        printf("  %-12s rows vs old, M = 8: max |difference| %.3g at an output scale of %.3g\n", sh.name, worst, scale);
        CK(hipFree(all));
    }
    return 0;
}
