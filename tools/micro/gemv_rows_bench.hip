// gemv_rows_bench.hip -- the MFMA weight-streaming GEMV (csrc/gemv_rows.hip) next to the kernels that ran before it
// (launch_gemv, launch_gemv_wide) at the four layer launches of a hidden-2048 / FFN-6144 decoder, M = 2 / 4 / 8,
// weights cold in HBM.
//
// Per shape: NL distinct weight sets, NL = 16 or as many as make NL x bytes exceed 512 MiB (twice the Infinity
// Cache: the 8 MB o projection needs 64 sets to stream from HBM), one hipGraph-captured chain of NL launches in
// stream order with the engine's operands (QKV and gate/up: fp32 x + norm_w; o and down: fp16 xh, the residual
// stream read and rewritten in place), median of 20 replays, us per launch:
//   rows    qasr::launch_gemv_rows
//   old     qasr::launch_gemv, or launch_gemv_wide for the 6144-long rows (untouched by this kernel's change)
//   read    a plain nontemporal read of the same NL sets in one launch: the bytes floor
// and the largest difference of the two kernels' outputs on one set (the same products, another summation order).
//
// build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -I../../include -I../../qwen3-asr.cpp_amd/csrc
//        gemv_rows_bench.hip -o gemv_rows_bench -L../../qwen3-asr.cpp_amd -lqasr
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

constexpr int REPS = 20, H = 2048, F = 6144;

struct Shape {
    const char *name;
    int epi, N, K;       // N output columns (SwiGLU: 2 N weight rows)
    bool f32x;           // fp32 x + norm_w (else xh, in-place residual)
};
static const Shape kShapes[4] = {{"qkv", qasr::EPI_F32, 4096, H, true},
                                 {"o", qasr::EPI_F32, H, H, false},
                                 {"gate/up", qasr::EPI_SWIGLU_F16, F, H, true},
                                 {"down", qasr::EPI_F32, H, F, false}};

__global__ __launch_bounds__(256) void read_kernel(const u32x4 *p, long n, unsigned *sink) {
    unsigned a = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const u32x4 v = __builtin_nontemporal_load(p + i);
        a ^= v[0] ^ v[1] ^ v[2] ^ v[3];
    }
    if (a == 0x12345678u) *sink = a;   // (keeps the loads)
}

static float *g_x, *g_nw, *g_o32;    // [8][H] residual stream, [H] norm weights, [8][4096] fp32 output
static uint16_t *g_xh, *g_o16;       // [8][F] fp16 input, [8][F] fp16 output

static qasr::GemvArgs args_of(const Shape &sh, const uint16_t *W, int M) {
    qasr::GemvArgs g{};
    g.W = W; g.K = sh.K; g.N = sh.N; g.M = M; g.eps = 1e-6f;
    if (sh.f32x) { g.x = g_x; g.ldx = H; g.norm_w = g_nw; }
    else { g.xh = g_xh; g.ldxh = sh.K; g.res = g_x; g.ldr = H; g.out_f32 = g_x; g.ldo = H; }
    if (sh.epi == qasr::EPI_SWIGLU_F16) { g.out_f16 = g_o16; g.ldo16 = sh.N; }
    else if (sh.f32x) { g.out_f32 = g_o32; g.ldo = sh.N; }
    return g;
}

static void launch(const Shape &sh, const uint16_t *W, int M, bool rows, hipStream_t s) {
    const qasr::GemvArgs g = args_of(sh, W, M);
    bool ok = true;
    if (rows) ok = qasr::launch_gemv_rows(sh.epi, g, s);
    else if (sh.K > 4096) ok = qasr::launch_gemv_wide(sh.epi, g, s);
    else qasr::launch_gemv(sh.epi, g, s);
    std::string msg;
    if (!ok || qasr::take_declined(&msg)) { printf("%s declined at M = %d: %s\n", sh.name, M, msg.c_str()); exit(1); }
}

// median us per launch over REPS timed replays of the captured chain (one warm-up replay first)
static float time_chain(const Shape &sh, const std::vector<uint16_t *> &w, int M, bool rows, hipStream_t s) {
    hipGraph_t gr;
    hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (uint16_t *p : w) launch(sh, p, M, rows, s);
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
    std::vector<uint16_t> hx(8 * F);
    std::vector<float> hnw(H);
    for (auto &v : hx) v = __builtin_bit_cast(uint16_t, (_Float16)rnd());
    for (auto &v : hnw) v = 1.f + 0.1f * rnd();
    CK(hipMalloc(&g_xh, hx.size() * 2));
    CK(hipMemcpy(g_xh, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
    CK(hipMalloc(&g_nw, H * 4));
    CK(hipMemcpy(g_nw, hnw.data(), H * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&g_x, 8 * H * 4));
    CK(hipMalloc(&g_o32, 8 * 4096 * 4));
    CK(hipMalloc(&g_o16, 8 * F * 2));
    unsigned *sink;
    CK(hipMalloc(&sink, 4));
    std::vector<float> hx0(8 * H);
    for (auto &v : hx0) v = rnd();
    auto reset_x = [&]() { CK(hipMemcpy(g_x, hx0.data(), hx0.size() * 4, hipMemcpyHostToDevice)); };

    for (const Shape &sh : kShapes) {
        const size_t wn = (size_t)sh.N * (sh.epi == qasr::EPI_SWIGLU_F16 ? 2 : 1) * sh.K;
        const int NL = (int)std::max<size_t>(16, ((size_t)512 << 20) / (wn * 2) + 1);
        std::vector<uint16_t> hw(wn);
        const float wscale = 1.7f / sqrtf((float)sh.K);
        for (auto &v : hw) v = __builtin_bit_cast(uint16_t, (_Float16)(rnd() * wscale));
        uint16_t *all;
        CK(hipMalloc(&all, NL * wn * 2));
        std::vector<uint16_t *> w;
        for (int l = 0; l < NL; l++) {
            w.push_back(all + l * wn);
            CK(hipMemcpy(w[l], hw.data(), wn * 2, hipMemcpyHostToDevice));
        }
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
        const double bw = NL * wn * 2 / (rd[REPS / 2] * 1e-3), floor_us = wn * 2 / bw * 1e6;
        printf("%s  N %d K %d: %d weight sets of %.1f MB; read %.0f GB/s, bytes floor %.2f us a launch\n", sh.name, sh.N, sh.K, NL,
               wn * 2 / 1e6, bw / 1e9, floor_us);
        for (int M : {2, 4, 8}) {
            reset_x();
            const float t_old = time_chain(sh, w, M, false, s);
            reset_x();
            const float t_new = time_chain(sh, w, M, true, s);
            printf("  %-8s M = %d: rows %.2f us (%.2f x floor)  old %.2f us (%.2f x floor)  rows / old %.3f\n", sh.name, M, t_new,
                   t_new / floor_us, t_old, t_old / floor_us, t_new / t_old);
        }
        // both kernels on one set from the same state
        const int on = sh.epi == qasr::EPI_SWIGLU_F16 ? sh.N : sh.f32x ? sh.N : H;
        std::vector<float> o[2];
        for (int v = 0; v < 2; v++) {
            reset_x();
            launch(sh, w[0], 8, v == 1, s);
            CK(hipStreamSynchronize(s));
            o[v].resize(8 * on);
            if (sh.epi == qasr::EPI_SWIGLU_F16) {
                std::vector<uint16_t> h(8 * on);
                CK(hipMemcpy(h.data(), g_o16, h.size() * 2, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < h.size(); i++) o[v][i] = (float)__builtin_bit_cast(_Float16, h[i]);
            } else {
                CK(hipMemcpy(o[v].data(), sh.f32x ? g_o32 : g_x, o[v].size() * 4, hipMemcpyDeviceToHost));
            }
        }
        double worst = 0, scale = 0;
        for (size_t i = 0; i < o[0].size(); i++) {
            worst = std::max(worst, (double)fabsf(o[0][i] - o[1][i]));
            scale = std::max(scale, (double)fabsf(o[0][i]));
        }
        printf("  %-8s rows vs old, M = 8: max |difference| %.3g at an output scale of %.3g\n", sh.name, worst, scale);
        CK(hipFree(all));
    }
    return 0;
}
