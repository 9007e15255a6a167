// score_bench.hip -- device time of the score head (csrc/score_head.hip) against the dense LM-head GEMM
// it shares its main loop with (launch_gemm, EPI_ARGMAX, out_f32 = NULL) at the same shape, both grid
// orders of the score head, alternating in one process (HIP events around each launch group).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iqwen3-asr.cpp_amd/csrc -Iinclude tools/micro/score_bench.hip \
//         -Lqwen3-asr.cpp_amd -lqasr -Wl,-rpath,'$ORIGIN/../../qwen3-asr.cpp_amd' -o tools/micro/score_bench
//   tools/micro/score_bench [reps]        -> profiles/score/score_head.txt
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "kernels.h"

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
            return 1;                                                              \
        }                                                                          \
    } while (0)

using namespace qasr;

int main(int argc, char **argv) {
    const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 10;
    const int N = 151936, K = 1024, RMAX = 4096;
    std::mt19937 rng(1);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<_Float16> hW((size_t)N * K), hA((size_t)RMAX * K);
    for (auto &v : hW) v = (_Float16)(nd(rng) * 0.0625f);
    for (auto &v : hA) v = (_Float16)nd(rng);
    std::vector<int32_t> htg(RMAX);
    for (int r = 0; r < RMAX; r++) htg[r] = (int32_t)(rng() % N);
    uint16_t *W, *A;
    int32_t *tg, *gid;
    float *lp, *glp;
    unsigned long long *amax;
    void *scratch;
    CK(hipMalloc((void **)&W, hW.size() * 2));
    CK(hipMalloc((void **)&A, hA.size() * 2));
    CK(hipMalloc((void **)&tg, RMAX * 4));
    CK(hipMalloc((void **)&gid, RMAX * 4));
    CK(hipMalloc((void **)&lp, RMAX * 4));
    CK(hipMalloc((void **)&glp, RMAX * 4));
    CK(hipMalloc((void **)&amax, RMAX * 8));
    CK(hipMalloc(&scratch, score_head_scratch(RMAX, N)));
    CK(hipMemcpy(W, hW.data(), hW.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(A, hA.data(), hA.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(tg, htg.data(), RMAX * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    printf("score head vs dense EPI_ARGMAX GEMM (out_f32 = NULL), N = %d, K = %d, %d alternating repetitions, median ms\n", N, K, reps);
    printf("%6s %12s %12s %12s %9s %9s %12s %12s\n", "R", "dense", "score", "score(cols)", "ratio", "ratio(c)", "TFLOP/s", "W GB/s");
    for (int R : {17, 512, 4096}) {
        GemmArgs g{};
        g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = R; g.N = N; g.K = K; g.amax = amax;
        ScoreHeadArgs s{};
        s.A = A; s.lda = K; s.W = W; s.ldw = K; s.R = R; s.N = N; s.K = K;
        s.target = tg; s.lp = lp; s.gid = gid; s.glp = glp; s.scratch = scratch;
        std::vector<float> t[3];
        for (int it = -2; it < reps; it++)   // two warm-up rounds
            for (int v = 0; v < 3; v++) {
                CK(hipMemsetAsync(amax, 0, RMAX * 8, nullptr));
                CK(hipEventRecord(e0, nullptr));
                if (v == 0) {
                    launch_gemm(AM_DENSE, EPI_ARGMAX, g, nullptr);
                } else {
                    s.cols_fast = v == 2;
                    if (!launch_score_head(s, nullptr)) { fprintf(stderr, "declined\n"); return 1; }
                }
                CK(hipEventRecord(e1, nullptr));
                CK(hipEventSynchronize(e1));
                float ms = 0.f;
                CK(hipEventElapsedTime(&ms, e0, e1));
                if (it >= 0) t[v].push_back(ms);
            }
        CK(hipGetLastError());
        float med[3];
        for (int v = 0; v < 3; v++) {
            std::sort(t[v].begin(), t[v].end());
            med[v] = t[v][t[v].size() / 2];
        }
        const double flop = 2.0 * R * (double)N * K, wb = (double)N * K * 2;
        printf("%6d %12.4f %12.4f %12.4f %9.3f %9.3f %12.1f %12.1f\n", R, med[0], med[1], med[2], med[1] / med[0], med[2] / med[0],
               flop / (med[1] * 1e-3) / 1e12, wb / (med[1] * 1e-3) / 1e9);
    }
    return 0;
}
