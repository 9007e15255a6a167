// gemv_rows_core.h -- what the two MFMA weight-streaming GEMVs for 2 .. 8 decode rows (gemv_rows.hip: f16 weights,
// gemv_rows_q8.hip: Q8_0) share on the host: the launch of one instantiation, the chunk ladder, the part of the coverage
// rule that both ask, and the decline reporting.  Their x prologue is act_prologue.h's xp_rows.  The device kernels stay
// two texts (gemv_rows.hip tells the layout): merged into one skeleton over an operand policy they gave the same bits,
// registers and main loop, but the launches without a norm (o, down) measured 0.3 .. 2.7 % slower for a cause that was
// not found (profiles/gemv_rows_core/bench_ab.txt).
#pragma once

#include <type_traits>

#include "act_prologue.h"
#include "dev_common.h"
#include "gemm_epi.h"
#include "kernels.h"

namespace qasr {

// static LDS of a kernel: red + part (nr: weight row tiles an output tile)
constexpr int rows_static_lds(int nr) { return 4 * 8 * 8 + 2 * 3 * nr * 64 * 16; }

// One instantiation's launch.  Every tile's workgroup resident at once where the CUs hold them: two a CU by registers
// (two chunk buffers), fewer by LDS (160 KiB a CU); the grid strides over the tiles beyond.
template <auto Kernel>
static void run_rows(const GemvArgs &g, hipStream_t s, int dyn_lds, int static_lds, int max_dyn_lds, const char *family, int epi, int c) {
    static int ncu_dev[64];   // per device: CU count once the LDS attribute is set (rows above 64 KiB need it)
    int dev = 0;
    (void)hipGetDevice(&dev);
    int &ncu = ncu_dev[dev & 63];
    if (!ncu) {
        int n = 0;
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        (void)hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_dyn_lds);
        ncu = n > 0 ? n : 256;
    }
    const int fit = (160 * 1024) / (dyn_lds + static_lds);
    const int cap = ncu * (fit < 1 ? 1 : fit > 2 ? 2 : fit), ntiles = (g.N + 15) / 16;
    note_kernel(family, 2, epi, c);
    hipLaunchKernelGGL(Kernel, dim3(ntiles < cap ? ntiles : cap), dim3(256), dyn_lds, s, g);
}

// 32-element units a chunk: a wave's quarter K / 4 is whole chunks.  f(std::integral_constant<int, C>)
template <class F>
static void rows_chunk_ladder(int K, F f) {
    if (K % 2048 == 0) f(std::integral_constant<int, 16>{});
    else if (K % 1024 == 0) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 2>{});
}

// what both covers ask: 2 <= M <= 8, K % 256 == 0, 256 <= K <= 8192, any N with the nr N rows of weights inside the
// descriptor's 32-bit range, the input by launch_gemv's rules (fp32 x / the gathered embd rows with ldx % 4 == 0,
// optionally norm_w; else xh with ldxh % 8 == 0), no argmax
static bool rows_shape_ok(const GemvArgs &g, int nr, int elem_bytes) {
    if (g.M < 2 || g.M > 8 || g.N < 1 || !g.W || g.amax) return false;
    if (g.K % 256 != 0 || g.K < 256 || g.K > 8192) return false;
    if ((unsigned long long)g.N * nr * g.K * elem_bytes > 0xffff0000ull) return false;
    if (g.norm_w || g.x || g.embd_ids) return (g.embd_ids ? g.embd != nullptr : g.x != nullptr) && g.ldx % 4 == 0 && g.ldx >= g.K;
    return g.xh && g.ldxh % 8 == 0 && g.ldxh >= g.K;
}

// a declined launch is recorded, nothing launched or written
static bool rows_declined(const char *what, bool epi_known, int epi, const GemvArgs &g) {
    if (epi_known) note_declined_shape(what, g.M, g.N, g.K);
    else note_declined(what, 0, epi);
    return false;
}

}  // namespace qasr
