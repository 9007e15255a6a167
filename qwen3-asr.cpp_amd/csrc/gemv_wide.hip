// gemv_wide.hip -- batch <= 8 f16 projections with long rows (4096 < K <= 8192):
// the 6144-wide down projection of a hidden-2048 decoder.
//
// launch_gemv's kernels give a wave whole weight rows: gemv_kernel keeps MR x K
// fp16 of x in LDS (96 KiB at M = 8, K = 6144: one workgroup a CU), and a
// one-wave-per-row kernel would hold K / 512 = 12 16-byte loads a row in every
// lane.  Here the workgroup's four waves split K instead of the columns:
//
//   work     a workgroup owns CPW output columns for all M rows; wave w takes the
//            K quarter [w K/4, (w + 1) K/4) of each of those weight rows, NQ =
//            K / 2048 sweeps of 64 lanes x 8 halves: CPW x NQ loads a lane
//   weights  nontemporal 16-byte buffer loads through a bounds-checked descriptor
//            (rows past N: zeros, no memory access, no branch in front of a vmcnt
//            join); a column group's loads are all requested before x is read,
//            and the next group's while this one computes (the grid strides)
//   x        each wave holds its own quarter of the M rows in registers as fp16
//            (rounded once, as ggml's mul_mat rounds its activations); no LDS
//   sums     per lane fp32 fma chains over the quarter, wave_sum per (column,
//            row), partials to LDS [4][CPW][MR]; after one barrier thread
//            (c, m) adds them in wave order 0, 1, 2, 3, then bias, then the
//            residual, and stores.  No atomics: the result is a function of the
//            operands alone.
//
// LDS is 2 x 4 x CPW x MR floats (two copies so one barrier a group is enough);
// registers and occupancy per instantiation: profiles/gemv_wide/resources.txt.
// That is the kernel of 2 .. 8 rows.  One row runs one wave per output row
// (gemv_wide_row_kernel below), which measured faster there.
#include <type_traits>

#include "dev_common.h"
#include "kernels.h"

namespace qasr {

// what a finishing thread reads where the launch has no bias / residual (and what
// the other threads read): unconditional loads, see process() below
__device__ __attribute__((aligned(64))) float gw_zero_line[16];

template <int EPI, int CPW, int MR, int NQ>
__global__ __launch_bounds__(256) void gemv_wide_kernel(GemvArgs g) {
    constexpr int K = NQ * 2048;
    __shared__ float part[2][4][CPW][MR];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    trace_mark(g.trace, 0);
    stamp_start(g.stamp);
    if (g.zero8 && blockIdx.x == 0 && tid < 8) g.zero8[tid * 16] = 0u;   // fused o-proj counters (as gemv1_kernel)
    const int ncg = (g.N + CPW - 1) / CPW;
    const int kq = wid * (K / 4) + lane * 8;   // sweep t of this lane: elements kq + 512 t .. + 8, all inside the wave's quarter
    half8 wv[2][CPW][NQ];                      // double-buffered over column groups
    const uint32_t wbytes = (uint32_t)((long)g.N * K * 2);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc((void *)g.W, (short)0, (int)wbytes, 0x00020000);
    auto wload = [&](auto bc, int cgi) {
        constexpr int b = decltype(bc)::value;
#pragma unroll
        for (int c = 0; c < CPW; c++)
#pragma unroll
            for (int t = 0; t < NQ; t++) {
                const int o = cgi * CPW + c;
                const uint32_t off = o < g.N ? (uint32_t)(((long)o * K + kq + t * 512) * 2) : wbytes;
                wv[b][c][t] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(wsrd, off, 0, 2));   // nt
            }
    };
    int cg = blockIdx.x;
    wload(std::integral_constant<int, 0>{}, cg);
    // ---- this wave's quarter of the x rows (rows past M repeat row M - 1; never stored)
    half8 xq[MR][NQ];
    if (g.xh) {
#pragma unroll
        for (int m = 0; m < MR; m++)
#pragma unroll
            for (int t = 0; t < NQ; t++)
                xq[m][t] = *(const half8 *)(g.xh + (long)min(m, g.M - 1) * g.ldxh + kq + t * 512);
    } else {
#pragma unroll
        for (int m = 0; m < MR; m++)
#pragma unroll
            for (int t = 0; t < NQ; t++) {
                const float *p = g.x + (long)min(m, g.M - 1) * g.ldx + kq + t * 512;
                const float4 a = *(const float4 *)p, b = *(const float4 *)(p + 4);
                xq[m][t] = half8{f2h(a.x), f2h(a.y), f2h(a.z), f2h(a.w), f2h(b.x), f2h(b.y), f2h(b.z), f2h(b.w)};
            }
    }
    // the thread that finishes output (column fc of the group, row fm)
    const bool fin = tid < CPW * MR;
    const int fc = fin ? tid / MR : 0, fm = fin ? tid % MR : 0;
    // one column group from buffer b, the group after it (nxt; past the end: no memory access) requested meanwhile
    auto process = [&](auto bc, int cgi, int nxt) {
        constexpr int b = decltype(bc)::value;
        const int col0 = cgi * CPW;
        // bias / residual requested ahead of the next group's weights (vmcnt counts in issue order: behind them
        // the finishing wave would wait for that whole buffer), and unconditionally (a conditional load makes the
        // compiler wait for everything in flight at the join)
        const bool live = fin && col0 + fc < g.N && fm < g.M;   // this thread stores an output of the group
        const float bv = *(live && g.bias ? g.bias + col0 + fc : gw_zero_line);
        float rv = 0.f;
        if constexpr (EPI == EPI_F32) rv = *(live && g.res ? g.res + (long)fm * g.ldr + col0 + fc : gw_zero_line);
        wload(std::integral_constant<int, 1 - b>{}, nxt);
        float acc[CPW][MR];
#pragma unroll
        for (int c = 0; c < CPW; c++)
#pragma unroll
            for (int m = 0; m < MR; m++) acc[c][m] = 0.0f;
        // x stays packed fp16 across the groups: opaque here, or the compiler hoists the fp16 -> fp32 conversions
        // out of the group loop and holds the quarter twice as wide (v_fma_mix_f32 converts both operands for free)
#pragma unroll
        for (int m = 0; m < MR; m++)
#pragma unroll
            for (int t = 0; t < NQ; t++) asm volatile("" : "+v"(xq[m][t]));
#pragma unroll
        for (int t = 0; t < NQ; t++)
#pragma unroll
            for (int m = 0; m < MR; m++)
#pragma unroll
                for (int c = 0; c < CPW; c++)
#pragma unroll
                    for (int e = 0; e < 8; e++) acc[c][m] = fmaf((float)wv[b][c][t][e], (float)xq[m][t][e], acc[c][m]);
#pragma unroll
        for (int c = 0; c < CPW; c++)
#pragma unroll
            for (int m = 0; m < MR; m++) {
                const float v = wave_sum(acc[c][m]);
                if (lane == 0) part[b][wid][c][m] = v;
            }
        __syncthreads();
        if (live) {
            float y = fadd_rn(fadd_rn(fadd_rn(part[b][0][fc][fm], part[b][1][fc][fm]), part[b][2][fc][fm]), part[b][3][fc][fm]);
            if (g.bias) y = fadd_rn(y, bv);
            if constexpr (EPI == EPI_F16) {
                g.out_f16[(long)fm * g.ldo16 + col0 + fc] = f_to_u16(y);
            } else {
                if (g.res) y = fadd_rn(y, rv);
                g.out_f32[(long)fm * g.ldo + col0 + fc] = y;
            }
        }
    };
    // part[b] is rewritten two groups later, behind the barrier of the group between
    const int stride = gridDim.x;
    while (cg < ncg) {
        const int n1 = cg + stride, n2 = n1 + stride;
        process(std::integral_constant<int, 0>{}, cg, n1);
        if (n1 >= ncg) break;
        process(std::integral_constant<int, 1>{}, n1, n2);
        cg = n2;
    }
    if (g.trace) { __syncthreads(); trace_mark(g.trace, 1); }
    stamp_end(g.stamp);
}

// M = 1: one wave per output row, gemv1_kernel's arithmetic (gemv.hip) at K = NQ x 2048 with the loads through
// the same descriptor: K / 512 loads a lane, no LDS, no barrier.  At the one shape measured (N = 2048, K = 6144,
// tools/micro/gemv_wide_bench.hip, profiles/gemv_wide/micro.txt) it beat the K split at one row, 6.12 against
// 6.84 us a launch: the split pays a barrier and an LDS round trip for a single output column pair.
template <int EPI, int NQ, bool XH>
__global__ __launch_bounds__(256) void gemv_wide_row_kernel(GemvArgs g) {
    constexpr int K = NQ * 2048, NT = K / 512;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    trace_mark(g.trace, 0);
    stamp_start(g.stamp);
    if (g.zero8 && blockIdx.x == 0 && threadIdx.x < 8) g.zero8[threadIdx.x * 16] = 0u;
    const uint32_t wbytes = (uint32_t)((long)g.N * K * 2);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc((void *)g.W, (short)0, (int)wbytes, 0x00020000);
    half8 wv[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint32_t off = row < g.N ? (uint32_t)(((long)row * K + t * 512 + lane * 8) * 2) : wbytes;
        wv[t] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(wsrd, off, 0, 2));   // nt
    }
    // x a sweep at a time behind the weights (XH: the fp16 input, else fp32 rounded here): held whole it cost
    // 150 VGPRs against 63
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        half8 xv;
        if constexpr (XH) {
            xv = *(const half8 *)(g.xh + t * 512 + lane * 8);
        } else {
            const float *p = g.x + t * 512 + lane * 8;
            const float4 a = *(const float4 *)p, b = *(const float4 *)(p + 4);
            xv = half8{f2h(a.x), f2h(a.y), f2h(a.z), f2h(a.w), f2h(b.x), f2h(b.y), f2h(b.z), f2h(b.w)};
        }
#pragma unroll
        for (int e = 0; e < 8; e++) acc = fmaf((float)wv[t][e], (float)xv[e], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0 && row < g.N) {
        float y = acc;
        if (g.bias) y = fadd_rn(y, g.bias[row]);
        if constexpr (EPI == EPI_F16) {
            g.out_f16[row] = f_to_u16(y);
        } else {
            if (g.res) y = fadd_rn(y, g.res[row]);
            g.out_f32[row] = y;
        }
    }
    if (g.trace) { __syncthreads(); trace_mark(g.trace, 1); }
    stamp_end(g.stamp);
}

template <int EPI, int NQ>
static void run_gemv_wide_row(const GemvArgs &g, hipStream_t s) {
    note_kernel("gemv_wide_row", 2, EPI, NQ);
    if (g.xh) hipLaunchKernelGGL((gemv_wide_row_kernel<EPI, NQ, true>), dim3((g.N + 3) / 4), dim3(256), 0, s, g);
    else hipLaunchKernelGGL((gemv_wide_row_kernel<EPI, NQ, false>), dim3((g.N + 3) / 4), dim3(256), 0, s, g);
}

template <int EPI, int CPW, int MR, int NQ>
static void run_gemv_wide(const GemvArgs &g, hipStream_t s) {
    // the workgroups 256 CUs hold at once, grid-stride beyond: 4 a CU while the x quarter is at most 24 VGPRs
    // (MR x NQ x 4), 3 up to 48, else 2 (profiles/gemv_wide/resources.txt); N = 2048 at CPW = 2 is 1024 groups
    constexpr int xregs = MR * NQ * 4, cap = 256 * (xregs <= 24 ? 4 : xregs <= 48 ? 3 : 2);
    const int ncg = (g.N + CPW - 1) / CPW;
    note_kernel("gemv_wide", 4, EPI, CPW, MR, NQ);
    hipLaunchKernelGGL((gemv_wide_kernel<EPI, CPW, MR, NQ>), dim3(ncg < cap ? ncg : cap), dim3(256), 0, s, g);
}

template <int EPI, int MR>
static void gemv_wide_nq(const GemvArgs &g, hipStream_t s) {
    if (g.K == 6144) run_gemv_wide<EPI, 2, MR, 3>(g, s);
    else run_gemv_wide<EPI, 2, MR, 4>(g, s);
}

template <int EPI>
static void gemv_wide_mr(const GemvArgs &g, hipStream_t s) {
    // one row: the one-wave-per-row form (measured faster at K = 6144; K = 8192 follows it unmeasured)
    if (g.M <= 1) return g.K == 6144 ? run_gemv_wide_row<EPI, 3>(g, s) : run_gemv_wide_row<EPI, 4>(g, s);
    if (g.M <= 2) gemv_wide_nq<EPI, 2>(g, s);
    else if (g.M <= 4) gemv_wide_nq<EPI, 4>(g, s);
    else gemv_wide_nq<EPI, 8>(g, s);
}

bool launch_gemv_wide(int epi, const GemvArgs &g, hipStream_t s) {
    if (g.M < 1 || g.M > 8 || g.N < 1 || !g.W || g.Wd || g.norm_w || g.embd_ids || g.amax) return false;
    if (g.K <= 4096 || g.K > 8192 || g.K % 2048 != 0) return false;
    if ((unsigned long long)g.N * g.K * 2 > 0xffff0000ull) return false;   // the descriptor's 32-bit range
    if (g.xh ? g.ldxh % 8 != 0 || g.ldxh < g.K : !g.x || g.ldx % 4 != 0 || g.ldx < g.K) return false;
    switch (epi) {
        case EPI_F32:
            if (!g.out_f32 || (g.res && g.ldr < g.N) || g.ldo < g.N) return false;
            gemv_wide_mr<EPI_F32>(g, s);
            return true;
        case EPI_F16:
            if (!g.out_f16 || g.res || g.ldo16 < g.N) return false;
            gemv_wide_mr<EPI_F16>(g, s);
            return true;
        default: return false;
    }
}

}  // namespace qasr
