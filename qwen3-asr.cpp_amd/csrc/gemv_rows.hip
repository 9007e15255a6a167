// gemv_rows.hip -- batch 2 .. 8 f16 projections on the matrix units: the four layer launches of a decode step
// (QKV, o, gate/up, down) for K % 256 == 0, 256 <= K <= 8192.
//
// launch_gemv / launch_gemv_wide multiply on the vector ALU, M fp32 fmas a weight element.  A 16x16x32 f16 MFMA
// takes 16 activation rows for the price of one, so here 2 rows cost what 8 do and the weights are the only stream:
//
//   work     a workgroup of four waves owns 16-column tiles of the output (tile t = blockIdx.x, + gridDim.x, ...;
//            SwiGLU: the tile's 16 gate rows, then its 16 up rows).  The waves split K, not the columns: wave w
//            takes the quarter [w K/4, (w + 1) K/4) of the tile's 16 weight rows, in chunks of CH MFMA steps.
//   weights  global memory straight into MFMA A-operand registers: lane (c = lane & 15, q = lane >> 4) loads the
//            8 halves of weight row c at k = 32 step + 8 q.  Nontemporal 16-byte buffer loads through a
//            bounds-checked descriptor (rows past N: zeros, no memory access, no branch); a chunk's CH loads are
//            all requested before the chunk in front of it is multiplied (two register buffers; the chunks of a
//            workgroup's tiles form one stream, so the next tile's first chunk is in flight behind this tile's
//            last).  Every weight byte is used once: weights never touch LDS.
//   x        prepared once a workgroup, fp16 in LDS [M][K]: the fp32 path with gemv_kernel's prologue arithmetic
//            (gemm.hip: the same thread owns the same elements, double sum of fp32 squares, the same reduction,
//            fmul_rn(fmul_rn(v, scale), w), one rounding to fp16 -- the same bits), xh copied, the layer-0
//            embedding gather done (x_store by workgroup 0).  16-byte chunk ch of row r sits at chunk
//            ch ^ (r & 15) of the row (lmhead.hip's lmh_off): rows are a multiple of 512 B apart, and the row
//            lanes of a B fragment would otherwise hit one bank group.  Lanes whose row is >= M feed zeros and
//            read nothing.
//   sums     v_mfma_f32_16x16x32_f16, fp32, K ascending inside a wave; waves 1 .. 3 hand their 16x16 partials to
//            wave 0 through LDS (two copies, so one barrier a tile), which adds them in wave order 0, 1, 2, 3,
//            then bias, then the residual, and stores rows < M.  No atomics, no waits between workgroups: the
//            result is a function of the operands alone.
//
// Registers, LDS and occupancy of every instantiation: profiles/gemv_rows/resources.txt.
#include "gemv_rows_core.h"

namespace qasr {

// what the finishing wave reads where the launch has no bias / residual (unconditional loads, see finish below)
__device__ __attribute__((aligned(64))) float gr_zero_line[16];

// element offset of (row, k) in the swizzled x rows
__device__ __forceinline__ int gr_off(int row, int k, int K) { return row * K + ((((k >> 3) ^ (row & 15))) << 3) + (k & 7); }

template <int EPI, int CH>
__global__ __launch_bounds__(256) void gemv_rows_kernel(GemvArgs g) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xs[];   // [M][K], gr_off
    constexpr int NR = EPI == EPI_SWIGLU_F16 ? 2 : 1;               // weight row tiles an output tile
    __shared__ double red[4][8];
    __shared__ floatx4 part[2][3][NR][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = lane & 15, q = lane >> 4;
    trace_mark(g.trace, 0);
    stamp_start(g.stamp);
    if (g.zero8 && blockIdx.x == 0 && tid < 8) g.zero8[tid * 16] = 0u;   // fused o-proj counters (as gemv1_kernel)
    const int K = g.K, M = g.M, kw = K >> 2, nch = kw / (32 * CH), ntiles = (g.N + 15) >> 4;
    const uint32_t wbytes = (uint32_t)((long)g.N * NR * K * 2);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc((void *)g.W, (short)0, (int)wbytes, 0x00020000);
    half8 wv[2][CH];
    // chunk j of row tile r of output tile t (past the last tile: no memory access)
    auto wload = [&](auto bc, int t, int r, int j) {
        constexpr int b = decltype(bc)::value;
        const int o = 16 * t + c;
        const long wrow = NR == 2 ? 32L * t + c + 16 * r : o;
        const uint32_t off = t < ntiles && o < g.N ? (uint32_t)((wrow * K + wid * kw + j * (CH * 32) + 8 * q) * 2) : wbytes;
#pragma unroll
        for (int s = 0; s < CH; s++)
            wv[b][s] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(wsrd, off + s * 64, 0, 2));   // nt
    };
    int t = blockIdx.x, r = 0, j = 0;
    wload(std::integral_constant<int, 0>{}, t, r, j);

    // ---- x rows -> fp16 in LDS (act_prologue.h: gemv_kernel's arithmetic and thread-to-element map)
    if (g.norm_w || g.x || g.embd_ids) {
        xp_rows(g, red, [&](int m, int k, const float4 &v, float scale) {
            *(uint2 *)(xs + gr_off(m, k, K)) = xp_f16x4(g, v, k, scale);
        });
    } else {
        for (int k = tid * 8; k < K; k += 256 * 8)
            for (int m = 0; m < M; m++) *(u32x4 *)(xs + gr_off(m, k, K)) = *(const u32x4 *)(g.xh + (long)m * g.ldxh + k);
    }
    __syncthreads();

    const bool rowlive = c < M;                                    // this lane's B column is a row of x
    const uint16_t *xrow = xs + (rowlive ? c : 0) * K;
    const int kch0 = (wid * kw >> 3) + q;                          // 16-byte chunk of step 0 of chunk 0
    floatx4 cur = {0.f, 0.f, 0.f, 0.f}, gate = {0.f, 0.f, 0.f, 0.f};
    float bv[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f};
    int nt = 0;                                                    // tiles this workgroup has finished (part copy)
    // one chunk from buffer b, the chunk after it requested meanwhile
    auto step = [&](auto bc) {
        constexpr int b = decltype(bc)::value;
        const int t0 = t, r0 = r, j0 = j;
        if (++j == nch) { j = 0; if (++r == NR) { r = 0; t += gridDim.x; } }
        const bool last = j0 == nch - 1 && r0 == NR - 1;           // the tile's sums are complete behind this chunk
        // wave 0 lane (c, q) finishes row c, columns 16 t0 + 4 q .. + 3.  Bias / residual requested ahead of the
        // next chunk's weights (vmcnt counts in issue order: behind them wave 0 would wait for that whole
        // buffer), and unconditionally (a conditional load makes the compiler wait for everything in flight)
        if constexpr (EPI != EPI_SWIGLU_F16) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int o = 16 * t0 + 4 * q + i;
                const bool live = last && wid == 0 && rowlive && o < g.N;
                bv[i] = *(live && g.bias ? g.bias + o : gr_zero_line);
                if constexpr (EPI == EPI_F32) rv[i] = *(live && g.res ? g.res + (long)c * g.ldr + o : gr_zero_line);
            }
        }
        wload(std::integral_constant<int, 1 - b>{}, t, r, j);
        if (j0 == 0) cur = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < CH; s++) {
            half8 x8 = {0, 0, 0, 0, 0, 0, 0, 0};
            if (rowlive) x8 = *(const half8 *)(xrow + (((kch0 + (j0 * CH + s) * 4) ^ c) << 3));
            cur = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[b][s], x8, cur, 0, 0, 0);
        }
        if (j0 != nch - 1) return;
        if (wid) part[nt & 1][wid - 1][r0][lane] = cur;
        if (!last) { gate = cur; return; }
        __syncthreads();
        if (wid == 0) {
            floatx4 y[NR];
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                const floatx4 own = NR == 2 && rr == 0 ? gate : cur;
#pragma unroll
                for (int i = 0; i < 4; i++)
                    y[rr][i] = fadd_rn(fadd_rn(fadd_rn(own[i], part[nt & 1][0][rr][lane][i]), part[nt & 1][1][rr][lane][i]),
                                       part[nt & 1][2][rr][lane][i]);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int o = 16 * t0 + 4 * q + i;
                if (!rowlive || o >= g.N) continue;
                if constexpr (EPI == EPI_SWIGLU_F16) {
                    g.out_f16[(long)c * g.ldo16 + o] = f_to_u16(silu_f(y[0][i]) * y[NR - 1][i]);
                } else {
                    float v = y[0][i];
                    if (g.bias) v = fadd_rn(v, bv[i]);
                    if constexpr (EPI == EPI_F16) {
                        g.out_f16[(long)c * g.ldo16 + o] = f_to_u16(v);
                    } else {
                        if (g.res) v = fadd_rn(v, rv[i]);
                        g.out_f32[(long)c * g.ldo + o] = v;
                    }
                }
            }
        }
        nt++;   // part[nt & 1] is rewritten two tiles later, behind the barrier of the tile between
    };
    while (t < ntiles) {
        step(std::integral_constant<int, 0>{});
        if (t >= ntiles) break;
        step(std::integral_constant<int, 1>{});
    }
    if (g.trace) { __syncthreads(); trace_mark(g.trace, 1); }
    stamp_end(g.stamp);
}

template <int EPI>
static void gemv_rows_ch(const GemvArgs &g, hipStream_t s) {
    rows_chunk_ladder(g.K, [&](auto ch) {   // MFMA steps a chunk
        constexpr int CH = decltype(ch)::value;
        run_rows<gemv_rows_kernel<EPI, CH>>(g, s, g.M * g.K * 2, rows_static_lds(EPI == EPI_SWIGLU_F16 ? 2 : 1), 8 * 8192 * 2, "gemv_rows", EPI, CH);
    });
}

// What launch_gemv_rows takes: f16 W rows K apart (no Wd), rows_shape_ok's shapes and inputs, and
//   EPI_F32         + bias, + res (out_f32 may be res)
//   EPI_F16         + bias
//   EPI_SWIGLU_F16  N % 16 == 0, gemv1_kernel's 16-row gate / up interleave; no bias, no res
// with trace / stamp / zero8 as gemv_kernel honours them.  Everything else -- EPI_ARGMAX, M = 1, M > 8, Q8_0
// among it -- is declined: recorded (note_declined / note_declined_shape), nothing launched or written.
bool gemv_rows_covers(int epi, const GemvArgs &g) {
    if (epi != EPI_F32 && epi != EPI_F16 && epi != EPI_SWIGLU_F16) return false;
    if (g.Wd || !rows_shape_ok(g, epi == EPI_SWIGLU_F16 ? 2 : 1, 2)) return false;
    switch (epi) {
        case EPI_F32: return g.out_f32 && g.ldo >= g.N && (!g.res || g.ldr >= g.N);
        case EPI_F16: return g.out_f16 && !g.res && g.ldo16 >= g.N;
        default: return g.out_f16 && !g.res && !g.bias && g.N % 16 == 0 && g.ldo16 >= g.N;
    }
}

bool launch_gemv_rows(int epi, const GemvArgs &g, hipStream_t s) {
    if (!gemv_rows_covers(epi, g))
        return rows_declined("launch_gemv_rows", epi == EPI_F32 || epi == EPI_F16 || epi == EPI_SWIGLU_F16, epi, g);
    switch (epi) {
        case EPI_F32: gemv_rows_ch<EPI_F32>(g, s); break;
        case EPI_F16: gemv_rows_ch<EPI_F16>(g, s); break;
        default: gemv_rows_ch<EPI_SWIGLU_F16>(g, s); break;
    }
    return true;
}

}  // namespace qasr
