// gemv_rows_q8.hip -- batch 2 .. 8 Q8_0 projections on the int8 matrix units: the four layer launches of a decode
// step (QKV, o, gate/up, down) of a Q8_0 model for K % 256 == 0, 256 <= K <= 8192.  The Q8_0 sibling of gemv_rows.hip.
//
// gemv_q8_kernel (gemm.hip) pays four v_dot4, a shuffle, a conversion, a multiply and an fma per block, column and
// activation row.  One int8 MFMA takes 16 activation rows against 16 weight rows, so here 2 rows cost what 8 do:
//
//   work     as gemv_rows.hip: a workgroup of four waves owns 16-column output tiles (tile t = blockIdx.x,
//            + gridDim.x, ...; SwiGLU: the tile's 16 gate rows, then its 16 up rows); wave w takes the quarter
//            [w K/4, (w + 1) K/4) of the tile's 16 weight rows, K ascending, in chunks of CB Q8_0 blocks.
//   weights  global memory straight into the MFMA A operand: lane (c = lane & 15, q = lane >> 4) loads the 16 bytes
//            of weight row c at k = 64 step + 16 q, so one load instruction covers 16 rows x 64 contiguous bytes
//            = two Q8_0 blocks a row.  Nontemporal buffer loads through a bounds-checked descriptor (rows past N:
//            zeros, no access, no branch), two register buffers: a chunk's loads are all requested before the
//            chunk in front of it is multiplied, across the workgroup's tiles.  Weights never touch LDS.
//   blocks   v_mfma_i32_16x16x64_i8 sums over all 64 k of a step, which would mix the step's two blocks (their
//            scales differ).  Lanes q = 0, 1 hold block 0 and q = 2, 3 block 1 in A and in B alike, so each step
//            issues two MFMAs from a zero accumulator, the B operand zeroed in the other block's lanes: each gives
//            one block's exact integer dots.
//   scales   the fp16 block scales the lane needs on the C layout (weight rows 4 q .. 4 q + 3, the chunk's CB
//            blocks: CB / 2 dwords a row) are requested with the chunk's weights through a second descriptor
//            and ride in the same two buffers; the 16 lanes of a q share each address.
//   x        prepared once a workgroup with act_prologue.h (gemv_q8_kernel's arithmetic and thread-to-element map:
//            the same quants and scales): int8 in LDS [M][K], 16-byte piece p of row r at piece p ^ (r & 15) (rows
//            are a multiple of 256 B apart: the row lanes of a B fragment would otherwise share a bank group), the
//            fp32 block scales behind them as [K / 32][8] (a fragment's rows on consecutive banks).  Lanes whose row
//            is >= M feed zeros and read nothing.
//   sums     per block acc = fma(d_w * d_x, (float)sumi, acc) on the C layout (lane (c, q): activation row c, columns
//            4 q .. 4 q + 3; q8_scale_acc: the bits of the scalar fmul + fma).  Waves 1 .. 3 hand their partials to
//            wave 0 through LDS (two copies, one barrier a tile), which adds them in wave order, then bias, then the
//            residual (SwiGLU: silu(gate) * up), and stores rows < M.  No atomics, no waits between workgroups.
//
// The other operand form -- 8-byte loads, one v_mfma_i32_16x16x32_i8 a block -- and what was measured: DESIGN.md 5.13.
// Registers, LDS and occupancy of every instantiation: profiles/gemv_rows_q8/resources.txt.
#include "gemv_rows_core.h"

namespace qasr {

// what the finishing wave reads where the launch has no bias / residual (unconditional loads, as gemv_rows.hip)
__device__ __attribute__((aligned(64))) float grq_zero_line[16];

// byte offset of (row, k) in the swizzled int8 rows
__device__ __forceinline__ int grq_off(int row, int k, int K) { return row * K + ((((k >> 4) ^ (row & 15))) << 4) + (k & 15); }

template <int EPI, int CB>
__global__ __launch_bounds__(256) void gemv_rows_q8_kernel(GemvArgs g) {
    extern __shared__ __attribute__((aligned(16))) int8_t xq[];     // [M][K] int8 (grq_off), then [K / 32][8] fp32 scales
    constexpr int NR = EPI == EPI_SWIGLU_F32 ? 2 : 1;               // weight row tiles an output tile
    constexpr int NS = CB / 2;                                      // 64-byte steps (= scale dwords a row) a chunk
    __shared__ double red[4][8];
    __shared__ floatx4 part[2][3][NR][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = lane & 15, q = lane >> 4;
    trace_mark(g.trace, 0);
    stamp_start(g.stamp);
    if (g.zero8 && blockIdx.x == 0 && tid < 8) g.zero8[tid * 16] = 0u;
    const int K = g.K, M = g.M, nb = K >> 5, kw = K >> 2, nch = kw / (32 * CB), ntiles = (g.N + 15) >> 4;
    float *xd = (float *)(xq + M * K);
    const uint32_t wbytes = (uint32_t)((long)g.N * NR * K), dbytes = (uint32_t)((long)g.N * NR * nb * 2);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc((void *)g.W, (short)0, (int)wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t dsrd = __builtin_amdgcn_make_buffer_rsrc((void *)g.Wd, (short)0, (int)dbytes, 0x00020000);
    u32x4 wv[2][NS];
    uint32_t wd[2][4][NS];
    // chunk j of row tile r of output tile t, and its scales (past the last tile or row: no memory access)
    auto wload = [&](auto bc, int t, int r, int j) {
        constexpr int b = decltype(bc)::value;
        const int o = 16 * t + c;
        const long wrow = NR == 2 ? 32L * t + c + 16 * r : o;
        const uint32_t off = t < ntiles && o < g.N ? (uint32_t)(wrow * K + wid * kw + j * (CB * 32) + 16 * q) : wbytes;
#pragma unroll
        for (int s = 0; s < NS; s++)
            wv[b][s] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wsrd, off + s * 64, 0, 2));   // nt
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int oi = 16 * t + 4 * q + i;
            const long drow = NR == 2 ? 32L * t + 4 * q + i + 16 * r : oi;
            const uint32_t doff = t < ntiles && oi < g.N ? (uint32_t)((drow * nb + (wid * kw >> 5) + j * CB) * 2) : dbytes;
            if constexpr (NS >= 4) {
#pragma unroll
                for (int s = 0; s < NS; s += 4) {
                    const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(dsrd, doff + s * 4, 0, 0));
                    wd[b][i][s] = v[0]; wd[b][i][s + 1] = v[1]; wd[b][i][s + 2] = v[2]; wd[b][i][s + 3] = v[3];
                }
            } else {
                static_assert(NS == 1, "a chunk is 2, 8 or 16 blocks");
                wd[b][i][0] = __builtin_amdgcn_raw_buffer_load_b32(dsrd, doff, 0, 0);
            }
        }
    };
    int t = blockIdx.x, r = 0, j = 0;
    wload(std::integral_constant<int, 0>{}, t, r, j);

    // ---- x rows -> Q8_0 in LDS.  Thread tid owns elements p * 1024 + 4 tid .. + 3 of every row (act_prologue.h)
    {
        auto xput = [&](int m, int k, const float4 &v, float scale) {   // every lane of the wave, k < K or not
            float d;
            const uint32_t u = q8p_quant(g, v, k, scale, k < K, d);
            if (k < K) {
                *(uint32_t *)(xq + grq_off(m, k, K)) = u;
                if ((tid & 7) == 0) xd[(k >> 5) * 8 + m] = d;
            }
        };
        if (K <= 2048) {   // the rows stay in registers between the sum and the quantisation
            float4 xr[8][2];
#pragma unroll
            for (int m = 0; m < 8; m++) {
                double ss = 0.0;
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    const int k = p * 1024 + tid * 4;
                    xr[m][p] = m < M && k < K ? xp_load(g, m, k) : make_float4(0.f, 0.f, 0.f, 0.f);
                    xp_sq(ss, xr[m][p]);
                }
                if (g.norm_w) {
                    ss = wave_sum_d(ss);
                    if (lane == 0) red[wid][m] = ss;
                }
            }
            if (g.norm_w) __syncthreads();
#pragma unroll
            for (int m = 0; m < 8; m++) {
                if (m >= M) break;
                const float scale = xp_row_scale(g, red[0][m], red[1][m], red[2][m], red[3][m]);
#pragma unroll
                for (int p = 0; p < 2; p++) xput(m, p * 1024 + tid * 4, xr[m][p], scale);
            }
        } else {           // longer rows are read twice (the second time from the caches)
            const int np = (K + 1023) >> 10;
            if (g.norm_w) {
                for (int m = 0; m < M; m++) {
                    double ss = 0.0;
                    for (int k = tid * 4; k < K; k += 1024) xp_sq(ss, xp_load(g, m, k));
                    ss = wave_sum_d(ss);
                    if (lane == 0) red[wid][m] = ss;
                }
                __syncthreads();
            }
            for (int m = 0; m < M; m++) {
                const float scale = xp_row_scale(g, red[0][m], red[1][m], red[2][m], red[3][m]);
                for (int p = 0; p < np; p++) {
                    const int k = p * 1024 + tid * 4;
                    xput(m, k, k < K ? xp_load(g, m, k) : make_float4(0.f, 0.f, 0.f, 0.f), scale);
                }
            }
        }
    }
    __syncthreads();

    const bool rowlive = c < M;                                    // this lane's B column is a row of x
    const int8_t *xrow = xq + (rowlive ? c : 0) * K;
    const float *xdl = xd + (rowlive ? c : 0);
    const int kb0 = wid * kw >> 5;                                 // the wave's first block
    const uint32_t m0 = q < 2 ? 0xffffffffu : 0u, m1 = ~m0;        // B lanes of a step's first / second block
    floatx4 cur = {0.f, 0.f, 0.f, 0.f}, gate = {0.f, 0.f, 0.f, 0.f};
    float bv[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f};
    int nt = 0;                                                    // tiles this workgroup has finished (part copy)
    // one chunk from buffer b, the chunk after it requested meanwhile
    auto step = [&](auto bc) {
        constexpr int b = decltype(bc)::value;
        const int t0 = t, r0 = r, j0 = j;
        if (++j == nch) { j = 0; if (++r == NR) { r = 0; t += gridDim.x; } }
        const bool last = j0 == nch - 1 && r0 == NR - 1;           // the tile's sums are complete behind this chunk
        // wave 0 lane (c, q) finishes row c, columns 16 t0 + 4 q .. + 3: bias / residual requested ahead of the next
        // chunk's weights and unconditionally (gemv_rows.hip says why)
        if constexpr (EPI == EPI_F32) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int o = 16 * t0 + 4 * q + i;
                const bool live = last && wid == 0 && rowlive && o < g.N;
                bv[i] = *(live && g.bias ? g.bias + o : grq_zero_line);
                rv[i] = *(live && g.res ? g.res + (long)c * g.ldr + o : grq_zero_line);
            }
        }
        wload(std::integral_constant<int, 1 - b>{}, t, r, j);
        if (j0 == 0) cur = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int kb = kb0 + j0 * CB + 2 * s;                  // the step's first block
            u32x4 xv = {0u, 0u, 0u, 0u};
            float dx0 = 0.f, dx1 = 0.f;
            if (rowlive) {
                xv = *(const u32x4 *)(xrow + (((2 * kb + q) ^ c) << 4));
                dx0 = xdl[kb * 8];
                dx1 = xdl[kb * 8 + 8];
            }
            const intx4 a = __builtin_bit_cast(intx4, wv[b][s]);
            const intx4 x0 = __builtin_bit_cast(intx4, u32x4{xv[0] & m0, xv[1] & m0, xv[2] & m0, xv[3] & m0});
            const intx4 x1 = __builtin_bit_cast(intx4, u32x4{xv[0] & m1, xv[1] & m1, xv[2] & m1, xv[3] & m1});
            const intx4 s0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, x0, intx4{0, 0, 0, 0}, 0, 0, 0);
            const intx4 s1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, x1, intx4{0, 0, 0, 0}, 0, 0, 0);
            floatx4 d0, d1;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                d0[i] = u16_to_f((uint16_t)(wd[b][i][s] & 0xffffu));
                d1[i] = u16_to_f((uint16_t)(wd[b][i][s] >> 16));
            }
            q8_scale_acc(cur, dx0, d0, s0);
            q8_scale_acc(cur, dx1, d1, s1);
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
                if constexpr (EPI == EPI_SWIGLU_F32) {
                    g.out_f32[(long)c * g.ldo + o] = silu_f(y[0][i]) * y[NR - 1][i];
                } else {
                    float v = y[0][i];
                    if (g.bias) v = fadd_rn(v, bv[i]);
                    if (g.res) v = fadd_rn(v, rv[i]);
                    g.out_f32[(long)c * g.ldo + o] = v;
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

// dynamic LDS of a launch: the rows and their scales
static int grq_dynamic_lds(int M, int K) { return M * K + (K / 32) * 8 * 4; }

template <int EPI>
static void gemv_rows_q8_cb(const GemvArgs &g, hipStream_t s) {
    rows_chunk_ladder(g.K, [&](auto cb) {   // Q8_0 blocks a chunk
        constexpr int CB = decltype(cb)::value;
        run_rows<gemv_rows_q8_kernel<EPI, CB>>(g, s, grq_dynamic_lds(g.M, g.K), rows_static_lds(EPI == EPI_SWIGLU_F32 ? 2 : 1),
                                               grq_dynamic_lds(8, 8192), "gemv_rows_q8", EPI, CB);
    });
}

// What launch_gemv_rows_q8 takes: Q8_0 W (int8 rows K apart, fp16 scales Wd [rows][K / 32]), rows_shape_ok's shapes,
// fp32 x or the gathered embd rows (+ x_store), optionally norm_w -- launch_gemv's Q8_0 rules -- and
//   EPI_F32         + bias, + res (out_f32 may be res)
//   EPI_SWIGLU_F32  N % 16 == 0, the 16-row gate / up interleave; no bias, no res
// with trace / stamp / zero8 honoured.  Everything else -- f16 weights (no Wd), xh input, EPI_ARGMAX and the fp16
// epilogues, M = 1, M > 8 among it -- is declined: recorded (note_declined / note_declined_shape), nothing launched.
bool gemv_rows_q8_covers(int epi, const GemvArgs &g) {
    if (epi != EPI_F32 && epi != EPI_SWIGLU_F32) return false;
    if (!g.Wd || g.xh || !rows_shape_ok(g, epi == EPI_SWIGLU_F32 ? 2 : 1, 1)) return false;
    if (!g.out_f32 || g.ldo < g.N) return false;
    if (epi == EPI_F32) return !g.res || g.ldr >= g.N;
    return !g.res && !g.bias && g.N % 16 == 0;
}

bool launch_gemv_rows_q8(int epi, const GemvArgs &g, hipStream_t s) {
    if (!gemv_rows_q8_covers(epi, g)) return rows_declined("launch_gemv_rows_q8", epi == EPI_F32 || epi == EPI_SWIGLU_F32, epi, g);
    if (epi == EPI_F32) gemv_rows_q8_cb<EPI_F32>(g, s);
    else gemv_rows_q8_cb<EPI_SWIGLU_F32>(g, s);
    return true;
}

}  // namespace qasr
