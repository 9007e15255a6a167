// score_head.hip -- teacher-forced scoring head: for R normed
// hidden rows A [R][K] against the tied embedding W [N][K] (both fp16) and one
// target id a row,
//   lp[r]  = logit[r][target[r]] - logsumexp(logit[r][0 .. n_valid))
//   gid[r] = argmax of the row (argmax_key order: ties to the lower id)
//   glp[r] = that token's log-probability
// without a logit ever leaving the registers.
//
// Launch 1 (score_head_kernel): the LDS-DMA MFMA main loop of the dense LM head
// (gemm_glds.h) on 128 x 128 tiles.  The epilogue reduces each tile row over
// the tile's valid columns to one argmax key and s = sum exp(v - m), m the
// key's value (tile row-max first, then one exp a logit: no serial (m, s)
// chain through the 4 values a lane holds, and every term is <= 1), stores
// them to scratch [row][column tile], and the one lane that owns column
// target[row] stores that logit.  Launch 2 (score_merge_kernel), behind it on
// the stream: one wave a row merges the row's column-tile partials -- lane l
// takes tiles l, l + 64, ... in ascending order, then the 64 lanes merge in a
// fixed butterfly -- and writes the three outputs.  The order is fixed and no
// floating-point atomic exists, so two runs give the same bits.
//
// Grid: row tiles on the fast axis (N >> R): the workgroups sharing a
// 128-column slice of W are dispatched together and W streams once.
#include "gemm_glds.h"

namespace qasr {

__device__ __attribute__((aligned(64))) uint32_t g_score_zero_line[16];

namespace {

constexpr int SBM = 128, SBN = 128, SNB = 3;

struct ScoreKArgs {
    GemmArgs g;                      // A, lda, W, ldw, M = R, N, K, n_valid (> 0)
    const int32_t *target;
    unsigned long long *part_key;    // [R][nt]
    float *part_s;                   // [R][nt]
    float *tgt;                      // [R]
    int nt;                          // column tiles
};

template <bool COLS_FAST>
__global__ __launch_bounds__(256) void score_head_kernel(ScoreKArgs p) {
    constexpr int FM = SBM / 32, FN = SBN / 32;
    __shared__ unsigned long long s_key[2][2][64];
    __shared__ float s_sum[2][2][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int mt = COLS_FAST ? blockIdx.y : blockIdx.x, ct = COLS_FAST ? blockIdx.x : blockIdx.y;
    const int m0 = mt * SBM, n0 = ct * SBN;
    const int R = p.g.M, nv = p.g.n_valid;
    if (n0 >= nv) {   // no valid column in the tile: empty partials, no GEMM (block-uniform)
        if (tid < SBM && m0 + tid < R) {
            p.part_key[(size_t)(m0 + tid) * p.nt + ct] = 0ull;
            p.part_s[(size_t)(m0 + tid) * p.nt + ct] = 0.0f;
        }
        return;
    }
    floatx4 acc[FM][FN];
    glds_mainloop<SBM, SBN, 1, SNB, AM_DENSE, 2>(p.g, m0, n0, g_score_zero_line, acc);

    // acc[i][j][r]: row m0 + wr*64 + 16i + 4(lane>>4) + r, column n0 + wc*64 + 16j + (lane&15)
    const int cbase = n0 + wc * 64 + (lane & 15);
#pragma unroll
    for (int i = 0; i < FM; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int rl = 16 * i + 4 * (lane >> 4) + r;   // row inside the wave's 64
            const int row = m0 + wr * 64 + rl;
            const int tg = row < R ? p.target[row] : -1;
            unsigned long long best = 0ull;
#pragma unroll
            for (int j = 0; j < FN; j++) {
                const int col = cbase + 16 * j;
                const float v = acc[i][j][r];
                const unsigned long long key = col < nv ? argmax_key(v, col) : 0ull;
                best = key > best ? key : best;
                if (col == tg) p.tgt[row] = v;
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const unsigned long long other = __shfl_xor(best, o, 64);
                best = other > best ? other : best;
            }
            // (best == 0: the wave's 64 columns are all past n_valid)
            const float m = best ? argmax_key_val(best) : 0.0f;
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < FN; j++) s += cbase + 16 * j < nv ? lse_exp(acc[i][j][r] - m) : 0.0f;
            s = row16_sum(s);
            if ((lane & 15) == 0) {
                s_key[wr][wc][rl] = best;
                s_sum[wr][wc][rl] = s;
            }
        }
    __syncthreads();
    if (wc == 0) {   // lane l: row l of the wave pair's 64; the two column halves in ascending order
        const int row = m0 + wr * 64 + lane;
        if (row < R) {
            const unsigned long long k0 = s_key[wr][0][lane], k1 = s_key[wr][1][lane];
            float m = argmax_key_val(k0), s = s_sum[wr][0][lane];   // (k0 != 0: n0 < n_valid)
            // (k1 == 0, the upper 64 columns all past n_valid: the empty pair (-inf, 0))
            lse_merge(m, s, k1 ? argmax_key_val(k1) : -INFINITY, s_sum[wr][1][lane]);
            p.part_key[(size_t)row * p.nt + ct] = k1 > k0 ? k1 : k0;
            p.part_s[(size_t)row * p.nt + ct] = s;
        }
    }
}

// one wave a row: the row's nt partials -> lp, gid, glp
__global__ __launch_bounds__(256) void score_merge_kernel(const unsigned long long *__restrict__ part_key,
                                                          const float *__restrict__ part_s, const float *__restrict__ tgt, int nt,
                                                          int R, float *__restrict__ lp, int32_t *__restrict__ gid,
                                                          float *__restrict__ glp) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;   // wave-uniform
    unsigned long long best = 0ull;
    float m = -INFINITY, s = 0.0f;
    for (int t = lane; t < nt; t += 64) {
        const unsigned long long k = part_key[(size_t)row * nt + t];
        if (!k) continue;   // a tile past n_valid
        lse_merge(m, s, argmax_key_val(k), part_s[(size_t)row * nt + t]);
        best = k > best ? k : best;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {   // lse_merge gives the same bits on both sides
        const unsigned long long k2 = __shfl_xor(best, o, 64);
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        lse_merge(m, s, m2, s2);
        best = k2 > best ? k2 : best;
    }
    if (lane == 0) {
        lp[row] = lse_logprob(tgt[row], m, s);
        gid[row] = argmax_key_idx(best);
        glp[row] = lse_logprob(argmax_key_val(best), m, s);
    }
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

size_t score_head_scratch(int R, int N) {
    if (R <= 0 || N <= 0) return 0;
    const size_t nt = (size_t)(N + SBN - 1) / SBN;
    return align256((size_t)R * nt * 8) + align256((size_t)R * nt * 4) + align256((size_t)R * 4);
}

bool launch_score_head(const ScoreHeadArgs &a, hipStream_t s) {
    if (a.R < 1 || a.N < SBN || a.N % SBN != 0 || a.K < 128 || a.K % 128 != 0 || a.lda < a.K || a.ldw < a.K || a.lda % 8 != 0 ||
        a.ldw % 8 != 0 || a.n_valid < 0 || a.n_valid > a.N)
        return false;
    if (!a.A || !a.W || !a.target || !a.lp || !a.gid || !a.glp || !a.scratch) return false;
    const int nt = a.N / SBN, mt = (a.R + SBM - 1) / SBM;
    if ((a.cols_fast ? mt : nt) > 65535) return false;   // grid.y
    ScoreKArgs p{};
    p.g.A = a.A; p.g.lda = a.lda; p.g.W = a.W; p.g.ldw = a.ldw;
    p.g.M = a.R; p.g.N = a.N; p.g.K = a.K; p.g.n_valid = a.n_valid ? a.n_valid : a.N;
    p.target = a.target;
    char *sc = (char *)a.scratch;
    p.part_key = (unsigned long long *)sc;
    p.part_s = (float *)(sc + align256((size_t)a.R * nt * 8));
    p.tgt = (float *)(sc + align256((size_t)a.R * nt * 8) + align256((size_t)a.R * nt * 4));
    p.nt = nt;
    note_kernel("score_head", 5, SBM, SBN, 1, SNB, a.cols_fast ? 1 : 0);
    if (a.cols_fast) hipLaunchKernelGGL(score_head_kernel<true>, dim3(nt, mt), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(score_head_kernel<false>, dim3(mt, nt), dim3(256), 0, s, p);
    hipLaunchKernelGGL(score_merge_kernel, dim3((a.R + 3) / 4), dim3(256), 0, s, p.part_key, p.part_s, p.tgt, nt, a.R, a.lp, a.gid,
                       a.glp);
    return true;
}

}  // namespace qasr
