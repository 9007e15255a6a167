// gemm_glds.h -- the LDS-DMA main loop of the tiled fp16 GEMM, shared by
// gemm_glds_kernel (gemm.hip) and the score head (score_head.hip): the tile's
// accumulators are left in registers for the caller's epilogue.
//
// The same tile, fragments and swizzle as gemm_kernel, but the operands go
// global -> LDS by LDS-DMA (global_load_lds_dwordx4: no staging registers, no
// ds_write pass) through an NB-deep ring of stages (KS 32-deep slabs each),
// NB - 1 stages in flight behind the one being multiplied; one raw barrier per
// stage after a counted vmcnt (each wave waits only for its own pieces of the
// stage it is about to read).  The swizzle is applied on the source side: lane
// l of a 1-KiB piece lands at row l>>2, chunk position l&3, and fetches chunk
// (l&3) ^ ((row>>1)&3) -- the position the fragment reads expect.  Rows past M
// and conv taps in the padding fetch a global zero line (LDS-DMA has no
// per-lane predicate).
#pragma once
#include "gemm_epi.h"

namespace qasr {

typedef __attribute__((address_space(3))) void lds_void_g;
typedef __attribute__((address_space(1))) void glb_void_g;

template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// WNW: waves along N (2: 4 waves in a 2 x 2 grid, each BM/2 x BN/2; 4: 8 waves
// in 2 x 4, each BM/2 x BN/4 -- the 256-row tiles, whose 128 KiB of stages leave
// one workgroup a CU).  zero_line: 64 zero bytes in global memory (one object a
// translation unit).  Called by every thread of the workgroup (barriers inside);
// no barrier follows the last stage's reads.
template <int BM, int BN, int KS, int NB, int AMODE, int WNW>
__device__ __forceinline__ void glds_mainloop(const GemmArgs &g, int m0, int n0, const uint32_t *zero_line,
                                              floatx4 (&acc)[BM / 32][BN / (16 * WNW)]) {
    constexpr int NWAVE = 2 * WNW, NTHR = 64 * NWAVE;
    constexpr int FM = BM / 32, FN = BN / (16 * WNW);
    constexpr int ROWS = BM + BN;
    constexpr int SLAB = ROWS * 32;        // halves per 32-deep slab
    constexpr int RG = ROWS / 16;          // 1-KiB pieces per slab
    constexpr int NP = KS * RG;            // pieces per stage
    constexpr int NW = (NP + NWAVE - 1) / NWAVE;   // pieces per wave per stage (uniform: vmcnt counts)
    constexpr int PAD = NW * NWAVE - NP;   // dummy pieces (zero line -> a scratch KiB) keep it uniform
    static_assert(ROWS % 16 == 0, "16-row pieces");
    static_assert(NB >= 2 && NB <= 4 && (NB - 2) * NW < 64, "ring depth");
    constexpr int INFO = AMODE == AM_DENSE ? 0 : BM * 8;   // int4 row descriptors (conv modes)
    constexpr int SCR = PAD ? 512 : 0;
    __shared__ __attribute__((aligned(16))) uint16_t smem[NB * KS * SLAB + SCR + INFO];
    int4 *rowinfo = (int4 *)(smem + NB * KS * SLAB + SCR);

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid / WNW, wc = wid % WNW;
    const int M = g.M, K = g.K;

    if constexpr (AMODE != AM_DENSE) {
        for (int r = tid; r < BM; r += NTHR) {
            const int row = m0 + r;
            int4 info = make_int4(-1, 0, 0, 0);
            if (row < M) {
                const int c = find_chunk(g.row_start, g.n_chunks, row);
                const ChunkDesc cd = g.chunks[c];
                const int local = row - g.row_start[c];
                int oh, ow, base, Win;
                if constexpr (AMODE == AM_CONV2) {
                    ow = local % cd.W2; oh = local / cd.W2; base = cd.row1; Win = cd.W1;
                } else {
                    oh = local % 16; ow = local / 16; base = cd.row2; Win = cd.W2;
                }
                info = make_int4(base, 2 * oh - 1, 2 * ow - 1, Win);
            }
            rowinfo[r] = info;
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < FM; i++)
#pragma unroll
        for (int j = 0; j < FN; j++) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    const int lrow = lane >> 2, lpos = lane & 3;
    auto issue = [&](int k0, int buf) {
        int tap = 0, kh = 0, kw = 0;
        if constexpr (AMODE != AM_DENSE) {   // one 3x3 tap per stage (host: C % (32*KS) == 0)
            tap = k0 / g.C;
            kh = tap / 3;
            kw = tap - kh * 3;
        }
#pragma unroll
        for (int p = 0; p < NW; p++) {
            const int i = wid + NWAVE * p;
            if (PAD && i >= NP) {   // wave-uniform
                __builtin_amdgcn_global_load_lds((glb_void_g *)zero_line, (lds_void_g *)(smem + NB * KS * SLAB), 16, 0, 0);
                continue;
            }
            const int s = i / RG, rg = i - s * RG;
            const int r = rg * 16 + lrow;
            const int k = k0 + s * 32 + ((lpos ^ ((r >> 1) & 3)) << 3);
            const uint16_t *src = (const uint16_t *)zero_line;
            if (rg * 16 < BM) {
                const int row = m0 + r;
                if constexpr (AMODE == AM_DENSE) {
                    if (row < M) src = g.A + (long)row * g.lda + k;
                } else {
                    const int4 ri = rowinfo[r];
                    const int ih = ri.y + kh, iw = ri.z + kw;
                    const int Hin = AMODE == AM_CONV2 ? 64 : 32;
                    if (ri.x >= 0 && ih >= 0 && ih < Hin && iw >= 0 && iw < ri.w)
                        src = g.A + ((long)(ri.x + ih * ri.w + iw) * g.C + (k - tap * g.C));
                }
            } else {
                src = g.W + (long)(n0 + r - BM) * g.ldw + k;
            }
            __builtin_amdgcn_global_load_lds((glb_void_g *)src, (lds_void_g *)(smem + (buf * KS + s) * SLAB + rg * 512), 16, 0,
                                             0);
        }
    };

    const int nk = K / (32 * KS);
#pragma unroll
    for (int st = 0; st < NB - 1; st++)
        if (st < nk) issue(st * 32 * KS, st);
    int buf = 0;
    for (int kt = 0; kt < nk; kt++) {
        // this wave's pieces of stage kt have landed once at most the later
        // stages' pieces are outstanding
        const int ahead = nk - 1 - kt;
        if constexpr (NB >= 4) {
            if (ahead >= 2) wait_vm<2 * NW>();
            else if (ahead == 1) wait_vm<NW>();
            else wait_vm<0>();
        } else if constexpr (NB == 3) {
            if (ahead >= 1) wait_vm<NW>();
            else wait_vm<0>();
        } else {
            wait_vm<0>();
        }
        asm volatile("s_barrier" ::: "memory");   // every wave's pieces landed; stage kt-1's readers done
        if (kt + NB - 1 < nk) {
            int nb = buf + NB - 1;
            if (nb >= NB) nb -= NB;
            issue((kt + NB - 1) * 32 * KS, nb);
        }
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const uint16_t *sl = smem + (buf * KS + s) * SLAB;
            half8 af[FM], bf[FN];
            const int q = lane >> 4;
#pragma unroll
            for (int i = 0; i < FM; i++) {
                const int r = wr * (BM / 2) + i * 16 + (lane & 15);
                af[i] = *(const half8 *)(sl + r * 32 + ((q ^ ((r >> 1) & 3)) << 3));
            }
#pragma unroll
            for (int j = 0; j < FN; j++) {
                const int r = BM + wc * (BN / WNW) + j * 16 + (lane & 15);
                bf[j] = *(const half8 *)(sl + r * 32 + ((q ^ ((r >> 1) & 3)) << 3));
            }
#pragma unroll
            for (int i = 0; i < FM; i++)
#pragma unroll
                for (int j = 0; j < FN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (++buf == NB) buf = 0;
    }
}

}  // namespace qasr
