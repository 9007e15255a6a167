// beam.hip -- the two device pieces of beam search (kernels.h "beam search"):
//   kv_fork_kernel      cache slot b continues slot parent[b]'s history: K, V and V^T of a position
//                       range copied between the rows of a group, in place
//   beam_select_kernel  the next W live rows of every group from the step's W x W candidates
// Both read their per-row arguments from device memory, so a captured decode step replays them
// with the values the previous kernel wrote.
#include <algorithm>

#include "dev_common.h"
#include "kernels.h"

namespace qasr {

// ------------------------------------------------------------------ KV fork
// One workgroup per (8-key block, group x kv head, layer), 128 threads.  Per row and block the data is
// 2 KiB of K, 2 KiB of V (8 rows of 128 fp16) and one 2 KiB V^T block ([128 d][8 keys]): 128 16-B
// accesses each, one per thread.  Thread t reads and writes only access t of every row's three
// blocks, and no other thread or workgroup touches those bytes, so a permutation of the rows (swaps,
// cycles, shared parents) is safe in place by the thread's own program order: every load into
// registers, s_waitcnt vmcnt(0), then the stores.  (The barrier after the wait is not what the
// safety rests on; it keeps the workgroup's stores together.)  A V^T block only partly inside
// [from, to) is blended with the row's own block, 16 bits a key.
static constexpr int kForkRows = 8;   // largest group

__global__ __launch_bounds__(128) void kv_fork_kernel(KvForkArgs a) {
    const int blk = blockIdx.x, g = blockIdx.y / a.n_kv_head, h = blockIdx.y % a.n_kv_head, l = blockIdx.z;
    const int t = threadIdx.x, k0 = blk * 8, row0 = g * a.group;
    if (k0 >= a.max_ctx) return;
    const size_t kv_head = (size_t)a.max_ctx * 128, vt_head = (size_t)128 * vt_ctx(a.max_ctx);
    const size_t kv_layer = (size_t)a.slots * a.n_kv_head * kv_head, vt_layer = (size_t)a.slots * a.n_kv_head * vt_head;
    uint16_t *kc = a.kc + l * kv_layer, *vc = a.vc + l * kv_layer, *vt = a.vt + l * vt_layer;
    auto kv_at = [&](uint16_t *base, int slot) { return (uint4 *)(base + ((size_t)slot * a.n_kv_head + h) * kv_head + (size_t)k0 * 128); };
    auto vt_at = [&](int slot) { return (uint4 *)(vt + ((size_t)slot * a.n_kv_head + h) * vt_head + (size_t)blk * 1024); };
    uint4 rk[kForkRows], rv[kForkRows], rt[kForkRows];
    int lo[kForkRows], hi[kForkRows];   // the row's keys of this block: [lo, hi), empty = nothing to do
    const int key = t >> 4;             // K / V: 16 accesses a key row
    bool any = false;
#pragma unroll
    for (int i = 0; i < kForkRows; i++) {
        lo[i] = hi[i] = 0;
        rk[i] = rv[i] = rt[i] = make_uint4(0u, 0u, 0u, 0u);
        const int b = row0 + i, p = i < a.group ? a.parent[b] : b;
        int x = 0, y = 0;
        if (p != b && p >= row0 && p < row0 + a.group) {   // (a parent outside the group is never followed)
            const int f = max(a.from[b], 0), e = min(a.to[b], a.max_ctx);
            x = max(f, k0) - k0;
            y = min(e, k0 + 8) - k0;
        }
        if (x < y) {
            lo[i] = x;
            hi[i] = y;
            any = true;
            if (key >= x && key < y) {
                rk[i] = kv_at(kc, p)[t];
                rv[i] = kv_at(vc, p)[t];
            }
            uint4 pt = vt_at(p)[t];   // dimension t's 8 keys
            if (y - x < 8) {
                const uint4 own = vt_at(b)[t];
                uint32_t pw[4] = {pt.x, pt.y, pt.z, pt.w};
                const uint32_t ow[4] = {own.x, own.y, own.z, own.w};
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    const uint32_t m = ((2 * w >= x && 2 * w < y) ? 0xffffu : 0u) | ((2 * w + 1 >= x && 2 * w + 1 < y) ? 0xffff0000u : 0u);
                    pw[w] = (pw[w] & m) | (ow[w] & ~m);
                }
                pt = make_uint4(pw[0], pw[1], pw[2], pw[3]);
            }
            rt[i] = pt;
        }
    }
    if (!any) return;   // (uniform: every value above is the same for the whole workgroup)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kForkRows; i++) {
        if (lo[i] >= hi[i]) continue;
        const int b = row0 + i;
        if (key >= lo[i] && key < hi[i]) {
            kv_at(kc, b)[t] = rk[i];
            kv_at(vc, b)[t] = rv[i];
        }
        vt_at(b)[t] = rt[i];
    }
}

bool launch_kv_fork(const KvForkArgs &a, hipStream_t s) {
    if (a.group < 1 || a.group > kForkRows || a.B <= 0 || a.B % a.group != 0 || a.B > a.slots || a.blocks <= 0 || a.layers <= 0 ||
        a.n_kv_head <= 0 || a.max_ctx <= 0)
        return false;
    const int blocks = std::min(a.blocks, (a.max_ctx + 7) / 8);
    kv_fork_kernel<<<dim3(blocks, (a.B / a.group) * a.n_kv_head, a.layers), 128, 0, s>>>(a);
    return true;
}

// -------------------------------------------------------------- beam select
// One workgroup (one wave) per group.  The W x W candidates (row r, rank j) are ranked by counting:
// candidate c = r * W + j precedes c' when its score is larger, or equal with c < c' (lower row,
// then lower rank).  Lane 0 then walks them in order (DESIGN.md "Beam search", the normative rule).
__global__ __launch_bounds__(64) void beam_select_kernel(BeamSelectArgs a) {
    const int g = blockIdx.x, W = a.W, row0 = g * W, c = threadIdx.x, n = W * W;
    __shared__ float s_score[64], s_lp[64];
    __shared__ int32_t s_id[64];
    __shared__ int s_order[64];
    const int t = a.t[g];
    const bool first = t == 0, frozen = a.done[g] != 0;
    if (c < n) {
        const int r = c / W, j = c % W;
        // the first step ranks the prefill's logits: one row a clip (row g), which every row of the group stands for
        const int src = first ? g : row0 + r;
        const float lp = a.tk_lp[(size_t)src * W + j];
        s_lp[c] = lp;
        s_id[c] = a.tk_id[(size_t)src * W + j];
        s_score[c] = a.cum[row0 + r] + lp;
    }
    __syncthreads();
    if (c < n) {
        const float sc = s_score[c];
        int rank = 0;
        for (int o = 0; o < n; o++) rank += (s_score[o] > sc || (s_score[o] == sc && o < c)) ? 1 : 0;
        s_order[rank] = c;
    }
    __syncthreads();
    if (c != 0) return;
    const int P = a.P[g], hslot = t - a.hist_base;
    const int32_t eos = *a.eos;   // (device memory: a captured step serves runs with and without ignore_eos)
    if (frozen) {   // a done group: identity parents, no records
        for (int b = 0; b < W; b++) {
            a.parent[row0 + b] = row0 + b;
            a.from[row0 + b] = a.to[row0 + b] = 0;
        }
        return;
    }
    int nl = 0, nfin = a.n_fin[g];
    float ncum[8];
    for (int i = 0; i < n && nl < W; i++) {
        const int cc = s_order[i], r = cc / W;
        const int32_t id = s_id[cc];
        if (id == eos) {   // (eos < 0 with ignore_eos: never equal)
            if (i < W && nfin < W) {
                const int e = row0 + nfin++;
                a.fin_row[e] = row0 + r;
                a.fin_t[e] = t;
                a.fin_sum[e] = s_score[cc];
                a.fin_lp[e] = s_lp[cc];
            }
            continue;
        }
        const int b = row0 + nl;
        a.parent[b] = first ? row0 : row0 + r;   // (first step: every row is a copy of the prefilled row 0)
        a.from[b] = first ? 0 : P;
        a.to[b] = P + t;
        a.tok[b] = id;
        ncum[nl] = s_score[cc];
        const size_t hs = (size_t)hslot * a.hist_stride + b;
        a.h_par[hs] = row0 + r;
        a.h_id[hs] = id;
        a.h_lp[hs] = s_lp[cc];
        nl++;
    }
    for (int b = 0; b < nl; b++) a.cum[row0 + b] = ncum[b];   // (nl == W: the W * W candidates of W >= 2 hold at most W EOS)
    a.n_fin[g] = nfin;
    if (nfin == W) a.done[g] = t + 1;
    a.t[g] = t + 1;
}

bool launch_beam_select(const BeamSelectArgs &a, hipStream_t s) {
    if (a.W < 2 || a.W > 8 || a.G <= 0 || !a.eos) return false;
    beam_select_kernel<<<a.G, 64, 0, s>>>(a);
    return true;
}

}  // namespace qasr
