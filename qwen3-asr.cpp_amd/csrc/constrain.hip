// constrain.hip -- decoding constraints (kernels.h "decoding constraints"): the repetition
// penalty, the token bias list and the no-repeat n-gram ban as sparse edits of the fp32 logits row a decode
// step or prefill wrote, then a new greedy choice.
//   constrain_edit_kernel    one workgroup a logits row: the three edits in the rule's order with barriers
//                            between them, then the best key among the edited columns E.  The raw argmax g is
//                            known, and every column outside E keeps its bits, so with g outside E the row's
//                            answer is the larger of key(l[g], g) and E's best: no pass over the row.  Only
//                            with g inside E the row is flagged for the scan.
//   constrain_scan_kernel    grid (column slice, row); returns at once for a row not flagged, else folds its
//                            slice's best key of the edited row into skey[row] by one 64-bit atomicMax
//   constrain_finish_kernel  the token out of skey into d_tok / d_hist, skey and the flag re-armed
// Every edit is one rounded fp32 operation and the choice is a maximum of distinct keys, so the result does
// not depend on the grid or on the order threads and workgroups finish in.  The parameters and the bias list
// are read from device memory: a captured step serves any of their values.
#include <algorithm>

#include "dev_common.h"
#include "kernels.h"

namespace qasr {

static constexpr int kEditThreads = 256, kScanThreads = 256;

__device__ __forceinline__ unsigned long long key_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// the workgroup's largest key (every thread calls it; thread 0 holds the result)
template <int THREADS>
__device__ __forceinline__ unsigned long long block_key_max(unsigned long long best, unsigned long long *s_best) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = key_max(best, __shfl_xor(best, o, 64));
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < THREADS / 64; w++) best = key_max(best, s_best[w]);
    }
    return best;
}

// ------------------------------------------------------------------ phrases
// Step 2b for one row, called by every thread of its workgroup (barriers inside; the caller's edits of step 2 are
// behind a barrier, and this returns behind one).  s_node[j] becomes the trie node h[t - j .. t) spells, or -1:
// thread j walks from the root, each level a binary search in the node's ascending child tokens.  The nodes are
// then taken deepest first, a barrier between depths: the thread whose atomicOr marks a child token in the
// bitmap adds its bonus, a marked token is skipped -- so the deepest node that has the token decides, which with
// the compiler's eff is the rule's maximum.  The children of one node are distinct: no two threads of a depth
// touch one column.  Returns whether this thread boosted column g.
__device__ __forceinline__ int phrase_boost(const PhraseTrie &ph, float *l, const int32_t *h, int t, int g, int n_valid,
                                            uint32_t *s_seen, int *s_node) {
    const int tid = threadIdx.x;
    int *s_h = s_node + kPhraseWalkMax + 1;   // the last 15 tokens, s_h[i] = h[t - m + i]
    const int m = min(t, kPhraseWalkMax);
    for (int i = tid; i < (n_valid + 31) >> 5; i += kEditThreads) s_seen[i] = 0u;   // (the penalty's marks are spent)
    if (tid < m) s_h[tid] = h[t - m + tid];
    __syncthreads();
    if (tid <= kPhraseWalkMax) {
        int u = tid <= m ? 0 : -1;
        for (int i = 0; i < tid && u >= 0; i++) {
            const int x = s_h[m - tid + i];
            int lo = ph.child_off[u];
            const int end = ph.child_off[u + 1];
            int hi = end;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ph.tok[mid] < x) lo = mid + 1; else hi = mid;
            }
            u = lo < end && ph.tok[lo] == x ? ph.dst[lo] : -1;
            if ((unsigned)u >= (unsigned)ph.n_nodes) u = -1;   // (a header that does not fit its arrays: no walk out of them)
        }
        s_node[tid] = u;
    }
    __syncthreads();
    int hit = 0;
    for (int j = m; j >= 0; j--) {
        const int u = s_node[j];
        if (u >= 0) {
            const int end = ph.child_off[u + 1];
            for (int e = ph.child_off[u] + tid; e < end; e += kEditThreads) {
                const int v = ph.tok[e];
                if ((unsigned)v >= (unsigned)n_valid) continue;
                const uint32_t bit = 1u << (v & 31);
                if (!(atomicOr(&s_seen[v >> 5], bit) & bit)) {
                    l[v] = l[v] + ph.bonus[e];
                    hit |= v == g;
                }
            }
        }
        __syncthreads();
    }
    return hit;
}

// the best key among the boosted columns as they stand (after the ban): the saved nodes' child lists again
__device__ __forceinline__ unsigned long long phrase_keys(const PhraseTrie &ph, const float *l, int t, int n_valid, const int *s_node) {
    unsigned long long best = 0ull;
    for (int j = min(t, kPhraseWalkMax); j >= 0; j--) {
        const int u = s_node[j];
        if (u < 0) continue;
        const int end = ph.child_off[u + 1];
        for (int e = ph.child_off[u] + threadIdx.x; e < end; e += kEditThreads) {
            const int v = ph.tok[e];
            if ((unsigned)v < (unsigned)n_valid) best = key_max(best, argmax_key(l[v], v));
        }
    }
    return best;
}

// ------------------------------------------------------------------ edit
// LDS: one bit a column (dynamic, n_valid bits): the thread whose atomicOr sets a token's bit first is the
// one that applies its penalty, so a token the window holds many times is penalised once, in O(window) work.
__global__ __launch_bounds__(kEditThreads) void constrain_edit_kernel(ConstrainArgs a) {
    extern __shared__ uint32_t s_seen[];
    __shared__ unsigned long long s_best[kEditThreads / 64];
    __shared__ int s_node[2 * (kPhraseWalkMax + 1)];   // the matched node per depth, then the last tokens
    const int q = blockIdx.x, tid = threadIdx.x;
    float *l = a.logits + (size_t)q * a.ld;
    const int32_t *h = a.hist_in + (size_t)q * a.src_div * a.hist_stride;
    const int gr = a.greedy[q], g = (unsigned)gr < (unsigned)a.n_valid ? gr : 0;   // (the row's argmax: always inside)
    const ConstrainParams prm = *a.prm;
    const PhraseTrie ph = a.ph ? *a.ph : PhraseTrie{};   // (read with the parameters: no load waits behind the edits)
    const int t = min(max(*a.step, 0), a.hist_stride);
    const bool pen = prm.p != 1.0f;
    // the penalty's window h[lo .. t)
    const int lo = !pen ? t : (prm.last_n > 0 && prm.last_n < t ? t - prm.last_n : 0);
    const int nb = min(max(prm.n_bias, 0), kConstrainBiasMax);
    int hit = 0;   // this thread edited column g
    unsigned long long best = 0ull;
    // 1. penalty: once per distinct token of the window, one multiply of the raw value
    if (pen) {
        for (int i = tid; i < (a.n_valid + 31) >> 5; i += kEditThreads) s_seen[i] = 0u;
        __syncthreads();
        for (int i = lo + tid; i < t; i += kEditThreads) {
            const int v = h[i];
            if ((unsigned)v >= (unsigned)a.n_valid) continue;
            const uint32_t bit = 1u << (v & 31);
            if (!(atomicOr(&s_seen[v >> 5], bit) & bit)) {
                const float x = l[v];
                l[v] = x > 0.f ? x * prm.inv_p : x * prm.p;
            }
            hit |= v == g;
        }
        __syncthreads();
    }
    // 2. bias: the ids are distinct, one add each
    for (int k = tid; k < nb; k += kEditThreads) {
        const int v = a.bias_ids[k];
        if ((unsigned)v >= (unsigned)a.n_valid) continue;
        l[v] = l[v] + a.bias[k];
        hit |= v == g;
    }
    __syncthreads();
    // 2b. phrases: the nodes the row's last tokens spell, then one add a child token
    if (ph.n_nodes > 0) hit |= phrase_boost(ph, l, h, t, g, a.n_valid, s_seen, s_node);
    // 3. ban: every token that followed an earlier occurrence of the last n - 1 tokens (the value is final:
    // its key is taken here)
    const int n = prm.ngram;
    if (n >= 1 && n <= kConstrainNgramMax && t >= n - 1) {
        const int32_t *suf = h + (t - n + 1);
        for (int i = tid; i <= t - n; i += kEditThreads) {
            bool same = true;
            for (int k = 0; k < n - 1; k++) same = same && h[i + k] == suf[k];
            if (!same) continue;
            const int v = h[i + n - 1];
            if ((unsigned)v >= (unsigned)a.n_valid) continue;
            l[v] = -INFINITY;
            best = key_max(best, argmax_key(-INFINITY, v));
            hit |= v == g;
        }
    }
    __syncthreads();
    // 4. the best key among the penalised and biased columns, as they stand now
    for (int i = lo + tid; i < t; i += kEditThreads) {
        const int v = h[i];
        if ((unsigned)v < (unsigned)a.n_valid) best = key_max(best, argmax_key(l[v], v));
    }
    for (int k = tid; k < nb; k += kEditThreads) {
        const int v = a.bias_ids[k];
        if ((unsigned)v < (unsigned)a.n_valid) best = key_max(best, argmax_key(l[v], v));
    }
    if (ph.n_nodes > 0) best = key_max(best, phrase_keys(ph, l, t, a.n_valid, s_node));
    const int any_hit = __syncthreads_or(hit);
    best = block_key_max<kEditThreads>(best, s_best);
    if (tid == 0) {
        if (any_hit) a.flag[q] = 1;   // the scan folds the whole edited row into skey (zero at rest)
        else a.skey[q] = key_max(best, argmax_key(l[g], g));   // (column g kept its bits)
    }
}

// ------------------------------------------------------------------ scan
// grid (slice, row), 256 threads; a slice is `slice_groups` groups of 4 consecutive columns
__global__ __launch_bounds__(kScanThreads) void constrain_scan_kernel(ConstrainArgs a, int slice_groups) {
    __shared__ unsigned long long s_best[kScanThreads / 64];
    const int q = blockIdx.y, tid = threadIdx.x;
    if (!a.flag[q]) return;
    const float *l = a.logits + (size_t)q * a.ld;
    const bool vec = (a.ld & 3) == 0;   // rows 16-byte aligned
    const int g0 = blockIdx.x * slice_groups, g1 = min(g0 + slice_groups, (a.n_valid + 3) >> 2);
    unsigned long long best = 0ull;
    for (int grp = g0 + tid; grp < g1; grp += kScanThreads) {
        const int j0 = 4 * grp;
        if (vec && j0 + 4 <= a.n_valid) {
            const float4 v = *(const float4 *)(l + j0);
            best = key_max(best, key_max(key_max(argmax_key(v.x, j0), argmax_key(v.y, j0 + 1)),
                                         key_max(argmax_key(v.z, j0 + 2), argmax_key(v.w, j0 + 3))));
        } else {
            for (int j = j0; j < min(j0 + 4, a.n_valid); j++) best = key_max(best, argmax_key(l[j], j));
        }
    }
    best = block_key_max<kScanThreads>(best, s_best);
    if (tid == 0 && best) atomicMax(a.skey + q, best);
}

// ------------------------------------------------------------------ finish
// one thread a logits row: its token to every token row it serves
__global__ __launch_bounds__(256) void constrain_finish_kernel(ConstrainArgs a) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.R / a.src_div) return;
    const int tok = argmax_key_idx(a.skey[q]);
    for (int i = 0; i < a.src_div; i++) {
        const int r = q * a.src_div + i;
        a.tok[r] = tok;
        if (a.hist) a.hist[(size_t)r * a.hist_stride + *a.step] = tok;
    }
    if (a.gtok) a.gtok[q] = tok;
    if (a.scanned) a.scanned[q] = a.flag[q];
    a.skey[q] = 0ull;   // zero at rest
    a.flag[q] = 0;
}

int constrain_slices(int R, int n_valid) {
    const int groups = (n_valid + 3) / 4;
    // groups a thread, as the sampler's column pass: 1 up to 4 rows, 2 up to 32, then 4
    const int per = R <= 4 ? 1 : R <= 32 ? 2 : 4;
    return std::max(1, (groups + kScanThreads * per - 1) / (kScanThreads * per));
}

bool launch_constrain(const ConstrainArgs &a, int slices, hipStream_t s) {
    if (a.R <= 0 || a.ld <= 0 || a.n_valid <= 0 || a.n_valid > a.ld || a.n_valid > kConstrainVocabMax || a.src_div < 1 ||
        a.R % a.src_div != 0 || a.R / a.src_div > 65535 || slices < 0 || a.hist_stride < 1 || !a.logits || !a.greedy || !a.hist_in ||
        !a.step || !a.prm || !a.bias_ids || !a.bias || !a.skey || !a.flag || !a.tok)
        return false;
    const int rows = a.R / a.src_div;
    const size_t seen_bytes = (size_t)((a.n_valid + 31) / 32) * 4;
    // beyond the default dynamic LDS: ask for it on this device (128 KiB at 2^20 columns)
    if (seen_bytes > 48 * 1024 && hipFuncSetAttribute((const void *)constrain_edit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      kConstrainVocabMax / 8) != hipSuccess)
        return false;
    const int groups = (a.n_valid + 3) / 4;
    if (slices == 0) slices = constrain_slices(rows, a.n_valid);
    slices = std::min(slices, groups);
    const int slice_groups = (groups + slices - 1) / slices;
    hipLaunchKernelGGL(constrain_edit_kernel, dim3(rows), dim3(kEditThreads), seen_bytes, s, a);
    hipLaunchKernelGGL(constrain_scan_kernel, dim3((groups + slice_groups - 1) / slice_groups, rows), dim3(kScanThreads), 0, s, a,
                       slice_groups);
    hipLaunchKernelGGL(constrain_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, a);
    note_kernel("constrain", 3, slices, slice_groups);
    return true;
}

}  // namespace qasr
