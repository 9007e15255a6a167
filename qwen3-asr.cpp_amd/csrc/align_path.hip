// align_path.hip -- the forced aligner's monotone path for gfx950: the maximum-score non-decreasing class path over
// the classify head's fp32 logits, and the log-probability of every chosen class.
//
// The rule is csrc/align_path_host.h's.  path and score are exact functions of the logits: every
// dp value is one fp32 add of a logit and a maximum, and maxima have no rounding, so the bits depend neither on the
// template the launcher picks nor on the batch a clip runs in.  No atomics, no scratch.
//
// align_path_kernel<THREADS, CPT>: one workgroup a clip, thread t owns the CPT consecutive classes from t * CPT on,
// dp for them stays in CPT registers from the first row to the last.  A row is
//   1. the next row's logits requested (16-byte loads into CPT registers that nothing reads until the row after),
//   2. a running (max, argmax) over the thread's own run, as argmax_key's 64-bit keys: ordered value bits above,
//      0xffffffff - class below, so an unsigned max keeps the smaller class among equal values,
//   3. an inclusive prefix-max scan of the threads' totals over the wavefront (six __shfl_up steps) and its shift by
//      one lane, the maximum over every class before the thread's run inside the wave,
//   4. with more than one wave: each wave's total through LDS (two buffers, by row parity: one barrier a row) and a
//      maximum over the waves before this one,
//   5. per class max(prefix, running): its value plus the logit is the new dp, its class the backpointer.
// Backpointers leave as uint16 rows of bp_ld = C rounded up to 16 elements, a thread's run as one or two 16-byte
// stores.  After the last row the workgroup reduces the final arg-max and walks back: AP_BT_ELEMS / bp_ld backpointer
// rows at a time are copied into LDS by all threads (they are contiguous in global memory), then thread 0 follows
// them there, one LDS read a row, and writes the path.
//
// align_lse_kernel: one workgroup of 256 a timestamp row.  Row maximum, then the sum of expf(z - max) over all
// classify_num classes: each thread over its 16-byte groups in ascending order, the wave by wave_sum, the four wave
// sums in order; lse = max + logf(sum), logprob = z[path] - lse.
#include <algorithm>

#include "dev_common.h"
#include "kernels.h"

namespace qasr {

#define AP_BT_ELEMS 16384   // uint16 backpointers of one backtrack block in LDS (32 KB)
#define AP_LSE_THREADS 256

__device__ __forceinline__ float ap_neg_inf() { return __uint_as_float(0xff800000u); }

// the CPT logits of a thread's run in row `row`: classes >= C are -inf (they follow every allowed class, so no
// allowed class's prefix sees them); + 0.0f turns a -0 into +0, after which the key order is the order of the values
template <int CPT>
__device__ __forceinline__ void ap_load(const float *__restrict__ row, int C, int c0, float (&v)[CPT]) {
    if constexpr (CPT == 1) {
        v[0] = c0 < C ? row[c0] + 0.0f : ap_neg_inf();
    } else {
#pragma unroll
        for (int q = 0; q < CPT; q += 4) {
            const int c = c0 + q;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < C) t = *(const float4 *)(row + c);   // (c + 3 < ld: ld % 4 == 0 and C <= ld)
            v[q + 0] = c + 0 < C ? t.x + 0.0f : ap_neg_inf();
            v[q + 1] = c + 1 < C ? t.y + 0.0f : ap_neg_inf();
            v[q + 2] = c + 2 < C ? t.z + 0.0f : ap_neg_inf();
            v[q + 3] = c + 3 < C ? t.w + 0.0f : ap_neg_inf();
        }
    }
}

__device__ __forceinline__ unsigned long long ap_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

template <int THREADS, int CPT>
__global__ __launch_bounds__(THREADS) void align_path_kernel(const float *__restrict__ logits, long ld,
                                                             const AlignClip *__restrict__ clips, uint16_t *__restrict__ bp_all,
                                                             int32_t *__restrict__ path, float *__restrict__ score) {
    constexpr int WAVES = THREADS / WAVE;
    __shared__ unsigned long long wtot[2][WAVES];
    __shared__ __attribute__((aligned(16))) uint16_t bt[AP_BT_ELEMS];
    const AlignClip cl = clips[blockIdx.x];
    const int NT = cl.NT, C = cl.C;
    if (NT <= 0) return;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE, c0 = tid * CPT;
    const int bp_ld = align_path_bp_ld(C);
    const float *z = logits + cl.row_off * ld;
    uint16_t *bp = bp_all + cl.bp_off;

    float dp[CPT], zn[CPT], zc[CPT];
    ap_load<CPT>(z, C, c0, dp);
    if (NT > 1) ap_load<CPT>(z + ld, C, c0, zn);
    for (int i = 1; i < NT; i++) {
#pragma unroll
        for (int k = 0; k < CPT; k++) zc[k] = zn[k];
        if (i + 1 < NT) ap_load<CPT>(z + (long)(i + 1) * ld, C, c0, zn);   // in flight across the scan below
        unsigned long long run[CPT];
        run[0] = argmax_key(dp[0], c0);
#pragma unroll
        for (int k = 1; k < CPT; k++) run[k] = ap_max(run[k - 1], argmax_key(dp[k], c0 + k));
        unsigned long long inc = run[CPT - 1];
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const unsigned long long t = __shfl_up(inc, o);
            if (lane >= o) inc = ap_max(inc, t);
        }
        unsigned long long exc = __shfl_up(inc, 1);
        if (lane == 0) exc = 0ull;   // (below every key of a float: the identity)
        if constexpr (WAVES > 1) {
            if (lane == WAVE - 1) wtot[i & 1][wave] = inc;
            __syncthreads();
            for (int w = 0; w < wave; w++) exc = ap_max(exc, wtot[i & 1][w]);
        }
        uint16_t b[CPT];
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const unsigned long long mk = ap_max(exc, run[k]);
            dp[k] = fadd_rn(zc[k], argmax_key_val(mk));
            b[k] = (uint16_t)argmax_key_idx(mk);
        }
        if (c0 < C) {   // (c0 + CPT <= bp_ld: bp_ld is C rounded up to 16 and CPT divides 16)
            uint16_t *dst = bp + (long)i * bp_ld + c0;
            if constexpr (CPT == 1) {
                dst[0] = b[0];
            } else {
#pragma unroll
                for (int q = 0; q < CPT; q += 8)
                    *(uint4 *)(dst + q) = make_uint4(b[q] | (uint32_t)b[q + 1] << 16, b[q + 2] | (uint32_t)b[q + 3] << 16,
                                                     b[q + 4] | (uint32_t)b[q + 5] << 16, b[q + 6] | (uint32_t)b[q + 7] << 16);
            }
        }
    }

    // the last row's arg-max: the smallest class among equal values
    unsigned long long best = argmax_key(dp[0], c0);
#pragma unroll
    for (int k = 1; k < CPT; k++) best = ap_max(best, argmax_key(dp[k], c0 + k));
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) best = ap_max(best, __shfl_xor(best, o));
    __syncthreads();   // (wtot may still be read by the last row; the backpointer rows are the workgroup's to read)
    if (lane == 0) wtot[0][wave] = best;
    __threadfence_block();
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; w++) best = ap_max(best, wtot[0][w]);
    int cur = argmax_key_idx(best);
    int32_t *p = path + cl.row_off;
    if (tid == 0) {
        score[blockIdx.x] = argmax_key_val(best);
        p[NT - 1] = cur;
    }

    // walk back: rows hi, hi - 1 .. lo of the backpointers at a time through LDS
    const int R = AP_BT_ELEMS / bp_ld;
    for (int hi = NT - 1; hi >= 1; hi -= R) {
        const int lo = max(1, hi - R + 1);
        const uint4 *src = (const uint4 *)(bp + (long)lo * bp_ld);
        const int n16 = (hi - lo + 1) * (bp_ld / 8);
        for (int idx = tid; idx < n16; idx += THREADS) ((uint4 *)bt)[idx] = src[idx];
        __syncthreads();
        if (tid == 0)
            for (int i = hi; i >= lo; i--) {
                cur = bt[(i - lo) * bp_ld + cur];
                p[i - 1] = cur;
            }
        __syncthreads();
    }
}

__global__ __launch_bounds__(AP_LSE_THREADS) void align_lse_kernel(const float *__restrict__ logits, long ld, int N,
                                                                   const int32_t *__restrict__ path, float *__restrict__ lse_out,
                                                                   float *__restrict__ logprob) {
    __shared__ float sh[2][AP_LSE_THREADS / WAVE];
    const long r = blockIdx.x;
    const float *row = logits + r * ld;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    float mx = ap_neg_inf();
    for (int c = 4 * tid; c < N; c += 4 * AP_LSE_THREADS) {
        const float4 t = *(const float4 *)(row + c);   // (c + 3 < ld: ld % 4 == 0 and N <= ld)
        mx = fmaxf(mx, t.x);
        if (c + 1 < N) mx = fmaxf(mx, t.y);
        if (c + 2 < N) mx = fmaxf(mx, t.z);
        if (c + 3 < N) mx = fmaxf(mx, t.w);
    }
    mx = wave_max(mx);
    if (lane == 0) sh[0][wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sh[0][0], sh[0][1]), fmaxf(sh[0][2], sh[0][3]));
    float s = 0.0f;
    for (int c = 4 * tid; c < N; c += 4 * AP_LSE_THREADS) {
        const float4 t = *(const float4 *)(row + c);
        s = fadd_rn(s, expf(fsub_rn(t.x, mx)));
        if (c + 1 < N) s = fadd_rn(s, expf(fsub_rn(t.y, mx)));
        if (c + 2 < N) s = fadd_rn(s, expf(fsub_rn(t.z, mx)));
        if (c + 3 < N) s = fadd_rn(s, expf(fsub_rn(t.w, mx)));
    }
    s = wave_sum(s);
    if (lane == 0) sh[1][wave] = s;
    __syncthreads();
    if (tid == 0) {
        const float tot = fadd_rn(fadd_rn(fadd_rn(sh[1][0], sh[1][1]), sh[1][2]), sh[1][3]);
        const float lse = fadd_rn(mx, logf(tot));
        if (lse_out) lse_out[r] = lse;
        logprob[r] = fsub_rn(row[min(max(path[r], 0), N - 1)], lse);   // (the path kernel's classes are in [0, C))
    }
}

int align_path_bt_rows(int C) { return AP_BT_ELEMS / align_path_bp_ld(C); }

long align_path_layout(AlignClip *clips, int B) {
    long rows = 0, bp = 0;
    for (int b = 0; b < B; b++) {
        clips[b].row_off = rows;
        clips[b].bp_off = bp;
        rows += std::max(clips[b].NT, 0);
        bp += (long)std::max(clips[b].NT, 0) * align_path_bp_ld(std::max(clips[b].C, 1));
    }
    return bp;
}

template <int THREADS, int CPT>
static void ap_launch(const AlignPathArgs &a, hipStream_t st) {
    note_kernel("align_path", 2, THREADS, CPT);
    hipLaunchKernelGGL((align_path_kernel<THREADS, CPT>), dim3(a.B), dim3(THREADS), 0, st, a.logits, a.ld, a.d_clips, a.bp, a.path,
                       a.score);
}

bool launch_align_path(const AlignPathArgs &a, hipStream_t st) {
    const auto misaligned = [](const void *p, uintptr_t k) { return ((uintptr_t)p & (k - 1)) != 0; };
    long rows = 0;
    int maxC = 0;
    bool ok = a.B >= 0 && a.classify_num >= 1 && a.classify_num <= a.ld && a.ld % 4 == 0 && (a.B == 0 || (a.clips && a.d_clips));
    for (int b = 0; ok && b < a.B; b++) {
        const AlignClip &cl = a.clips[b];
        ok = cl.NT >= 0 && cl.C >= 1 && cl.C <= kAlignPathMaxC && cl.C <= a.classify_num && cl.row_off == rows && cl.bp_off % 8 == 0 &&
             cl.bp_off >= 0;
        rows += cl.NT;
        maxC = std::max(maxC, cl.C);
    }
    if (ok && rows > 0)
        ok = a.logits && a.bp && a.path && a.logprob && a.score && !misaligned(a.logits, 16) && !misaligned(a.bp, 16) &&
             !misaligned(a.path, 4) && !misaligned(a.logprob, 4) && !misaligned(a.score, 4) && !misaligned(a.lse, 4);
    if (!ok) {
        note_declined_shape("launch_align_path", a.B, maxC, a.classify_num);
        return false;
    }
    if (rows == 0) {
        note_kernel("align_path", 2, 0, 0);
        return true;
    }
    if (maxC <= 64) ap_launch<64, 1>(a, st);
    else if (maxC <= 512) ap_launch<64, 8>(a, st);
    else if (maxC <= 4096) ap_launch<256, 16>(a, st);
    else ap_launch<512, 16>(a, st);
    if (a.between) (void)hipEventRecord(a.between, st);
    hipLaunchKernelGGL(align_lse_kernel, dim3((unsigned)rows), dim3(AP_LSE_THREADS), 0, st, a.logits, a.ld, a.classify_num,
                       (const int32_t *)a.path, a.lse, a.logprob);
    return true;
}

}  // namespace qasr
