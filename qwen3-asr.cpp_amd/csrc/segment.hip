// segment.hip -- pause segmentation of long recordings for gfx950: frame energy, its smoothing and the cuts.
//
// The rule is csrc/segment_host.h's.  Every sum below has one order and every square of an fp32 is
// exact in fp64, so each value has one possible result: the bits depend neither on the tile, the grid nor the batch
// a recording runs in.  No atomics, no scratch.
//
// seg_energy_kernel: one workgroup = SEG_TILE consecutive frames of one recording (the block list names recording
// and first frame, as the resampler's).  It needs e over the tile and an H-frame halo on both sides, at most
// SEG_TILE + 2 * 64 frames, recomputed from the PCM and not exchanged between workgroups.  The window's samples are
// one contiguous span of global memory -- recordings start anywhere in the pool, so the span's unaligned head is
// peeled and the rest read as 16-byte loads, a wavefront's 64 lanes on 1 KB -- staged SEG_ROWS frames at a time
// into LDS rows of SEG_LD = 161
// dwords: thread r then walks row r in order, and at column i the lanes of a wavefront sit on banks
// (161 r + i) % 64, all different (a 160-dword stride would put them on 2 banks).  SEG_ROWS = 96 keeps the static
// LDS under 64 KB, two workgroups a CU; SEG_TILE = 182 makes the window of the default H = 5 two full passes.
//
// seg_cut_kernel: one workgroup a recording runs the rule's loop.  An iteration is an arg-min over the window
// [lo, hi] of s (values are non-negative, so their fp64 bits order them as integers; equal bits go to the larger
// frame), then the maximum of s over the segment [a, c) that the cut closes.  The loop is serial by design: a cut
// depends on the one before it.
#include "dev_common.h"
#include "kernels.h"

namespace qasr {

#define SEG_TILE 182
#define SEG_ROWS 96
#define SEG_LD 161
#define SEG_HOP 160
#define SEG_HMAX 64
#define SEG_THREADS 256

__global__ __launch_bounds__(SEG_THREADS) void seg_energy_kernel(const float *__restrict__ pcm, const SegmentRec *__restrict__ recs,
                                                                 const int2 *__restrict__ blocks, int H, double *__restrict__ e_out,
                                                                 double *__restrict__ s_out) {
    __shared__ float rows[SEG_ROWS * SEG_LD];
    __shared__ double el[SEG_TILE + 2 * SEG_HMAX];
    const int2 bi = blocks[blockIdx.x];
    const SegmentRec rc = recs[bi.x];
    const int f0 = bi.y, tid = threadIdx.x, F = rc.F;
    const float *x = pcm + rc.off;
    const int tn = min(SEG_TILE, F - f0);      // frames of this tile
    const int w0 = f0 - H, wn = tn + 2 * H;    // the window: frames w0 .. w0 + wn - 1 (those outside [0, F) count 0)
    const long n_valid = (long)F * SEG_HOP;
    for (int p0 = 0; p0 < wn; p0 += SEG_ROWS) {
        const int nr = min(SEG_ROWS, wn - p0);
        const long base = (long)(w0 + p0) * SEG_HOP;
        const int total = nr * SEG_HOP;
        // the span [base, base + total) in 16-byte chunks from its first aligned sample on: `head` samples before it
        // (a recording starts anywhere in the pool), then chunks whose four samples are one load where all of them
        // are the recording's, and guarded dwords at the recording's and the span's ends
        const int head = (int)((4 - ((((long)((uintptr_t)x >> 2)) + base) & 3)) & 3);
        if (tid < head && tid < total) {
            const long src = base + tid;
            rows[tid] = src >= 0 && src < n_valid ? x[src] : 0.0f;   // (head < 4: row 0)
        }
        for (int idx = head + 4 * tid; idx < total; idx += 4 * SEG_THREADS) {
            const long src = base + idx;
            float v[4];
            if (src >= 0 && src + 3 < n_valid && idx + 3 < total) {
                const float4 q = *(const float4 *)(x + src);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int j = 0; j < 4; j++) v[j] = src + j >= 0 && src + j < n_valid && idx + j < total ? x[src + j] : 0.0f;
            }
            for (int j = 0; j < 4; j++) {
                const int r = (idx + j) / SEG_HOP;
                if (idx + j < total) rows[r * SEG_LD + (idx + j - r * SEG_HOP)] = v[j];
            }
        }
        __syncthreads();
        if (tid < nr) {
            const float *row = rows + tid * SEG_LD;
            double acc = 0.0;
            for (int i = 0; i < SEG_HOP; i++) {
                const double d = (double)row[i];
                acc = fma(d, d, acc);   // (d * d is exact: the bits of a multiply and an add)
            }
            el[p0 + tid] = acc;
        }
        __syncthreads();
    }
    if (tid < tn) {
        const int f = f0 + tid;
        const int k0 = max(0, f - H), k1 = min(F - 1, f + H);
        double acc = 0.0;
        for (int k = k0; k <= k1; k++) acc = acc + el[k - w0];
        s_out[rc.frame_off + f] = acc;
        if (e_out) e_out[rc.frame_off + f] = el[tid + H];
    }
}

struct SegKey {
    unsigned long long bits;
    int f;
};
// the smaller value, equal values to the larger frame
__device__ __forceinline__ SegKey seg_min(SegKey a, SegKey b) {
    return (b.bits < a.bits || (b.bits == a.bits && b.f > a.f)) ? b : a;
}

// arg-min of s over [lo, hi] (not empty) by the whole workgroup; every thread returns the frame
__device__ __forceinline__ int seg_block_argmin(const double *__restrict__ s, int lo, int hi, SegKey *sh) {
    const int tid = threadIdx.x;
    SegKey k{~0ull, -1};
    for (int f = lo + tid; f <= hi; f += SEG_THREADS) k = seg_min(k, SegKey{(unsigned long long)__double_as_longlong(s[f]), f});
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        SegKey other;
        other.bits = __shfl_down(k.bits, o);
        other.f = __shfl_down(k.f, o);
        k = seg_min(k, other);
    }
    __syncthreads();   // (sh may still be read from the call before)
    if ((tid & (WAVE - 1)) == 0) sh[tid / WAVE] = k;
    __syncthreads();
    SegKey r = sh[0];
    for (int w = 1; w < SEG_THREADS / WAVE; w++) r = seg_min(r, sh[w]);
    return r.f;
}

// maximum of s over [b, e) as fp64 bits (0 for an empty range) by the whole workgroup; every thread returns it
__device__ __forceinline__ unsigned long long seg_block_max(const double *__restrict__ s, int b, int e, unsigned long long *sh) {
    const int tid = threadIdx.x;
    unsigned long long m = 0ull;
    for (int f = b + tid; f < e; f += SEG_THREADS) m = max(m, (unsigned long long)__double_as_longlong(s[f]));
    for (int o = WAVE / 2; o > 0; o >>= 1) m = max(m, __shfl_down(m, o));
    __syncthreads();
    if ((tid & (WAVE - 1)) == 0) sh[tid / WAVE] = m;
    __syncthreads();
    unsigned long long r = sh[0];
    for (int w = 1; w < SEG_THREADS / WAVE; w++) r = max(r, sh[w]);
    return r;
}

__global__ __launch_bounds__(SEG_THREADS) void seg_cut_kernel(const double *__restrict__ s_all, const SegmentRec *__restrict__ recs,
                                                              int max_frames, int min_frames, int *__restrict__ cuts,
                                                              double *__restrict__ peak, int *__restrict__ n_seg,
                                                              double *__restrict__ peak_rec) {
    __shared__ SegKey shk[SEG_THREADS / WAVE];
    __shared__ unsigned long long shm[SEG_THREADS / WAVE];
    const SegmentRec rc = recs[blockIdx.x];
    const double *s = s_all + rc.frame_off;
    const int F = rc.F, tid = threadIdx.x;
    int *cu = cuts + rc.seg_off;
    double *pk = peak + rc.seg_off;
    int a = 0, K = 0;
    unsigned long long top = 0ull;
    // (K < cap always: every closed segment has at least min_frames and cap > F / min_frames; the test keeps a
    // wrong cap from writing past the recording's slots)
    while (F - a > max_frames && K + 1 < rc.cap) {
        const int lo = a + min_frames, hi = min(a + max_frames, F - min_frames);
        const int c = seg_block_argmin(s, lo, hi, shk);
        const unsigned long long m = seg_block_max(s, a, c, shm);
        if (tid == 0) {
            cu[K] = a;
            pk[K] = __longlong_as_double((long long)m);
        }
        top = max(top, m);
        K++;
        a = c;
    }
    const unsigned long long m = seg_block_max(s, a, F, shm);
    top = max(top, m);
    if (tid == 0) {
        cu[K] = a;
        pk[K] = __longlong_as_double((long long)m);
        n_seg[blockIdx.x] = K + 1;
        peak_rec[blockIdx.x] = __longlong_as_double((long long)top);
    }
}

void launch_segment(const float *pcm, const SegmentRec *recs, int B, const int2 *blocks, int n_blocks, int max_frames,
                    int min_frames, int H, double *e, double *s, int *cuts, double *peak, int *n_seg, double *peak_rec,
                    hipStream_t st, hipEvent_t between) {
    if (n_blocks > 0) hipLaunchKernelGGL(seg_energy_kernel, dim3(n_blocks), dim3(SEG_THREADS), 0, st, pcm, recs, blocks, H, e, s);
    if (between) (void)hipEventRecord(between, st);
    if (B > 0)
        hipLaunchKernelGGL(seg_cut_kernel, dim3(B), dim3(SEG_THREADS), 0, st, (const double *)s, recs, max_frames, min_frames, cuts,
                           peak, n_seg, peak_rec);
}

int segment_tile() { return SEG_TILE; }

}  // namespace qasr
