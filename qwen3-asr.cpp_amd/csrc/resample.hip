// resample.hip -- batched polyphase windowed-sinc resampler to 16 kHz for gfx950.
//
// The rule is csrc/resample_host.h's: output n of a clip at rate sr reads the 2H + 1 input samples
// around i = n * M / L through phase p = n * M % L of an fp32 tap table, accumulated in fp64 in tap order.  Both
// factors are fp32, so each fp64 product is exact and the chain of fmas below has one possible result per output:
// the bits do not depend on the tile, the grid or the batch a clip runs in.
//
// Layout: one workgroup = RS_TILE consecutive outputs of one clip (the block list names clip and first output, as
// the mel kernel's), one launch for a batch of clips at mixed rates.  The tile's input window -- (RS_TILE - 1) * M / L
// + 2H + 1 samples at most -- is staged in LDS with zeros outside the clip, so the tap loop has no bounds test.
// Thread t owns outputs t and t + 256 of the tile; neighbouring lanes own neighbouring outputs, whose phases differ.
// The table is stored [k][r] with r = n % L (kernels.h ResampleClip), so at tap k a wavefront reads L-periodic
// consecutive floats: one or two cache lines from L2 for the rational rates (L = 40 .. 640, tables up to ~120 KB,
// shared by every workgroup of the rate), and a table of at most RS_TAPS_LDS floats (L = 1 .. 4: 8, 12, 24, 32,
// 48, 96, 192 kHz) is copied to LDS first.
#include "dev_common.h"
#include "kernels.h"

namespace qasr {

#define RS_TILE 512
#define RS_WIN 7168        // floats: 511 * 12 + 2 * 401 + 1 at 192 kHz, the widest supported window
#define RS_TAPS_LDS 4096   // floats

// two outputs' chains side by side (independent accumulators hide the fp64 fma latency)
// (TP: the table's pointer type -- LDS, or global memory by name so the loads are global_load, not flat)
typedef const __attribute__((address_space(1))) float *GlobalTaps;
template <class TP>
__device__ __forceinline__ void resample_chains(TP tp, int L, int T, const float *__restrict__ w0,
                                                const float *__restrict__ w1, int r0, int r1, double &a0, double &a1) {
    for (int k = 0; k < T; k++) {
        const TP row = tp + (size_t)k * L;
        a0 = fma((double)row[r0], (double)w0[k], a0);
        a1 = fma((double)row[r1], (double)w1[k], a1);
    }
}

__global__ __launch_bounds__(256) void resample_kernel(const float *__restrict__ in, const ResampleClip *__restrict__ clips,
                                                       const int2 *__restrict__ blocks, float *__restrict__ out) {
    __shared__ float win[RS_WIN];
    __shared__ float tl[RS_TAPS_LDS];
    const int2 bi = blocks[blockIdx.x];
    const ResampleClip c = clips[bi.x];
    const int n0 = bi.y, tid = threadIdx.x;
    const float *x = in + c.in_off;
    float *y = out + c.out_off;
    if (c.L == 1 && c.M == 1) {   // 16 kHz: the samples as they are
        for (int t = tid; t < RS_TILE; t += 256)
            if (t < c.n_out - n0) y[n0 + t] = x[n0 + t];
        return;
    }
    const int L = c.L, M = c.M, H = c.H, T = 2 * H + 1;
    const long q0 = (long)n0 * M;
    const long i0 = q0 / L;
    const int p0 = (int)(q0 - i0 * L);
    const int wlen = (p0 + (RS_TILE - 1) * M) / L + T;   // <= RS_WIN (resample_fits)
    for (int idx = tid; idx < wlen; idx += 256) {
        const long src = i0 - H + idx;
        win[idx] = src >= 0 && src < c.n_in ? x[src] : 0.0f;
    }
    const bool lds_taps = L * T <= RS_TAPS_LDS;
    if (lds_taps)
        for (int idx = tid; idx < L * T; idx += 256) tl[idx] = ((GlobalTaps)c.taps)[idx];
    __syncthreads();
    const int e0 = p0 + tid * M, e1 = p0 + (tid + 256) * M;   // q - i0 * L of the two outputs (< 2^31: 512 * 441 + 640)
    const int d0 = e0 / L, d1 = e1 / L;                       // their first window sample
    const int rb = n0 % L;
    const int r0 = (rb + tid) % L, r1 = (rb + tid + 256) % L;
    double a0 = 0.0, a1 = 0.0;
    if (lds_taps) resample_chains((const float *)tl, L, T, win + d0, win + d1, r0, r1, a0, a1);
    else resample_chains((GlobalTaps)c.taps, L, T, win + d0, win + d1, r0, r1, a0, a1);
    if (tid < c.n_out - n0) y[n0 + tid] = (float)a0;
    if (tid + 256 < c.n_out - n0) y[n0 + tid + 256] = (float)a1;
}

void launch_resample(const float *in, const ResampleClip *clips, const int2 *blocks, int n_blocks, float *out, hipStream_t s) {
    if (n_blocks > 0) hipLaunchKernelGGL(resample_kernel, dim3(n_blocks), dim3(256), 0, s, in, clips, blocks, out);
}

int resample_tile() { return RS_TILE; }

bool resample_fits(int L, int M, int H) {
    if (L < 1 || M < 1 || H < 0) return false;
    return ((long)(L - 1) + (long)(RS_TILE - 1) * M) / L + 2L * H + 1 <= RS_WIN;
}

}  // namespace qasr
