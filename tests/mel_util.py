"""Shared by the log-mel tests (tests/test_mel_util_host.py, tests/test_gpu_mel_kernels.py): a float64 reference of
the front end written from the operation (numpy.fft, not the kernel's DFT loop), a per-element bound derived from the
arithmetic, the seeded signals and lengths, the ctypes bindings of qasr_mel_engine_* and qasr_mel_filters, and the
comparator.  Nothing here is measured on the code under test.

The operation (csrc/mel.hip, include/qasr_capi.h).  n samples -> TF = n // 160 + 1 frames of 400 taken at hop 160
from the signal reflect-padded by 200 on both sides (padded[i] = x[200 - i], padded[n + 200 + i] = x[n - 2 - i];
where that index is outside the clip the value is 0), periodic Hann, 201 DFT bins, |X|^2, the filterbank product
[128][201], log10(max(s, 1e-10)); the last frame is dropped, the maximum m is taken over the T = n // 160 kept
frames of the clip, and the output is (max(v, m - 8) + 4) / 4 as float32 [128][T].

The bound.  u = 2^-53; one frame's samples x_t, windowed a_t = h_t x_t, S1 = sum_t |x_t| (>= sum_t |a_t|).  Both the
code under test and this reference are within `one side` of the exact value; the bound on their difference is twice it.
  window   h_t = 0.5 (1 - cos(.)): |dh_t| <= 2u absolute (cos within 1 ulp of a value <= 1, one subtraction), the
           product one rounding: |da_t| <= 3u |x_t|.
  DFT      a component of X_k is sum_t a_t c_t, c_t = cos or sin of 2 pi k t / 400.  The code under test evaluates
           the angle as 2.0 * M_PI * k * t / 400 (three roundings and pi's own: relative 4u of an angle up to
           2 pi 200 * 399 / 400 = 1253.5), so |dc_t| <= TAU = (4 * 1253.5 + 2) u; 400 FMAs in any order add
           gamma_400 = 400u / (1 - 400u) times sum |a_t|.  Per component |d| <= (gamma_400 + TAU + 3u) S1 = GAMMA S1,
           so |dX_k| <= e = sqrt(2) GAMMA S1.  (An FFT's error is below the direct sum's: Higham, Accuracy and
           Stability of Numerical Algorithms, thm 24.2, gives ||dX||_2 <= ~7u log2(400) sqrt(400) ||a||_2 <= 1300u S1
           < GAMMA S1; test_mel_util_host.py checks numpy's rfft against a long double direct sum under this figure.)
  |X|^2    with Xm = |X_k| + e (|X_k| the reference's): |dP_k| <= 2 Xm e + e^2 + 2u Xm^2.
  filters  f_jk >= 0, 201 FMAs in any order: |ds_j| <= sum_k f_jk |dP_k| + gamma_201 sum_k f_jk (P_k + |dP_k|).
  floor    max(s, 1e-10) is 1-Lipschitz: nothing added.
  log10    between two values >= sm = max(s - ds, 1e-10): |dv| <= ds / (ln 10 * sm), plus ROUND (|v| + 8) u for the
           log10 itself (2 ulp each side) and the three roundings of m - 8, + 4 and / 4 each side (ROUND = 32).
  maximum  the code's arg-max is an element i with v_i + dv_i >= max_j (v_j - dv_j); dm = the largest dv_i among
           those (the maximum of the reference is one of them): |m' - m| <= dm.
  clamp    max(v, m - 8) is 1-Lipschitz in (v, m): max(dv, dm); where v + dv < m - 8 - dm both sides output the
           clamp, and the bound is dm alone.
  output   / 4, and half an ulp of the float32 output taken at |ref| + bound (the wider binade at a boundary).
"""
import ctypes as C

import numpy as np

from kernel_util import _ok

U = 2.0 ** -53
HOP, FS, NB, NMEL, PAD = 160, 400, 201, 128, 200
TAU = (4 * 2 * np.pi * 200 * 399 / 400 + 2) * U
GAMMA = 400 * U / (1 - 400 * U) + TAU + 3 * U
GAMMA_201 = 201 * U / (1 - 201 * U)
ROUND = 32
FLOOR = 1e-10
SR = 16000

SEAMS = [160 * t + r for t in (7, 8, 9, 15, 16, 17) for r in (0, 1, 159)]
SHORT = [160, 199, 200, 201, 202, 359, 360, 399, 400, 401]
LENGTHS = SHORT + SEAMS
TAIL_T = (7, 8, 9, 15, 16, 17)          # tail_burst's property: n = 160 T + 159 (members of SEAMS)


# ------------------------------------------------------------------ bindings
_bound = False


def lib():
    import qasr
    global _bound
    L = qasr.lib()
    if not _bound:
        F, P = C.POINTER(C.c_float), C.c_void_p
        L.qasr_mel_filters.argtypes = [F]
        L.qasr_mel_filters.restype = C.c_int
        L.qasr_mel_engine_create.argtypes = [C.c_int, C.POINTER(P)]
        L.qasr_mel_engine_create.restype = C.c_int
        L.qasr_mel_engine_free.argtypes = [P]
        L.qasr_mel_engine_free.restype = None
        L.qasr_mel_engine_run.argtypes = [P, F, C.c_int, F, F]
        L.qasr_mel_engine_run.restype = C.c_int
        _bound = True
    return L


def _f(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


_filters = None


def filters():
    """the project's table, qasr_mel_filters (host arithmetic; tests/test_oracle_golden.py pins its values)"""
    global _filters
    if _filters is None:
        out = np.zeros((NMEL, NB), np.float32)
        assert lib().qasr_mel_filters(_f(out)) == 0
        out.setflags(write=False)
        _filters = out
    return _filters


class Engine:
    """qasr_mel_engine; a HIP error ends the session (kernel_util._ok)"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _ok(lib(), lib().qasr_mel_engine_create(device, C.byref(self.h)))

    def run_rc(self, pcm, n, filt=None):
        """the raw call: (return code, out [128][max(n, 0) // 160])"""
        pcm = np.ascontiguousarray(pcm, np.float32)
        T = max(n, 0) // HOP
        out = np.zeros(max(1, NMEL * T), np.float32)
        fl = None if filt is None else np.ascontiguousarray(filt, np.float32)
        assert fl is None or fl.shape == (NMEL, NB)
        rc = lib().qasr_mel_engine_run(self.h, _f(pcm), n, _f(fl), _f(out))
        return rc, out[:NMEL * T].reshape(NMEL, T)

    def run(self, pcm, filt=None):
        rc, out = self.run_rc(pcm, len(pcm), filt)
        _ok(lib(), rc)
        return out

    def close(self):
        if self.h:
            lib().qasr_mel_engine_free(self.h)
            self.h = C.c_void_p()


def ctx_mel_rc(ctx, clips, lens=None):
    """qasr_mel on a qasr.Context as Context.mel calls it, the return code not yet judged: (rc, [out [128][T_b]]);
    lens: lengths to pass in place of the clips' own (argument checks)"""
    clips = [np.ascontiguousarray(c, np.float32) for c in clips]
    n = np.array([len(c) for c in clips] if lens is None else lens, np.int32)
    T = [max(int(k), 0) // HOP for k in n]
    out = np.zeros(max(1, NMEL * sum(T)), np.float32)
    ptrs = (C.POINTER(C.c_float) * len(clips))(*[_f(c) for c in clips])
    rc = lib().qasr_mel(ctx.h, ptrs, n.ctypes.data_as(C.POINTER(C.c_int)), len(clips), _f(out))
    offs = np.concatenate([[0], np.cumsum(T)]) * NMEL
    return rc, [out[offs[b]:offs[b + 1]].reshape(NMEL, T[b]) for b in range(len(clips))]


def ctx_mel(ctx, clips):
    """Context.mel with the HIP-error rule of the kernel tests: QASR_ERR_DEVICE ends the session, nothing is retried"""
    rc, outs = ctx_mel_rc(ctx, clips)
    _ok(lib(), rc)
    return outs


def oracle_log_mel(pcm, filt=None):
    """the C oracle (oracle/qasr_oracle.c qo_log_mel) with a filterbank of the caller's; None: oracle_py.log_mel"""
    import oracle_py as op
    if filt is None:
        return op.log_mel(pcm)
    pcm = np.ascontiguousarray(pcm, np.float32)
    fl = np.ascontiguousarray(filt, np.float32)
    T = len(pcm) // HOP
    out = np.zeros(max(1, NMEL * T), np.float32)
    assert op.olib().qo_log_mel(_f(pcm), len(pcm), _f(fl), _f(out)) == T
    return out[:NMEL * T].reshape(NMEL, T)


# ----------------------------------------------------------------- reference
def hann(periodic=True):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(FS) / (FS if periodic else FS - 1))


def reflect_pad(x, shift=0):
    """shift: the deliberate mistake of a reflect index off by one (x[199 - i] and x[n - 1 - i])"""
    n = len(x)
    xp = np.zeros(n + 2 * PAD)
    xp[PAD:PAD + n] = x
    i = np.arange(PAD)
    for dst, src in ((i, PAD - shift - i), (n + PAD + i, n - 2 + shift - i)):
        ok = (src >= 0) & (src < n)
        xp[dst[ok]] = np.asarray(x, np.float64)[src[ok]]
    return xp


def frames_of(x, shift=0):
    """[TF][400] frames of the padded clip, float64"""
    xp = reflect_pad(x, shift)
    TF = len(x) // HOP + 1
    return xp[np.arange(TF)[:, None] * HOP + np.arange(FS)[None, :]]


def log_power(x, filt=None, *, periodic=True, shift=0, floor=True, want_bound=False):
    """float64 log10(max(filters . |rfft(window * frame)|^2, 1e-10)) as [128][TF] (every frame, the dropped one too),
    and its bound dv of the same shape when asked"""
    f64 = np.asarray(filters() if filt is None else filt, np.float64)
    fr = frames_of(x, shift)
    X = np.fft.rfft(fr * hann(periodic)[None, :], axis=1)
    P = X.real ** 2 + X.imag ** 2                                   # [TF][201]
    s = P @ f64.T                                                   # [TF][128]
    with np.errstate(divide="ignore"):
        v = np.log10(np.maximum(s, FLOOR) if floor else s)
    if not want_bound:
        return v.T, None
    e = np.sqrt(2.0) * GAMMA * np.abs(fr).sum(1)[:, None]           # [TF][1]
    Xm = np.sqrt(P) + e
    dP = 2 * Xm * e + e * e + 2 * U * Xm * Xm
    ds = 2 * (dP @ f64.T + GAMMA_201 * ((P + dP) @ f64.T))          # both sides
    sm = np.maximum(s - ds, FLOOR)
    dv = ds / (np.log(10.0) * sm) + 2 * ROUND * U * (np.abs(v) + 8)
    return v.T, dv.T


def finish(v, dv=None, *, all_frames=False, clamp=8.0, m=None):
    """[128][TF] log power -> the output [128][TF - 1] (float64) and its bound; m: a maximum given from outside (the
    deliberate mistake of a maximum shared by a batch); all_frames: the mistake of a maximum over the dropped frame too"""
    T = v.shape[1] - 1
    kept = v[:, :T]
    if T == 0:
        return kept.copy(), (None if dv is None else kept.copy())
    if m is None:
        m = (v if all_frames else kept).max()
    out = (np.maximum(kept, m - clamp) + 4.0) / 4.0
    if dv is None:
        return out, None
    dk = dv[:, :T]
    dm = dk[kept + dk >= (kept - dk).max()].max()
    b = np.where(kept + dk < m - clamp - dm, dm, np.maximum(dk, dm)) / 4.0
    return out, b + 0.5 * ulp32(np.abs(out) + b)


def ulp32(a):
    """the spacing of float32 at |a| (float64 in, float64 out; normal range)"""
    a = np.maximum(np.abs(np.asarray(a, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def log_mel_reference(pcm, filt=None, want_bound=True):
    """(ref float64 [128][n // 160], bound of the same shape or None)"""
    v, dv = log_power(pcm, filt, want_bound=want_bound)
    return finish(v, dv)


def check(got, ref, bound, tag):
    """asserts |got - ref| <= bound everywhere (a NaN or an infinity on either side fails); -> the worst error / bound"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    r = ratio(got, ref, bound)
    assert r <= 1.0, f"{tag}: error / bound = {r:.4g} at {np.unravel_index(int(np.argmax(_ratios(got, ref, bound))), ref.shape)}"
    return r


def _ratios(got, ref, bound):
    with np.errstate(invalid="ignore"):
        r = np.abs(np.asarray(got, np.float64) - ref) / bound
    return np.where(np.isfinite(r), r, np.inf)


def ratio(got, ref, bound):
    """the worst error / bound without asserting (the mutation tests report it)"""
    return float(_ratios(got, ref, bound).max()) if ref.size else 0.0


# -------------------------------------------------------------------- signals
def _rng(name, n):
    return np.random.default_rng([sum(name.encode()), n])


def _noise(name, n, scale):
    return (_rng(name, n).uniform(-1.0, 1.0, n) * scale).astype(np.float32)


def quiet_1e3(n):
    """noise at 1e-3: the clip maximum is below 0 (the negative branch of the max key)"""
    return _noise("quiet3", n, 1e-3)


def quiet_1e5(n):
    return _noise("quiet5", n, 1e-5)


def silence(n):
    """digital silence: every value on the floor, the maximum -10"""
    return np.zeros(n, np.float32)


def silence_one(n):
    """all zeros but one sample: floor values next to a flat spectrum"""
    x = np.zeros(n, np.float32)
    x[n // 3] = 0.25
    return x


def dc(n):
    return np.full(n, 0.5, np.float32)


def full_scale(n):
    """a +-1 square wave at 1 kHz (16 samples a period)"""
    return np.where((np.arange(n) // 8) % 2 == 0, 1.0, -1.0).astype(np.float32)


def tone_on_silence(n):
    """a 440 Hz sine in the first half, exact zeros in the second: floor and clamp both active"""
    x = np.zeros(n, np.float32)
    h = n // 2
    x[:h] = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(h) / SR)).astype(np.float32)
    return x


def tail_burst(n, burst=True):
    """noise at 1e-3 and the last 100 samples at +-1.  At n = 160 T + 159 the last kept frame ends at sample
    160 T + 39 and the burst starts at 160 T + 59: only the dropped frame (and the reflection only it reads) sees it"""
    x = _noise("tail", n, 1e-3)
    k = min(100, n)
    x[n - k:] = np.where(np.arange(k) % 2 == 0, 1.0, -1.0) if burst else 0.0
    return x


def impulse(n):
    """one sample at 0 and one at n - 1: the two samples a reflection must not repeat"""
    x = np.zeros(n, np.float32)
    x[0] = 1.0
    x[n - 1] = -0.5
    return x


FAMILIES = {"quiet_1e-3": quiet_1e3, "quiet_1e-5": quiet_1e5, "silence": silence, "silence_one_sample": silence_one, "dc": dc,
            "full_scale": full_scale, "tone_on_silence": tone_on_silence, "tail_burst": tail_burst, "impulse": impulse}


def batch_clips():
    """the ragged batch of the isolation tests: loud next to quiet, two zero-frame clips in the middle"""
    return [full_scale(SR), quiet_1e3(SR // 2), np.zeros(0, np.float32), quiet_1e3(100), dc(int(0.3 * SR)),
            silence(int(0.2 * SR)), tail_burst(160 * 9 + 159)]
