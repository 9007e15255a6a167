"""The resampler's rule in NumPy (csrc/resample_host.h) and the ctypes binding of the kernel
harness qasr_kt_resample (include/qasr_capi.h, csrc/kernel_harness.hip).

The rule, for an input rate sr:
  g = gcd(16000, sr), L = 16000 / g, M = sr / g; sr == 16000 is a plain copy, bit-identical, no filter.
  Supported: 4000 <= sr <= 192000 with L <= 640.
  Z = 32, BETA = 9.0, ROLL = 0.96; s = min(1, 16000 / sr) * ROLL, H = ceil(Z / s) (fp64).
  n_out = (n_in * L + M - 1) / M in 64-bit arithmetic.
  h[p][k], p = 0 .. L-1, k = 0 .. 2H, in fp64: d = (k - H) - p / L, u = d / (H + 1),
    w = I0(BETA * sqrt(1 - u^2)) / I0(BETA) for |u| < 1 else 0, raw = s * sinc(s * d) * w with
    sinc(x) = sin(pi x) / (pi x); each phase divided by the fp64 sum of its raw values in order of k, then
    rounded to fp32.
  Output n: q = n * M (64-bit), i = q / L, p = q % L; an fp64 accumulator from 0; for k = 0 .. 2H in this order
    acc = acc + (double)h[p][k] * (double)x[i + k - H], x zero outside [0, n_in); the result is (float)acc.
Both factors are fp32, so each fp64 product is exact: an fma and a multiply-add give the same bits.
"""
import ctypes as C
import math

import numpy as np

import qasr

OUT_RATE = 16000
Z, BETA, ROLL = 32.0, 9.0, 0.96
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)
f32, f64 = np.float32, np.float64


def supported(sr: int) -> bool:
    return 4000 <= sr <= 192000 and OUT_RATE // math.gcd(OUT_RATE, sr) <= 640


def plan(sr: int):
    """(L, M, H); 16000 -> (1, 1, 0)"""
    assert supported(sr), sr
    g = math.gcd(OUT_RATE, sr)
    L, M = OUT_RATE // g, sr // g
    if L == 1 and M == 1:
        return 1, 1, 0
    s = min(1.0, OUT_RATE / sr) * ROLL
    return L, M, int(math.ceil(Z / s))


def out_len(n_in: int, sr: int) -> int:
    L, M, _ = plan(sr)
    return (int(n_in) * L + M - 1) // M


def i0(x):
    """I0 by its power series, run until no element's sum changes (fp64)"""
    x = np.asarray(x, f64)
    y = x * x / 4.0
    tot, term = np.ones_like(y), np.ones_like(y)
    for j in range(1, 1000):
        term = term * (y / (float(j) * float(j)))
        nxt = tot + term
        if np.array_equal(nxt, tot):
            break
        tot = nxt
    return tot


def taps(sr: int) -> np.ndarray:
    """h[L][2H + 1], fp32"""
    L, M, H = plan(sr)
    if L == 1 and M == 1:
        return np.ones((1, 1), f32)
    s = min(1.0, OUT_RATE / sr) * ROLL
    i0b = float(i0(BETA))
    k = np.arange(2 * H + 1, dtype=f64)
    h = np.zeros((L, 2 * H + 1), f32)
    for p in range(L):
        d = (k - H) - p / L
        u = d / (H + 1)
        inside = np.abs(u) < 1.0
        w = np.where(inside, i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / i0b, 0.0)
        x = s * d
        safe = np.where(x == 0.0, 1.0, x)
        sinc = np.where(x == 0.0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
        raw = s * sinc * w
        tot = 0.0
        for v in raw.tolist():   # in order of k
            tot += v
        h[p] = (raw / tot).astype(f32)
    return h


def resample(x, sr: int, h=None) -> np.ndarray:
    """the rule over a whole clip: all outputs at once, the taps one after another (the accumulation order)"""
    x = np.ascontiguousarray(x, f32)
    L, M, H = plan(sr)
    if L == 1 and M == 1:
        return x.copy()
    h = taps(sr) if h is None else np.asarray(h, f32)
    assert h.shape == (L, 2 * H + 1)
    n_in, n_out = len(x), out_len(len(x), sr)
    q = np.arange(n_out, dtype=np.int64) * M
    i, p = q // L, q % L
    xp = np.zeros(n_in + 2 * H + 1, f64)   # x[j] at xp[j + H], zeros outside
    xp[H:H + n_in] = x
    hp = h.astype(f64)
    acc = np.zeros(n_out, f64)
    for k in range(2 * H + 1):
        acc = acc + hp[p, k] * xp[i + k]
    return acc.astype(f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------ the harness
class ResampleCall(C.Structure):
    """qasr_kt_resample_args"""
    _fields_ = [("B", C.c_int32), ("guard", C.c_int32), ("launches", C.c_int32),
                ("n_in", C.POINTER(C.c_int32)), ("rate", C.POINTER(C.c_int32)), ("pcm", C.POINTER(C.c_float)),
                ("out", C.POINTER(C.c_float)), ("out2", C.POINTER(C.c_float)), ("tile", C.c_int32)]


def kt_resample(clips, rates, guard=64, launches=1):
    """-> (outputs per clip, guards intact, second launch's outputs or None, tile).  The guards are the `guard`
    floats of 0xFF bytes before and after every clip's output; the input is followed by as many NaN floats."""
    L = qasr.lib()
    L.qasr_kt_resample.argtypes = [C.c_int, C.POINTER(ResampleCall)]
    L.qasr_kt_resample.restype = C.c_int
    clips = [np.ascontiguousarray(c, f32) for c in clips]
    n = np.array([len(c) for c in clips], np.int32)
    r = np.ascontiguousarray(rates, np.int32)
    pcm = np.concatenate(clips + [np.zeros(1, f32)])
    no = [qasr.resample_len(len(c), int(sr)) for c, sr in zip(clips, r)]   # (raises for an unsupported rate)
    total = sum(no) + 2 * guard * len(clips)
    out, out2 = np.zeros(max(total, 1), f32), np.zeros(max(total, 1), f32)
    a = ResampleCall(len(clips), guard, launches, qasr._i32(n), qasr._i32(r), qasr._f(pcm), qasr._f(out),
                     qasr._f(out2) if launches == 2 else None, 0)
    rc = L.qasr_kt_resample(0, C.byref(a))
    if rc:
        raise qasr.QasrError(f"qasr_kt_resample: {L.qasr_last_error().decode(errors='replace')}")

    def split(buf):
        res, ok, o = [], True, 0
        raw = buf.view(np.uint32)
        for k in no:
            ok = ok and bool((raw[o:o + guard] == 0xFFFFFFFF).all()) and bool((raw[o + guard + k:o + 2 * guard + k] == 0xFFFFFFFF).all())
            res.append(buf[o + guard:o + guard + k].copy())
            o += k + 2 * guard
        return res, ok
    res, ok = split(out)
    res2 = None
    if launches == 2:
        res2, ok2 = split(out2)
        ok = ok and ok2
    return res, ok, res2, a.tile
