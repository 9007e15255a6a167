"""The pause segmentation's rule in NumPy (csrc/segment_host.h) and the ctypes binding of the kernel
harness qasr_kt_segment (include/qasr_capi.h, csrc/kernel_harness.hip).

The rule, for a recording of n samples at 16 kHz (fp32, finite), F = n // 160 frames, parameters max_frames,
min_frames, smooth_half = H, skip_ratio:
  1. e[f] = sum_{i = 0 .. 159} float64(x[160 f + i])^2, fp64, in ascending i (the square of an fp32 is exact in fp64).
  2. s[f] = sum_{k = max(0, f - H) .. min(F - 1, f + H)} e[k], fp64, in ascending k.
  3. a = 0, cuts = [0]; while F - a > max_frames: lo = a + min_frames, hi = min(a + max_frames, F - min_frames),
     c = the frame of [lo, hi] with the smallest s, equal values to the LARGER f; append c; a = c.
  4. segment k covers samples [160 cuts[k], 160 cuts[k + 1]), the last one ends at n; at least one segment always.
  5. peak[k] = max of s over the segment's frames (0 without frames), peak_rec = max of s over the recording; with
     skip_ratio >= 0 segment k is silent iff peak[k] <= skip_ratio * peak_rec; skip_ratio < 0: never.
Ranges: 1 <= min_frames, 2 min_frames <= max_frames <= 2^20, 0 <= smooth_half <= 64, skip_ratio not NaN.

The sums below are loops over the terms, all frames at once: the order of the additions is the rule's, not np.sum's.
"""
import ctypes as C

import numpy as np

import qasr

HOP = 160
f32, f64 = np.float32, np.float64


def frames(n: int) -> int:
    return int(n) // HOP


def energy(x) -> np.ndarray:
    x = np.ascontiguousarray(x, f32)
    F = frames(len(x))
    xf = x[:F * HOP].astype(f64).reshape(F, HOP)
    acc = np.zeros(F, f64)
    for i in range(HOP):   # ascending i, every frame at once
        acc = acc + xf[:, i] * xf[:, i]
    return acc


def smooth(e, H: int) -> np.ndarray:
    e = np.asarray(e, f64)
    F = len(e)
    ep = np.zeros(F + 2 * H, f64)   # e[k] at ep[k + H]
    ep[H:H + F] = e
    f = np.arange(F)
    acc = np.zeros(F, f64)
    for d in range(-H, H + 1):   # ascending k = f + d; a k outside [0, F) is no term of the sum
        k = f + d
        inside = (k >= 0) & (k < F)
        acc = np.where(inside, acc + ep[k + H], acc)
    return acc


def cuts_of(s, max_frames: int, min_frames: int):
    s = np.asarray(s, f64)
    F = len(s)
    a, cuts = 0, [0]
    while F - a > max_frames:
        lo, hi = a + min_frames, min(a + max_frames, F - min_frames)
        w = s[lo:hi + 1]
        c = lo + int(np.flatnonzero(w == w.min())[-1])   # the smallest value, the larger frame among equals
        cuts.append(c)
        a = c
    return cuts


def rule(x, max_frames=3000, min_frames=1000, smooth_half=5, skip_ratio=-1.0):
    """-> dict(e, s, cuts, start, n, peak, peak_rec, silent); start / n in samples"""
    x = np.ascontiguousarray(x, f32)
    e = energy(x)
    s = smooth(e, smooth_half)
    cuts = cuts_of(s, max_frames, min_frames)
    F = len(s)
    ends = cuts[1:] + [F]
    peak = np.array([s[b:t].max() if t > b else 0.0 for b, t in zip(cuts, ends)], f64)
    peak_rec = f64(s.max()) if F else f64(0.0)
    silent = [bool(skip_ratio >= 0 and p <= f64(skip_ratio) * peak_rec) for p in peak]
    start = [c * HOP for c in cuts]
    stop = start[1:] + [len(x)]
    return dict(e=e, s=s, cuts=cuts, start=start, n=[t - b for b, t in zip(start, stop)], peak=peak, peak_rec=peak_rec, silent=silent)


def bits(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


# ------------------------------------------------------------ the harness
class SegmentCall(C.Structure):
    """qasr_kt_segment_args"""
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _fields_ = [("B", C.c_int32), ("guard", C.c_int32), ("launches", C.c_int32), ("cap", C.c_int32),
                ("prm", qasr.SegmentParams), ("n", IP), ("pcm", C.POINTER(C.c_float)),
                ("e", DP), ("s", DP), ("peak", DP), ("peak_rec", DP), ("cuts", IP), ("n_seg", IP),
                ("e2", DP), ("s2", DP), ("peak2", DP), ("peak_rec2", DP), ("cuts2", IP), ("n_seg2", IP),
                ("tile", C.c_int32)]


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def kt_segment(recs, max_frames, min_frames, smooth_half, guard=16, launches=1):
    """-> (results per launch, guards intact, tile).  A launch's results: per recording a dict(e, s, cuts, peak,
    peak_rec).  The recordings are packed back to back, so one of odd length shifts the next to an odd offset."""
    L = qasr.lib()
    L.qasr_kt_segment.argtypes = [C.c_int, C.POINTER(SegmentCall)]
    L.qasr_kt_segment.restype = C.c_int
    recs = [np.ascontiguousarray(c, f32) for c in recs]
    B = len(recs)
    n = np.array([len(c) for c in recs], np.int32)
    F = [frames(k) for k in n]
    cap = max(f // min_frames + 1 for f in F)
    pcm = np.concatenate(recs + [np.zeros(1, f32)])
    G = guard

    def outs():
        return dict(e=np.zeros(sum(F) + 2 * G, f64), s=np.zeros(sum(F) + 2 * G, f64), peak=np.zeros(B * cap + 2 * G, f64),
                    peak_rec=np.zeros(B + 2 * G, f64), cuts=np.zeros(B * cap + 2 * G, np.int32), n_seg=np.zeros(B + 2 * G, np.int32))
    o = [outs(), outs()]

    def ptrs(d):
        return [_d(d["e"]), _d(d["s"]), _d(d["peak"]), _d(d["peak_rec"]), qasr._i32(d["cuts"]), qasr._i32(d["n_seg"])]
    two = ptrs(o[1]) if launches == 2 else [None] * 6
    a = SegmentCall(B, G, launches, cap, qasr.SegmentParams(max_frames, min_frames, smooth_half, -1.0), qasr._i32(n), qasr._f(pcm),
                    *ptrs(o[0]), *two, 0)
    rc = L.qasr_kt_segment(0, C.byref(a))
    if rc:
        raise qasr.QasrError(f"qasr_kt_segment: {L.qasr_last_error().decode(errors='replace')}")
    ok = True
    res = []
    off = np.concatenate([[0], np.cumsum(F)])
    for d in o[:launches]:
        for v in d.values():
            raw = v.view(np.uint8)
            gb = G * v.itemsize
            ok = ok and bool((raw[:gb] == 0xFF).all()) and bool((raw[len(raw) - gb:] == 0xFF).all())
        per = []
        for b in range(B):
            K = int(d["n_seg"][G + b])
            assert 1 <= K <= cap, (b, K, cap)
            # the slots past a recording's K segments stay as they were filled
            ok = ok and bool((d["cuts"][G + b * cap + K:G + (b + 1) * cap] == -1).all())
            per.append(dict(e=d["e"][G + off[b]:G + off[b + 1]].copy(), s=d["s"][G + off[b]:G + off[b + 1]].copy(),
                            cuts=d["cuts"][G + b * cap:G + b * cap + K].tolist(), peak=d["peak"][G + b * cap:G + b * cap + K].copy(),
                            peak_rec=f64(d["peak_rec"][G + b])))
        res.append(per)
    return res, ok, a.tile
