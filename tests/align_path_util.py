"""The forced aligner's monotone path: the rule in NumPy float32 and the ctypes wrapper of the
kernel harness (qasr_kt_align_path).  Nothing else lives here."""
import ctypes as C

import numpy as np

import qasr

f32, f64 = np.float32, np.float64


def rule(z, Cn):
    """the rule: z [NT][>= Cn] fp32, Cn classes allowed -> (path int32 [NT], score fp32).  dp[i][c] = z[i][c] +
    max_{c' <= c} dp[i-1][c'] (one fp32 add), the backpointer the smallest c' attaining the maximum; the path ends at
    the smallest class attaining the last row's maximum"""
    z = np.ascontiguousarray(z, f32)
    NT = z.shape[0]
    if NT == 0:
        return np.zeros(0, np.int32), f32(0)
    ar = np.arange(Cn)
    dp = z[0, :Cn].copy()
    bp = np.zeros((NT, Cn), np.int64)
    for i in range(1, NT):
        m = np.maximum.accumulate(dp)
        new = np.concatenate([[True], dp[1:] > m[:-1]])      # a strictly larger value: the first class attaining m
        bp[i] = np.maximum.accumulate(np.where(new, ar, 0))
        dp = (z[i, :Cn] + m).astype(f32)
    path = np.zeros(NT, np.int32)
    path[-1] = int(np.argmax(dp))                            # (argmax: the first of equal values)
    for i in range(NT - 1, 0, -1):
        path[i - 1] = bp[i, path[i]]
    return path, f32(dp[path[-1]])


def lse64(z, N):
    """float64 log-sum-exp of every row over its first N columns"""
    z = np.asarray(z, f64)[:, :N]
    mx = z.max(axis=1)
    return mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))


class PathCall(C.Structure):
    """qasr_kt_align_path_args"""
    FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _fields_ = [("B", C.c_int32), ("guard", C.c_int32), ("launches", C.c_int32), ("classify_num", C.c_int32), ("ld", C.c_int64),
                ("NT", IP), ("C", IP), ("logits", FP), ("path", IP), ("path2", IP),
                ("logprob", FP), ("lse", FP), ("score", FP), ("logprob2", FP), ("lse2", FP), ("score2", FP),
                ("bt_rows", C.c_int32), ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


def kt_align_path(clips, Cs, classify_num, guard=8, launches=1, nt=None):
    """clips: per clip its logits [NT][ld] (one ld for all), Cs: its allowed classes -> (results per launch, guards
    intact, info).  A launch's results: per clip dict(path, logprob, lse, score); info: dict(declined, tag, msg,
    bt_rows).  The clips' rows follow each other, so one with an odd NT shifts the next to an odd row offset.  With
    declined set, every output must still be all 0xFF bytes: that is part of `guards intact`."""
    L = qasr.lib()
    L.qasr_kt_align_path.argtypes = [C.c_int, C.POINTER(PathCall)]
    L.qasr_kt_align_path.restype = C.c_int
    clips = [np.ascontiguousarray(c, f32) for c in clips]
    B, ld, G = len(clips), clips[0].shape[1], guard
    NT = np.array([c.shape[0] for c in clips] if nt is None else nt, np.int32)   # (nt: a count the launcher must decline)
    Ca = np.array(Cs, np.int32)
    rows = int(np.maximum(NT, 0).sum())
    z = np.concatenate(clips + [np.zeros((1, ld), f32)])

    def outs():
        return dict(path=np.zeros(rows + 2 * G, np.int32), logprob=np.zeros(rows + 2 * G, f32), lse=np.zeros(rows + 2 * G, f32),
                    score=np.zeros(B + 2 * G, f32))
    o = [outs(), outs()]
    two = o[1] if launches == 2 else dict(path=None, logprob=None, lse=None, score=None)
    p = lambda a, f: None if a is None else f(a)
    a = PathCall(B, G, launches, classify_num, ld, qasr._i32(NT), qasr._i32(Ca), qasr._f(z), qasr._i32(o[0]["path"]), p(two["path"], qasr._i32),
                 qasr._f(o[0]["logprob"]), qasr._f(o[0]["lse"]), qasr._f(o[0]["score"]), p(two["logprob"], qasr._f), p(two["lse"], qasr._f),
                 p(two["score"], qasr._f))
    if L.qasr_kt_align_path(0, C.byref(a)):
        raise qasr.QasrError(f"qasr_kt_align_path: {L.qasr_last_error().decode(errors='replace')}")
    ok, res = True, []
    off = np.concatenate([[0], np.cumsum(NT)])
    for d in o[:launches]:
        per = []
        for k, v in d.items():
            raw = v.view(np.uint8).reshape(len(v), 4)
            live = np.zeros(len(v), bool)
            if not a.declined:
                if k == "score":
                    live[G:G + B] = NT > 0
                else:
                    live[G:G + rows] = True
            ok = ok and bool((raw[~live] == 0xFF).all())
        for b in range(B):
            s = slice(G + off[b], G + off[b + 1])
            per.append(dict(path=d["path"][s].copy(), logprob=d["logprob"][s].copy(), lse=d["lse"][s].copy(), score=d["score"][G + b]))
        res.append(per)
    return res, ok, dict(declined=bool(a.declined), tag=a.tag.decode(), msg=a.msg.decode(), bt_rows=a.bt_rows)
