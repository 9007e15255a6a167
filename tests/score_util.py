"""Shared by the score-head tests (tests/test_gpu_score_kernel.py, tests/test_score_host.py):
the ctypes binding of qasr_kt_score_head (include/qasr_capi.h, csrc/kernel_harness.hip), the
float64 reference over the same fp16 operands, the bound, and a float32 numpy restatement of the
kernel's reduction order (csrc/score_head.hip).  Nothing here is measured on the code under test.
"""
import ctypes as C

import numpy as np

from kernel_util import GUARD, _ok, _set, dense_bound, dense_terms

_P = C.c_void_p
LSE_BAR = 2e-5   # tests/test_gpu_logprobs.py's bar for the fp32 (m, s) scheme over 151,936-wide rows


class ScoreCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("R", "N", "K", "lda", "ldw", "n_valid", "cols_fast", "guard", "launches")] + [
        (n, _P) for n in ("A", "W", "target", "lp", "gid", "glp")] + [
        ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


class ScoreResult:
    def __init__(self, call, lp, gid, glp):
        self.tag, self.declined, self.msg = call.tag.decode(), bool(call.declined), call.msg.decode()
        self.lp, self.gid, self.glp = lp, gid, glp   # whole allocations: GUARD + R + GUARD entries


def run_score_head(A, W, target, n_valid=0, cols_fast=0, launches=1, K=None):
    """A fp16 bits [R][lda], W fp16 bits [N][ldw] (K: the smaller width unless given), target int32 [R]"""
    import qasr
    L = qasr.lib()
    L.qasr_kt_score_head.argtypes = [C.c_int, C.POINTER(ScoreCall)]
    L.qasr_kt_score_head.restype = C.c_int
    R, N, K = A.shape[0], W.shape[0], K or min(A.shape[1], W.shape[1])
    c = ScoreCall(R=R, N=N, K=K, lda=A.shape[1], ldw=W.shape[1], n_valid=n_valid, cols_fast=cols_fast, guard=GUARD,
                  launches=launches)
    lp, gid, glp = np.zeros(R + 2 * GUARD, np.float32), np.zeros(R + 2 * GUARD, np.int32), np.zeros(R + 2 * GUARD, np.float32)
    keep = _set(c, [], A=A, W=W, target=np.asarray(target, np.int32), lp=lp, gid=gid, glp=glp)
    rc = L.qasr_kt_score_head(0, C.byref(c))
    _ok(L, rc)
    del keep
    return ScoreResult(c, lp, gid, glp)


def body(buf, R, what):
    """guards untouched, every entry written, no NaN; returns the R entries"""
    raw = buf.view(np.uint32)
    assert (raw[:GUARD] == 0xFFFFFFFF).all() and (raw[GUARD + R:] == 0xFFFFFFFF).all(), f"{what}: guard entries overwritten"
    out = buf[GUARD:GUARD + R]
    assert not (raw[GUARD:GUARD + R] == 0xFFFFFFFF).any(), f"{what}: entries never written"
    if buf.dtype == np.float32:
        assert not np.isnan(out).any(), f"{what}: NaN"
    return out


# ---------------------------------------------------------------- reference
def lse64(logits):
    m = logits.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))[..., 0]


def lp64(logits, target):
    """float64 log softmax(logits)[target] per row"""
    lg = np.asarray(logits, np.float64)
    return lg[np.arange(lg.shape[0]), np.asarray(target)] - lse64(lg)


def reference(A16, W16, target, n_valid=0):
    """float64 logits of the fp16 operands over the valid columns -> (logits, lp, glp, bound per row).
    Bound: the target's logit and the log-sum-exp (a weighted mean of the logits' movements) each move by at
    most the dot-product bound of the row's largest |a||w| sum, plus LSE_BAR for the fp32 reduction."""
    ref, mag = dense_terms(A16, W16)
    nv = n_valid or ref.shape[1]
    ref, mag = ref[:, :nv], mag[:, :nv]
    K = A16.shape[1]
    bound = 2 * dense_bound(K, mag.max(axis=1)) + LSE_BAR
    return ref, lp64(ref, target), ref.max(axis=1) - lse64(ref), bound


def check_gid(gid, ref, bound, what="gid"):
    """the greedy id: exactly the first maximum (kernel_util.check_argmax) on the rows whose float64 top-2
    gap exceeds the bound on a logit pair; a tie or near-tie inside it accepts either id"""
    from kernel_util import check_argmax
    top2 = np.partition(ref, -2, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > bound
    if clear.any():
        check_argmax(np.asarray(gid)[clear], ref[clear], what=what)
    for r in np.flatnonzero(~clear):
        assert ref[r].max() - ref[r, gid[r]] <= bound[r], f"{what}: row {r} id {gid[r]} is not within the bound of the maximum"
    return int(clear.sum())


# ---------------------------------------------- the kernel's order, in float32
f32 = np.float32


def _merge(m, s, m2, s2):
    """lse_merge (csrc/dev_common.h) on float32 arrays"""
    mn = np.maximum(m, m2)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(m == mn, s, s * np.exp((m - mn).astype(f32), dtype=f32))
        b = np.where(m2 == mn, s2, s2 * np.exp((m2 - mn).astype(f32), dtype=f32))
    return mn, (a.astype(f32) + b.astype(f32)).astype(f32)


def simulate(logits32, n_valid=0):
    """float32 restatement of score_head.hip over fp32 logits [R][N] (N % 128 == 0): per 64-column half
    tile the maximum, then s = sum exp(v - m) -- lane l (0..15) adds columns l, l + 16, l + 32, l + 48 in
    order, the 16 lanes add by the DPP butterfly (xor 1, xor 2, half mirror, mirror; lane 0's value) --
    the two halves of a 128-column tile merged in order, lane l of the merge wave taking tiles l, l + 64,
    ... in ascending order, then the 64 lanes by the xor butterfly.  Returns (m, s) per row."""
    lg = np.asarray(logits32, f32)
    R, N = lg.shape
    nv = n_valid or N
    valid = (np.arange(N) < nv)
    x = np.where(valid[None, :], lg, -np.inf).reshape(R, N // 64, 4, 16)   # [row][half][j][lane]
    m = x.max(axis=(2, 3))
    with np.errstate(invalid="ignore"):
        e = np.where(np.isfinite(x), np.exp((x - m[:, :, None, None]).astype(f32), dtype=f32), f32(0)).astype(f32)
    lane = np.zeros((R, N // 64, 16), f32)
    for j in range(4):
        lane = (lane + e[:, :, j, :]).astype(f32)
    idx = np.arange(16)
    for perm in (idx ^ 1, idx ^ 2, (idx & 8) | (7 - (idx & 7)), 15 - idx):
        lane = (lane + lane[:, :, perm]).astype(f32)
    s = lane[:, :, 0]
    s = np.where(np.isfinite(m), s, f32(0))
    tm, ts = _merge(m[:, 0::2], s[:, 0::2], m[:, 1::2], s[:, 1::2])     # [row][tile]
    nt = tm.shape[1]
    pad = (-nt) % 64
    tm = np.concatenate([tm, np.full((R, pad), -np.inf, f32)], axis=1).reshape(R, -1, 64)
    ts = np.concatenate([ts, np.zeros((R, pad), f32)], axis=1).reshape(R, -1, 64)
    lm, ls = np.full((R, 64), -np.inf, f32), np.zeros((R, 64), f32)
    for k in range(tm.shape[1]):
        nm, ns = _merge(lm, ls, tm[:, k], ts[:, k])
        skip = ~np.isfinite(tm[:, k])   # (an empty tile is skipped)
        lm, ls = np.where(skip, lm, nm), np.where(skip, ls, ns)
    i64 = np.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        lm, ls = _merge(lm, ls, lm[:, i64 ^ o], ls[:, i64 ^ o])
    return lm[:, 0], ls[:, 0]


def simulate_lp(logits32, target, n_valid=0):
    """lse_logprob of the simulated (m, s): float32(double(v) - (double(m) + log(double(s))))"""
    m, s = simulate(logits32, n_valid)
    v = np.asarray(logits32, f32)[np.arange(len(m)), np.asarray(target)]
    return (v.astype(np.float64) - (m.astype(np.float64) + np.log(s.astype(np.float64)))).astype(f32)


# -------------------------------------------------------------------- inputs
def make_case(seed, R, N, K, n_valid=0):
    """fp16 operands with logits of a few units, the special rows and targets of the kernel tests:
    row 0 all zeros; row 1 (R >= 3) = 16 W[j]: one logit >= 30 above the rest, target = that j;
    row 2: target = its float64 argmax; the other targets cycle through 0, n_valid - 1, 127, 128, 128"""
    rng = np.random.default_rng(seed)
    nv = n_valid or N
    A = rng.standard_normal((R, K)).astype(np.float16)
    W = (rng.standard_normal((N, K)) * (2.0 / np.sqrt(K))).astype(np.float16)
    A[0] = 0
    tg = np.array([(0, 0, 0, nv - 1, 127, 128, 128, 0)[i % 8] for i in range(R)], np.int32)
    if R >= 3:
        j = (nv * 3) // 5
        A[1] = (16.0 * W[j].astype(np.float32)).astype(np.float16)
        tg[1] = j
        ref2 = A[2].astype(np.float64) @ W[:nv].astype(np.float64).T
        tg[2] = int(np.argmax(ref2))
    return A, W, tg
