"""Shared by the LM-head tests (tests/test_gpu_lmhead_kernels.py, tests/test_lmhead_util_host.py): the ctypes bindings
of qasr_kt_lmhead / qasr_kt_rows (include/qasr_capi.h, csrc/kernel_harness.hip), the input families, float64
references and comparators.  Nothing here is measured on the code under test; buffer-state checks, the dense bound
and the RMS prologue are kernel_util's.

References.  Logits: float64 dense_terms of rms_prologue's fp16 rows against W, bound dense_bound(1024) + tie_slack.
Token and top-K ids: exact, the descending argmax-key order (value, then the lower column) of the kernel's own fp32
logits over the valid columns.  Log-probabilities: float64 log-softmax of the kernel's own logits; the bar is the
project's 2e-5 (tests/test_gpu_logprobs.py) + 2^-24 |lp64|, the final fp32 rounding of a value of that size; a
-inf logit's log-probability is -inf and NaN never passes.

The numpy restatements of the row kernels (lse_add / lse_merge in fp32, the thread split of token_logprob_kernel,
the candidate count of topk_rows_kernel) exist for the host test: they show on the CPU what the -inf rows do to the
old and the new lse_add and that the candidate-pressure row stays inside TOPK_CAND.
"""
import ctypes as C

import numpy as np

import kernel_util as ku
from kernel_util import GUARD, Result, _ok, _P, _set

K_HID = 1024
EPS = 1e-6
LP_BAR = 2e-5
TOPK_CAND = 2048       # csrc/elementwise.hip
WPG = 8                # waves a workgroup of lmhead_batch_kernel
OPS = dict(token_logprob=0, topk_rows=1, argmax_finish=2, embed=3, gather_rows=4, step_advance=5, fill_u64=6)


# ------------------------------------------------------------------ bindings
class LmheadCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("M", "N", "K", "ldx", "ldo", "hist_stride", "n_valid", "keep_step", "tk_k", "guard",
                                         "launches")] + [("eps", C.c_float)] + [
        (n, _P) for n in ("x", "norm_w", "W", "out_f32", "tok_out", "hist", "pos", "nkv", "step")] + [
        ("use_lp_part", C.c_int32), ("lp_out", _P), ("lp_hist", _P), ("use_tk_part", C.c_int32)] + [
        (n, _P) for n in ("tk_out", "tk_lp", "tk_hist", "tk_lphist", "amax", "done")] + [
        ("grid", C.c_int32), ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


class RowsCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("op", "B", "ld", "in_rows", "in_rows2", "n_valid", "K", "src_div", "hist_stride", "step",
                                         "guard")] + [("fill", C.c_uint64)] + [
        (n, _P) for n in ("f_in", "h_in", "i_in", "i_in2", "u_in", "f_out", "f_hist", "i_out", "i_hist", "u_out")] + [
        ("step_out", C.c_int32), ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


def _lib():
    import qasr
    L = qasr.lib()
    for name, typ in (("qasr_kt_lmhead", LmheadCall), ("qasr_kt_rows", RowsCall)):
        fn = getattr(L, name)
        fn.argtypes = [C.c_int, C.POINTER(typ)]
        fn.restype = C.c_int
    L.qasr_kt_lmhead_grid.argtypes = [C.c_int, C.POINTER(C.c_int32)]
    L.qasr_kt_lmhead_grid.restype = C.c_int
    return L


def lmhead_grid():
    L, g = _lib(), C.c_int32(0)
    _ok(L, L.qasr_kt_lmhead_grid(0, C.byref(g)))
    return int(g.value)


def _out(rows, ld, dtype):
    return np.zeros((rows + 2 * GUARD, ld), dtype)


def _io(rows, ld, dtype, init):
    """an in / out allocation: guard rows of 0xFF bytes, the rows = init"""
    a = np.empty((rows + 2 * GUARD, ld), dtype)
    a.view(np.uint8)[:] = 0xFF
    a[GUARD:GUARD + rows] = init
    return a


HIST_INIT, LPH_INIT, POS0, NKV0 = -7, 7.5, 100, 200


def run_lmhead(M, N, x, norm_w, W, *, K=K_HID, logits=True, lp=False, tk=0, n_valid=0, step=2, hist_stride=6, keep_step=0,
               launches=1, nkv=True, hist=True, lp_part=None, tk_part=None, drop=(), tk_k=None):
    """x [M][ldx] fp32, W [N][K] fp16.  lp / tk switch the groups on whole; lp_part / tk_part / drop / tk_k override
    single members (the partial groups a launcher must decline)"""
    c = LmheadCall(M=M, N=N, K=K, ldx=x.shape[1], ldo=N if logits else 0, hist_stride=hist_stride, n_valid=n_valid,
                   keep_step=keep_step, tk_k=tk if tk_k is None else tk_k, guard=GUARD, launches=launches, eps=EPS,
                   use_lp_part=int((lp or tk > 0) if lp_part is None else lp_part), use_tk_part=int(tk > 0 if tk_part is None else tk_part))
    rows = np.arange(M, dtype=np.int32)[:, None]
    kk = max(tk if tk_k is None else tk_k, 1)
    outs = dict(out_f32=_out(M, N, np.float32) if logits else None, tok_out=_out(M, 1, np.int32),
                hist=_io(M, hist_stride, np.int32, HIST_INIT) if hist else None, pos=_io(M, 1, np.int32, POS0 + rows),
                nkv=_io(M, 1, np.int32, NKV0 + rows) if nkv else None, step=np.array([step], np.int32),
                amax=_out(128, 1, np.uint64), done=np.full(1, 0xFFFFFFFF, np.uint32))
    if lp or tk:
        outs.update(lp_out=_out(M, 1, np.float32), lp_hist=_io(M, hist_stride, np.float32, LPH_INIT))
    if tk:
        outs.update(tk_out=_out(M, kk, np.int32), tk_lp=_out(M, kk, np.float32), tk_hist=_io(M, hist_stride * kk, np.int32, HIST_INIT),
                    tk_lphist=_io(M, hist_stride * kk, np.float32, LPH_INIT))
    for name in drop:
        outs[name] = None
    keep = _set(c, [], x=np.asarray(x, np.float32), norm_w=np.asarray(norm_w, np.float32), W=W, **outs)
    L = _lib()
    rc = L.qasr_kt_lmhead(0, C.byref(c))
    _ok(L, rc)
    del keep
    r = Result(c, outs)
    r.grid = int(c.grid)
    return r


def run_rows(op, B, *, ld=0, in_rows=0, in_rows2=0, n_valid=0, K=0, src_div=1, hist_stride=0, step=0, fill=0, f_in=None,
             h_in=None, i_in=None, i_in2=None, u_in=None, **outs):
    """outs: the output / in-out allocations by field name (f_out, f_hist, i_out, i_hist, u_out)"""
    c = RowsCall(op=OPS[op], B=B, ld=ld, in_rows=in_rows, in_rows2=in_rows2, n_valid=n_valid, K=K, src_div=src_div,
                 hist_stride=hist_stride, step=step, guard=GUARD, fill=fill)
    i32 = lambda a: None if a is None else np.asarray(a, np.int32)   # noqa: E731
    keep = _set(c, [], f_in=f_in, h_in=h_in, i_in=i32(i_in), i_in2=i32(i_in2), u_in=u_in, **outs)
    L = _lib()
    rc = L.qasr_kt_rows(0, C.byref(c))
    _ok(L, rc)
    del keep
    r = Result(c, outs)
    r.step_out = int(c.step_out)
    return r


# ----------------------------------------------------------------- key order
def argmax_keys(v, cols=None):
    """dev_common.h argmax_key: (order-preserving bits of the fp32 value) << 32 | 0xffffffff - column"""
    v = np.ascontiguousarray(v, np.float32)
    u = v.view(np.uint32)
    u = np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    cols = np.arange(v.shape[-1], dtype=np.uint64) if cols is None else np.asarray(cols, np.uint64)
    return (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - cols)


def topk_order(row, K, n_valid=0):
    """the K first columns of the row in descending key order over the valid columns, -1 where they run out"""
    nv = n_valid or len(row)
    k = argmax_keys(row[:nv])
    top = np.argsort(k)[::-1][:K]       # (keys are distinct)
    out = np.full(K, -1, np.int64)
    out[:len(top)] = top
    return out


def logsoftmax64(row, n_valid=0):
    v = np.asarray(row[:n_valid or len(row)], np.float64)
    m = v.max()
    with np.errstate(divide="ignore"):
        return v - (m + np.log(np.exp(v - m).sum()))


def lp_bar(want):
    return LP_BAR + ku.U * np.abs(np.where(np.isfinite(want), want, 0.0))


def check_lp(got, want, what="lp"):
    """|got - want| <= 2e-5 + 2^-24 |want|; -inf exactly where wanted; never NaN.  Returns the worst error / bar"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any(), f"{what}: NaN at {np.argwhere(np.isnan(got))[0]}"
    ninf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), ninf), f"{what}: -inf entries differ: got {got.ravel()[:8]} want {want.ravel()[:8]}"
    err = np.where(ninf, 0.0, np.abs(np.where(ninf, 0.0, got) - np.where(ninf, 0.0, want)))
    bad = ~(err <= lp_bar(want))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} values outside the bar, first {i}: got {got[i]!r} want {want[i]!r} err {err[i]:.3e}")
    return float((err / lp_bar(want)).max()) if err.size else 0.0


def expect_rows(logits, K, n_valid=0):
    """per row of fp32 logits: (ids [K], float64 log-probabilities [K], -inf under id -1) in key order"""
    B = logits.shape[0]
    ids, lps = np.full((B, K), -1, np.int64), np.full((B, K), -np.inf)
    for b in range(B):
        ids[b] = topk_order(logits[b], K, n_valid)
        ls = logsoftmax64(logits[b], n_valid)
        ok = ids[b] >= 0
        lps[b, ok] = ls[ids[b, ok]]
    return ids, lps


# ------------------------------------------------------- LM-head input families
def vocab_sizes(G):
    """the regimes of the issue, by workgroup count: half the workgroups idle; the 128-row ring's start-up and
    `later` branches; the ring wrapping; every batch-kernel wave busy and one with two units"""
    return dict(half=16 * (G // 2), g1=16 * (G + 1), g3=16 * (3 * G + 5), g5=16 * (5 * G + 7), g8=16 * (8 * G + 1))


def unit_owner(u, U, G, waves=WPG):
    """(wave, workgroup) of lmhead_batch_kernel and the workgroup of lmhead128_kernel that hold 16-column unit u:
    unit ranges [i U / T, (i + 1) U / T) over T = G * waves waves, or T = G workgroups"""
    def owner(T):
        i = -(-(u + 1) * T // U) - 1
        assert i * U // T <= u < (i + 1) * U // T
        return i
    gw = owner(G * waves)
    return gw, gw // waves, owner(G)


def tie_columns(N):
    """the tie row's four equal maxima: t, t + 1 (the next lane), t + 16 (the next unit), and the last unit"""
    return [3, 4, 19, N - 11]


def first_range_valid(N, G):
    """an n_valid inside the first workgroup's unit range (inside unit 0 where that workgroup holds less than a unit)"""
    return max(7, 16 * ((N // 16) // G) - 3)


ZERO_ROW, TIE_ROW = 2, 3
_CACHE = {}


def norm_weight(family):
    nw = (1.0 + 0.1 * np.random.default_rng(11).standard_normal(K_HID)).astype(np.float32)
    assert (nw > 0.5).all()
    return nw * np.float32(8) if family == "wide" else nw


def weights(N, family):
    """fp16 W [N][1024], std 1 / 32 (unit-variance logits for unit rows); `abs`: |normal|; otherwise row 3 copied to
    the tie columns"""
    key = ("W", N, "abs" if family == "abs" else "normal")
    if key not in _CACHE:
        W = ku.f16_normal(np.random.default_rng([N, 5]), (N, K_HID), 1 / 32)
        if family == "abs":
            W = (np.abs(W) + np.float16(2.0 ** -10)).astype(np.float16)
        else:
            W[tie_columns(N)[1:]] = W[tie_columns(N)[0]]
        _CACHE[key] = W
    return _CACHE[key]


def rows(N, family):
    """fp32 x [128][1024]: `normal` unit rows with the all-zero row and the tie row (= W[3], a 32-sigma maximum four
    columns share); `abs` -|normal| (with W = |normal| every logit is negative); `wide` row r near W[(7 + 37 r) % N] under
    norm_w x 8 (the maximum ~256 above logits of std 8: exp underflows nearly everywhere)"""
    rng = np.random.default_rng([N, 6, len(family)])
    X = rng.standard_normal((128, K_HID)).astype(np.float32)
    W = weights(N, family)
    if family == "abs":
        X = -np.abs(X) - np.float32(0.01)
    elif family == "wide":
        X = (W[(7 + 37 * np.arange(128)) % N].astype(np.float32) * 32 + np.float32(0.3) * X).astype(np.float32)
    else:
        X[ZERO_ROW] = 0
        X[TIE_ROW] = W[tie_columns(N)[0]].astype(np.float32)
    return X


def reference(N, family):
    """(x, norm_w, W, float64 logits [128][N], bound [128][N]) of a family at N, computed once"""
    key = ("ref", N, family)
    if key not in _CACHE:
        X, nw, W = rows(N, family), norm_weight(family), weights(N, family)
        h, _, tie = ku.rms_prologue(X, nw, EPS)
        ref, mag = ku.dense_terms(h, W)
        bound = ku.dense_bound(K_HID, mag) + ku.tie_slack(h, tie, W)
        for a in (ref, bound):
            a.setflags(write=False)
        _CACHE[key] = (X, nw, W, ref, bound)
    return _CACHE[key]


# ------------------------------------------------------ row-kernel input rows
def inf_rows(rng, ld, n_valid):
    """12 rows of normal logits (std 3), rows 1 .. 4 with -inf columns placed against the kernels' thread split
    (float4 path, ld % 4 == 0: thread t folds columns 4 (t + 1024 i) .. + 3, then the tail; scalar path: t + 1024 i):
    column 0 alone; the first float4 of thread 7; every column of thread 7; all columns but one"""
    lg = (rng.standard_normal((12, ld)) * 3).astype(np.float32)
    th = thread_of(np.arange(ld), ld, n_valid)
    lg[1, 0] = -np.inf
    first7 = np.flatnonzero(th == 7)[:4 if ld % 4 == 0 else 1]
    lg[2, first7] = -np.inf
    lg[3, th == 7] = -np.inf
    keep = lg[4, n_valid // 2]
    lg[4, :] = -np.inf
    lg[4, n_valid // 2] = keep
    return lg


def thread_of(col, ld, n_valid):
    """the thread of token_logprob_kernel / topk_rows_kernel that folds a column (-1: not a valid column)"""
    col = np.asarray(col)
    n4 = 0 if ld % 4 else n_valid >> 2
    t = np.where(col < 4 * n4, (col // 4) % 1024, (col - 4 * n4) % 1024)
    return np.where(col < n_valid, t, -1)


PRESSURE_N, PRESSURE_DECLINED_N, PRESSURE_THREADS = 253952, 254976, (5, 71, 200, 333, 512, 700, 900, 1023)


def pressure_row(K=8):
    """one row of 253952 columns (248 a thread): K - 1 threads hold every column at 10 .. 13 (integers: ties across
    threads), an eighth thread one column at 5, the rest below 4: the K-th largest thread maximum is the 5, so pass
    2 collects (K - 1) 248 + 1 keys"""
    rng = np.random.default_rng(253952)
    n = PRESSURE_N
    row = np.clip(rng.standard_normal(n) * 1.2, -4, 3.9).astype(np.float32)
    th = thread_of(np.arange(n), n, n)
    for t in PRESSURE_THREADS[1:K]:
        cols = np.flatnonzero(th == t)
        row[cols] = 10 + rng.integers(0, 4, len(cols))
    row[np.flatnonzero(th == PRESSURE_THREADS[0])[100]] = 5.0
    return row


# ----------------------------------------------- numpy restatements (host test)
def lse_add_np(m, s, v, fixed=True):
    """dev_common.h lse_add on fp32 arrays; fixed=False: as it was before a -inf value contributed nothing"""
    m, s, v = (np.asarray(a, np.float32) for a in (m, s, v))
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(-np.abs(v - m), dtype=np.float32)
        if fixed:
            e = np.where(np.isneginf(v), np.float32(0), e)
        s = np.where(v > m, s * e + np.float32(1), s + e).astype(np.float32)
    return np.fmax(m, v), s


def lse_merge_np(m, s, m2, s2):
    with np.errstate(invalid="ignore"):
        mn = np.fmax(m, m2)
        a = np.where(m == mn, s, s * np.exp(np.float32(m - mn), dtype=np.float32))
        b = np.where(m2 == mn, s2, s2 * np.exp(np.float32(m2 - mn), dtype=np.float32))
    return mn, (a + b).astype(np.float32)


def row_lse_np(row, ld, n_valid, fixed=True):
    """token_logprob_kernel's (m, s) of one row: the thread split, the xor-shuffle tree, the waves in order"""
    row = np.asarray(row, np.float32)
    m, s = np.full(1024, -np.inf, np.float32), np.zeros(1024, np.float32)
    tid = np.arange(1024)
    n4 = 0 if ld % 4 else n_valid >> 2
    for i0 in range(0, n4, 1024):
        for c in range(4):
            cols = 4 * (i0 + tid) + c
            act = (i0 + tid) < n4
            m2, s2 = lse_add_np(m, s, row[np.where(act, cols, 0)], fixed)
            m, s = np.where(act, m2, m), np.where(act, s2, s)
    for i0 in range(4 * n4, n_valid, 1024):
        cols = i0 + tid
        act = cols < n_valid
        m2, s2 = lse_add_np(m, s, row[np.where(act, cols, 0)], fixed)
        m, s = np.where(act, m2, m), np.where(act, s2, s)
    o = 32
    while o:
        m, s = lse_merge_np(m, s, m[tid ^ o], s[tid ^ o])
        o >>= 1
    M, S = m[0], s[0]
    for w in range(1, 16):
        M, S = lse_merge_np(M, S, m[64 * w], s[64 * w])
    return np.float32(M), np.float32(S)


def row_logprob_np(row, ld, n_valid, col, fixed=True):
    m, s = row_lse_np(row, ld, n_valid, fixed)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(np.float64(row[col]) - (np.float64(m) + np.log(np.float64(s))))


def topk_candidates(row, ld, n_valid, K):
    """the number of keys topk_rows_kernel's second pass collects: those >= T, the K-th largest thread maximum"""
    keys = argmax_keys(row[:n_valid])
    th = thread_of(np.arange(n_valid), ld, n_valid)
    mk = np.zeros(1024, np.uint64)
    np.maximum.at(mk, th, keys)
    top = np.sort(mk[mk > 0])[::-1]
    T = top[K - 1] if len(top) >= K else np.uint64(1)
    return int((keys >= T).sum())
