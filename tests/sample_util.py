"""Shared by the sampling tests: the normative sampling rule restated in numpy, the
float64 reference and acceptance band the device draws are held to, and the ctypes binding of
qasr_kt_sample (include/qasr_capi.h, csrc/kernel_harness.hip).  Nothing here is measured on the code
under test except `G_DEV_ERR`, which tests/test_gpu_sample_kernel.py's G(u) test verifies on the device.

The rule.  A draw is identified by (seed, clip, sample, t).  For column j of the row's fp32 logits l[0 .. n_valid):
  1. w = Philox4x32-10(counter {j >> 2, t, clip, sample}, key {seed & 0xffffffff, seed >> 32})[j & 3]
  2. u = ((w >> 9) + 0.5) * 2^-23          (exact in fp32, inside (0, 1))
  3. G = -logf(-logf(u))
  4. j is a candidate iff l[j] >= l[g] + cut in fp32 (g the greedy token, cut = T * logf(min_p), -inf for
     min_p <= 0); a NaN logit never is, g always is
  5. key = fmaf(l[j], 1 / T, G)
  6. the drawn token is the candidate with the largest key, equal keys by lower column
"""
import ctypes as C

import numpy as np

f32 = np.float32
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 values, key: 2 -> 4 uint32 arrays; vectorised over the counters"""
    c = [np.asarray(x, np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def draw_bits(seed, clip, sample, t, n):
    """w for columns 0 .. n - 1 of one draw"""
    grp = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((grp, t, clip, sample), (seed & MASK, (seed >> 32) & MASK))
    return np.stack(w, axis=1).reshape(-1)[:n]


def u_of(w):
    """step 2 as float64 (every value is exact in fp32 too)"""
    return ((np.asarray(w, np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel64(u):
    return -np.log(-np.log(np.asarray(u, np.float64)))


def host_scalars(T, min_p):
    """(inv_T, cut) as the host computes them, in fp32"""
    T = f32(T)
    inv_T = f32(1.0) / T
    with np.errstate(divide="ignore"):
        cut = f32(T * np.log(f32(min_p), dtype=f32)) if min_p > 0 else f32(-np.inf)
    return f32(inv_T), f32(cut)


def candidates(l, g, cut):
    """step 4 in fp32"""
    l = np.asarray(l, f32)
    with np.errstate(invalid="ignore"):
        thr = f32(l[g] + f32(cut))
        c = l >= thr
    c[g] = True
    return c


def keys64(l, inv_T, seed, clip, sample, t):
    """the float64 reference keys of one draw over all of l's columns"""
    l = np.asarray(l, f32)
    G = gumbel64(u_of(draw_bits(seed, clip, sample, t, len(l))))
    with np.errstate(invalid="ignore"):
        return l.astype(np.float64) * np.float64(f32(inv_T)) + G


def draw(l, T, min_p, seed, clip, sample, t, g=None):
    """the rule's token, keys in float64 (-> token, key64 of it)"""
    l = np.asarray(l, f32)
    inv_T, cut = host_scalars(T, min_p)
    if g is None:
        g = int(np.nanargmax(l))
    k = keys64(l, inv_T, seed, clip, sample, t)
    k = np.where(candidates(l, g, cut), k, -np.inf)
    k[np.isnan(k)] = -np.inf
    if not np.isfinite(k).any() and not (k == np.inf).any():   # only -inf keys: the lowest candidate column
        return int(np.flatnonzero(candidates(l, g, cut))[0]), -np.inf
    j = int(np.argmax(k))   # (first maximum: equal keys by lower column)
    return j, float(k[j])


# ------------------------------------------------------------- acceptance band
# worst |G_device - G64| over all 2^23 values of u, measured once by the harness's dump mode: 1.5458e-06, at
# n = 2^23 - 2 where G = 15.54 (tests/test_gpu_sample_kernel.py::test_gumbel_all_u holds the device to it;
# DESIGN.md §5.5).  What two logf of at most 1 ulp allow is 2^-19 + 2^-23 = 2.03e-06: the outer one's ulp at
# |G| in [16, 16.64), plus the inner one's 2^-23 relative error, which moves the outer result by as much.
G_DEV_ERR = 1.546e-06


def delta(lg_scaled_abs):
    """the band: twice (the worst G error + one fp32 ulp at max(|l[g] * inv_T|, 17) for the fmaf)"""
    mag = max(float(lg_scaled_abs), 17.0)
    ulp = float(np.spacing(f32(mag)))
    return 2.0 * (G_DEV_ERR + ulp)


def check_draw(l, tok, key, T, min_p, seed, clip, sample, t, g=None, what="draw"):
    """one device draw against the band; returns True when the row is decided (then tok equals the reference)"""
    l = np.asarray(l, f32)
    inv_T, cut = host_scalars(T, min_p)
    if g is None:
        g = int(np.nanargmax(l))
    cand = candidates(l, g, cut)
    assert 0 <= tok < len(l) and cand[tok], f"{what}: token {tok} is not a candidate"
    k = keys64(l, inv_T, seed, clip, sample, t)
    k = np.where(cand & ~np.isnan(k), k, -np.inf)
    with np.errstate(invalid="ignore"):
        d = delta(abs(np.float64(l[g]) * np.float64(inv_T)))
    best = float(k.max())
    if not np.isfinite(best):   # +-inf keys: exact
        assert k[tok] == best and tok == int(np.argmax(k)), f"{what}: token {tok} with infinite keys"
        assert key is None or f32(key) == f32(best), f"{what}: key {key} != {best}"
        return True
    assert k[tok] >= best - d, f"{what}: key64[{tok}] = {k[tok]} below max {best} - {d}"
    if key is not None:
        assert abs(float(key) - float(k[tok])) <= d, f"{what}: returned key {key} vs key64 {k[tok]} (band {d})"
    top2 = np.partition(k, -2)[-2:] if len(k) > 1 else np.array([-np.inf, best])
    decided = not (top2[1] - top2[0] <= 2 * d)
    if decided:
        assert tok == int(np.argmax(k)), f"{what}: decided row drew {tok}, reference {int(np.argmax(k))}"
    return decided


def logsoftmax64(l, tok):
    l = np.asarray(l, np.float64)
    m = l.max()
    return float(l[tok] - (m + np.log(np.exp(l - m).sum())))


# ------------------------------------------------------------------ binding
_P = C.c_void_p
GUARD = 3


class SampleCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("R", "ld", "n_valid", "src_div", "slices", "guard", "launches")] + [
        ("inv_T", C.c_float), ("cut", C.c_float), ("seed", C.c_uint64)] + [
        (n, _P) for n in ("logits", "greedy", "clip", "sample", "t", "tok", "key", "hist", "t_out", "skey_out")] + [
        ("dump_n0", C.c_uint32), ("dump_n", C.c_uint32), ("dump", _P),
        ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


def _fn():
    import qasr
    L = qasr.lib()
    L.qasr_kt_sample.argtypes = [C.c_int, C.POINTER(SampleCall)]
    L.qasr_kt_sample.restype = C.c_int
    return L


def _ok(L, rc):
    assert rc == 0, L.qasr_last_error().decode(errors="replace")


def _body(buf, R, what):
    raw = buf.view(np.uint32)
    assert (raw[:GUARD] == 0xFFFFFFFF).all() and (raw[GUARD + R:] == 0xFFFFFFFF).all(), f"{what}: guard entries overwritten"
    return buf[GUARD:GUARD + R]


def run_sample(logits, greedy, clip, sample, t, T, min_p, seed, n_valid=0, src_div=1, slices=0, launches=1):
    """logits fp32 [R / src_div][ld] -> (tok [R], key [R], tag); checks the guards, the history slot, t + 1
    and the re-armed key scratch"""
    L = _fn()
    logits = np.ascontiguousarray(logits, f32)
    RS, ld = logits.shape
    R = RS * src_div
    inv_T, cut = host_scalars(T, min_p)
    arrs = [np.ascontiguousarray(x, np.int32) for x in (greedy, clip, sample, t)]
    assert len(arrs[0]) == RS and all(len(x) == R for x in arrs[1:])
    tok, hist = np.zeros(R + 2 * GUARD, np.int32), np.zeros(R + 2 * GUARD, np.int32)
    key = np.zeros(R + 2 * GUARD, f32)
    t_out, skey = np.zeros(R, np.int32), np.ones(R, np.uint64)
    c = SampleCall(R=R, ld=ld, n_valid=n_valid or ld, src_div=src_div, slices=slices, guard=GUARD, launches=launches,
                   inv_T=float(inv_T), cut=float(cut), seed=seed)
    for n, x in (("logits", logits), ("greedy", arrs[0]), ("clip", arrs[1]), ("sample", arrs[2]), ("t", arrs[3]),
                 ("tok", tok), ("key", key), ("hist", hist), ("t_out", t_out), ("skey_out", skey)):
        setattr(c, n, x.ctypes.data_as(_P))
    _ok(L, L.qasr_kt_sample(0, C.byref(c)))
    assert not c.declined, c.msg.decode()
    out_tok, out_key = _body(tok, R, "tok").copy(), _body(key, R, "key").copy()
    assert (_body(hist, R, "hist") == out_tok).all(), "the history slot differs from the tokens"
    assert (t_out == arrs[3] + 1).all(), "t was not advanced by one"
    assert (skey == 0).all(), "the key scratch was not re-armed"
    return out_tok, out_key, c.tag.decode()


def dump_gumbel(n0, n):
    L = _fn()
    out = np.zeros(n, f32)
    c = SampleCall(dump_n0=n0, dump_n=n)
    c.dump = out.ctypes.data_as(_P)
    _ok(L, L.qasr_kt_sample(0, C.byref(c)))
    return out
