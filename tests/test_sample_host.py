"""CPU: the sampling rule's numpy restatement (tests/sample_util.py) -- the Philox known answers, the u
mapping, the distribution the rule draws from, and the C-ABI's surface.  No device calls."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import qasr
import sample_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
QASR_ERR_ARG = 1
NAMES = ("qasr_set_sampling", "qasr_get_sampling", "qasr_set_sample_streams", "qasr_get_samples", "qasr_kt_sample")


def words(counter, key):
    return " ".join("%08x" % int(np.asarray(v).reshape(-1)[0]) for v in su.philox4x32_10(counter, key))


def test_philox_known_answers():
    assert words((0, 0, 0, 0), (0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_is_vectorised_over_counters():
    grp = np.arange(5, dtype=np.uint64)
    many = su.philox4x32_10((grp, 7, 3, 1), (11, 12))
    for g in range(5):
        one = su.philox4x32_10((g, 7, 3, 1), (11, 12))
        assert [int(x[g]) for x in many] == [int(np.asarray(x).reshape(-1)[0]) for x in one]
    w = su.draw_bits((12 << 32) | 11, 3, 1, 7, 18)
    assert len(w) == 18 and int(w[17]) == int(many[1][4]) and int(w[4]) == int(many[0][1])


def test_u_end_points_are_exact_and_open():
    u = su.u_of(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], np.uint32))
    assert u[0] == 2.0 ** -24 and u[1] == u[0] and u[2] == 3 * 2.0 ** -24 and u[3] == 1 - 2.0 ** -24
    assert (u.astype(f32).astype(np.float64) == u).all() and 0 < u.min() and u.max() < 1
    # every u is (2 n + 1) 2^-24, n < 2^23: a 24-bit odd integer times a power of two
    n = np.array([0, 1, 12345, 2 ** 23 - 1], np.uint32)
    assert (su.u_of(n << np.uint32(9)) == (2.0 * n + 1) * 2.0 ** -24).all()
    assert np.isfinite(su.gumbel64(u)).all()


def draw_many(l, T, min_p, seed, clips, ts):
    """the rule's token for every (clip, t) pair of one 16-column row, sample 0; vectorised"""
    l = np.asarray(l, f32)
    n = len(l)
    assert n % 4 == 0
    inv_T, cut = su.host_scalars(T, min_p)
    grp = np.arange(n // 4, dtype=np.uint64)[:, None]
    w = su.philox4x32_10((grp, np.asarray(ts, np.uint64)[None, :], np.asarray(clips, np.uint64)[None, :], 0),
                         (seed & su.MASK, seed >> 32))
    w = np.stack(w, axis=1).reshape(n, -1)   # [column][draw]
    keys = l.astype(np.float64)[:, None] * np.float64(inv_T) + su.gumbel64(su.u_of(w))
    keys[~su.candidates(l, int(np.argmax(l)), cut)] = -np.inf
    return np.argmax(keys, axis=0)


def chi2_sf(x, k):
    """P(chi^2_k > x) for odd k: Q(k / 2, x / 2) by Q(a + 1, y) = Q(a, y) + y^a e^-y / Gamma(a + 1), Q(1/2, y) = erfc(sqrt y)"""
    assert k % 2 == 1
    y, a = x / 2.0, 0.5
    q = math.erfc(math.sqrt(y))
    while a < k / 2.0:
        q += math.exp(a * math.log(y) - y - math.lgamma(a + 1))
        a += 1.0
    return q


def chi2_critical(p, k):
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_sf(mid, k) > p else (lo, mid)
    return hi


def test_chi2_helper():
    assert abs(chi2_sf(24.996, 15) - 0.05) < 1e-4      # the textbook 5 % point of 15 degrees of freedom
    assert abs(chi2_critical(0.05, 15) - 24.996) < 1e-2


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_rule_draws_from_softmax_of_l_over_T(T):
    rng = np.random.default_rng(5)
    l = (rng.standard_normal(16) * 0.5).astype(f32)   # (every cell's expected count stays above 5 at T = 0.5 too)
    N = 20000
    clips, ts = np.arange(N) % 200, np.arange(N) // 200
    tok = draw_many(l, T, 0.0, 0xC0FFEE123456789, clips, ts)
    p = np.exp(l.astype(np.float64) * np.float64(su.host_scalars(T, 0)[0]))
    p /= p.sum()
    obs = np.bincount(tok, minlength=16)
    assert (N * p).min() >= 5            # every cell large enough for the chi-square approximation
    stat = float(((obs - N * p) ** 2 / (N * p)).sum())
    crit = chi2_critical(1e-6, 15)       # 16 cells, 15 degrees of freedom
    print(f"T={T} chi2={stat:.2f} critical(1e-6)={crit:.2f}")
    assert 50 < crit < 65 and stat < crit
    # the scalar path gives the same tokens
    for i in (0, 1, 199, 200, 19999):
        assert su.draw(l, T, 0.0, 0xC0FFEE123456789, int(clips[i]), 0, int(ts[i]))[0] == tok[i]


def test_min_p_yields_only_candidates_and_small_T_the_argmax():
    rng = np.random.default_rng(6)
    l = (rng.standard_normal(16) * 1.5).astype(f32)
    g = int(np.argmax(l))
    N = 20000
    clips, ts = np.arange(N) % 200, np.arange(N) // 200
    for T in (0.5, 1.0, 2.0):
        tok = draw_many(l, T, 0.2, 77, clips, ts)
        # probability at least 0.2 x the greedy token's under softmax(l / T)
        ok = np.flatnonzero(su.candidates(l, g, su.host_scalars(T, 0.2)[1]))
        p = np.exp((l.astype(np.float64) - l[g]) / T)
        assert set(ok) == set(np.flatnonzero(p >= 0.2 * (1 - 1e-6))) or set(ok) == set(np.flatnonzero(p >= 0.2 * (1 + 1e-6)))
        assert set(np.unique(tok)) <= set(ok) and len(ok) < 16 and len(np.unique(tok)) > 1
    assert (draw_many(l, 1.0, 1.0, 77, clips, ts) == g).all()      # min_p = 1: the greedy token (no exact tie here)
    assert (draw_many(l, 1e-4, 0.0, 77, clips, ts) == g).all()     # T -> 0: the argmax
    # a NaN logit is never drawn; an exact tie of the maximum is a candidate at min_p = 1
    l2 = l.copy()
    l2[(g + 1) % 16] = np.nan
    l2[(g + 2) % 16] = l[g]
    c = su.candidates(l2, g, su.host_scalars(1.0, 1.0)[1])
    assert c.sum() == 2 and c[g] and c[(g + 2) % 16]
    toks = {su.draw(l2, 1.0, 0.0, 5, k, 0, 0, g=g)[0] for k in range(200)}
    assert (g + 1) % 16 not in toks and len(toks) > 2


def test_band_is_derived_not_tuned():
    # twice (worst G error + one fp32 ulp at max(|l[g] / T|, 17))
    assert su.delta(0.0) == 2 * (su.G_DEV_ERR + 2.0 ** -19) and su.delta(40.0) == 2 * (su.G_DEV_ERR + 2.0 ** -18)
    assert su.G_DEV_ERR <= 2.0 ** -19 + 2.0 ** -23   # never above what two 1-ulp logf allow


def test_capi_declares_and_exports_sampling(built):
    hdr = open(os.path.join(ROOT, "include", "qasr_capi.h")).read()
    decl = set(re.findall(r"\b(qasr_[a-z0-9_]+)\s*\(", hdr))
    lib = qasr.lib()
    for n in NAMES:
        assert n in decl and hasattr(lib, n), n
    assert set(NAMES[:4]) <= set(qasr.EXPORTS) and NAMES[4] not in qasr.EXPORTS
    assert "#define QASR_SAMPLE_MAX 8" in hdr and qasr.QASR_SAMPLE_MAX == 8
    assert C.sizeof(qasr.Sampling) == 24
    lib.qasr_kt_sample.argtypes = [C.c_int, C.c_void_p]
    lib.qasr_kt_sample.restype = C.c_int
    assert lib.qasr_kt_sample(0, None) == QASR_ERR_ARG
    assert lib.qasr_set_sampling(None, None) == QASR_ERR_ARG
