"""CPU: hand-made known answers of the decoding-constraint rule's numpy restatement (tests/constrain_util.py,
DESIGN.md §5.6) and qasr_constraints_validate on every range edge.  No device calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import constrain_util as cu
import qasr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NINF = f32(-np.inf)
QASR_ERR_ARG = 1
NAMES = ("qasr_constraints_validate", "qasr_set_constraints", "qasr_get_constraints", "qasr_kt_constrain")


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ------------------------------------------------------------------ the ban
@pytest.mark.parametrize("n, cases", [
    # h = 5 7 5 7 ...: (t, banned columns) at t = n - 2, n - 1, n
    (1, [(0, set()), (1, {5})]),
    (2, [(0, set()), (1, set()), (2, set()), (3, {7}), (4, {5})]),
    (3, [(1, set()), (2, set()), (3, set()), (4, {5}), (5, {7})]),
])
def test_ban_known_answers(n, cases):
    h = [5, 7, 5, 7, 5, 7]
    for t, want in cases:
        assert cu.banned(h[:t], n) == want, (n, t)
    l = np.arange(8, dtype=f32)
    for t, want in cases:
        out, tok, E = cu.apply(l, h[:t], n=n)
        assert E == want and all(out[v] == NINF for v in want)
        assert tok == (7 if 7 not in want else 6)
        keep = [j for j in range(8) if j not in want]
        assert (bits(out[keep]) == bits(l[keep])).all()


def test_ban_n1_bans_every_token_seen_and_nothing_before_a_history():
    assert cu.banned([], 1) == set() and cu.banned([3, 3, 4], 1) == {3, 4}
    assert cu.banned([1], 3) == set() and cu.banned([], 2) == set()   # t < n - 1
    # t = n - 1: the suffix is the whole history and only position 0 can match it -- which it does: the token
    # after it would be h[n - 1], not yet there, so i ranges over 0 .. t - n = -1: nothing
    assert cu.banned([1, 2], 3) == set()
    # the trigram 1 2 3 was seen: after ... 1 2 the token 3 is banned, 9 is not
    assert cu.banned([1, 2, 3, 9, 1, 2], 3) == {3}
    assert cu.banned([1, 2, 3, 1, 2, 4, 1, 2], 3) == {3, 4}
    assert cu.banned([4, 4, 4], 2) == {4} and cu.banned([4, 4, 4], 3) == {4}


def test_ngram_helper():
    assert cu.repeats_ngram([1, 2, 3, 1, 2], 2) and not cu.repeats_ngram([1, 2, 3, 2, 1], 2)
    assert cu.repeats_ngram([7, 7], 1) and not cu.repeats_ngram([7, 7], 2) and cu.repeats_ngram([7, 7, 7], 2)


# ------------------------------------------------------------------ the penalty
def test_penalty_once_per_distinct_token_and_its_sign_rule():
    l = np.array([2.0, -2.0, 0.0, -0.0, 3.0, 1.5], f32)
    p = 1.3
    inv_p = f32(1) / f32(p)
    out, tok, E = cu.apply(l, [0, 0, 1, 0, 1, 2, 3], p=p)
    assert E == {0, 1, 2, 3}
    assert out[0] == f32(2.0) * inv_p and out[0] != f32(2.0) * inv_p * inv_p       # three occurrences, one penalty
    assert out[1] == f32(-2.0) * f32(p)                                             # negative: times p
    assert bits(out[2]) == bits(f32(0.0)) and bits(out[3]) == bits(f32(-0.0))       # zeros are not > 0: times p, signs kept
    assert (bits(out[4:]) == bits(l[4:])).all() and tok == 4
    # one rounded multiply by the rounded reciprocal, not a division
    assert inv_p == f32(0.7692308) and out[0] == f32(2.0) * f32(0.7692308)
    # p < 1 rewards: a seen positive token grows
    out, tok, _ = cu.apply(l, [5], p=0.5)
    assert out[5] == f32(3.0) and tok == 4     # equal values: the lower id


@pytest.mark.parametrize("w, want", [(1, {4}), (3, {2, 3, 4}), (4, {1, 2, 3, 4}), (5, {1, 2, 3, 4}), (0, {1, 2, 3, 4})])
def test_penalty_window_edges(w, want):
    # t = 4: w = 1, t - 1, t, t + 1 and 0 (the whole history)
    l = np.full(6, 1.0, f32)
    out, tok, E = cu.apply(l, [1, 2, 3, 4], p=2.0, w=w)
    assert E == want
    assert all(out[v] == f32(0.5) for v in want) and all(out[v] == f32(1.0) for v in range(6) if v not in want)
    assert tok == min(set(range(6)) - want)


# ------------------------------------------------------------------ the bias
def test_ban_beats_a_positive_bias_and_order_of_the_steps():
    l = np.array([1.0, 5.0, 2.0, 0.5], f32)
    out, tok, E = cu.apply(l, [1, 3], n=1, bias={1: 100.0, 2: 0.25})
    assert out[1] == NINF and out[3] == NINF and out[2] == f32(2.25) and tok == 2 and E == {1, 2, 3}
    # penalty first, then the bias: (5 / 2) + 1, not (5 + 1) / 2
    out, tok, _ = cu.apply(l, [1], p=2.0, bias={1: 1.0})
    assert out[1] == f32(3.5) and tok == 1
    # -inf suppresses; a bias that makes two columns equal: the lower id wins
    out, tok, _ = cu.apply(l, [], bias={1: -np.inf})
    assert out[1] == NINF and tok == 2
    out, tok, _ = cu.apply(l, [], bias={2: 3.0})
    assert out[2] == out[1] and tok == 1
    out, tok, _ = cu.apply(l, [], bias={0: 4.0})
    assert out[0] == out[1] and tok == 0
    # every column banned: the lowest id
    assert cu.apply(l, [0, 1, 2, 3], n=1)[1] == 0


def test_negative_zero_bias_leaves_every_bit():
    l = np.array([0.0, -0.0, 1.5, -2.25, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38], f32)
    out, tok, E = cu.apply(l, [], bias={j: -0.0 for j in range(len(l))})
    assert (bits(out) == bits(l)).all() and E == set(range(len(l))) and tok == 4
    # (+0.0 would not: -0.0 + 0.0 = +0.0)
    assert bits(cu.apply(l, [], bias={1: 0.0})[0])[1] != bits(l)[1]


def test_selection_key_order():
    l = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, 1.0, np.inf], f32)
    k = cu.argmax_key(l, np.arange(7))
    assert (np.diff(k[[0, 1, 2, 3, 5, 4, 6]].astype(object)) > 0).all()     # (-0.0 below +0.0; equal values: lower id above)
    assert cu.select(l) == 6 and cu.select(l[:6]) == 4 and cu.select([NINF, NINF]) == 0
    assert int(cu.argmax_key(f32(1.0), 3)) == (0xBF800000 << 32) | (0xFFFFFFFF - 3)


# ------------------------------------------------------------------ the C ABI
def raw(n=0, p=1.0, w=0, ids=(), bias=()):
    ids, bias = np.array(ids, np.int32), np.array(bias, f32)
    k = qasr.Constraints(n, p, w, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)) if len(ids) else None,
                         bias.ctypes.data_as(C.POINTER(C.c_float)) if len(bias) else None)
    return k, (ids, bias)


def validate(vocab=100, **kw):
    k, _keep = raw(**kw)
    rc = qasr.lib().qasr_constraints_validate(C.byref(k), vocab)
    return rc, qasr.lib().qasr_last_error().decode()


def test_validate_every_range_edge(built):
    ok = lambda **kw: validate(**kw)[0] == 0
    def bad(word, **kw):
        rc, msg = validate(**kw)
        return rc == QASR_ERR_ARG and word in msg
    assert ok() and ok(n=0) and ok(n=8) and bad("no_repeat_ngram", n=-1) and bad("no_repeat_ngram", n=9)
    assert ok(p=10.0) and ok(p=1e-6) and bad("repetition_penalty", p=0.0) and bad("repetition_penalty", p=-1.0)
    assert bad("repetition_penalty", p=10.000001) and bad("repetition_penalty", p=float("nan")) and bad("repetition_penalty", p=float("inf"))
    assert ok(w=0) and ok(w=2 ** 31 - 1) and bad("penalty_last_n", w=-1)
    full = list(range(100))
    assert ok(ids=[0], bias=[1.0]) and ok(ids=[99], bias=[-np.inf]) and ok(ids=full, bias=[0.5] * 100)
    assert ok(vocab=2048, ids=list(range(1024)), bias=[0.0] * 1024)
    assert bad("outside the vocabulary", ids=[100], bias=[0.0]) and bad("outside the vocabulary", ids=[-1], bias=[0.0])
    assert ok(vocab=0, ids=[10 ** 6], bias=[0.0])            # vocab <= 0: no upper bound
    assert bad("listed twice", ids=[3, 4, 3], bias=[0.0] * 3)
    assert bad("finite or -inf", ids=[3], bias=[np.inf]) and bad("finite or -inf", ids=[3], bias=[np.nan])
    # n_bias outside 0 .. 1024, and a count without arrays
    k, _keep = raw(ids=list(range(1024)), bias=[0.0] * 1024)
    k.n_bias = 1025
    assert qasr.lib().qasr_constraints_validate(C.byref(k), 0) == QASR_ERR_ARG and "n_bias" in qasr.lib().qasr_last_error().decode()
    k.n_bias = -1
    assert qasr.lib().qasr_constraints_validate(C.byref(k), 0) == QASR_ERR_ARG
    k = qasr.Constraints(0, 1.0, 0, 1, None, None)
    assert qasr.lib().qasr_constraints_validate(C.byref(k), 0) == QASR_ERR_ARG
    assert qasr.lib().qasr_constraints_validate(None, 0) == QASR_ERR_ARG
    # the Python helper raises with the message
    qasr.constraints_validate(100, no_repeat_ngram=3, repetition_penalty=1.2, bias={5: 1.0}, suppress=[7])
    with pytest.raises(qasr.QasrError, match="no_repeat_ngram"):
        qasr.constraints_validate(100, no_repeat_ngram=9)
    k, keep = qasr.make_constraints(bias={5: 1.0, 7: 2.0}, suppress=[7, 9])
    assert k.n_bias == 3 and list(keep[0]) == [5, 7, 9] and list(keep[1]) == [1.0, NINF, NINF]


def test_capi_declares_and_exports_constraints(built):
    hdr = open(os.path.join(ROOT, "include", "qasr_capi.h")).read()
    decl = set(re.findall(r"\b(qasr_[a-z0-9_]+)\s*\(", hdr))
    lib = qasr.lib()
    for n in NAMES:
        assert n in decl and hasattr(lib, n), n
    assert set(NAMES[:3]) <= set(qasr.EXPORTS) and NAMES[3] not in qasr.EXPORTS
    assert "#define QASR_NGRAM_MAX 8" in hdr and "#define QASR_BIAS_MAX 1024" in hdr
    assert (qasr.QASR_NGRAM_MAX, qasr.QASR_BIAS_MAX) == (8, 1024) == (cu.NGRAM_MAX, cu.BIAS_MAX)
    assert C.sizeof(qasr.Constraints) == 32
    lib.qasr_kt_constrain.argtypes = [C.c_int, C.c_void_p]
    lib.qasr_kt_constrain.restype = C.c_int
    assert lib.qasr_kt_constrain(0, None) == QASR_ERR_ARG
    assert lib.qasr_set_constraints(None, None) == QASR_ERR_ARG
    assert lib.qasr_get_constraints(None, None, None, None, 0) == QASR_ERR_ARG
