"""The constraint kernels (csrc/constrain.hip) through qasr_kt_constrain against the normative rule
(tests/constrain_util.py), bit for bit: the token, the history slot, every column of the edited logits (columns
outside the edited set E keep the input's bits), the guard rows and the scratch at rest.  run_constrain itself
checks the guards, the history slot, the untouched history entries and the re-armed scratch of every call."""
import numpy as np
import pytest

import constrain_util as cu

pytestmark = pytest.mark.gpu
f32 = np.float32
V_FULL = 151936


def make_logits(rng, R, n, scale=3.0):
    return (rng.standard_normal((R, n)) * scale).astype(f32)


def greedy_of(l, nv):
    return np.array([cu.select(r[:nv]) for r in l], np.int32)


def make_hist(rng, R, HS, nv, g, pool=6, with_g=None):
    """histories [R][HS] over a small pool of tokens a row (so n-grams repeat); with_g given: row r holds its greedy
    token, as its first entry at least, where with_g[r], and nowhere otherwise (so under n = 1 or a penalty over the
    whole history g is in E exactly on those rows, once t >= 1)"""
    h = np.zeros((R, HS), np.int32)
    for r in range(R):
        ids = rng.choice(nv, size=min(pool, nv), replace=False)
        if with_g is not None:
            ids = ids[ids != g[r]]
            if with_g[r] or len(ids) == 0:
                ids = np.append(ids, g[r])
        h[r] = rng.choice(ids, size=HS)
        if with_g is not None and with_g[r]:
            h[r, 0] = g[r]
    return h


def run_and_check(l, hist, t, nv=0, src_div=1, slices=0, launches=1, **rule):
    RS, ld = l.shape
    nv = nv or ld
    g = greedy_of(l, nv)
    tok, edited, tag = cu.run_constrain(l, g, hist, t, n_valid=nv, src_div=src_div, slices=slices, launches=launches, **rule)
    assert tag.startswith("constrain"), tag
    hit = cu.check_rows(l, g, hist, t, tok, edited, n_valid=nv, src_div=src_div, **rule)
    return tok, edited, hit


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 4099])
def test_columns(gpu, n):
    rng = np.random.default_rng(100 + n)
    l = make_logits(rng, 8, n)
    g = greedy_of(l, n)
    with_g = np.arange(8) % 2 == 0
    h = make_hist(rng, 8, 40, n, g, with_g=with_g)
    ends = {0: 0.75, n - 1: -1.5}
    for rule in (dict(n=1), dict(n=2), dict(p=1.3), dict(p=1.3, w=4, n=3, bias=ends), dict(bias=ends)):
        _, _, hit = run_and_check(l, h, 33, **rule)
        if n >= 1023 and rule in (dict(n=1), dict(p=1.3)):
            assert hit == list(with_g)      # both paths of the stage in one launch


def test_full_rows(gpu):
    rng = np.random.default_rng(7)
    l = make_logits(rng, 3, V_FULL)
    g = greedy_of(l, V_FULL)
    h = make_hist(rng, 3, 64, V_FULL, g, with_g=[True, False, True])
    h[:, 40:48] = V_FULL - 1
    bias = {0: 0.5, V_FULL - 1: 2.0, 77777: -np.inf}
    assert not set(bias) & {int(x) for x in g}
    for rule in (dict(n=2, p=1.3, bias=bias), dict(n=1), dict(p=0.8, w=7)):
        _, _, hit = run_and_check(l, h, 63, **rule)
        assert hit == [True, False, True] or "w" in rule


@pytest.mark.parametrize("R", [1, 3, 8, 9, 130])
def test_rows(gpu, R):
    rng = np.random.default_rng(200 + R)
    l = make_logits(rng, R, 2052)
    g = greedy_of(l, 2052)
    with_g = rng.random(R) < 0.5
    h = make_hist(rng, R, 24, 2052, g, with_g=with_g)
    free = next(i for i in range(2052) if i not in {int(x) for x in g})
    _, _, hit = run_and_check(l, h, 20, n=2, p=1.2, bias={free: 0.25})
    assert hit == list(with_g)


@pytest.mark.parametrize("t", [0, 1, 255, 256, 257, 299])
def test_history_lengths(gpu, t):
    HS = 300
    rng = np.random.default_rng(300 + t)
    l = make_logits(rng, 4, 517)
    g = greedy_of(l, 517)
    h = make_hist(rng, 4, HS, 517, g, pool=4, with_g=[True, False, False, True])
    for rule in (dict(n=1), dict(n=3, p=1.5), dict(p=1.5, w=256), dict(p=1.5, w=1), dict(n=8)):
        run_and_check(l, h, t, **rule)


@pytest.mark.parametrize("n", range(1, 9))
def test_every_ngram_length(gpu, n):
    rng = np.random.default_rng(400 + n)
    l = make_logits(rng, 6, 260)
    g = greedy_of(l, 260)
    # two tokens a row: every short n-gram has occurred; row 5 one token, its greedy one (always banned once t >= n)
    h = make_hist(rng, 6, 64, 260, g, pool=2)
    h[5] = g[5]
    for t in (n - 2, n - 1, n, n + 1, 40):
        if t < 0:
            continue
        _, edited, hit = run_and_check(l, h, t, n=n)
        assert hit[5] == (t >= n)
        if t == 40 and n <= 3:
            assert all(np.isinf(edited[r]).any() for r in range(5))     # the pool is small enough to repeat


@pytest.mark.parametrize("nb", [0, 1, 1024])
def test_bias_counts(gpu, nb):
    rng = np.random.default_rng(500 + nb)
    nv = 3000
    l = make_logits(rng, 5, nv)
    g = greedy_of(l, nv)
    h = make_hist(rng, 5, 16, nv, g, with_g=[False] * 5)
    ids = [0, nv - 1][:nb] if nb <= 2 else [0, nv - 1] + [int(x) for x in rng.choice(np.arange(1, nv - 1), nb - 2, replace=False)]
    bias = {i: float(f32(rng.standard_normal() * 2)) for i in ids}
    if nb == 1024:
        bias[ids[5]] = -np.inf
        bias[ids[6]] = -0.0
    _, _, hit = run_and_check(l, h, 10, bias=bias, n=2)
    assert hit == [int(x) in bias for x in g]


def test_bias_overtakes_and_ties(gpu):
    rng = np.random.default_rng(11)
    l = make_logits(rng, 4, 1500, scale=1.0)
    h = np.zeros((4, 8), np.int32)
    # row 0: column 9 lifted over the maximum; rows 1, 2: made equal to it from either side (the lower id wins);
    # row 3: the maximum itself pushed below the second best
    for r in range(4):
        l[r, 9] = l[r, 1400] = f32(-20.0)
        l[r, 100 + r] = f32(12.0)
    l[3, 700] = f32(11.0)
    g = greedy_of(l, 1500)
    assert list(g) == [100, 101, 102, 103]
    for r, bias, want in ((0, {9: 33.0}, 9), (1, {9: 32.0}, 9), (2, {1400: 32.0}, int(g[2])), (3, {int(g[3]): -2.0}, 700)):
        tok, edited, hit = run_and_check(l[r:r + 1], h[r:r + 1], 0, bias=bias)
        assert tok[0] == want and hit == [r == 3]
    assert f32(-20.0) + f32(32.0) == f32(12.0)


def test_three_columns_two_banned(gpu):
    l = np.array([[1.0, 3.0, 2.0], [3.0, 1.0, 2.0], [0.5, 0.25, 0.125]], f32)
    h = np.array([[1, 2, 1, 2, 0], [0, 2, 2, 0, 0], [0, 1, 0, 1, 0]], np.int32)      # (t = 4: the last column is the slot)
    tok, edited, _ = run_and_check(l, h, 4, n=1)
    assert list(tok) == [0, 1, 2] and np.isinf(edited).sum() == 6
    # everything banned: the lowest id
    h = np.array([[0, 1, 2, 0, 0]] * 3, np.int32)
    tok, _, _ = run_and_check(l, h, 4, n=1)
    assert list(tok) == [0, 0, 0]


@pytest.mark.parametrize("nv, ld", [(1000, 1024), (1001, 1003), (5, 8)])
def test_columns_past_n_valid_are_left_alone(gpu, nv, ld):
    rng = np.random.default_rng(600 + ld)
    l = make_logits(rng, 4, ld)
    l[:, nv:] = np.inf
    g = greedy_of(l, nv)
    h = make_hist(rng, 4, 16, nv, g, with_g=[True, True, False, False])
    tok, edited, _ = run_and_check(l, h, 12, nv=nv, n=1, p=1.4, bias={nv - 1: 1.0})
    assert (tok < nv).all() and np.isposinf(edited[:, nv:]).all()


def test_src_div(gpu):
    rng = np.random.default_rng(12)
    l = make_logits(rng, 3, 1030)
    g = greedy_of(l, 1030)
    h = make_hist(rng, 9, 16, 1030, np.repeat(g, 3), with_g=[True] * 3 + [False] * 6)
    assert 3 not in g
    tok, _, hit = run_and_check(l, h, 9, src_div=3, n=1, bias={3: 0.5})
    assert hit == [True, False, False] and (tok.reshape(3, 3) == tok.reshape(3, 3)[:, :1]).all()
    run_and_check(l, h, 0, src_div=3, bias={int(g[1]): -np.inf})       # (the engine's case: an empty history)


def test_launches_and_slices_agree(gpu):
    rng = np.random.default_rng(13)
    l = make_logits(rng, 5, 4099)
    g = greedy_of(l, 4099)
    h = make_hist(rng, 5, 32, 4099, g, with_g=[True, True, True, False, True])
    rule = dict(n=2, p=1.3, bias={0: 1.0, 4098: -np.inf})
    base = cu.run_constrain(l, g, h, 30, **rule)
    again = cu.run_constrain(l, g, h, 30, launches=3, **rule)
    assert (base[0] == again[0]).all() and (base[1].view(np.uint32) == again[1].view(np.uint32)).all()
    for slices in (1, 2, 3, 5, 64, 1025, 5000):
        tok, edited, _ = run_and_check(l, h, 30, slices=slices, **rule)
        assert (tok == base[0]).all() and (edited.view(np.uint32) == base[1].view(np.uint32)).all()


def test_harness_refuses_bad_shapes(gpu):
    l = np.zeros((2, 8), f32)
    h = np.zeros((2, 4), np.int32)
    with pytest.raises(AssertionError, match="no_repeat_ngram"):
        cu.run_constrain(l, [0, 0], h, 2, n=9)
    with pytest.raises(AssertionError, match="bad arguments"):
        cu.run_constrain(l, [0, 0], h, 4)             # t must leave room for the slot
    with pytest.raises(AssertionError, match="history id"):
        cu.run_constrain(l, [0, 0], h + 8, 2)
