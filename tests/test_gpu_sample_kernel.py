"""The sampler kernels (csrc/sample.hip) through qasr_kt_sample against the normative rule in float64
(tests/sample_util.py): a device draw must be a candidate whose float64 key is within delta of the
largest, its returned fp32 key within delta of its float64 key, and on every decided row (the two best
float64 keys more than 2 delta apart) it must be the reference token exactly.  At most 1 % of a test's
rows may be undecided.  run_sample itself checks the guards, the history slot, t + 1 and the re-armed
key scratch of every call."""
import numpy as np
import pytest

import sample_util as su

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 0x5EEDC0DE12345678


def make_logits(rng, R, n, scale=3.0):
    return (rng.standard_normal((R, n)) * scale).astype(f32)


def greedy_of(l, nv):
    return np.array([int(np.nanargmax(r[:nv])) for r in l], np.int32)


def check(l, nv, tok, key, T, min_p, seed, clip, sample, t, src_div=1, what=""):
    """every row against the band; returns the number of undecided rows"""
    und = 0
    g = greedy_of(l, nv)
    for r in range(len(tok)):
        s = r // src_div
        und += not su.check_draw(l[s, :nv], int(tok[r]), float(key[r]), T, min_p, seed, int(clip[r]), int(sample[r]), int(t[r]),
                                 g=int(g[s]), what=f"{what} row {r}")
    assert und <= len(tok) // 100, f"{what}: {und} of {len(tok)} rows undecided"
    return und


def ids(R, base=0):
    """distinct (clip, sample, t) per row"""
    r = np.arange(R)
    return (base + r // 3).astype(np.int32), (r % 3).astype(np.int32), (r * 7 % 11).astype(np.int32)


def run_and_check(l, T, min_p, seed=SEED, nv=0, clip=None, sample=None, t=None, src_div=1, slices=0, launches=1, what=""):
    RS, ld = l.shape
    R = RS * src_div
    nv = nv or ld
    c0, s0, t0 = ids(R)
    clip, sample, t = (c0 if clip is None else clip), (s0 if sample is None else sample), (t0 if t is None else t)
    tok, key, tag = su.run_sample(l, greedy_of(l, nv), clip, sample, t, T, min_p, seed, n_valid=nv, src_div=src_div, slices=slices,
                                  launches=launches)
    assert tag.startswith("sample"), tag
    check(l, nv, tok, key, T, min_p, seed, clip, sample, t, src_div, what)
    return tok, key


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 4099])
def test_columns(gpu, n):
    rng = np.random.default_rng(100 + n)
    tok, _ = run_and_check(make_logits(rng, 8, n), 0.8, 0.0, what=f"n={n}")
    if n >= 1023:
        assert len(set(tok.tolist())) > 1   # the rows drew different tokens


def test_full_vocabulary_rows(gpu):
    """151,936 columns: the launcher's own slice counts at 3 rows and at 9 (another groups-per-thread)"""
    rng = np.random.default_rng(7)
    l = make_logits(rng, 9, 151936)
    tok9, key9 = run_and_check(l, 0.8, 0.0, what="V x 9")
    tok3, key3 = run_and_check(l[:3], 0.8, 0.0, what="V x 3")
    # a draw does not depend on the batch it rides in or on the grid
    assert np.array_equal(tok3, tok9[:3]) and np.array_equal(key3.view(np.uint32), key9[:3].view(np.uint32))
    tok1, key1 = run_and_check(l[:3], 0.8, 0.0, slices=1, what="V x 3, one slice")
    assert np.array_equal(tok1, tok3) and np.array_equal(key1.view(np.uint32), key3.view(np.uint32))


@pytest.mark.parametrize("R", [1, 3, 8, 9, 130])
def test_rows(gpu, R):
    rng = np.random.default_rng(200 + R)
    run_and_check(make_logits(rng, R, 4099), 1.3, 0.0, what=f"R={R}")


def test_n_valid_below_ld_with_inf_past_it(gpu):
    rng = np.random.default_rng(3)
    for ld, nv in ((1024, 1001), (1028, 1025), (4100, 4099), (8, 5)):
        l = make_logits(rng, 5, ld)
        l[:, nv:] = np.inf
        tok, _ = run_and_check(l, 0.8, 0.0, nv=nv, what=f"ld={ld} nv={nv}")
        assert (tok < nv).all()


def test_identity_words_each_change_the_draw(gpu):
    """counters that differ only in clip, sample, t or the seed's high word: different draws wherever the
    reference's differ (and it does differ for most of these 16 rows)"""
    rng = np.random.default_rng(4)
    row = make_logits(rng, 1, 4099)
    l = np.repeat(row, 16, axis=0)
    z = np.zeros(16, np.int32)
    var = np.arange(16, dtype=np.int32)
    base, _ = run_and_check(l, 1.0, 0.0, clip=z, sample=z, t=z, what="same identity")
    assert len(set(base.tolist())) == 1   # one identity, one draw, whatever the row
    for name, kw in (("clip", dict(clip=var, sample=z, t=z)), ("sample", dict(clip=z, sample=var, t=z)), ("t", dict(clip=z, sample=z, t=var))):
        tok, _ = run_and_check(l, 1.0, 0.0, what=name, **kw)
        want = [su.draw(row[0], 1.0, 0.0, SEED, int(kw["clip"][r]), int(kw["sample"][r]), int(kw["t"][r]))[0] for r in range(16)]
        assert len(set(want)) > 8 and tok.tolist() == want, name
    hi, _ = run_and_check(l, 1.0, 0.0, seed=SEED ^ (1 << 45), clip=z, sample=z, t=var, what="seed high word")
    lo, _ = run_and_check(l, 1.0, 0.0, seed=SEED, clip=z, sample=z, t=var, what="seed")
    assert (hi != lo).sum() > 8
    # clip, sample and t are different counter words: swapping their values changes the draw
    a, _ = run_and_check(l[:1], 1.0, 0.0, clip=[5], sample=[2], t=[9], what="(5, 2, 9)")
    b = [su.draw(row[0], 1.0, 0.0, SEED, *p)[0] for p in ((5, 2, 9), (2, 5, 9), (9, 2, 5), (5, 9, 2))]
    assert a[0] == b[0] and len(set(b)) > 1


@pytest.mark.parametrize("min_p", [0.0, 0.2, 1.0])
def test_min_p(gpu, min_p):
    rng = np.random.default_rng(5)
    l = make_logits(rng, 24, 4099, scale=1.0)
    l[3, 77] = l[3].max()          # an exact tie of the maximum, at a column after and before it
    l[4, 4098] = l[4].max()
    for T in (0.5, 2.0):
        tok, _ = run_and_check(l, T, min_p, what=f"min_p={min_p} T={T}")
        g = greedy_of(l, 4099)
        if min_p == 1.0:   # the greedy token or an exact tie of it
            assert all(l[r, tok[r]] == l[r, g[r]] for r in range(24))
            ties = {int(su.run_sample(l[3:5], g[3:5], [k, k], [0, 0], [0, 0], T, 1.0, SEED)[0][0]) for k in range(12)}
            assert len(ties) == 2
        elif min_p == 0.2:
            assert (tok != g).any()
        else:
            assert (tok != g).sum() > 12


def test_special_values(gpu):
    rng = np.random.default_rng(6)
    n = 1024
    l = make_logits(rng, 8, n)
    l[0, 5::7] = np.nan                       # NaN logits are never candidates
    l[1, :] = -np.inf                         # -inf logits: candidates with key -inf ...
    l[1, [9, 400, 1023]] = [1.0, 1.5, 0.5]    # ... that lose to any finite one
    l[2, :] = -np.inf                         # every key -inf: equal keys, the lowest column
    l[3, 511] = l[3, 512] = 30.0              # equal logits across the boundary of two slices (below: slices = 2)
    l[4, 40] = l[4, 41] = l[4, 43] = 30.0     # ... and inside one Philox group
    l[5, [100, 900]] = np.inf                 # +inf twice: equal keys at min_p = 1, the lower column
    for slices in (0, 2):
        for min_p in (0.0, 1.0):
            tok, key = run_and_check(l, 0.9, min_p, slices=slices, what=f"special slices={slices} min_p={min_p}")
            assert not np.isnan(l[0, tok[0]]) and tok[1] in (9, 400, 1023) and tok[2] == 0 and np.isneginf(key[2])
            assert tok[3] in (511, 512) and tok[4] in (40, 41, 43) and tok[5] == 100 and np.isposinf(key[5])
    # over 24 draws both sides of the boundary and every column of the group win somewhere
    rep = np.repeat(l[3:5], 24, axis=0)   # 24 x row 3, then 24 x row 4
    t = np.arange(48, dtype=np.int32)
    z = np.zeros(48, np.int32)
    tok, _ = run_and_check(rep, 0.9, 0.0, clip=z, sample=z, t=t, slices=2, what="ties")
    assert set(tok[:24].tolist()) == {511, 512} and set(tok[24:].tolist()) == {40, 41, 43}


def test_first_step_of_an_n_best_run_reads_one_row_a_clip(gpu):
    """src_div = N: rows g * N .. g * N + N - 1 draw from logits row g"""
    rng = np.random.default_rng(8)
    l = make_logits(rng, 3, 4099)
    N = 4
    r = np.arange(12)
    clip, sample, t = (r // N + 20).astype(np.int32), (r % N).astype(np.int32), np.zeros(12, np.int32)
    tok, key = run_and_check(l, 1.0, 0.0, clip=clip, sample=sample, t=t, src_div=N, what="src_div")
    wide, wkey = run_and_check(np.repeat(l, N, axis=0), 1.0, 0.0, clip=clip, sample=sample, t=t, what="repeated rows")
    assert np.array_equal(tok, wide) and np.array_equal(key.view(np.uint32), wkey.view(np.uint32))
    assert all(len(set(tok[g * N:(g + 1) * N].tolist())) > 1 for g in range(3))


def test_two_launches_are_bit_identical(gpu):
    rng = np.random.default_rng(9)
    l = make_logits(rng, 9, 4099)
    one = run_and_check(l, 0.8, 0.0, what="one launch")
    two = run_and_check(l, 0.8, 0.0, launches=2, what="two launches")   # (the key scratch re-armed in between)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1].view(np.uint32), two[1].view(np.uint32))


def test_gumbel_all_u(gpu, parity):
    """G(u) over all 2^23 values of u against float64: the worst error is the band's first term
    (sample_util.G_DEV_ERR) and stays inside what two 1-ulp logf allow"""
    n = 1 << 23
    dev = su.dump_gumbel(0, n).astype(np.float64)
    ref = su.gumbel64((2.0 * np.arange(n, dtype=np.float64) + 1) * 2.0 ** -24)
    err = np.abs(dev - ref)
    worst = float(err.max())
    at = int(err.argmax())
    print(f"worst |G_dev - G64| = {worst:.6g} at n = {at} (G = {ref[at]:.6f}); mean {err.mean():.3g}; G_DEV_ERR = {su.G_DEV_ERR:.6g}")
    parity("sample_gumbel", worst_abs=worst, at_n=at, mean_abs=float(err.mean()), bound=su.G_DEV_ERR)
    assert np.isfinite(dev).all() and worst <= su.G_DEV_ERR
    part = su.dump_gumbel(12345, 1000)   # a range in the middle: the same values
    assert np.array_equal(part.view(np.uint32), dev[12345:13345].astype(f32).view(np.uint32))
