"""The phrase matcher and boost of the constraint stage (csrc/constrain.hip) through qasr_kt_phrases
against the brute-force rule (tests/phrase_util.py), bit for bit: the token, the history slot, every column of the
edited logits (columns outside the edited set E keep the input's bits, columns past n_valid too), the guard rows,
the scratch at rest, and from the flags the launch returns which rows took the scan (their raw argmax was edited)
and which the fast path.  run_phrases itself checks the guards, the history slot, the untouched history entries and
the re-armed scratch of every call."""
import numpy as np
import pytest

import constrain_util as cu
import phrase_util as pu

pytestmark = pytest.mark.gpu
f32 = np.float32
NV, LD, V_FULL = 1000, 1024, 151936
POOL = 50
TS = (0, 1, 15, 16, 40)


def make_logits(rng, R, ld, nv, scale=3.0):
    l = (rng.standard_normal((R, ld)) * scale).astype(f32)
    l[:, nv:] = np.inf                      # (a column past n_valid is neither read nor written)
    return l


def greedy_of(l, nv):
    return np.array([cu.select(r[:nv]) for r in l], np.int32)


def make_hist(rng, rows, HS, pool=POOL):
    """histories over the first `pool` tokens"""
    return rng.integers(0, pool, (rows, HS)).astype(np.int32)


def run_and_check(l, hist, t, phrases, nv=NV, src_div=1, slices=0, launches=1, **rule):
    g = greedy_of(l, nv)
    tok, edited, scanned, tag = pu.run_phrases(l, g, hist, t, phrases, n_valid=nv, src_div=src_div, slices=slices, launches=launches, **rule)
    assert tag.startswith("constrain"), tag
    hit = pu.check_rows(l, g, hist, t, tok, edited, phrases, n_valid=nv, src_div=src_div, **rule)
    assert scanned == hit, (scanned, hit)       # the scan exactly for the rows whose raw argmax was edited
    return tok, edited, hit


def stem_list(rng, hist, t, n, src_div=1, vocab=POOL, far=()):
    """n phrases over `vocab` tokens: a third random, the rest a stem of 0 .. 15 of some row's last tokens and a random
    tail, so deep nodes exist, are matched and have many children; `far`: tokens the tails never use"""
    out = []
    rows = range(0, len(hist), src_div)
    allowed = np.setdiff1d(np.arange(vocab), np.array(list(far), int))
    for k in range(n):
        ln = int(rng.integers(1, 17))
        ids = rng.choice(allowed, ln).tolist()
        if k % 3 and t:
            r = int(rng.choice(list(rows)))
            j = int(rng.integers(0, min(t, 15, ln - 1) + 1))
            ids[:j] = hist[r, t - j:t].tolist()
        out.append((ids, float(rng.integers(1, 200)) / 2))
    return out


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("src_div", [1, 3])
@pytest.mark.parametrize("R", [1, 3, 9])
def test_rows_history_lengths_and_slices(gpu, R, src_div):
    """R logits rows serving R * src_div token rows, n_valid = 1000 in ld = 1024, every history length around the
    matcher's 15 tokens, one slice and the launcher's choice; the list mixes a one-token phrase, a 16-token phrase a row
    has spelled 15 tokens of, the max-not-deepest pair on a row's last two tokens and 300 phrases with shared stems"""
    rng = np.random.default_rng(1000 + 10 * R + src_div)
    l = make_logits(rng, R, LD, NV)
    g = greedy_of(l, NV)
    hist = make_hist(rng, R * src_div, 48)
    deep_seen = 0
    for t in TS:
        ph = [([int(g[0])], 3.0), ([NV - 1], 0.5)]
        if t >= 15:
            ph.append((hist[0, t - 15:t].tolist() + [777], 40.0))
        if t >= 2:
            a, b = (int(x) for x in hist[(R - 1) * src_div, t - 2:t])
            ph += [([a, b, 555], 1.0), ([b, 555], 8.0)]
        ph += stem_list(rng, hist, t, 300, src_div)
        for slices in (1, 0):
            tok, edited, hit = run_and_check(l, hist, t, ph, src_div=src_div, slices=slices)
        assert hit[0]                                           # ([g[0]] matches at position 0 in every row's list)
        assert (tok.reshape(R, src_div) == tok.reshape(R, src_div)[:, :1]).all()
        deep = max(pu.bonuses(ph, hist[q * src_div, :t])[1] for q in range(R))
        assert deep == min(t, 15) or t < 15 and deep >= min(t, 1)
        deep_seen = max(deep_seen, deep)
        if t >= 15:
            assert bits_eq(edited[0, 777], l[0, 777] + f32(40.0)) or 777 in {int(x) for x in hist[0, :t]}
        if t >= 2:
            assert edited[R - 1, 555] == l[R - 1, 555] + f32(8.0)       # the maximum, not the deepest node's raw boost
    assert deep_seen == 15


def bits_eq(a, b):
    return np.asarray(a, f32).view(np.uint32) == np.asarray(b, f32).view(np.uint32)


# ------------------------------------------------------------ phrase lists
def test_single_phrase_lists(gpu):
    rng = np.random.default_rng(21)
    l = make_logits(rng, 3, LD, NV)
    hist = make_hist(rng, 3, 48)
    long = hist[1, 25:40].tolist() + [901]
    a, b = (int(x) for x in hist[2, 38:40])
    lists = {
        "one token": [([400], 2.5)],
        "sixteen tokens": [(long, 6.0)],
        "max not deepest": [([a, b, 902], 1.0), ([b, 902], 8.0)],
        "duplicates": [([a, b, 903], 2.0), ([a, b, 903], 7.0), ([a, b, 903], 3.0)],
        "every position of one phrase": [(hist[0, 30:40].tolist() + [904], 4.0), (hist[0, 33:40].tolist() + [905], 2.0)],
    }
    for name, ph in lists.items():
        for t in TS:
            _, edited, _ = run_and_check(l, hist, t, ph)
            if t == 40 and name == "sixteen tokens":
                assert edited[1, 901] == l[1, 901] + f32(6.0) and bits_eq(edited[0, 901], l[0, 901]) and bits_eq(edited[2, 901], l[2, 901])
                assert edited[0, long[0]] == l[0, long[0]] + f32(6.0)                   # position 0 in every row
            if t == 40 and name == "max not deepest":
                assert edited[2, 902] == l[2, 902] + f32(8.0) and bits_eq(edited[0, 902], l[0, 902])
            if t == 40 and name == "duplicates":
                assert edited[2, 903] == l[2, 903] + f32(7.0)


@pytest.mark.parametrize("t", [16, 40])
def test_4096_phrases_over_50_tokens(gpu, t):
    """the largest list: the root and deep nodes have up to 50 children each, prefixes, suffixes and copies collide"""
    rng = np.random.default_rng(22 + t)
    l = make_logits(rng, 3, LD, NV)
    hist = make_hist(rng, 3, 48)
    ph = stem_list(rng, hist, t, 4096)
    n, ids, ln, _ = pu.flat(ph)
    assert n == 4096 and ids.max() < POOL
    tok, edited, hit = run_and_check(l, hist, t, ph)
    changed = (edited[:, :NV].view(np.uint32) != l[:, :NV].view(np.uint32)).sum(axis=1)
    assert (changed == POOL).all()                              # the root alone has every token as a child
    assert max(pu.bonuses(ph, hist[q, :t])[1] for q in range(3)) == 15
    assert (tok < POOL).all()                                   # boosts up to 99.5 over logits of scale 3


def test_full_vocabulary_rows(gpu):
    """n_valid = ld = 151,936: the bitmap spans the whole vocabulary, tokens at both ends and in the last word"""
    rng = np.random.default_rng(23)
    l = make_logits(rng, 3, V_FULL, V_FULL)
    hist = rng.integers(V_FULL - 40, V_FULL - 1, (3, 48)).astype(np.int32)
    hist[:, ::3] = rng.integers(0, 40, (3, 16))
    g = greedy_of(l, V_FULL)
    ph = [(ids, b / 10) for ids, b in stem_list(rng, hist, 40, 400, vocab=V_FULL)]
    ph += [([0], 1.0), ([V_FULL - 1], 2.0), (hist[1, 25:40].tolist() + [V_FULL - 1], 50.0), (hist[2, 38:40].tolist() + [int(g[2])], 0.25)]
    tok, edited, hit = run_and_check(l, hist, 40, ph, nv=V_FULL, n=2, p=1.3, bias={77777: -np.inf, 5: 0.5})
    # (row 1 has spelled 15 tokens of the 16-token phrase: its last token and, as in every row, its first get the 50)
    assert hit[2] and tok[1] in (V_FULL - 1, int(hist[1, 25])) and edited[1, V_FULL - 1] == l[1, V_FULL - 1] + f32(50.0)
    run_and_check(l, hist, 40, ph, nv=V_FULL, slices=1)


# ------------------------------------------------------- the stage's two paths
def test_flagged_rows_take_the_scan_and_the_others_the_fast_path(gpu):
    rng = np.random.default_rng(24)
    R = 9
    l = make_logits(rng, R, LD, NV)
    for q in range(R):
        l[q, 500 + q] = f32(15.0)
    g = greedy_of(l, NV)
    assert g.tolist() == [500 + q for q in range(R)]
    hist = make_hist(rng, R, 48)
    t = 40
    even = [q for q in range(R) if q % 2 == 0]
    # per even row a phrase of its last 2 tokens whose next token is that row's raw argmax; nothing else touches a g
    ph = [(hist[q, t - 2:t].tolist() + [int(g[q])], 0.5) for q in even]
    ph += stem_list(rng, hist, t, 200, far=())
    tails = {tuple(hist[q, t - 2:t]) for q in even}
    assert len(tails) == len(even) and not any(tuple(hist[q, t - 2:t]) in tails for q in range(R) if q % 2)
    tok, edited, hit = run_and_check(l, hist, t, ph)
    assert hit == [q % 2 == 0 for q in range(R)]
    assert all(edited[q, g[q]] == l[q, g[q]] + f32(0.5) for q in even)
    # a list that never touches g: every row answers from the fast path, and a large boost still moves the token
    never = stem_list(rng, hist, t, 200)
    tok, _, hit = run_and_check(l, hist, t, never)
    assert hit == [False] * R and (tok < POOL).any()
    # small boosts: the fast path's answer is the raw argmax itself
    tok, _, hit = run_and_check(l, hist, t, [(ids, 0.001) for ids, _ in never])
    assert hit == [False] * R and (tok == g).all()
    # g boosted in every row (position 0): all rows scan
    tok, _, hit = run_and_check(l, hist, t, [([int(x)], 1.0) for x in g])
    assert hit == [True] * R and (tok == g).all()


def test_two_launches_and_every_slice_count_give_identical_bits(gpu):
    rng = np.random.default_rng(25)
    l = make_logits(rng, 5, LD, NV)
    g = greedy_of(l, NV)
    hist = make_hist(rng, 5, 48)
    ph = stem_list(rng, hist, 40, 500) + [([int(g[1])], 2.0), ([int(g[3])], 90.0)]
    rule = dict(n=2, p=1.3, bias={0: 1.0, NV - 1: -np.inf})
    base = pu.run_phrases(l, g, hist, 40, ph, n_valid=NV, **rule)
    again = pu.run_phrases(l, g, hist, 40, ph, n_valid=NV, launches=2, **rule)
    assert (base[0] == again[0]).all() and (base[1].view(np.uint32) == again[1].view(np.uint32)).all() and base[2] == again[2]
    for slices in (1, 2, 3, 64, 5000):
        tok, edited, _ = run_and_check(l, hist, 40, ph, slices=slices, **rule)
        assert (tok == base[0]).all() and (edited.view(np.uint32) == base[1].view(np.uint32)).all()


# ------------------------------------------------- combinations with §5.6
def test_penalised_biased_and_boosted_column(gpu):
    rng = np.random.default_rng(26)
    l = make_logits(rng, 3, LD, NV)
    hist = make_hist(rng, 3, 48)
    t = 40
    x = int(hist[0, 10])                       # in row 0's history: penalised there; biased and boosted everywhere
    ph = [([x], 4.0), (hist[0, t - 3:t].tolist() + [x], 9.0)]
    for w in (0, 35):
        _, edited, _ = run_and_check(l, hist, t, ph, p=1.7, w=w, bias={x: -1.25, 3: 0.5})
        pen = l[0, x] * (f32(1) / f32(1.7)) if l[0, x] > 0 else l[0, x] * f32(1.7)
        assert edited[0, x] == f32(f32(pen + f32(-1.25)) + f32(9.0))               # three rounded operations in the rule's order
    # the bitmap is cleared between the penalty and the boost: a penalised token is still boosted, and once
    run_and_check(l, hist, t, [([x], 4.0), ([x], 2.0)] + [([int(v)], 1.5) for v in hist[1, :t]], p=1.7)


def test_a_banned_boosted_column_stays_banned(gpu):
    rng = np.random.default_rng(27)
    l = make_logits(rng, 3, LD, NV)
    hist = make_hist(rng, 3, 48)
    t = 40
    # bigram ban: the token after an earlier occurrence of the last token; boost exactly that token by 100
    last = hist[:, t - 1]
    for r in range(3):
        hist[r, 5] = last[r]
        hist[r, 6] = 600 + r
        l[r, 600 + r] = f32(12.0)             # the raw argmax: boosted, banned, and the row takes the scan
    ph = [([int(last[r]), 600 + r], 100.0) for r in range(3)]
    tok, edited, hit = run_and_check(l, hist, t, ph, n=2)
    for r in range(3):
        assert edited[r, 600 + r] == -np.inf and tok[r] != 600 + r and hit[r]
    # without the ban the boost decides
    tok, _, _ = run_and_check(l, hist, t, ph)
    assert tok.tolist() == [600, 601, 602]
    # n = 1 bans every token seen, among them every boosted one but the fresh tails
    run_and_check(l, hist, t, ph + stem_list(rng, hist, t, 100), n=1)


def test_phrases_alone_and_no_phrases(gpu):
    """n_bias = 0 and the neutral values with phrases only; an empty list is qasr_kt_constrain's result"""
    rng = np.random.default_rng(28)
    l = make_logits(rng, 4, LD, NV)
    g = greedy_of(l, NV)
    hist = make_hist(rng, 4, 48)
    ph = stem_list(rng, hist, 16, 64)
    run_and_check(l, hist, 16, ph)
    run_and_check(l, hist, 0, ph)
    for rule in (dict(), dict(n=2, p=1.3, bias={int(g[0]): -2.0})):
        a = pu.run_phrases(l, g, hist, 16, [], n_valid=NV, **rule)
        b = cu.run_constrain(l, g, hist, 16, n_valid=NV, **rule)
        assert (a[0] == b[0]).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all()
        assert a[2] == cu.check_rows(l, g, hist, 16, b[0], b[1], n_valid=NV, **rule)


def test_harness_refuses_bad_lists(gpu):
    l = np.zeros((2, 8), f32)
    h = np.zeros((2, 4), np.int32)
    with pytest.raises(AssertionError, match="1..16"):
        pu.run_phrases(l, [0, 0], h, 2, [[1] * 17])
    with pytest.raises(AssertionError, match="outside the vocabulary"):
        pu.run_phrases(l, [0, 0], h, 2, [[8]])
    with pytest.raises(AssertionError, match=r"\(0, 100\]"):
        pu.run_phrases(l, [0, 0], h, 2, [([1], 0.0)])
    with pytest.raises(AssertionError, match="no_repeat_ngram"):
        pu.run_phrases(l, [0, 0], h, 2, [[1]], n=9)
