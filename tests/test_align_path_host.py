"""qasr_align_path_host (csrc/align_path_host.h), the monotone path's rule in plain C++, against the
rule's NumPy float32 restatement (tests/align_path_util.py) and a float64 brute-force dynamic programme.  No device.
(NT = 0, an all-equal input and the refused ranges: tools/align_path_host_check.cpp.)"""
import numpy as np
import pytest

import align_path_util as au
import qasr

f32, f64 = np.float32, np.float64
EPS32 = 2.0 ** -23
SHAPES = [(1, 1), (1, 7), (2, 1), (2, 5), (9, 3), (12, 40), (33, 17)]   # (NT, C)


def _logits(kind, NT, ld, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":   # multiples of 0.25 in [-4, 4]: every fp32 (and fp64) add of the programme is exact
        return (rng.integers(-16, 17, (NT, ld)) * 0.25).astype(f32)
    return (rng.standard_normal((NT, ld)) * 3.0).astype(f32)


def _brute64(z, Cn):
    """float64, every maximum scanned from scratch; equal values to the smaller class -> (path, score, max |dp|)"""
    z = np.asarray(z, f64)
    NT = z.shape[0]
    dp = np.zeros((NT, Cn), f64)
    bp = np.zeros((NT, Cn), int)
    dp[0] = z[0, :Cn]
    for i in range(1, NT):
        for c in range(Cn):
            bp[i, c] = int(np.argmax(dp[i - 1, :c + 1]))
            dp[i, c] = z[i, c] + dp[i - 1, bp[i, c]]
    path = [int(np.argmax(dp[-1]))]
    for i in range(NT - 1, 0, -1):
        path.append(int(bp[i, path[-1]]))
    return np.array(path[::-1]), dp[-1].max(), np.abs(dp).max()


@pytest.mark.parametrize("kind", ["ties", "gauss"])
@pytest.mark.parametrize("NT,Cn", SHAPES)
def test_host_equals_the_rule_and_the_float64_optimum(kind, NT, Cn):
    """Path and score equal the NumPy float32 rule bit for bit.  On the tie-heavy logits every add is exact, so the
    float64 optimum, its path included, is reproduced exactly.  On Gaussian logits: the fp32 programme rounds once a
    row and rounding and max are monotone, so for ANY path P the fp32 value the programme holds at P's end is at
    least fl(sum along P) >= S64(P) - (NT - 1) u max|dp|, and the value of the chosen path Pf is the fp32 sum along
    Pf <= S64(Pf) + (NT - 1) u max|dp|; the chosen value is the largest, hence S64(P*) - S64(Pf) <=
    2 (NT - 1) u max|dp| <= 2 NT eps32 max|dp|."""
    ld = Cn + 3   # columns past C: in the log-sum-exp, never on the path
    z = _logits(kind, NT, ld, 100 * NT + Cn)
    cls, lp, score = qasr.align_path_host(z, Cn)
    want, wscore = au.rule(z, Cn)
    assert cls.tolist() == want.tolist()
    assert f32(score).view(np.uint32) == wscore.view(np.uint32)
    assert (np.diff(cls) >= 0).all() and cls.max() < Cn
    bpath, bscore, dpmax = _brute64(z, Cn)
    mine = float(np.asarray(z, f64)[np.arange(NT), cls].sum())
    if kind == "ties":
        assert cls.tolist() == bpath.tolist() and f64(score) == bscore == mine
    else:
        assert 0.0 <= bscore - mine <= 2 * NT * EPS32 * dpmax, (bscore - mine, 2 * NT * EPS32 * dpmax)
    # the log-probabilities: the chosen logit minus the row's log-sum-exp over all ld columns; the host sums ld <= 43
    # terms in order, each exp and the log within 1 ulp: (ld + 4) eps32 relative to a sum >= 1, plus the roundings of
    # the two results of magnitude |lse|, |logprob|
    ref = np.asarray(z, f64)[np.arange(NT), cls] - au.lse64(z, ld)
    tol = EPS32 * (ld + 4 + 2 * np.abs(au.lse64(z, ld)) + np.abs(ref))
    assert (np.abs(lp - ref) <= tol).all(), (np.abs(lp - ref).max(), tol.min())

