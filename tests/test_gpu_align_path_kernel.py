"""The monotone-path kernels (csrc/align_path.hip) through qasr_kt_align_path against the rule's
NumPy float32 restatement (tests/align_path_util.py): path and score bit for bit at every class count at which the
wave scan, the cross-wave step, the template and the blocked walk back change, the log-sum-exp against float64."""
import math

import numpy as np
import pytest

import align_path_util as au

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
EPS32 = 2.0 ** -23
# one wave's lanes (64), and one below, at and above every template switch of launch_align_path (64, 512, 4096)
CLASSES = [1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 5000]


def _logits(kind, NT, ld, rng):
    if kind == "ties":   # multiples of 0.25 in [-4, 4]: exact adds, and equal values everywhere
        return (rng.integers(-16, 17, (NT, ld)) * 0.25).astype(f32)
    return (rng.standard_normal((NT, ld)) * 3.0).astype(f32)


def _lse_tol(z, N):
    """The kernel's sum (align_lse_kernel): a thread adds its 4 ceil(N / 1024) terms in order, the wave adds 64
    partial sums in 6 levels, thread 0 the 4 wave sums in 3 adds: D = 4 ceil(N / 1024) + 9 roundings on any term's
    way into the sum, each <= eps32 relative (all terms positive).  A term is exp(z - mx): the subtraction's rounding
    moves it by eps32 |z - mx| relative, which weighted by the terms' shares of the sum is at most eps32 ln N (the
    entropy bound), and expf is within 1 ulp: + 2 eps32.  So the sum is off by <= eps32 (D + 2 + ln N) relative, and
    its log by the same absolutely; logf's own ulp adds eps32 |log s|, the last add eps32 |lse|."""
    l = au.lse64(z, N)
    D = 4 * math.ceil(N / 1024) + 9
    return l, EPS32 * (D + 2 + math.log(N)) + EPS32 * (np.abs(l - np.asarray(z, f64)[:, :N].max(axis=1)) + np.abs(l))


def _hold(got, z, Cn, N):
    """one clip's results against the rule and the float64 log-softmax -> the worst lse error over its bound"""
    want, wscore = au.rule(z, Cn)
    assert got["path"].tolist() == want.tolist(), (z.shape, Cn)
    if len(z) == 0:
        return 0.0
    assert got["score"].view(np.uint32) == wscore.view(np.uint32), (z.shape, Cn)
    l, tol = _lse_tol(z, N)
    ref = np.asarray(z, f64)[np.arange(len(z)), want] - l
    assert (np.abs(got["lse"] - l) <= tol).all(), (np.abs(got["lse"] - l).max(), tol.min())
    assert (np.abs(got["logprob"] - ref) <= tol + EPS32 * np.abs(ref)).all()
    return float((np.abs(got["lse"] - l) / tol).max())


@pytest.mark.parametrize("kind", ["ties", "gauss"])
@pytest.mark.parametrize("Cn", CLASSES)
def test_class_counts_and_row_counts_match_the_rule(gpu, Cn, kind):
    """NT = 1, 2, 33 and two past the rows of one LDS block of the walk back (that many backpointer rows plus row 0,
    and one more), one batch; classify_num = C + 5 with NaN between it and ld, so a sum that runs long shows.  One
    row carries its largest logit in its LAST valid column: a sum that stops short there is off by ~8, checked to be
    more than 100 bounds."""
    rng = np.random.default_rng(Cn)
    N = Cn + 5
    ld = (N + 3) // 4 * 4 + 4
    bt = 16384 // ((Cn + 15) // 16 * 16)
    clips = []
    for NT in (1, 2, 33, bt + 2):
        z = _logits(kind, NT, ld, rng)
        z[:, N:] = np.nan
        clips.append(z)
    clips[2][7, N - 1] = clips[2][7, :N].max() + 8.0
    l, tol = _lse_tol(clips[2], N)
    assert au.lse64(clips[2], N)[7] - au.lse64(clips[2], N - 1)[7] > 100 * tol[7]
    res, guards, info = au.kt_align_path(clips, [Cn] * 4, N)
    assert guards and not info["declined"] and info["bt_rows"] == bt, info
    worst = max(_hold(got, z, Cn, N) for z, got in zip(clips, res[0]))
    print(f"C {Cn} {kind} {info['tag']}: worst lse error / bound = {worst:.3f}")


def test_peaks_in_order_come_back_and_one_out_of_order_is_repaired(gpu):
    rng = np.random.default_rng(5)
    NT, Cn, N = 20, 377, 5000
    z = (rng.standard_normal((NT, 5056)) * 0.1).astype(f32)
    peaks = np.arange(NT) * 15 + 10
    peaks[5] = peaks[4]                            # (a repeated class is in order too)
    z[np.arange(NT), peaks] += 20.0
    moved = z.copy()
    k, bad = 10, int(peaks[6]) - 1                 # row 10's peak to before the peaks of rows 6 .. 9: moving those costs 80
    moved[k, peaks[k]] -= 20.0
    moved[k, bad] += 20.0
    res, guards, _ = au.kt_align_path([z, moved], [Cn, Cn], N)
    assert guards
    assert res[0][0]["path"].tolist() == peaks.tolist() == z[:, :Cn].argmax(axis=1).tolist()
    got = res[0][1]["path"]
    assert got[k] != moved[k, :Cn].argmax() == bad and (np.diff(got) >= 0).all()
    _hold(res[0][1], moved, Cn, N)


@pytest.fixture(scope="module")
def mixed(gpu):
    rng = np.random.default_rng(11)
    shape = [(0, 70), (1, 377), (5, 5), (33, 600), (0, 12), (8, 64), (3, 1)]   # (NT, C): odd row offsets, empty clips
    return [(_logits("ties" if i % 2 else "gauss", NT, 608, rng), Cn) for i, (NT, Cn) in enumerate(shape)]


def test_mixed_batch_guards_two_launches_and_each_clip_alone(mixed):
    zs, Cs = [z for z, _ in mixed], [c for _, c in mixed]
    res, guards, info = au.kt_align_path(zs, Cs, 605, guard=24, launches=2)
    assert guards and not info["declined"]          # nothing outside the rows; an empty clip's score untouched
    for (z, Cn), a, b in zip(mixed, res[0], res[1]):
        _hold(a, z, Cn, 605)
        for key in ("path", "logprob", "lse"):      # a second launch on the same state agrees bit for bit
            assert a[key].tobytes() == b[key].tobytes(), key
        assert a["score"].tobytes() == b["score"].tobytes()
    for i in (1, 2, 3, 5, 6):                       # alone: another template, another row offset, the same bits
        alone, g1, _ = au.kt_align_path([zs[i]], [Cs[i]], 605)
        assert g1
        for key in ("path", "logprob", "lse", "score"):
            assert alone[0][0][key].tobytes() == res[0][i][key].tobytes(), (i, key)


@pytest.mark.parametrize("Cn,N,ld,nt", [(0, 40, 40, None), (8193, 8200, 8200, None), (41, 40, 40, None), (8, 44, 40, None),
                                        (8, 38, 38, None), (8, 40, 40, [2, -1])])
def test_declined_shapes_write_nothing(gpu, Cn, N, ld, nt):
    """C < 1, C > 8192, C > classify_num, classify_num > ld, ld % 4 != 0, NT < 0"""
    zs = [np.zeros((2, ld), f32), np.zeros((1, ld), f32)]
    res, guards, info = au.kt_align_path(zs, [Cn, max(Cn, 1)], N, nt=nt)
    assert info["declined"] and "launch_align_path" in info["msg"], info
    assert guards                                   # every output byte still 0xFF
