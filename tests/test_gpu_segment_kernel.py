"""The segmentation kernels (csrc/segment.hip) through qasr_kt_segment against the rule's NumPy
restatement (tests/segment_util.py): e, s and the peaks bit for bit, cuts and counts exactly, at the frame counts at
which the tile, the halo and the LDS passes change, with recordings at odd offsets in a mixed batch, the guards around
every output, and the independence of the results from batch and launch.  Small parameters only: (8, 3, 2) and
(40, 10, 5), and H = 0 and 64."""
import numpy as np
import pytest

import segment_util as su

pytestmark = pytest.mark.gpu
f32 = np.float32
PARAMS = ((8, 3, 2), (40, 10, 5))


def _rec(rng, n):
    """amplitudes over several decades (frames then differ by far more than rounding), the edges carrying weight"""
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 0, n))).astype(f32)
    if n:
        x[0] = x[-1] = 1.0
    return x


@pytest.fixture(scope="module")
def tile(gpu):
    return su.kt_segment([np.zeros(3, f32)], 8, 3, 2)[2]


def _hold(got, x, mx, mn, H):
    want = su.rule(x, mx, mn, H)
    assert len(got["e"]) == len(want["e"]) == su.frames(len(x))
    assert (su.bits(got["e"]) == su.bits(want["e"])).all(), (len(x), int((su.bits(got["e"]) != su.bits(want["e"])).sum()))
    assert (su.bits(got["s"]) == su.bits(want["s"])).all(), (len(x), int((su.bits(got["s"]) != su.bits(want["s"])).sum()))
    assert got["cuts"] == want["cuts"], len(x)
    assert (su.bits(got["peak"]) == su.bits(want["peak"])).all(), len(x)
    assert su.bits(got["peak_rec"]) == su.bits(want["peak_rec"]), len(x)


@pytest.mark.parametrize("prm", PARAMS)
def test_edge_frame_counts_match_the_rule(tile, prm):
    mx, mn, H = prm
    assert tile >= 64
    rng = np.random.default_rng(mx)
    Fs = [0, 1, 2 * H, 2 * H + 1] + [t + d for t in (tile, 2 * tile) for d in (-1, 0, 1)]
    # every length once with whole frames and once with a 37-sample tail: all as one batch, whose recordings then
    # start at odd offsets too, each held to the rule on its own
    recs = [_rec(rng, 160 * F + tail) for F in Fs for tail in (0, 37)]
    res, guards, _ = su.kt_segment(recs, mx, mn, H)
    assert guards
    for x, got in zip(recs, res[0]):
        _hold(got, x, mx, mn, H)


@pytest.mark.parametrize("H", [0, 64])
def test_no_smoothing_and_the_widest_halo(tile, H):
    """H = 64: the halo reaches past both ends of every recording shorter than 64 frames, and past one end of a tile's
    window in the longer ones; the window of a full tile takes more LDS passes than at H = 5"""
    rng = np.random.default_rng(64 + H)
    recs = [_rec(rng, 160 * F + 9) for F in (1, 30, 63, 64, 65, 129, tile - 1, tile + 64, 2 * tile + 1)]
    res, guards, _ = su.kt_segment(recs, 40, 10, H)
    assert guards
    for x, got in zip(recs, res[0]):
        _hold(got, x, 40, 10, H)


@pytest.fixture(scope="module")
def mixed(gpu):
    rng = np.random.default_rng(7)
    sizes = [160 * 50 + 1, 160 * 400 + 33, 0, 77, 160 * 9, 160 * 200 + 159]   # odd offsets, one empty, one without a frame
    recs = [_rec(rng, n) for n in sizes]
    recs[1][160 * 100:160 * 130] = 0.0   # a pause: ties among equal zeros inside a window
    return recs


def test_mixed_batch_guards_and_two_launches(mixed):
    res, guards, _ = su.kt_segment(mixed, 40, 10, 5, guard=24, launches=2)
    assert guards                                   # nothing written before or after any output
    for x, a, b in zip(mixed, res[0], res[1]):
        _hold(a, x, 40, 10, 5)
        for k in ("e", "s", "peak"):                # a second launch on the same state agrees
            assert (su.bits(a[k]) == su.bits(b[k])).all(), k
        assert a["cuts"] == b["cuts"] and su.bits(a["peak_rec"]) == su.bits(b["peak_rec"])
    assert res[0][2]["cuts"] == [0] and len(res[0][2]["e"]) == 0 and res[0][2]["peak"].tolist() == [0.0]
    assert res[0][3]["cuts"] == [0] and res[0][3]["peak_rec"] == 0.0
    assert len(res[0][1]["cuts"]) > 10


def test_a_recording_alone_equals_itself_in_the_batch(mixed):
    batch, _, _ = su.kt_segment(mixed, 40, 10, 5)
    for b in (0, 1, 2, 5):
        alone, guards, _ = su.kt_segment([mixed[b]], 40, 10, 5)
        assert guards
        for k in ("e", "s", "peak"):
            assert (su.bits(alone[0][0][k]) == su.bits(batch[0][b][k])).all(), (b, k)
        assert alone[0][0]["cuts"] == batch[0][b]["cuts"]


def test_digital_silence_takes_the_larger_frame(gpu):
    res, guards, _ = su.kt_segment([np.zeros(160 * 100 + 5, f32)], 8, 3, 2)
    assert guards and res[0][0]["cuts"] == list(range(0, 100, 8))
