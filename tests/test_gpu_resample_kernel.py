"""The resample kernel (csrc/resample.hip) through qasr_kt_resample, bit for bit against the rule's
NumPy restatement (tests/resample_util.py) with the library's tap tables: every rate family (LDS tables L = 1, 2;
L2 tables L = 160, 640; the copy), the clip lengths at which the zero fill, the window and the tile change, one batch
of mixed rates, the guards around every output, and the independence of the bits from batch and launch."""
import numpy as np
import pytest

import qasr
import resample_util as ru

pytestmark = pytest.mark.gpu
f32 = np.float32
RATES = (8000, 11025, 44100, 48000, 96000, 16000)


def _clip(rng, n):
    x = rng.standard_normal(n).astype(f32)
    if n:
        x[0] = x[-1] = 1.0   # the clip's edges carry weight: a wrong zero fill shows
    return x


@pytest.fixture(scope="module")
def tables(gpu):
    return {sr: qasr.resample_taps(sr) for sr in RATES}


@pytest.fixture(scope="module")
def tile(gpu):
    return ru.kt_resample([np.zeros(3, f32)], [16000])[3]


def _in_around(n_out, sr):
    """the clip lengths whose output lengths are nearest to n_out from below and from above (an upsampler's output
    lengths skip values: 8 kHz gives even ones only)"""
    L, M, _ = ru.plan(sr)
    n = (n_out * M) // L
    while ru.out_len(n, sr) > n_out:
        n -= 1
    while ru.out_len(n + 1, sr) <= n_out:
        n += 1
    return [n] if ru.out_len(n, sr) == n_out else [n, n + 1]


@pytest.mark.parametrize("sr", RATES)
def test_edge_lengths_match_the_rule(tables, tile, sr):
    assert tile >= 64
    _L, _M, H = ru.plan(sr)
    rng = np.random.default_rng(sr)
    sizes = [0, 1, 2, H, H + 1, 2 * H + 1]
    targets = [t + d for t in (tile, 2 * tile) for d in (-1, 0, 1)]
    for t in targets:
        sizes += _in_around(t, sr)
    clips = [_clip(rng, n) for n in sizes]
    # all lengths as one batch (the kernel test's launches stay few), each clip held to the rule on its own
    got, guards, _, _ = ru.kt_resample(clips, [sr] * len(clips))
    assert guards
    outs = set()
    for x, y in zip(clips, got):
        want = ru.resample(x, sr, tables[sr])
        assert len(y) == len(want) == ru.out_len(len(x), sr)
        assert (ru.bits(y) == ru.bits(want)).all(), (sr, len(x), int((ru.bits(y) != ru.bits(want)).sum()))
        outs.add(len(y))
    L, M, _ = ru.plan(sr)
    if L <= M:   # every output length exists: one short of, at and one past the tile and twice it
        assert set(targets) <= outs
    for t in targets:   # an upsampler: the nearest lengths on both sides
        assert any(t - 2 <= o <= t for o in outs) and any(t <= o <= t + 2 for o in outs), (t, sorted(outs))


@pytest.fixture(scope="module")
def mixed(tables):
    rng = np.random.default_rng(7)
    rates = [48000, 44100, 8000, 16000, 11025, 96000]
    sizes = [3001, 5000, 700, 1234, 0, 9001]   # (one of them empty)
    clips = [_clip(rng, n) for n in sizes]
    want = [ru.resample(x, sr, tables[sr]) for x, sr in zip(clips, rates)]
    return clips, rates, want


def test_mixed_batch_guards_and_two_launches(mixed):
    clips, rates, want = mixed
    got, guards, again, _ = ru.kt_resample(clips, rates, guard=96, launches=2)
    assert guards                                   # nothing written before or after any clip's output
    for y, y2, w in zip(got, again, want):
        assert (ru.bits(y) == ru.bits(w)).all()
        assert (ru.bits(y2) == ru.bits(y)).all()    # a second launch on the same state agrees
    assert len(got[4]) == 0
    assert (ru.bits(got[3]) == ru.bits(clips[3])).all()   # the 16 kHz clip is copied


def test_a_clip_alone_equals_itself_in_the_batch(mixed):
    clips, rates, want = mixed
    for b in (0, 1, 4, 5):
        got, guards, _, _ = ru.kt_resample([clips[b]], [rates[b]])
        assert guards and (ru.bits(got[0]) == ru.bits(want[b])).all(), b


def test_unsupported_rate_is_refused():
    with pytest.raises(qasr.QasrError, match="44101"):
        ru.kt_resample([np.zeros(10, f32)], [44101])
