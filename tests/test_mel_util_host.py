"""The log-mel reference and its bound (tests/mel_util.py) before a GPU sees them: the C oracle lies inside the bound
on every signal x length the GPU tests use, every deliberate mistake the GPU tests are meant to catch lies outside it on
the case built for it (the ratios go to the parity record), and the values that are exact are exact.  No GPU."""
import numpy as np
import pytest

import mel_util as mu
import oracle_py as op


@pytest.fixture(scope="module", autouse=True)
def _libs(built):
    mu.filters()


@pytest.mark.parametrize("family", sorted(mu.FAMILIES))
def test_oracle_within_bound_of_reference(family, parity):
    worst = 0.0
    for n in mu.LENGTHS:
        x = mu.FAMILIES[family](n)
        ref, bound = mu.log_mel_reference(x)
        o = op.log_mel(x)
        assert o.shape == ref.shape == (128, n // 160)
        worst = max(worst, mu.check(o, ref, bound, f"{family} n={n}"))
    print(f"{family}: oracle worst error / bound {worst:.4g}")
    parity("mel_host_oracle_vs_reference", **{family: worst})


def test_rfft_within_its_share_of_the_bound():
    """numpy's rfft against a direct long double sum with angles reduced mod 400: below the 1300 u S1 the module
    docstring grants an FFT, itself below GAMMA S1"""
    ld = np.longdouble
    own = 8 if np.finfo(ld).eps < 2.0 ** -60 else 8 + 400   # the direct sum's own error where long double is double
    kt = (np.arange(mu.NB)[:, None] * np.arange(mu.FS)[None, :]) % mu.FS
    ang = 2 * ld(np.pi) * kt.astype(ld) / mu.FS           # pi rounded to double: relative 2^-53 of an angle < 2 pi
    cs, sn = np.cos(ang), np.sin(ang)
    assert (1300 + own) * mu.U < mu.GAMMA
    for fam in ("full_scale", "quiet_1e-3", "tone_on_silence", "impulse"):
        fr = mu.frames_of(mu.FAMILIES[fam](1281)) * mu.hann()[None, :]
        X = np.fft.rfft(fr, axis=1)
        re, im = fr.astype(ld) @ cs.T, -(fr.astype(ld) @ sn.T)
        err = np.sqrt(((X.real - re) ** 2 + (X.imag - im) ** 2).astype(np.float64))
        s1 = np.abs(fr).sum(1)[:, None]
        assert (err <= (1300 + own) * mu.U * s1 + 1e-300).all(), (fam, float((err / np.maximum(s1, 1e-300)).max() / mu.U))


# ------------------------------------------------------- deliberate mistakes
def _caught(parity, name, mutated, ref, bound):
    r = mu.ratio(mutated, ref, bound)
    print(f"mutation {name}: error / bound = {r:.4g}")
    parity("mel_host_mutations", **{name: min(r, 1e300)})
    assert r > 1.0, (name, r)
    return r


def test_mutation_max_over_the_dropped_frame(parity):
    for T in mu.TAIL_T:
        x = mu.tail_burst(160 * T + 159)
        v, dv = mu.log_power(x, want_bound=True)
        ref, bound = mu.finish(v, dv)
        _caught(parity, f"max_over_all_frames_T{T}", mu.finish(v, all_frames=True)[0], ref, bound)


def test_mutation_one_max_for_the_batch(parity):
    loud, quiet = mu.full_scale(1600), mu.quiet_1e3(1600)
    vq, dq = mu.log_power(quiet, want_bound=True)
    ref, bound = mu.finish(vq, dq)
    shared = max(mu.log_power(loud)[0][:, :-1].max(), vq[:, :-1].max())
    _caught(parity, "batch_shared_max", mu.finish(vq, m=shared)[0], ref, bound)


@pytest.mark.parametrize("family", ["quiet_1e-3", "full_scale", "dc", "impulse"])
def test_mutation_symmetric_hann(family, parity):
    x = mu.FAMILIES[family](1281)
    ref, bound = mu.log_mel_reference(x)
    _caught(parity, f"symmetric_hann_{family}", mu.finish(mu.log_power(x, periodic=False)[0])[0], ref, bound)


def test_mutation_reflect_off_by_one(parity):
    """n = 1280: the last kept frame reads 40 reflected samples; the first frame reads the left reflection"""
    x = mu.impulse(1280)
    ref, bound = mu.log_mel_reference(x)
    bad = mu.finish(mu.log_power(x, shift=1)[0])[0]
    _caught(parity, "reflect_off_by_one_left", bad[:, :1], ref[:, :1], bound[:, :1])
    _caught(parity, "reflect_off_by_one_right", bad[:, -1:], ref[:, -1:], bound[:, -1:])


def test_mutation_clamp_7(parity):
    x = mu.tone_on_silence(1281)
    v, dv = mu.log_power(x, want_bound=True)
    ref, bound = mu.finish(v, dv)
    _caught(parity, "clamp_7", mu.finish(v, clamp=7.0)[0], ref, bound)


def test_mutation_no_floor(parity):
    x = mu.silence(1281)
    ref, bound = mu.log_mel_reference(x)
    _caught(parity, "no_floor", mu.finish(mu.log_power(x, floor=False)[0])[0], ref, bound)


# --------------------------------------------------------------- exact values
@pytest.mark.parametrize("n", [160, 401, 1281, 2879])
def test_silence_is_minus_one_and_a_half(n):
    ref, bound = mu.log_mel_reference(mu.silence(n))
    assert np.abs(ref + 1.5).max() <= 4 * mu.U and (ref.astype(np.float32) == np.float32(-1.5)).all()
    assert (bound < mu.ulp32(1.5)).all()                   # the bound admits -1.5 alone
    assert (op.log_mel(mu.silence(n)) == np.float32(-1.5)).all()


@pytest.mark.parametrize("n", [0, 1, 100, 159])
def test_no_frames_below_160_samples(n):
    ref, bound = mu.log_mel_reference(mu.quiet_1e3(n))
    assert ref.shape == bound.shape == (128, 0) and op.log_mel(mu.quiet_1e3(n)).shape == (128, 0)


@pytest.mark.parametrize("T", mu.TAIL_T)
def test_tail_burst_reaches_only_the_dropped_frame(T):
    """the premise of the GPU test: with the burst zeroed the kept frames are the same bits, in the reference and in
    the oracle, while the dropped frame differs"""
    n = 160 * T + 159
    a, b = mu.tail_burst(n), mu.tail_burst(n, burst=False)
    va, vb = mu.log_power(a)[0], mu.log_power(b)[0]
    assert np.array_equal(va[:, :T], vb[:, :T]) and va[:, T].max() > va[:, :T].max() + 3
    assert np.array_equal(mu.finish(va)[0], mu.finish(vb)[0])
    assert np.array_equal(op.log_mel(a), op.log_mel(b))


def test_quiet_clips_have_a_negative_maximum():
    """the premise of the quiet families: the per-clip maximum is below 0"""
    for fam in ("quiet_1e-3", "quiet_1e-5", "silence"):
        for n in (160, 1281):
            assert mu.log_power(mu.FAMILIES[fam](n))[0][:, :-1].max() < 0, (fam, n)


def test_custom_filterbank_reaches_the_reference():
    x = mu.quiet_1e3(1281)
    half = mu.filters() * np.float32(0.5)
    ref, bound = mu.log_mel_reference(x, half)
    mu.check(mu.oracle_log_mel(x, half), ref, bound, "filters * 0.5")
    assert mu.ratio(mu.oracle_log_mel(x), ref, bound) > 1.0      # the built-in bank is told apart from it
