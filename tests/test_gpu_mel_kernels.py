"""csrc/mel.hip (mel_power_kernel, mel_norm_kernel) through Context.mel and the standalone engine, against the float64
reference and bound of tests/mel_util.py (derived there; tests/test_mel_util_host.py shows they tell the mistakes of
interest apart) and against the C oracle at the 1e-5 the parity tests use.  The signals reach what synth_pcm does not:
a negative clip maximum (the other branch of the atomicMax key), content only the dropped frame sees, floor and
clamp, reflect padding of clips shorter than the pad, frame-block seams, per-clip isolation in a batch, and state a
context or an engine keeps between calls.  A HIP error in any call ends the session (mel_util.ctx_mel / Engine.run)."""
import time

import numpy as np
import pytest

import mel_util as mu
import oracle_py as op
import qasr

pytestmark = pytest.mark.gpu

WORST, EQUAL = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _record(gpu, parity):
    t0 = time.time()
    yield
    parity("mel_reference_tests", wall_s=time.time() - t0,
           **{f"{k}_worst_over_bound": v for k, v in sorted(WORST.items())},
           **{f"{k}_bit_equal_to_oracle": v for k, v in sorted(EQUAL.items())})


@pytest.fixture(scope="module")
def model(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    yield m
    m.close()


@pytest.fixture(scope="module")
def ctx(model):
    c = qasr.Context(model, max_batch=4, max_ctx=640)
    yield c
    c.close()


@pytest.fixture(scope="module")
def engine(gpu):
    e = mu.Engine()
    yield e
    e.close()


def _fresh(model, clips):
    c = qasr.Context(model, max_batch=4, max_ctx=640)
    try:
        return mu.ctx_mel(c, clips)
    finally:
        c.close()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------- every signal x length
@pytest.mark.parametrize("family", sorted(mu.FAMILIES))
def test_family_against_reference_and_oracle(ctx, family):
    worst, eq, total = 0.0, 0, 0
    for n in mu.LENGTHS:
        x = mu.FAMILIES[family](n)
        g = mu.ctx_mel(ctx, [x])[0]
        ref, bound = mu.log_mel_reference(x)
        o = op.log_mel(x)
        assert g.shape == o.shape == (128, n // 160)
        r = mu.check(g, ref, bound, f"{family} n={n}")
        err = float(np.abs(g - o).max())
        print(f"{family} n={n}: error / bound {r:.4g}, |gpu - oracle| {err:.3g}, bit-equal {(g == o).mean():.4f}")
        assert err <= 1e-5, (family, n, err)
        worst, eq, total = max(worst, r), eq + int((g == o).sum()), total + g.size
    WORST[family], EQUAL[family] = worst, eq / total


def test_context_mel_is_the_call_these_tests_make(ctx):
    x = mu.quiet_1e3(1281)
    assert _same_bits(ctx.mel([x])[0], mu.ctx_mel(ctx, [x])[0])


@pytest.mark.parametrize("n", [160, 401, 1281, 2879])
def test_silence_is_minus_one_and_a_half(ctx, engine, n):
    for g in (mu.ctx_mel(ctx, [mu.silence(n)])[0], engine.run(mu.silence(n))):
        assert g.shape == (128, n // 160) and (g.view(np.uint32) == np.float32(-1.5).view(np.uint32)).all()


@pytest.mark.parametrize("T", mu.TAIL_T)
def test_tail_burst_stays_in_the_dropped_frame(ctx, T):
    """only frame TF - 1 sees the burst (test_mel_util_host.py shows it on the reference): with it zeroed the kept
    frames are the same bits -- a maximum that took the dropped frame in would raise the clamp over most of them"""
    n = 160 * T + 159
    a = mu.ctx_mel(ctx, [mu.tail_burst(n)])[0]
    b = mu.ctx_mel(ctx, [mu.tail_burst(n, burst=False)])[0]
    assert a.shape == (128, T) and _same_bits(a, b)


# ------------------------------------------------------ batches and state
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_batch_equals_one_clip_per_call(ctx, order):
    clips = mu.batch_clips()[::1 if order == "forward" else -1]
    single = [mu.ctx_mel(ctx, [x])[0] for x in clips]
    batched = mu.ctx_mel(ctx, clips)
    for b, (x, s, g) in enumerate(zip(clips, single, batched)):
        assert g.shape == (128, len(x) // 160) and _same_bits(s, g), (order, b, len(x))
        ref, bound = mu.log_mel_reference(x)
        mu.check(g, ref, bound, f"batch {order} clip {b}")


def test_quiet_after_loud_on_one_context(model):
    loud, quiet = mu.full_scale(3 * mu.SR), mu.quiet_1e5(int(0.2 * mu.SR))
    want = _fresh(model, [quiet])[0]
    c = qasr.Context(model, max_batch=4, max_ctx=640)
    try:
        mu.ctx_mel(c, [loud])
        got = mu.ctx_mel(c, [quiet])[0]
    finally:
        c.close()
    assert _same_bits(got, want)
    ref, bound = mu.log_mel_reference(quiet)
    mu.check(got, ref, bound, "quiet after loud")


def test_batch_of_one_after_batch_of_four(model):
    four = [mu.full_scale(mu.SR), mu.dc(4000), mu.tone_on_silence(8000), mu.full_scale(5000)]
    one = [mu.quiet_1e3(1281)]
    want = _fresh(model, one)[0]
    c = qasr.Context(model, max_batch=4, max_ctx=640)
    try:
        mu.ctx_mel(c, four)
        got = mu.ctx_mel(c, one)[0]
    finally:
        c.close()
    assert _same_bits(got, want)


def test_ragged_batch_three_times_same_bits(ctx):
    clips = mu.batch_clips()
    first = mu.ctx_mel(ctx, clips)
    for _ in range(2):
        for a, b in zip(first, mu.ctx_mel(ctx, clips)):
            assert _same_bits(a, b)


# ------------------------------------------------------ standalone engine
def test_engine_equals_context(ctx, engine):
    for x in (mu.quiet_1e3(1281), mu.full_scale(2560), mu.tail_burst(1599), mu.impulse(201), mu.tone_on_silence(2879)):
        assert _same_bits(engine.run(x), mu.ctx_mel(ctx, [x])[0]), len(x)


def test_engine_short_after_long_and_quiet_after_loud(ctx):
    long_loud, short_quiet = mu.full_scale(3 * mu.SR), mu.quiet_1e5(401)
    e = mu.Engine()
    try:
        a = e.run(long_loud)
        b = e.run(short_quiet)
    finally:
        e.close()
    assert _same_bits(a, mu.ctx_mel(ctx, [long_loud])[0]) and _same_bits(b, mu.ctx_mel(ctx, [short_quiet])[0])
    ref, bound = mu.log_mel_reference(short_quiet)
    mu.check(b, ref, bound, "engine: short quiet after long loud")


def test_engine_filterbanks(ctx):
    """a custom bank is used, and neither the built-in table passed explicitly nor filters = NULL ("the built-in
    generate_mel_filters values", include/qasr_capi.h) inherits it from the call before"""
    x = mu.quiet_1e3(1281)
    builtin = mu.ctx_mel(ctx, [x])[0]
    half = mu.filters() * np.float32(0.5)
    holed = mu.filters().copy()
    holed[40] = 0.0
    e = mu.Engine()
    try:
        for name, bank in (("filters * 0.5", half), ("band 40 zeroed", holed)):
            g = e.run(x, bank)
            ref, bound = mu.log_mel_reference(x, bank)
            mu.check(g, ref, bound, f"engine, {name}")
            assert float(np.abs(g - mu.oracle_log_mel(x, bank)).max()) <= 1e-5
            assert not _same_bits(g, builtin)
        assert _same_bits(e.run(x, mu.filters()), builtin)          # the built-in table, explicitly
        e.run(x, half)
        null = e.run(x, None)                                       # NULL after a custom bank
    finally:
        e.close()
    ref, bound = mu.log_mel_reference(x)
    mu.check(null, ref, bound, "engine, filters = NULL after a custom bank")
    assert _same_bits(null, builtin)


# ---------------------------------------------------------- argument edges
def test_no_samples_no_frames(ctx, engine):
    for n in (0, 100):
        x = mu.quiet_1e3(n)
        assert mu.ctx_mel(ctx, [x])[0].shape == (128, 0) and engine.run(x).shape == (128, 0)


def test_negative_length_is_an_argument_error(ctx, engine):
    x = mu.quiet_1e3(400)
    rc, _ = mu.ctx_mel_rc(ctx, [x], lens=[-1])
    assert rc == 1, rc                                              # QASR_ERR_ARG
    rc, _ = mu.ctx_mel_rc(ctx, [x, x], lens=[400, -160])
    assert rc == 1, rc
    rc, _ = engine.run_rc(x, -1)
    assert rc == 1, rc
    assert _same_bits(mu.ctx_mel(ctx, [x])[0], engine.run(x))       # both still serve the next call
