"""The batch-1 fused launch's pipelined chain role (attention.hip
fx1_chain_body / fx1_gather_weights: producer waves publish the softmax
weights in 256-key chunks through an LDS progress word, the chain waves run
behind them) against the separate exact kernels of fa_exact.hip: the
decode-step logits are bit-identical across the chunk seams with live maxima
and at the upper end of the fused range (DX_KC = 2048 keys).

The context's device error word has no accessor in the Python binding and no
option exposes it, so "no stuck wave reported" is not asserted here (a wait
that runs out makes the next call fail with the error's text all the same)."""
import numpy as np
import pytest

import qasr

pytestmark = pytest.mark.gpu

CHUNK = 256   # fx_chain.h FX_PC


@pytest.fixture(scope="module")
def model(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    yield m
    m.close()


def _run(c, fused, steps, expect=None):
    """decode_step over steps = [(token, n_past)] with the fused QKV +
    attention + o-projection launch (fused = 1) or the separate launches;
    expect: the fused_exact value per step where it is not `fused`"""
    c.set_option("fuse_qkv", fused)
    c.set_option("fuse_o", fused)
    out = []
    for i, (tok, n_past) in enumerate(steps):
        lg, _ = c.decode_step([tok], [n_past])
        want = fused if expect is None else expect[i]
        assert c.get_option("fused_exact") == want, (fused, n_past)
        if want == fused:
            assert c.get_option("fused_mode") == 2 * fused, (fused, n_past)
        out.append(lg[0].copy())
    return out


def test_chunk_seams_with_live_maxima(model):
    """Positions 0 .. 2 C + 7 on seeded random tokens: the single chunk, the
    255/256/257 and 511/512/513 seams with real scores, new maxima in first,
    middle and last chunks and in the chunk that holds the new key"""
    hp = model.hp
    toks = np.random.default_rng(20261).integers(0, hp.vocab_size, 2 * CHUNK + 8).tolist()
    steps = [(int(t), k) for k, t in enumerate(toks)]
    c = qasr.Context(model, max_batch=1, max_ctx=640)
    try:
        out = {fused: _run(c, fused, steps) for fused in (1, 0)}
    finally:
        c.close()
    for k in range(len(steps)):
        assert np.isfinite(out[1][k]).all(), k
        assert np.array_equal(out[1][k], out[0][k]), (k, float(np.abs(out[1][k] - out[0][k]).max()))


def test_upper_end_of_the_fused_range(model):
    """Single steps on the zero-initialised cache at n_past 2046 and 2047
    (2047 and 2048 keys: the last full weights image) take the fused launch
    and are bit-equal; n_past 2048 (2049 keys) falls back to the separate
    launches (fused_exact == 0) and is finite.  The parent build, with one
    chain workgroup a kv group, behaves the same way at these three positions
    (this test passes on it unchanged), so the limit is the issue's"""
    steps = [(4321, 2046), (4322, 2047), (4323, 2048)]
    c = qasr.Context(model, max_batch=1, max_ctx=2112)
    try:
        out1 = _run(c, 1, steps, expect=[1, 1, 0])
        out0 = _run(c, 0, steps)
    finally:
        c.close()
    for k, (_, n_past) in enumerate(steps):
        assert np.isfinite(out1[k]).all(), n_past
        if n_past < 2048:
            assert np.array_equal(out1[k], out0[k]), (n_past, float(np.abs(out1[k] - out0[k]).max()))
