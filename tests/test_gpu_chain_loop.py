"""The batch-1 fused launch's chain loop (attention.hip fx1_chain_body: the
unclamped main loop from a scalar base, the clamped tail, the per-chain
bitmap of buffers holding a new maximum) against the separate exact kernels
of fa_exact.hip, the independent implementation of the same arithmetic: the
decode-step logits are bit-identical at every key count across the 64-key
buffer seams and at the benchmark's context size."""
import numpy as np
import pytest

import qasr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    yield m
    m.close()


def _run(c, fused, steps):
    """decode_step over steps = [(token, n_past)] with the fused QKV +
    attention + o-projection launch (fused = 1) or the separate launches"""
    c.set_option("fuse_qkv", fused)
    c.set_option("fuse_o", fused)
    out = []
    for tok, n_past in steps:
        lg, _ = c.decode_step([tok], [n_past])
        assert c.get_option("fused_exact") == fused and c.get_option("fused_mode") == 2 * fused, (fused, n_past)
        out.append(lg[0].copy())
    return out


def test_chain_every_key_count_across_buffer_seams(model):
    """Key counts 1 .. 200 from position 0: the empty main loop, the first
    full buffer, the 63/64/65 and 127/128/129 seams of both register sets,
    the clamped tail at every offset, buffers with and without new maxima"""
    hp = model.hp
    toks = np.random.default_rng(20260).integers(0, hp.vocab_size, 200).tolist()
    steps = [(int(t), k) for k, t in enumerate(toks)]
    c = qasr.Context(model, max_batch=1, max_ctx=320)
    try:
        out = {fused: _run(c, fused, steps) for fused in (1, 0)}
    finally:
        c.close()
    for k in range(len(steps)):
        assert np.isfinite(out[1][k]).all(), k
        assert np.array_equal(out[1][k], out[0][k]), (k, float(np.abs(out[1][k] - out[0][k]).max()))


def test_chain_benchmark_context_seams(model):
    """max_ctx of the 92 s clip: one step at the split-bucket and buffer seams
    on the zero-initialised cache (equal scores: a single maximum at key 0,
    every later buffer on the fast path); the fused launch must still be taken"""
    steps = [(1234 + i, n_past) for i, n_past in enumerate((1215, 1279, 1280, 1407, 1532))]
    c = qasr.Context(model, max_batch=1, max_ctx=1541)
    try:
        out = {fused: _run(c, fused, steps) for fused in (1, 0)}
    finally:
        c.close()
    for k, (_, n_past) in enumerate(steps):
        assert np.isfinite(out[1][k]).all(), n_past
        assert np.array_equal(out[1][k], out[0][k]), (n_past, float(np.abs(out[1][k] - out[0][k]).max()))
