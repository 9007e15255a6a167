"""The batch-1 fused launch's request order (attention.hip qkv_attn1_kernel:
q-row QKV blocks first, only the last split waiting for the new token's k and v
granules, the kvw_delay / k_stagger / vt_stagger options) against the separate
launches: the decode-step logits are bit-identical at every position across the
split seams (where the last split holds only the new key) and the 256-key chunk
seam, the cache rows the last split writes are those of the separate launches,
and the three options change no bit at 0 or at a large value.

A wait that runs out at the default poll_limit fails the call that ran it
(QASR_ERR_DEVICE -> QasrError), so every call below returning is the check
that none did."""
import numpy as np
import pytest

import qasr

pytestmark = pytest.mark.gpu

SR = 16000


@pytest.fixture(scope="module")
def model(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    yield m
    m.close()


@pytest.fixture(scope="module")
def tokens(model):
    return [int(t) for t in np.random.default_rng(20262).integers(0, model.hp.vocab_size, 331)]


def _fuse(c, fused):
    c.set_option("fuse_qkv", fused)
    c.set_option("fuse_o", fused)


def _steps(c, fused, tokens, lo, hi, keep=None):
    """decode_step at n_past lo .. hi - 1 with the fused QKV + attention +
    o-projection launch (fused = 1) or the separate launches; returns the logits
    of the positions in keep (default: all)"""
    _fuse(c, fused)
    out = {}
    for k in range(lo, hi):
        lg, _ = c.decode_step([tokens[k]], [k])
        assert c.get_option("fused_mode") == 2 * fused, (fused, k)
        if keep is None or k in keep:
            out[k] = lg[0].copy()
    return out


def _assert_equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.isfinite(a[k]).all(), (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k] - b[k]).max()))


@pytest.fixture(scope="module")
def separate_0_330(model, tokens):
    """the separate launches' logits at n_past 0 .. 330 (computed once)"""
    c = qasr.Context(model, max_batch=1, max_ctx=640)
    try:
        return _steps(c, 0, tokens, 0, 331)
    finally:
        c.close()


def test_split_and_chunk_seams(model, tokens, separate_0_330):
    """n_past 0 .. 330: the 64-key split seams 63/64/65 .. 319/320/321 (at a
    multiple of 64 the last split holds the new key alone) and the 255/256/257
    chunk seam"""
    c = qasr.Context(model, max_batch=1, max_ctx=640)
    try:
        fused = _steps(c, 1, tokens, 0, 331)
    finally:
        c.close()
    _assert_equal(fused, separate_0_330, "spl 64")


def test_split_seams_128_key_splits(model, tokens):
    """att_spl1 = 128: n_past 120 .. 135 (the 127/128/129 split seam) and
    250 .. 262 (the chunk seam, a split seam too), each position stepped with
    the separate launches and then again, over the same cache, with the fused
    one; the positions between are filled with the separate launches"""
    c = qasr.Context(model, max_batch=1, max_ctx=640)
    sep, fused = {}, {}
    try:
        c.set_option("att_spl1", 128)
        _steps(c, 0, tokens, 0, 120, keep=())
        for lo, hi in ((120, 136), (250, 263)):
            for k in range(lo, hi):
                sep.update(_steps(c, 0, tokens, k, k + 1))
                fused.update(_steps(c, 1, tokens, k, k + 1))
            if hi < 250:
                _steps(c, 0, tokens, hi, 250, keep=())
    finally:
        c.close()
    assert len(fused) == 29
    _assert_equal(fused, sep, "spl 128")


def test_cache_rows_written_by_the_last_split(model, tokens, separate_0_330):
    """steps 0 .. 199 fused, then step 200 with the separate launches, against
    201 separate steps: step 200 reads the K and V^T (exact attention) rows of
    every earlier position, so they were all written, and written identically,
    although one split a step now reads the new k and v.  The V rows, which the
    exact attention does not read, are checked the same way with the fp32
    split-K attention over a shorter run (fa_exact_decode = 0)"""
    c = qasr.Context(model, max_batch=1, max_ctx=640)
    try:
        _steps(c, 1, tokens, 0, 200, keep=())
        got = _steps(c, 0, tokens, 200, 201)
    finally:
        c.close()
    _assert_equal(got, {200: separate_0_330[200]}, "K / V^T rows")
    out = {}
    for first in (1, 0):
        c = qasr.Context(model, max_batch=1, max_ctx=640)
        try:
            c.set_option("fa_exact_decode", 0)
            _steps(c, first, tokens, 0, 70, keep=())
            out[first] = _steps(c, 0, tokens, 70, 71)
        finally:
            c.close()
    _assert_equal(out[1], out[0], "V rows")


def test_fp32_split_k_mode(model, tokens):
    """fa_exact_decode = 0 (the splits take V from the cache and combine in
    fp32): 70 consecutive steps across the 63/64/65 seam"""
    out = {}
    for fused in (1, 0):
        c = qasr.Context(model, max_batch=1, max_ctx=640)
        try:
            c.set_option("fa_exact_decode", 0)
            out[fused] = _steps(c, fused, tokens, 0, 70)
        finally:
            c.close()
    _assert_equal(out[1], out[0], "split-K")


def test_staggered_requests_past_the_first_chunk(model, tokens, separate_0_330):
    """the three options together where they reach code the 2 s clip below does
    not: past 256 keys the splits of the second chunk delay their K request and
    the chain waves pull the second chunk's V^T behind the barrier"""
    c = qasr.Context(model, max_batch=1, max_ctx=640)
    try:
        _steps(c, 0, tokens, 0, 300, keep=())
        for name in ORDER_CASES:
            c.set_option(name, 6)
        got = _steps(c, 1, tokens, 300, 331)
    finally:
        c.close()
    _assert_equal(got, {k: separate_0_330[k] for k in got}, "staggered")


@pytest.mark.parametrize("vpf", [2, 6])
def test_vt_pull_shared_by_the_two_heads(model, tokens, separate_0_330, vpf):
    """fx_vpf 6 (a kv group's two chain workgroups pull half of its V^T each)
    and 2 (each pulls all of it): n_past 250 .. 330, where a wave's share runs
    over several key blocks and the 256-key seam is crossed"""
    c = qasr.Context(model, max_batch=1, max_ctx=640)
    try:
        _steps(c, 0, tokens, 0, 250, keep=())
        c.set_option("fx_vpf", vpf)
        got = _steps(c, 1, tokens, 250, 331)
    finally:
        c.close()
    _assert_equal(got, {k: separate_0_330[k] for k in got}, "fx_vpf")


# the request-order options (s_sleep(8) units): the values each must leave every bit alone at
ORDER_CASES = {"kvw_delay": (0, 64), "k_stagger": (0, 64), "vt_stagger": (0, 64)}


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_order_option_matches_default(model, name):
    """each option at 0 and at a large value: decode-step logits (behind a
    prefill of a 2 s clip) and 8 greedy tokens bit-equal to the defaults'"""
    pcm = qasr.synth_pcm(19000, 2 * SR)
    c = qasr.Context(model, max_batch=1, max_ctx=160)
    try:
        feats = c.encode(c.mel([pcm]))[0]
        ids, pos = model.build_prompt(feats.shape[0])

        def run():
            c.prefill([ids], [feats], [pos], want_logits=False)
            lg, _ = c.decode_step([1234], [len(ids)])
            assert c.get_option("fused_mode") == 2
            lg = lg.copy()
            return lg, c.transcribe([pcm], max_tokens=8, ignore_eos=True).tokens
        default = c.get_option(name)
        base = run()
        alt = {}
        for val in ORDER_CASES[name]:
            c.set_option(name, val)
            assert c.get_option(name) == val
            alt[val] = run()
        c.set_option(name, default)
    finally:
        c.close()
    assert np.isfinite(base[0]).all() and len(base[1][0]) == 8
    for val, (lg, toks) in alt.items():
        assert np.array_equal(lg, base[0]), (name, val, float(np.abs(lg - base[0]).max()))
        assert toks == base[1], (name, val)
