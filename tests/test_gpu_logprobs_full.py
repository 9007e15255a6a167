"""Token log-probabilities at the Qwen3-ASR-0.6B dimensions (synthetic f16):
the fused variant of the one-launch LM head (lmhead.hip, LSE = true), which
needs the 1024-wide hidden size.

One model, one oracle, one 1.1 s clip.  Bars as in test_gpu_logprobs.py:
2e-5 absolute against the float64 log-sum-exp of the row's own logits,
2 * delta against the oracle (delta = the step's measured max |logits_gpu -
logits_oracle|), and 4e-5 between the fused value and the stand-alone kernel's
on the fallback GEMM (two values each within 2e-5 of the same logits' float64
one: the two paths' logits are bit-identical)."""
import os

import numpy as np
import pytest

import oracle_py as op
import qasr

pytestmark = pytest.mark.gpu
SR = 16000
SELF_BAR = 2e-5
N_STEPS = 3


def lp64(logits, tok):
    v = np.asarray(logits, np.float64)
    m = v.max()
    return float(v[tok] - (m + np.log(np.exp(v - m).sum())))


@pytest.fixture(scope="module")
def full(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    op.set_threads(min(16, os.cpu_count() or 1))
    om = op.OracleModel(full_f16_gguf)
    pcm = qasr.synth_pcm(9300, int(1.1 * SR))
    feats = om.encode(op.log_mel(pcm))
    ids, pos = m.build_prompt(feats.shape[0])
    yield {"m": m, "om": om, "pcm": pcm, "feats": feats, "ids": ids, "pos": pos, "oracle": {}}
    m.close()


def oracle_logits(full, toks):
    """the oracle's logits at the prefill and after each of toks[:-1], teacher-forced;
    computed once per token sequence (every batch size gives the same one)"""
    key = tuple(int(t) for t in toks)
    if key not in full["oracle"]:
        d = op.OracleDecoder(full["om"], 128)
        ids = full["ids"]
        out = [d.forward(ids, 0, full["feats"], full["pos"])]
        for k, t in enumerate(key[:-1]):
            out.append(d.forward([t], len(ids) + k))
        full["oracle"][key] = out
    return full["oracle"][key]


def stepwise(c, full, B, n_steps, want_logits=True):
    """prefill + n_steps greedy steps of B copies -> per step (row 0's logits or None, tokens, step_logprobs)"""
    ids, feats, pos = full["ids"], full["feats"], full["pos"]
    lg, am = c.prefill([ids] * B, [feats] * B, [pos] * B, want_logits=want_logits)
    out = [(lg[0].copy() if want_logits else None, am.copy(), c.step_logprobs(B))]
    n_past = np.full(B, len(ids), np.int32)
    for _ in range(n_steps):
        lg, am = c.decode_step(am, n_past, want_logits=want_logits)
        out.append((lg[0].copy() if want_logits else None, am.copy(), c.step_logprobs(B)))
        n_past = n_past + 1
    return out


@pytest.mark.parametrize("B", [9, 64, 65, 128])
def test_full_fused_logprobs(full, parity, B):
    """9: one row tile with rows past M; 64: four tiles; 65: the register-row
    kernel with empty waves; 128: that kernel full.  Prefill (tiled GEMM + the
    stand-alone kernel) and 3 decode steps (the fused LM head), logits requested."""
    c = qasr.Context(full["m"], max_batch=B, max_ctx=128)
    try:
        c.set_option("token_logprobs", 1)
        fused = stepwise(c, full, B, N_STEPS)
        again = stepwise(c, full, B, N_STEPS)
        c.set_option("lmh", 0)   # the fallback GEMM + the stand-alone kernel: the logits round trip
        plain = stepwise(c, full, B, N_STEPS)
    finally:
        c.close()
    toks = [int(s[1][0]) for s in fused]
    ora = oracle_logits(full, toks)
    w_self = w_fb = w_ora = 0.0
    for k, ((lg, am, lp), (_, am2, lp2), (lgp, amp, lpp)) in enumerate(zip(fused, again, plain)):
        assert (am == am[0]).all() and (lp.view(np.uint32) == lp.view(np.uint32)[0]).all(), k   # rows bit-identical
        assert np.array_equal(am, am2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)), k   # deterministic
        assert np.array_equal(am, amp), k
        e_self = abs(float(lp[0]) - lp64(lg, am[0]))
        e_fb = float(np.abs(lp.astype(np.float64) - lpp.astype(np.float64)).max())
        delta = float(np.abs(lg.astype(np.float64) - ora[k]).max())
        e_ora = abs(float(lp[0]) - lp64(ora[k], am[0]))
        print(f"B={B} step {k}: self {e_self:.3g}  fused-fallback {e_fb:.3g}  oracle {e_ora:.3g} (delta {delta:.3g})")
        w_self, w_fb, w_ora = max(w_self, e_self), max(w_fb, e_fb), max(w_ora, e_ora / (2 * delta))
        assert e_self <= SELF_BAR, (k, e_self)
        assert e_fb <= 4e-5, (k, e_fb)
        assert e_ora <= 2 * delta, (k, e_ora, delta)
    parity(f"full_logprobs_B{B}", self_abs_max=w_self, fused_vs_fallback_abs_max=w_fb, oracle_over_bound=w_ora)


def test_full_fused_logprobs_without_logits(full):
    """transcribe of 64 copies with no logits requested anywhere: the decode
    steps are the fused LM head alone (nothing written to the logits buffer);
    values equal the stepwise fused ones bit for bit, tokens the option-off run's"""
    pcm, B = full["pcm"], 64
    c = qasr.Context(full["m"], max_batch=B, max_ctx=128)
    try:
        c.set_option("token_logprobs", 1)
        r = c.transcribe([pcm] * B, max_tokens=6, ignore_eos=True)
        feats = c.encode(c.mel([pcm] * B))
        ids, pos = full["m"].build_prompt(feats[0].shape[0])
        lg, am = c.prefill([ids] * B, feats, [pos] * B, want_logits=False)
        steps = [(am.copy(), c.step_logprobs(B))]
        n_past = np.full(B, len(ids), np.int32)
        for _ in range(5):
            lg, am = c.decode_step(am, n_past, want_logits=False)
            steps.append((am.copy(), c.step_logprobs(B)))
            n_past = n_past + 1
        c.set_option("token_logprobs", 0)
        off = c.transcribe([pcm] * B, max_tokens=6, ignore_eos=True)
    finally:
        c.close()
    assert off.tokens == r.tokens and off.logprobs is None
    for b in range(B):
        assert [int(s[0][b]) for s in steps] == r.tokens[b]
        assert np.array_equal(np.array([s[1][b] for s in steps], np.float32).view(np.uint32),
                              np.array(r.logprobs[b], np.float32).view(np.uint32)), b


def test_full_batch1_transcribe_logprobs_match_oracle(full, parity):
    """batch 1 (the GEMV LM head + the stand-alone kernel inside the captured
    step): transcribe's values within 2 * delta of the oracle's, delta from the
    logits of the same steps replayed through prefill + decode_step"""
    m, om = full["m"], full["om"]
    pcm = qasr.synth_pcm(12000, 2 * SR)
    c = qasr.Context(m, max_batch=1, max_ctx=256)
    try:
        c.set_option("token_logprobs", 1)
        r = c.transcribe([pcm], max_tokens=8, ignore_eos=True)
        feats_g = c.encode(c.mel([pcm]))
        ids, pos = m.build_prompt(feats_g[0].shape[0])
        lg, am = c.prefill([ids], feats_g, [pos])
        gl = [lg[0].copy()]
        for k, t in enumerate(r.tokens[0][:-1]):
            lg, am = c.decode_step([t], [len(ids) + k])
            gl.append(lg[0].copy())
    finally:
        c.close()
    feats = om.encode(op.log_mel(pcm))
    d = op.OracleDecoder(om, 256)
    lo = d.forward(ids, 0, feats, pos)
    worst = 0.0
    for k, t in enumerate(r.tokens[0]):
        assert int(np.argmax(gl[k])) == t, k   # the replay is the run
        delta = float(np.abs(gl[k].astype(np.float64) - lo).max())
        err = abs(r.logprobs[0][k] - lp64(lo, t))
        print(f"step {k}: |lp - oracle| = {err:.3g}, delta = {delta:.3g}")
        worst = max(worst, err / (2 * delta))
        assert err <= 2 * delta, (k, err, delta)
        lo = d.forward([t], len(ids) + k)
    parity("full_logprobs_batch1_transcribe", oracle_over_bound=worst)
