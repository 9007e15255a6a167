"""Token log-probabilities (context option "token_logprobs") on the tiny model.

Its hidden width is 256, so every path here takes the stand-alone row kernel
(token_logprob_kernel over the fp32 logits): batch <= 8 decode, batches on the
fallback GEMM, and every prefill.  The one-launch LM head's fused variant is
covered at full size in test_gpu_logprobs_full.py.

Bars:
  self-consistency 2e-5 absolute against the float64 logit[argmax] - logsumexp
      of the logits the same call returned: a CPU simulation of the per-lane
      fp32 online scheme gave at most 1.3e-6 over 151,936-wide rows (logit
      standard deviations 0.5 .. 8 and one peaked row); 2e-5 is ~15x that and
      three orders below the logit disagreement with the oracle, so it tells a
      dropped or double-counted column from rounding.
  oracle 2 * delta, delta = that step's measured max |logits_gpu - logits_oracle|:
      the chosen logit and the log-sum-exp each move by at most delta.
  streams 2 * 1e-2 * max |oracle logits|: 1e-2 of the scale is the logit bar
      test_gpu_parity.py holds for this model.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as op
import qasr

pytestmark = pytest.mark.gpu
SR = 16000
SELF_BAR = 2e-5
QASR_ERR_STATE = 5


def lp64(logits, tok):
    """float64 log softmax(logits)[tok]"""
    v = np.asarray(logits, np.float64)
    m = v.max()
    return float(v[tok] - (m + np.log(np.exp(v - m).sum())))


@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=12, max_ctx=640)
    c.set_option("token_logprobs", 1)
    yield m, c
    c.close()
    m.close()


_CLIPS = {}


def clip(tiny_oracle, i):
    """clip i (ragged lengths): pcm and the oracle's features / prompt, computed once"""
    if i not in _CLIPS:
        pcm = qasr.synth_pcm(8100 + i, SR + 1733 * i)
        feats = tiny_oracle.encode(op.log_mel(pcm))
        _CLIPS[i] = (pcm, feats, tiny_oracle.prompt(feats.shape[0]))
    return _CLIPS[i]


def stepwise(c, ids, feats, n_steps, want_logits=True):
    """prefill + n_steps greedy steps -> per step (logits or None, tokens, step_logprobs)"""
    B = len(ids)
    lg, am = c.prefill(ids, feats, [9] * B, want_logits=want_logits)
    out = [(lg, am.copy(), c.step_logprobs(B))]
    n_past = np.array([len(x) for x in ids], np.int32)
    for _ in range(n_steps):
        lg, am = c.decode_step(am, n_past, want_logits=want_logits)
        out.append((lg, am.copy(), c.step_logprobs(B)))
        n_past = n_past + 1
    return out


@pytest.mark.parametrize("B", [1, 3, 12])
def test_step_logprobs_match_own_logits(tiny, tiny_oracle, parity, B):
    """prefill (GEMV at B <= 8, tiled GEMM above) and 4 decode steps (the GEMV
    with fused bookkeeping at B <= 8, the fallback GEMM at 12): the device value
    against the float64 one of the logits the same call returned"""
    _, c = tiny
    cl = [clip(tiny_oracle, i % 5) for i in range(B)]
    worst = 0.0
    for lg, am, lp in stepwise(c, [x[2] for x in cl], [x[1] for x in cl], 4):
        assert np.array_equal(am, lg.argmax(axis=1))
        for b in range(B):
            worst = max(worst, abs(float(lp[b]) - lp64(lg[b], am[b])))
    print(f"B={B} max |lp - lp64| = {worst:.3g}")
    parity(f"tiny_logprobs_self_B{B}", abs_max=worst, bar=SELF_BAR)
    assert worst <= SELF_BAR, worst


def test_step_logprobs_match_oracle(tiny, tiny_oracle, parity):
    """teacher-forced with the GPU's tokens: |lp_gpu - lp_oracle(gpu token)| <= 2 delta"""
    _, c = tiny
    cl = [clip(tiny_oracle, i) for i in range(3)]
    steps = stepwise(c, [x[2] for x in cl], [x[1] for x in cl], 4)
    ratio = 0.0
    for b, (_, feats, ids) in enumerate(cl):
        d = op.OracleDecoder(tiny_oracle, 512)
        lo = d.forward(ids, 0, feats, 9)
        for k, (lg, am, lp) in enumerate(steps):
            delta = float(np.abs(lg[b].astype(np.float64) - lo).max())
            err = abs(float(lp[b]) - lp64(lo, am[b]))
            print(f"row {b} step {k}: |lp - oracle| = {err:.3g}, delta = {delta:.3g}")
            ratio = max(ratio, err / (2 * delta))
            assert err <= 2 * delta, (b, k, err, delta)
            lo = d.forward([int(am[b])], len(ids) + k)
    parity("tiny_logprobs_oracle", worst_over_bound=ratio)


@pytest.mark.parametrize("B", [1, 3])
def test_transcribe_logprobs_equal_stepwise(tiny, B):
    """RunResult.logprobs (the captured decode graph, logits not requested by the
    caller) against prefill + decode_step on the same context, bit for bit"""
    _, c = tiny
    pcms = [qasr.synth_pcm(8200 + i, SR + 977 * i) for i in range(B)]
    r = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
    assert [len(x) for x in r.logprobs] == [len(t) for t in r.tokens] == [8] * B
    feats = c.encode(c.mel(pcms))
    ids = [c.model.build_prompt(f.shape[0])[0] for f in feats]
    steps = stepwise(c, ids, feats, 7)
    for b in range(B):
        assert [int(s[1][b]) for s in steps] == r.tokens[b]
        assert np.array_equal(np.array([s[2][b] for s in steps], np.float32), np.array(r.logprobs[b], np.float32)), b
    assert all(v <= 0.0 for row in r.logprobs for v in row)


def test_natural_eos_lengths_and_prefix(tiny):
    """ignore_eos=False: a popped trailing EOS drops its value too, and what
    remains is the prefix of the ignore_eos run"""
    _, c = tiny
    pcms = [qasr.synth_pcm(8300 + i, SR + 611 * i) for i in range(3)]
    r = c.transcribe(pcms, max_tokens=12, ignore_eos=False)
    full = c.transcribe(pcms, max_tokens=12, ignore_eos=True)
    for b in range(3):
        n = len(r.tokens[b])
        assert len(r.logprobs[b]) == n and 151645 not in r.tokens[b]
        assert r.tokens[b] == full.tokens[b][:n] and r.logprobs[b] == full.logprobs[b][:n]
    # run_staged returns them too, for the rows it ran
    c.stage_audio(pcms)
    rs = c.run_staged([2, 0], max_tokens=12, ignore_eos=True)
    assert rs.tokens == [full.tokens[2], full.tokens[0]] and rs.logprobs == [full.logprobs[2], full.logprobs[0]]


# ------------------------------------------------------------------ streams
N_STREAM = 10
BUDGETS = [3, 9, 5, 7, 1, 6, 8, 4, 9, 2]


def _stream_clip(i):
    return qasr.synth_pcm(8400 + i, SR // 2 + 2311 * i)


@pytest.fixture(scope="module")
def stream_ref(tiny, tiny_oracle):
    """per clip, once: the single-clip transcribe tokens (option on) and the
    oracle's teacher-forced log-probabilities of them, with the oracle's logit scale"""
    m, _ = tiny
    ref = []
    c1 = qasr.Context(m, max_batch=1, max_ctx=640)
    try:
        c1.set_option("token_logprobs", 1)
        for i in range(N_STREAM):
            pcm = _stream_clip(i)
            toks = c1.transcribe([pcm], max_tokens=BUDGETS[i], ignore_eos=True).tokens[0]
            feats = tiny_oracle.encode(op.log_mel(pcm))
            ids = tiny_oracle.prompt(feats.shape[0])
            d = op.OracleDecoder(tiny_oracle, 512)
            lo = d.forward(ids, 0, feats, 9)
            lps, scale = [], 0.0
            for k, t in enumerate(toks):
                lps.append(lp64(lo, t))
                scale = max(scale, float(np.abs(lo).max()))
                if k + 1 < len(toks):
                    lo = d.forward([t], len(ids) + k)
            ref.append((toks, lps, scale))
    finally:
        c1.close()
    return ref


def _queue(items):
    it = iter(items)
    return lambda: next(it, None)


STREAM_CASES = {
    "slots4": (4, {}, False),
    "slots4_staged": (4, {}, True),
    "slots4_refill_group2": (4, {"refill_group": 2}, False),
    "slots12_live_prefix": (12, {"live_prefix": 1}, False),
    # decode chunks narrower than the slots (16 of 20 rows): the rows past them are not read back
    "slots20_live_prefix_refill_group3_staged": (20, {"live_prefix": 1, "refill_group": 3}, True),
}


@pytest.mark.parametrize("case", list(STREAM_CASES))
def test_stream_logprobs(tiny, stream_ref, parity, case):
    m, _ = tiny
    slots, opts, staged = STREAM_CASES[case]
    clips = [_stream_clip(i) for i in range(N_STREAM)]
    c = qasr.Context(m, max_batch=slots, max_ctx=640)
    try:
        c.set_option("token_logprobs", 1)
        for k, v in opts.items():
            c.set_option(k, v)

        def run():
            if staged:
                c.stage_audio(clips)
                return c.run_stream_staged(_queue([(i, BUDGETS[i]) for i in range(N_STREAM)]), max_tokens=16, ignore_eos=True,
                                           logprobs=True)[0]
            return c.run_stream(_queue([(i, clips[i], BUDGETS[i]) for i in range(N_STREAM)]), max_tokens=16, ignore_eos=True,
                                logprobs=True)[0]
        out, again = run(), run()
        # the default return shape is unchanged
        plain = c.run_stream(_queue([(0, clips[0], BUDGETS[0])]), max_tokens=16, ignore_eos=True)[0]
    finally:
        c.close()
    assert sorted(out) == list(range(N_STREAM)) and plain[0] == stream_ref[0][0]
    worst = 0.0
    for i, (toks, lps, scale) in enumerate(stream_ref):
        t, lp = out[i]
        assert t == toks and len(lp) == len(toks) == BUDGETS[i], i
        err = float(np.abs(np.array(lp, np.float64) - np.array(lps)).max())
        worst = max(worst, err / (2e-2 * scale))
        assert err <= 2e-2 * scale, (i, err, scale)
        assert again[i][0] == t and again[i][1] == lp, i   # bit-identical across runs
    parity(f"tiny_logprobs_stream_{case}", worst_over_bound=worst)


def test_option_off_again(tiny):
    """off: the getters report QASR_ERR_STATE, results carry no log-probs, and
    the tokens are the on-run's"""
    m, _ = tiny
    pcms = [qasr.synth_pcm(8500 + i, SR + 500 * i) for i in range(3)]
    c = qasr.Context(m, max_batch=3, max_ctx=640)
    try:
        lib, buf = qasr.lib(), (C.c_float * 64)()
        assert lib.qasr_get_logprobs(c.h, buf, 3, 8) == QASR_ERR_STATE   # off, nothing has run
        c.set_option("token_logprobs", 1)
        assert lib.qasr_get_logprobs(c.h, buf, 3, 8) == QASR_ERR_STATE   # on, nothing has run
        assert lib.qasr_get_step_logprobs(c.h, buf, 3) == QASR_ERR_STATE
        assert lib.qasr_stream_logprobs(c.h, buf, 64) == -QASR_ERR_STATE  # outside a sink call
        on = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert lib.qasr_get_logprobs(c.h, buf, 3, 8) == 0
        assert lib.qasr_get_logprobs(c.h, buf, 2, 8) == 1 and lib.qasr_get_logprobs(c.h, buf, 3, 7) == 1   # short: QASR_ERR_ARG
        assert lib.qasr_get_logprobs(c.h, None, 3, 8) == 1
        s_on = c.run_stream(_queue([(i, p, 5) for i, p in enumerate(pcms)]), max_tokens=8, ignore_eos=True, logprobs=True)[0]
        c.set_option("token_logprobs", 0)
        assert lib.qasr_get_logprobs(c.h, buf, 3, 8) == QASR_ERR_STATE
        assert lib.qasr_get_step_logprobs(c.h, buf, 3) == QASR_ERR_STATE
        off = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert off.logprobs is None and on.logprobs is not None and off.tokens == on.tokens
        s_off = c.run_stream(_queue([(i, p, 5) for i, p in enumerate(pcms)]), max_tokens=8, ignore_eos=True)[0]
        assert {i: t for i, (t, _) in s_on.items()} == s_off
        with pytest.raises(qasr.QasrError):
            c.run_stream(_queue([(0, pcms[0], 3)]), max_tokens=8, ignore_eos=True, logprobs=True)
    finally:
        c.close()
