"""Top-K token alternatives (context option "top_k") on the tiny model.

Its hidden width is 256, so every path here takes the stand-alone row kernel
(topk_rows_kernel over the fp32 logits): every prefill, batch <= 8 decode and
batches on the fallback GEMM.  The one-launch LM heads are covered at full
size in test_gpu_topk_full.py.

Ids carry no tolerance: the kernel compares fp32 values exactly, so they equal
np.argsort(-logits, kind="stable")[:K] of the logits the same call returned.
Float bars are those of test_gpu_logprobs.py: 2e-5 absolute against float64 of
the same call's logits, and for streams 2 * 1e-2 * max |oracle logits| against
the oracle's teacher-forced log softmax at the returned id.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as op
import qasr
from test_gpu_logprobs import BUDGETS, N_STREAM, STREAM_CASES, _queue, _stream_clip
from topk_util import check_rows, logsoftmax64, write_tied_copy

pytestmark = pytest.mark.gpu
SR = 16000
QASR_ERR_ARG, QASR_ERR_STATE = 1, 5


@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=12, max_ctx=640)
    c.set_option("token_logprobs", 1)
    yield m, c
    c.close()
    m.close()


def prompts(c, pcms):
    """the clips' features and prompts through the context's own front end"""
    feats = c.encode(c.mel(pcms))
    built = [c.model.build_prompt(f.shape[0]) for f in feats]
    return feats, [b[0] for b in built], [b[1] for b in built]


def stepwise(c, pcms, n_steps, want_logits=True, logprobs=True):
    """prefill + n_steps greedy steps -> per step (logits or None, tokens, (ids, lps), step_logprobs or None)"""
    B = len(pcms)
    feats, ids, pos = prompts(c, pcms)
    lg, am = c.prefill(ids, feats, pos, want_logits=want_logits)
    out = [(lg, am.copy(), c.step_topk(B), c.step_logprobs(B) if logprobs else None)]
    n_past = np.array([len(x) for x in ids], np.int32)
    for _ in range(n_steps):
        lg, am = c.decode_step(am, n_past, want_logits=want_logits)
        out.append((lg, am.copy(), c.step_topk(B), c.step_logprobs(B) if logprobs else None))
        n_past = n_past + 1
    return out


def ragged(B, seed=8600):
    return [qasr.synth_pcm(seed + i, SR + 1733 * (i % 5)) for i in range(B)]


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("B", [1, 3, 12])
def test_step_topk_matches_own_logits(tiny, parity, B, K):
    """prefill (GEMV at B <= 8, tiled GEMM above) and 4 decode steps (the GEMV with
    fused bookkeeping at B <= 8, the fallback GEMM at 12), token_logprobs on too"""
    _, c = tiny
    c.set_option("top_k", K)
    worst = 0.0
    for lg, am, (ids, lps), lp in stepwise(c, ragged(B), 4):
        assert np.array_equal(am, lg.argmax(axis=1))
        worst = max(worst, check_rows(lg, am, ids, lps, K))
        assert np.array_equal(lps[:, 0].view(np.uint32), lp.view(np.uint32))   # entry 0 is token_logprobs' value, bitwise
    print(f"B={B} K={K} max |lp - lp64| = {worst:.3g}")
    parity(f"tiny_topk_self_B{B}_K{K}", abs_max=worst, bar=2e-5)


def test_q8_step_topk_matches_own_logits(gpu, tiny_q8_gguf, parity):
    m = qasr.Model(tiny_q8_gguf)
    c = qasr.Context(m, max_batch=3, max_ctx=640)
    try:
        c.set_option("top_k", 8)
        c.set_option("token_logprobs", 1)
        worst = 0.0
        for lg, am, (ids, lps), lp in stepwise(c, ragged(3), 4):
            worst = max(worst, check_rows(lg, am, ids, lps, 8))
            assert np.array_equal(lps[:, 0].view(np.uint32), lp.view(np.uint32))
    finally:
        c.close()
        m.close()
    parity("tiny_q8_topk_self_B3_K8", abs_max=worst, bar=2e-5)


@pytest.mark.parametrize("B", [1, 3])
def test_transcribe_topk_equals_stepwise(tiny, B):
    """RunResult.topk (the captured decode graph, logits not requested by the
    caller) against prefill + decode_step on the same context, bit for bit"""
    _, c = tiny
    c.set_option("top_k", 8)
    pcms = [qasr.synth_pcm(8200 + i, SR + 977 * i) for i in range(B)]
    r = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
    assert [x[0].shape for x in r.topk] == [x[1].shape for x in r.topk] == [(8, 8)] * B
    steps = stepwise(c, pcms, 7, want_logits=False)
    for b in range(B):
        assert [int(s[1][b]) for s in steps] == r.tokens[b] == r.topk[b][0][:, 0].tolist()
        assert np.array_equal(np.stack([s[2][0][b] for s in steps]), r.topk[b][0]), b
        assert np.array_equal(np.stack([s[2][1][b] for s in steps]).view(np.uint32), r.topk[b][1].view(np.uint32)), b
        assert np.array_equal(r.topk[b][1][:, 0], np.array(r.logprobs[b], np.float32)), b


def test_natural_eos_lengths_and_prefix(tiny):
    """ignore_eos=False: a popped trailing EOS drops its alternatives too, and what
    remains is the prefix of the ignore_eos run; run_staged returns the rows it ran"""
    _, c = tiny
    c.set_option("top_k", 3)
    pcms = [qasr.synth_pcm(8300 + i, SR + 611 * i) for i in range(3)]
    r = c.transcribe(pcms, max_tokens=12, ignore_eos=False)
    full = c.transcribe(pcms, max_tokens=12, ignore_eos=True)
    for b in range(3):
        n = len(r.tokens[b])
        assert r.topk[b][0].shape == r.topk[b][1].shape == (n, 3) and 151645 not in r.tokens[b]
        assert r.tokens[b] == full.tokens[b][:n]
        assert np.array_equal(r.topk[b][0], full.topk[b][0][:n]) and np.array_equal(r.topk[b][1], full.topk[b][1][:n])
    c.stage_audio(pcms)
    rs = c.run_staged([2, 0], max_tokens=12, ignore_eos=True)
    assert rs.tokens == [full.tokens[2], full.tokens[0]]
    for got, b in zip(rs.topk, [2, 0]):
        assert np.array_equal(got[0], full.topk[b][0]) and np.array_equal(got[1], full.topk[b][1])


# ------------------------------------------------------------------ streams
@pytest.fixture(scope="module")
def stream_ref(tiny, tiny_oracle):
    """per clip, once: the single-clip transcribe tokens and, per step, the
    oracle's teacher-forced log softmax over the whole row, with its logit scale"""
    m, _ = tiny
    ref = []
    c1 = qasr.Context(m, max_batch=1, max_ctx=640)
    try:
        for i in range(N_STREAM):
            pcm = _stream_clip(i)
            toks = c1.transcribe([pcm], max_tokens=BUDGETS[i], ignore_eos=True).tokens[0]
            feats = tiny_oracle.encode(op.log_mel(pcm))
            ids = tiny_oracle.prompt(feats.shape[0])
            d = op.OracleDecoder(tiny_oracle, 512)
            lo = d.forward(ids, 0, feats, 9)
            rows, scale = [], 0.0
            for k, t in enumerate(toks):
                rows.append(logsoftmax64(lo))
                scale = max(scale, float(np.abs(lo).max()))
                if k + 1 < len(toks):
                    lo = d.forward([t], len(ids) + k)
            ref.append((toks, rows, scale))
    finally:
        c1.close()
    return ref


@pytest.mark.parametrize("case", list(STREAM_CASES))
def test_stream_topk(tiny, stream_ref, parity, case):
    m, _ = tiny
    slots, opts, staged = STREAM_CASES[case]
    K = 4
    clips = [_stream_clip(i) for i in range(N_STREAM)]
    c = qasr.Context(m, max_batch=slots, max_ctx=640)
    try:
        c.set_option("top_k", K)
        for k, v in opts.items():
            c.set_option(k, v)

        def run():
            if staged:
                c.stage_audio(clips)
                return c.run_stream_staged(_queue([(i, BUDGETS[i]) for i in range(N_STREAM)]), max_tokens=16, ignore_eos=True,
                                           topk=True)[0]
            return c.run_stream(_queue([(i, clips[i], BUDGETS[i]) for i in range(N_STREAM)]), max_tokens=16, ignore_eos=True,
                                topk=True)[0]
        out, again = run(), run()
        plain = c.run_stream(_queue([(0, clips[0], BUDGETS[0])]), max_tokens=16, ignore_eos=True)[0]   # the default shape
    finally:
        c.close()
    assert sorted(out) == list(range(N_STREAM)) and plain[0] == stream_ref[0][0]
    worst = 0.0
    for i, (toks, rows, scale) in enumerate(stream_ref):
        t, (ids, lps) = out[i]
        assert t == toks and ids.shape == lps.shape == (BUDGETS[i], K), i
        assert ids[:, 0].tolist() == t, i   # entry 0 is the delivered token
        for k in range(len(t)):
            err = float(np.abs(lps[k].astype(np.float64) - rows[k][ids[k]]).max())
            worst = max(worst, err / (2e-2 * scale))
            assert err <= 2e-2 * scale, (i, k, err, scale)
        assert again[i][0] == t and np.array_equal(again[i][1][0], ids), i
        assert np.array_equal(again[i][1][1].view(np.uint32), lps.view(np.uint32)), i   # bit-identical across runs
    parity(f"tiny_topk_stream_{case}", worst_over_bound=worst)


# --------------------------------------------------------------------- ties
@pytest.fixture(scope="module")
def tied(tiny, tiny_gguf, tmp_path_factory):
    """the tiny model with embedding rows t + 1, t + 16 and (t + V / 2) % V made
    copies of row t, t the unpatched model's prefill argmax for a fixed clip"""
    _, c = tiny
    pcm = qasr.synth_pcm(8700, SR + 500)
    c.set_option("top_k", 1)
    feats, ids, pos = prompts(c, [pcm])
    t = int(c.prefill(ids, feats, pos)[1][0])
    path = str(tmp_path_factory.mktemp("tied") / "tiny-tied.gguf")
    four = write_tied_copy(tiny_gguf, path, t)
    assert not set(four) - {t} & set(int(x) for x in ids[0]), (four, t)   # the copies are no prompt tokens
    m = qasr.Model(path)
    yield m, pcm, four
    m.close()


@pytest.mark.parametrize("B", [1, 12])
def test_equal_logits_order_by_lower_id(tied, B):
    m, pcm, four = tied
    c = qasr.Context(m, max_batch=B, max_ctx=640)
    try:
        c.set_option("top_k", 8)
        steps = stepwise(c, [pcm] * B, 1, logprobs=False)
    finally:
        c.close()
    checked = 0
    for k, (lg, am, (ids, lps), _) in enumerate(steps):
        check_rows(lg, am, ids, lps, 8)
        if k > 0 and int(am[0]) not in four:
            continue   # this step's argmax is elsewhere: the four columns need not lead
        for b in range(B):
            assert ids[b, :4].tolist() == four, (k, b, ids[b])
            assert len(set(lps[b, :4].view(np.uint32).tolist())) == 1, (k, b, lps[b])
        checked += 1
    assert checked >= 1   # (the prefill at least)


# ------------------------------------------------------------------- errors
def test_option_range_getters_and_tokens(tiny):
    m, _ = tiny
    pcms = [qasr.synth_pcm(8500 + i, SR + 500 * i) for i in range(3)]
    c = qasr.Context(m, max_batch=3, max_ctx=640)
    try:
        lib, ids, lps = qasr.lib(), (C.c_int32 * 512)(), (C.c_float * 512)()
        for bad in (9, -1):
            assert lib.qasr_ctx_set_option(c.h, b"top_k", bad) == QASR_ERR_ARG
        assert c.get_option("top_k") == 0
        assert lib.qasr_get_topk(c.h, ids, lps, 3, 8, 4) == QASR_ERR_STATE   # off, nothing has run
        c.set_option("top_k", 4)
        assert lib.qasr_get_topk(c.h, ids, lps, 3, 8, 4) == QASR_ERR_STATE   # on, nothing has run
        assert lib.qasr_get_step_topk(c.h, ids, lps, 3, 4) == QASR_ERR_STATE
        assert lib.qasr_stream_topk(c.h, ids, lps, 64, 4) == -QASR_ERR_STATE   # outside a sink call
        on = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert lib.qasr_get_topk(c.h, ids, lps, 3, 8, 4) == 0
        assert lib.qasr_get_topk(c.h, ids, lps, 3, 8, 3) == QASR_ERR_ARG     # K differs from the option
        assert lib.qasr_get_step_topk(c.h, ids, lps, 3, 8) == QASR_ERR_ARG
        assert lib.qasr_get_topk(c.h, ids, lps, 2, 8, 4) == QASR_ERR_ARG and lib.qasr_get_topk(c.h, ids, lps, 3, 7, 4) == QASR_ERR_ARG
        assert lib.qasr_get_topk(c.h, None, lps, 3, 8, 4) == QASR_ERR_ARG and lib.qasr_get_topk(c.h, ids, None, 3, 8, 4) == QASR_ERR_ARG
        assert lib.qasr_get_step_topk(c.h, None, lps, 3, 4) == QASR_ERR_ARG
        s_on = c.run_stream(_queue([(i, p, 5) for i, p in enumerate(pcms)]), max_tokens=8, ignore_eos=True, topk=True)[0]
        c.set_option("top_k", 0)
        assert lib.qasr_get_topk(c.h, ids, lps, 3, 8, 4) == QASR_ERR_STATE   # switched off
        assert lib.qasr_get_step_topk(c.h, ids, lps, 3, 4) == QASR_ERR_STATE
        off = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert off.topk is None and on.topk is not None and off.tokens == on.tokens
        s_off = c.run_stream(_queue([(i, p, 5) for i, p in enumerate(pcms)]), max_tokens=8, ignore_eos=True)[0]
        assert {i: t for i, (t, _) in s_on.items()} == s_off
        with pytest.raises(qasr.QasrError):
            c.run_stream(_queue([(0, pcms[0], 3)]), max_tokens=8, ignore_eos=True, topk=True)
    finally:
        c.close()
