"""Top-K token alternatives at the Qwen3-ASR-0.6B dimensions (synthetic f16):
decode batches on the one-launch LM heads (lmhead.hip, 9..64 and 65..128 rows),
the fallback GEMM, and batch 1 inside the captured step.

One model, one 1.1 s clip, max_ctx 128.  Ids are exact against the logits the
same call returned; values within 2e-5 of their float64 ones, and within 4e-5
between two paths whose logits are bit-identical (test_gpu_logprobs_full.py)."""
import numpy as np
import pytest

import qasr
from topk_util import PATH_BAR, check_rows, write_tied_copy

pytestmark = pytest.mark.gpu
SR = 16000


@pytest.fixture(scope="module")
def full(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    pcm = qasr.synth_pcm(9300, int(1.1 * SR))
    c = qasr.Context(m, max_batch=1, max_ctx=128)
    try:
        feats = c.encode(c.mel([pcm]))[0]
        ids, pos = m.build_prompt(feats.shape[0])
        t = int(c.prefill([ids], [feats], [pos])[1][0])
    finally:
        c.close()
    yield {"m": m, "path": full_f16_gguf, "pcm": pcm, "feats": feats, "ids": ids, "pos": pos, "argmax": t}
    m.close()


def stepwise(c, full, B, want_logits=True, keep_logits=True):
    """prefill of B copies, one decode step that feeds row b the token 1000 + 37 b
    (every row's logits differ from there on), then 2 greedy steps ->
    per step (logits or None, tokens, (ids, lps)); keep_logits=False drops the logits it asked for"""
    ids, feats, pos = full["ids"], full["feats"], full["pos"]
    lg, am = c.prefill([ids] * B, [feats] * B, [pos] * B, want_logits=want_logits)
    out = [(lg if keep_logits else None, am.copy(), c.step_topk(B))]
    n_past = np.full(B, len(ids), np.int32)
    feed = np.array([1000 + 37 * b for b in range(B)], np.int32)
    for _ in range(3):
        lg, am = c.decode_step(feed, n_past, want_logits=want_logits)
        out.append((lg if keep_logits else None, am.copy(), c.step_topk(B)))
        feed, n_past = am, n_past + 1
    return out


@pytest.mark.parametrize("B,K", [(9, 8), (64, 8), (65, 8), (128, 8), (64, 1), (64, 3)])
def test_full_topk(full, parity, B, K):
    """9: one row tile with rows past M; 64: four tiles (both the fused top-K
    variant of lmhead_batch_kernel); 65 / 128: the register-row kernel, then the
    row kernel.  A second run is bit-identical; lmh_topk = 0 and lmh = 0 (the row
    kernel after the one-launch head / the fallback GEMM) give the same ids and
    values within 4e-5."""
    c = qasr.Context(full["m"], max_batch=B, max_ctx=128)
    try:
        c.set_option("top_k", K)
        c.set_option("lmh_topk", 2)   # the fused variant at every K (the default takes it only where it is the faster)
        first = stepwise(c, full, B)
        again = stepwise(c, full, B, keep_logits=False)
        c.set_option("lmh_topk", 0)   # the one-launch head writes its logits, the row kernel reads them
        rowk = stepwise(c, full, B, keep_logits=False)
        c.set_option("lmh", 0)
        plain = stepwise(c, full, B, keep_logits=False)
    finally:
        c.close()
    w_self = w_fb = 0.0
    for k, ((lg, am, (ids, lps)), (_, am2, (ids2, lps2)), (_, amp, (idsp, lpsp))) in enumerate(zip(first, again, plain)):
        w_self = max(w_self, check_rows(lg, am, ids, lps, K))
        if k >= 1:
            assert not np.array_equal(lg[0], lg[1]), k   # the rows' logits do differ: a row mix-up cannot hide
        assert np.array_equal(am, am2) and np.array_equal(ids, ids2), k
        assert np.array_equal(lps.view(np.uint32), lps2.view(np.uint32)), k
        assert np.array_equal(am, amp) and np.array_equal(ids, idsp), k
        e_fb = float(np.abs(lps.astype(np.float64) - lpsp.astype(np.float64)).max())
        w_fb = max(w_fb, e_fb)
        assert e_fb <= PATH_BAR, (k, e_fb)
        assert np.array_equal(am, rowk[k][1]) and np.array_equal(ids, rowk[k][2][0]), k
        assert float(np.abs(lps.astype(np.float64) - rowk[k][2][1].astype(np.float64)).max()) <= PATH_BAR, k
    print(f"B={B} K={K}: self {w_self:.3g}  lmh on/off {w_fb:.3g}")
    parity(f"full_topk_B{B}_K{K}", self_abs_max=w_self, lmh_vs_fallback_abs_max=w_fb)


def test_full_topk_without_logits(full):
    """transcribe of 64 copies, no logits requested by the caller: ids and values
    equal the stepwise want_logits=False ones bit for bit, tokens the option-off run's"""
    pcm, B, K = full["pcm"], 64, 8
    c = qasr.Context(full["m"], max_batch=B, max_ctx=128)
    try:
        c.set_option("top_k", K)
        c.set_option("lmh_topk", 2)   # the fused variant, nothing written to the logits buffer
        r = c.transcribe([pcm] * B, max_tokens=6, ignore_eos=True)
        feats = c.encode(c.mel([pcm] * B))
        ids, pos = full["m"].build_prompt(feats[0].shape[0])
        _, am = c.prefill([ids] * B, feats, [pos] * B, want_logits=False)
        steps = [(am.copy(), c.step_topk(B))]
        n_past = np.full(B, len(ids), np.int32)
        for _ in range(5):
            _, am = c.decode_step(am, n_past, want_logits=False)
            steps.append((am.copy(), c.step_topk(B)))
            n_past = n_past + 1
        c.set_option("top_k", 0)
        off = c.transcribe([pcm] * B, max_tokens=6, ignore_eos=True)
    finally:
        c.close()
    assert off.tokens == r.tokens and off.topk is None
    for b in range(B):
        assert [int(s[0][b]) for s in steps] == r.tokens[b]
        assert np.array_equal(np.stack([s[1][0][b] for s in steps]), r.topk[b][0]), b
        assert np.array_equal(np.stack([s[1][1][b] for s in steps]).view(np.uint32), r.topk[b][1].view(np.uint32)), b


def test_full_batch1_transcribe_topk(full):
    """batch 1 (the GEMV LM head + the row kernel inside the captured step): ids
    exact against the logits of the same steps replayed through prefill + decode_step"""
    m, K = full["m"], 8
    pcm = qasr.synth_pcm(12000, 2 * SR)
    c = qasr.Context(m, max_batch=1, max_ctx=256)
    try:
        c.set_option("top_k", K)
        r = c.transcribe([pcm], max_tokens=8, ignore_eos=True)
        feats = c.encode(c.mel([pcm]))
        ids, pos = m.build_prompt(feats[0].shape[0])
        lg, am = c.prefill([ids], feats, [pos])
        gl = [lg[0].copy()]
        for k, t in enumerate(r.tokens[0][:-1]):
            lg, am = c.decode_step([t], [len(ids) + k])
            gl.append(lg[0].copy())
    finally:
        c.close()
    got_ids, got_lps = r.topk[0]
    assert got_ids.shape == (8, K)
    for k, t in enumerate(r.tokens[0]):
        assert int(np.argmax(gl[k])) == t, k   # the replay is the run
        check_rows(gl[k][None], np.array([t]), got_ids[k][None], got_lps[k][None], K)


@pytest.fixture(scope="module")
def tied(full, tmp_path_factory):
    """the full model with embedding rows t + 1 (the same 16-column unit unless t % 16
    == 15), t + 16 (the same lane of the next unit) and (t + V / 2) % V (another
    workgroup's range) copies of row t, the unpatched prefill argmax"""
    t = full["argmax"]
    path = str(tmp_path_factory.mktemp("tied") / "full-tied.gguf")
    four = write_tied_copy(full["path"], path, t)
    assert not set(four) - {t} & set(int(x) for x in full["ids"]), (four, t)
    m = qasr.Model(path)
    yield m, four
    m.close()


@pytest.mark.parametrize("B", [9, 128])
def test_full_equal_logits_order_by_lower_id(full, tied, B):
    m, four = tied
    ids, feats, pos = full["ids"], full["feats"], full["pos"]
    c = qasr.Context(m, max_batch=B, max_ctx=128)
    try:
        c.set_option("top_k", 8)
        c.set_option("lmh_topk", 2)   # B = 9: the fused variant
        lg, am = c.prefill([ids] * B, [feats] * B, [pos] * B)
        steps = [(lg, am.copy(), c.step_topk(B))]
        lg, am = c.decode_step(am, np.full(B, len(ids), np.int32))
        steps.append((lg, am.copy(), c.step_topk(B)))
    finally:
        c.close()
    checked = 0
    for k, (lg, am, (tid, lps)) in enumerate(steps):
        check_rows(lg, am, tid, lps, 8)
        if k > 0 and int(am[0]) not in four:
            continue   # this step's argmax is elsewhere: the four columns need not lead
        for b in range(B):
            assert tid[b, :4].tolist() == four, (k, b, tid[b])
            assert len(set(lps[b, :4].view(np.uint32).tolist())) == 1, (k, b, lps[b])
        checked += 1
    assert checked >= 1   # (the prefill at least)
