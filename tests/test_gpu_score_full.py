"""Teacher-forced scoring at full size (f16, hidden 1024): qasr_score of 2 clips x 4 hypotheses x 16 tokens
against the float64 log-softmax of qasr_prefill_chunk's own logits (three sampled entries of every sequence), run
twice.  That the rows go through the score head's kernel at this width is tests/test_gpu_score_kernel.py's tag
assertion at 151,936 x 1024; a declined launch fails the call, there is no other path."""
import numpy as np
import pytest

import qasr

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
SR = 16000
LSE_BAR = 2e-5   # the fp32 reduction's bar (tests/test_gpu_logprobs.py)
U = 2.0 ** -24


def bar_of(lg_chunk, lg_oneshot, K):
    """The entry and the logits it is compared with come from different launches of the same arithmetic:
    (a) the layers run as prompt + chunk here and in qasr_score, but the GEMM tiling follows the row count, and
    two tilings of the same rows move the logits; that movement is measured on the yardstick itself, delta =
    max |logits(prompt, then chunk) - logits(one prefill of the whole prefix)|, two existing paths;
    (b) the LM head sums the K products in another order (GEMV here, MFMA tiles in the score head): at most
    (K + 2) 2^-24 sum |a w| a logit, with sum |a w| -- not observable from outside -- taken as the row's largest
    |logit|.  The target's logit and the log-sum-exp each move by at most (a) + (b)."""
    delta = float(np.abs(lg_chunk.astype(np.float64) - lg_oneshot.astype(np.float64)).max())
    return LSE_BAR + 2 * (delta + (K + 2) * U * float(np.abs(lg_chunk).max())), delta


def lp64(logits, tok):
    v = np.asarray(logits, np.float64)
    m = v.max()
    return float(v[tok] - (m + np.log(np.exp(v - m).sum())))


def test_full_size_score(gpu, full_f16_gguf, parity):
    m = qasr.Model(full_f16_gguf)
    c = qasr.Context(m, max_batch=8, max_ctx=256)
    try:
        pcms = [qasr.synth_pcm(8600 + i, int(1.1 * SR)) for i in range(2)]
        rng = np.random.default_rng(11)
        clips = [0, 1, 0, 1, 0, 1, 0, 1]
        hyps = [rng.integers(0, 151643, 16).tolist() for _ in clips]
        c.stage_audio(pcms)
        a = c.score(clips, hyps, include_eos=True)
        b = c.score(clips, hyps, include_eos=True)
        for x, y in zip(a, b):
            assert x.logprobs.tobytes() == y.logprobs.tobytes() and x.greedy_ids.tobytes() == y.greedy_ids.tobytes()
            assert x.greedy_logprobs.tobytes() == y.greedy_logprobs.tobytes() and x.sum == y.sum
        feats = c.encode(c.mel(pcms))
        worst = w_err = w_delta = 0.0
        bars = []
        for s in range(len(clips)):   # three sampled entries of every sequence
            ids, pos = m.build_prompt(feats[clips[s]].shape[0])
            for k in (0, 3 + s, 16):   # entry k: the row after k tokens
                one, _ = c.prefill([list(ids) + hyps[s][:k]], [feats[clips[s]]], [pos])
                lg = one
                if k > 0:
                    c.prefill([ids], [feats[clips[s]]], [pos], want_logits=False)
                    lg, _ = c.prefill_chunk([hyps[s][:k]], [len(ids)])
                bar, delta = bar_of(lg[0], one[0], m.hp.hidden_size)
                tg = hyps[s][k] if k < 16 else m.hp.eos_id
                err = abs(float(a[s].logprobs[k]) - lp64(lg[0], tg))
                gerr = abs(float(a[s].greedy_logprobs[k]) - lp64(lg[0], int(np.argmax(lg[0]))))
                print(f"sequence {s} entry {k}: |lp - lp64(own logits)| {err:.3g}, greedy {gerr:.3g} (bar {bar:.3g}, delta {delta:.3g})")
                worst, w_err, w_delta = max(worst, err / bar, gerr / bar), max(w_err, err, gerr), max(w_delta, delta)
                bars.append(bar)
                assert err <= bar and gerr <= bar, (s, k, err, gerr, bar)
        print(f"24 entries: worst error {w_err:.3g}, bars {min(bars):.3g} .. {max(bars):.3g}, largest delta {w_delta:.3g}")
        parity("full_score_own_logits", worst_over_bar=worst, abs_max=w_err, bar_min=min(bars), bar_max=max(bars), delta_max=w_delta)
    finally:
        c.close()
        m.close()

