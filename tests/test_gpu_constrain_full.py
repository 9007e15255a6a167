"""Decoding constraints at the Qwen3-ASR-0.6B dimensions (synthetic f16): the device loop of qasr_run against the
host loop over the stage calls and both against the rule on the raw logits, bit for bit.  2 rows run the GEMV LM
head and 9 rows the one-launch LM head, with the logits store forced and launch_token_logprob / the top-K row
kernel in place of its fused groups."""
import numpy as np
import pytest

import qasr
from test_gpu_constrain import bits, check_against_rule, stage_loop, turn_on

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
SR = 16000


@pytest.fixture(scope="module")
def full(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    yield m
    m.close()


@pytest.mark.parametrize("rule", [dict(n=2), dict(p=1.3)], ids=["n2", "p1.3"])
@pytest.mark.parametrize("B", [2, 9])
def test_full_device_loop_equals_host_loop_equals_rule(full, B, rule):
    pcms = [qasr.synth_pcm(9900 + i, SR + 1600 * (i % 4)) for i in range(B)]
    c = qasr.Context(full, max_batch=B, max_ctx=128)
    try:
        c.set_option("token_logprobs", 1)
        c.set_option("top_k", 2)
        turn_on(c, **rule)
        toks, edited = stage_loop(c, pcms, 8)
        r = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        again = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert r.tokens == toks and again.tokens == toks
        assert np.array_equal(bits(r.logprobs), bits(again.logprobs))
        assert all(r.topk[b][0][:, 0].tolist() == toks[b] for b in range(B))
        in_E = check_against_rule(c, pcms, toks, edited, rule)
        print(f"full B={B} {rule}: rows with the raw argmax edited per step {in_E}")
    finally:
        c.close()
