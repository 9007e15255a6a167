"""Temperature sampling at the Qwen3-ASR-0.6B dimensions (synthetic f16): the device loop of qasr_run against
the host loop over the stage calls, bit for bit, with every draw checked against the logits its step returned.
9 rows and 65 rows run the two one-launch LM heads (up to 64 rows, up to 128) with the logits store forced and
launch_token_logprob in place of their fused log-sum-exp."""
import numpy as np
import pytest

import qasr
from test_gpu_sample import SEED, bits, host_loop

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
SR = 16000


@pytest.fixture(scope="module")
def full(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    yield m
    m.close()


@pytest.mark.parametrize("B,max_tokens", [(9, 4), (65, 3)])
def test_full_transcribe_equals_host_loop(full, B, max_tokens):
    pcms = [qasr.synth_pcm(9900 + i, SR + 1600 * (i % 4)) for i in range(B)]
    c = qasr.Context(full, max_batch=B, max_ctx=128)
    try:
        want_t, want_l = host_loop(c, pcms, 0.8, 0.05, SEED, list(range(B)), [0] * B, max_tokens)
        c.set_sampling(0.8, 0.05, SEED, 1)
        c.set_option("token_logprobs", 1)
        r = c.transcribe(pcms, max_tokens=max_tokens, ignore_eos=True)
        again = c.transcribe(pcms, max_tokens=max_tokens, ignore_eos=True)
    finally:
        c.close()
    assert r.tokens == want_t and again.tokens == want_t
    assert np.array_equal(bits(r.logprobs), bits(want_l)) and np.array_equal(bits(again.logprobs), bits(want_l))
    assert [s[0].tokens for s in r.samples] == want_t
