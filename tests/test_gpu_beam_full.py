"""Beam search at the Qwen3-ASR-0.6B dimensions (synthetic f16, 5 s clips): the
device loop of qasr_run against the host loop of beam_util.py over the stage
calls, bit for bit.  W = 4 with one clip runs the batch <= 8 GEMV path; W = 2
with 5 clips runs 10 rows, the one-launch LM head with its fused top-K (K = 2)."""
import pytest

import qasr
from beam_util import host_beam, same_hyps

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
SR = 16000


@pytest.fixture(scope="module")
def full(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    yield m
    m.close()


@pytest.mark.parametrize("W,n_clips,max_tokens", [(4, 1, 6), (2, 5, 4)])
def test_full_device_loop_equals_host_loop(full, W, n_clips, max_tokens):
    pcms = [qasr.synth_pcm(9900 + i, 5 * SR + 3200 * i) for i in range(n_clips)]
    c = qasr.Context(full, max_batch=W * n_clips, max_ctx=256)
    try:
        want = host_beam(c, pcms, W, max_tokens, True)
        c.set_option("beam_width", W)
        r = c.transcribe(pcms, max_tokens=max_tokens, ignore_eos=True)
        again = c.transcribe(pcms, max_tokens=max_tokens, ignore_eos=True)
    finally:
        c.close()
    for g, (hyps, _) in enumerate(want):
        same_hyps(r.beams[g], hyps)
        same_hyps(again.beams[g], hyps)
        assert len(hyps) == W and r.tokens[g] == hyps[0].tokens and len(r.tokens[g]) == max_tokens
