"""A 70 s recording at the default segmentation through transcribe_long on the full-size synthetic model
(DESIGN.md §5.9): the segment table equals the host rule, and every segment that is not silent decodes to the tokens
of its samples transcribed on their own."""
import numpy as np
import pytest

import qasr
import segment_util as su

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
f32 = np.float32
NTOK = 8


def test_seventy_seconds_at_the_defaults(gpu, full_f16_gguf):
    m = qasr.Model(full_f16_gguf)
    # the context of a max_frames clip plus the budget
    ctx = qasr.lib().qasr_prompt_len(qasr.encoder_frames(qasr.mel_frames(3000 * 160 + 159))) + NTOK
    c = qasr.Context(m, max_batch=4, max_ctx=ctx)
    try:
        n = 70 * 16000 + 91
        x = qasr.synth_pcm(7800, n)
        x = (x * (0.05 + np.abs(np.sin(np.arange(n) * (2 * np.pi / 300000.0))))).astype(f32)
        x[16000 * 20:16000 * 22] = 0.0   # digital silence inside the first window: s = 0 on frames 2005 .. 2194
        text, parts = c.transcribe_long(x, max_tokens=NTOK, ignore_eos=True, skip_ratio=1e-9)
        segs = [s for s, _ in parts]
        want = qasr.segment_host(x, skip_ratio=1e-9)
        assert [(s.start, s.n, su.bits(s.peak).item(), s.silent) for s in segs] == [(s.start, s.n, su.bits(s.peak).item(), s.silent) for s in want]
        assert 3 <= len(segs) <= 7 and all(1000 <= s.n // 160 <= 3000 for s in segs)
        assert segs[1].start == 2194 * 160   # the larger frame of the equal zeros
        for k, (s, toks) in enumerate(parts):
            if s.silent:
                assert toks == []
                continue
            one = c.transcribe([x[s.start:s.start + s.n]], max_tokens=NTOK, ignore_eos=True)
            assert toks == one.tokens[0], k
        assert text == " ".join(t for t in (m.detokenize(toks) for s, toks in parts if not s.silent) if t)
    finally:
        c.close()
        m.close()
