"""Audio at other sample rates through the engine (tiny model): Context.resample against the rule,
clips staged with a rate against the same clips resampled in NumPy and staged at 16 kHz (tokens, log-probabilities
and mel bit for bit), the unchanged 16 kHz path, the stream with rates, scoring over a pool staged with rates, the
error cases and the CLI's --resample."""
import os
import subprocess

import numpy as np
import pytest

import qasr
import resample_util as ru

pytestmark = pytest.mark.gpu
f32 = np.float32
NTOK = 8


@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=4, max_ctx=640)
    c.set_option("token_logprobs", 1)
    yield m, c
    c.close()
    m.close()


@pytest.fixture(scope="module")
def raw():
    """(clips, rates, the clips resampled to 16 kHz by the rule with the library's tables), computed once"""
    rates = [48000, 44100, 8000, 16000]
    lens = [48000 + 123, 2 * 44100 + 7, 8000 + 55, 16000 + 9]   # about 1, 2, 1, 1 s
    clips = [qasr.synth_pcm(9100 + i, n) for i, n in enumerate(lens)]
    want = [ru.resample(x, sr, qasr.resample_taps(sr)) for x, sr in zip(clips, rates)]
    return clips, rates, want


def _same(a, b):
    return len(a) == len(b) and bool((ru.bits(a) == ru.bits(b)).all())


def test_context_resample_equals_the_rule(tiny, raw):
    _m, c = tiny
    clips, rates, want = raw
    got = c.resample(clips + [np.zeros(0, f32)], rates + [11025])
    assert len(got) == 5 and len(got[4]) == 0
    for y, w in zip(got, want):
        assert _same(y, w)
    assert _same(got[3], clips[3])   # 16 kHz: a copy
    # the mel of the device's clips is the mel of NumPy's
    for a, b in zip(c.mel(got[:2]), c.mel(want[:2])):
        assert a.shape == b.shape and (ru.bits(a.ravel()) == ru.bits(b.ravel())).all()


def test_staged_with_rates_equals_numpy_resampled(tiny, raw):
    _m, c = tiny
    clips, rates, want = raw
    a = c.transcribe(clips[:2], max_tokens=NTOK, ignore_eos=True, rates=rates[:2])   # 48000 and 44100
    b = c.transcribe(want[:2], max_tokens=NTOK, ignore_eos=True)
    assert a.tokens == b.tokens and a.logprobs == b.logprobs
    # the whole mixed batch, and a subset of the pool it leaves (qasr_run_staged serves it unchanged)
    c.stage_audio(clips, rates)
    a4 = c.run(NTOK, ignore_eos=True)
    sub = c.run_staged([2, 0], NTOK, ignore_eos=True)
    c.stage_audio(want)
    b4 = c.run(NTOK, ignore_eos=True)
    assert a4.tokens == b4.tokens and a4.logprobs == b4.logprobs
    assert sub.tokens == [b4.tokens[2], b4.tokens[0]]


def test_no_rates_and_all_16000_are_todays_path(tiny):
    _m, c = tiny
    clips = [qasr.synth_pcm(9200 + i, 16000 + 311 * i) for i in range(3)]
    base = c.transcribe(clips, max_tokens=NTOK, ignore_eos=True)
    none = c.transcribe(clips, max_tokens=NTOK, ignore_eos=True, rates=None)
    same = c.transcribe(clips, max_tokens=NTOK, ignore_eos=True, rates=[16000] * 3)
    assert base.tokens == none.tokens == same.tokens and base.logprobs == none.logprobs == same.logprobs
    x = np.array([0.0, -0.0, 1e-45, -1.5, 3.0e38], f32)
    assert _same(c.resample([x], [16000])[0], x)


def test_stream_with_rates_equals_clip_by_clip(tiny, raw):
    _m, c = tiny
    clips, rates, want = raw
    budgets = [5, 3, 7, 4]
    items = iter([(20 + i, x, sr, b) for i, (x, sr, b) in enumerate(zip(clips, rates, budgets))])
    out, st = c.run_stream(lambda: next(items, None), max_tokens=16, ignore_eos=True, slots=2, logprobs=True, with_rates=True)
    assert st.n_clips == 4 and st.n_errors == 0
    for i, (w, b) in enumerate(zip(want, budgets)):
        one = c.transcribe([w], max_tokens=b, ignore_eos=True)
        assert out[20 + i][0] == one.tokens[0] and out[20 + i][1] == one.logprobs[0], i


def test_score_over_a_pool_staged_with_rates(tiny, raw):
    _m, c = tiny
    clips, rates, want = raw
    hyps = [[5, 6, 7], [8, 9], [10, 11, 12, 13]]
    c.stage_audio(clips[:3], rates[:3])
    a = c.score([0, 1, 2], hyps)
    c.stage_audio(want[:3])
    b = c.score([0, 1, 2], hyps)
    for x, y in zip(a, b):
        assert (ru.bits(x.logprobs) == ru.bits(y.logprobs)).all() and x.sum == y.sum


def test_unsupported_rate_is_refused(tiny, raw):
    _m, c = tiny
    clips, _rates, want = raw
    with pytest.raises(qasr.QasrError, match="44101"):
        c.stage_audio(clips[:2], [48000, 44101])
    with pytest.raises(qasr.QasrError, match="44101"):
        c.resample(clips[:1], [44101])
    # in the stream the clip fails alone, the rate named through the sink
    items = iter([(0, clips[0], 48000, 3), (1, clips[1], 44101, 3), (2, clips[3], 16000, 3)])
    out, st = c.run_stream(lambda: next(items, None), max_tokens=8, ignore_eos=True, slots=2, with_rates=True)
    assert st.n_clips == 2 and st.n_errors == 1
    assert isinstance(out[1], qasr.QasrError) and "44101" in str(out[1])
    assert out[0] == c.transcribe([want[0]], max_tokens=3, ignore_eos=True).tokens[0]
    assert out[2] == c.transcribe([want[3]], max_tokens=3, ignore_eos=True).tokens[0]


def test_context_check_uses_the_resampled_length(tiny):
    """an 8 kHz clip doubles in length: its raw length's prompt fits the context, its resampled one does not"""
    m, _c = tiny
    budget = 4
    n_raw = 3 * 8000

    def prompt(n):
        return qasr.lib().qasr_prompt_len(qasr.encoder_frames(qasr.mel_frames(n)))
    p_raw, p_out = prompt(n_raw), prompt(ru.out_len(n_raw, 8000))
    assert p_raw + 2 < p_out
    c = qasr.Context(m, max_batch=2, max_ctx=p_raw + budget + 2)
    try:
        long8 = qasr.synth_pcm(9300, n_raw)
        short = qasr.synth_pcm(9301, 4000)
        items = iter([(0, long8, 8000, budget), (1, short, 8000, budget)])
        out, st = c.run_stream(lambda: next(items, None), max_tokens=budget, ignore_eos=True, with_rates=True)
        assert st.n_clips == 1 and st.n_errors == 1
        assert isinstance(out[0], qasr.QasrError) and "Context length exceeded" in str(out[0])
        assert len(out[1]) == budget
        # the same clip as 16 kHz samples of its raw length fits
        items = iter([(0, long8, 16000, budget)])
        out, st = c.run_stream(lambda: next(items, None), max_tokens=budget, ignore_eos=True, with_rates=True)
        assert st.n_errors == 0 and len(out[0]) == budget
        with pytest.raises(qasr.QasrError, match="Context length exceeded"):
            c.transcribe([long8], max_tokens=budget, ignore_eos=True, rates=[8000])
    finally:
        c.close()


def test_cli_resample_flag(tiny, tiny_gguf, tmp_path):
    """a 48 kHz WAV: the present error without --resample; with it, the text of the Python path fed the loaded samples"""
    m, c = tiny
    cli = os.path.join(os.path.dirname(qasr.LIB_PATH), "qwen3-asr-cli")
    wav = str(tmp_path / "clip48.wav")
    qasr.write_wav(wav, qasr.synth_pcm(9400, 48000 + 77), 48000)
    pcm, sr = qasr.load_wav(wav)   # (the file's 16-bit samples)
    assert sr == 48000
    want = c.transcribe([pcm], max_tokens=10, ignore_eos=False, rates=[sr]).tokens[0]
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(cli))
    base = [cli, "-m", tiny_gguf, "-f", wav, "--max-tokens", "10", "--no-timing"]
    bad = subprocess.run(base, capture_output=True, text=True, env=env, timeout=120)
    assert bad.returncode != 0 and "Audio must be 16kHz, got 48000 Hz" in bad.stderr, bad.stderr
    r = subprocess.run(base + ["--resample"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == m.detokenize(want) + "\n", (r.stdout, want)
    # two files, one of them at 16 kHz (the batch path): "bad audio" without the flag, both texts with it
    wav16 = str(tmp_path / "clip16.wav")
    qasr.write_wav(wav16, qasr.synth_pcm(9401, 16000 + 5), 16000)
    pcm16, _ = qasr.load_wav(wav16)
    two = [cli, "-m", tiny_gguf, "-f", wav, "-f", wav16, "--max-tokens", "10", "--no-timing"]
    bad = subprocess.run(two, capture_output=True, text=True, env=env, timeout=120)
    assert bad.returncode != 0 and "bad audio" in bad.stderr, bad.stderr
    r = subprocess.run(two + ["--resample"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    want16 = c.transcribe([pcm16], max_tokens=10, ignore_eos=False).tokens[0]
    assert r.stdout == m.detokenize(want) + "\n" + m.detokenize(want16) + "\n", r.stdout
