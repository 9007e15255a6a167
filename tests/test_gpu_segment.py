"""Long recordings through the engine (tiny model): the table qasr_stage_long leaves against the host
rule, the zero-copy pool entries against the same samples staged on their own (tokens and log-probability bits), the
staged stream over the pool, a 48 kHz recording, two recordings in one call, the silent flag and transcribe_long, and
the error cases."""
import ctypes as C

import numpy as np
import pytest

import qasr
import segment_util as su

pytestmark = pytest.mark.gpu
f32 = np.float32
NTOK = 6
QASR_ERR_ARG, QASR_ERR_STATE = 1, 5
PRM = dict(max_frames=100, min_frames=40, smooth_half=5)


@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=4, max_ctx=640)
    c.set_option("token_logprobs", 1)
    yield m, c
    c.close()
    m.close()


@pytest.fixture(scope="module")
def rec3():
    """3 s and 37 samples, louder and quieter stretches"""
    x = qasr.synth_pcm(7700, 48000 + 37)
    env = 0.05 + np.abs(np.sin(np.arange(len(x)) * (2 * np.pi / 23000.0)))
    return (x * env).astype(f32)


def _table(segs):
    return [(s.rec, s.start, s.n, su.bits(s.peak).item(), s.silent) for s in segs]


def _bits32(v):
    return np.asarray(v, f32).view(np.uint32).tolist()


def test_stage_long_equals_the_host_rule(tiny, rec3):
    _m, c = tiny
    segs = c.stage_long([rec3], **PRM)
    assert len(segs) >= 3 and _table(segs) == _table(qasr.segment_host(rec3, **PRM)) == _table(c.get_segments(0))
    want = su.rule(rec3, **PRM)
    assert [s.start for s in segs] == want["start"] and [s.n for s in segs] == want["n"]
    assert segs[-1].start + segs[-1].n == len(rec3)   # the tail samples belong to the last segment
    # the stage-level call: the same table, e and s the rule's bits, the pool untouched
    tab, e, s = c.segment([rec3], want_energy=True, **PRM)
    assert _table(tab[0]) == _table(segs)
    assert (su.bits(e[0]) == su.bits(want["e"])).all() and (su.bits(s[0]) == su.bits(want["s"])).all()
    us, cut_us = c.segment_last_us()
    assert us > 0 and 0 <= cut_us <= us
    assert _table(c.get_segments()) == _table(segs)


def test_pool_entries_are_the_segments_alone(tiny, rec3):
    """run_staged([k]) reads the recording where it lies; the same samples staged on their own give the same tokens
    and the same log-probability bits, so the mel stage sees the segment and nothing around it"""
    _m, c = tiny
    segs = c.stage_long([rec3], **PRM)
    pool = [c.run_staged([k], NTOK, ignore_eos=True) for k in range(len(segs))]
    both = c.run_staged([1, 0], NTOK, ignore_eos=True)
    items = iter(range(len(segs)))
    stream, st = c.run_stream_staged(lambda: next(items, None), NTOK, ignore_eos=True, slots=2, logprobs=True)
    assert st.n_clips == len(segs) and st.n_errors == 0
    for k, s in enumerate(segs):
        one = c.transcribe([rec3[s.start:s.start + s.n]], max_tokens=NTOK, ignore_eos=True)   # (a fresh staging)
        assert pool[k].tokens == one.tokens, k
        assert _bits32(pool[k].logprobs[0]) == _bits32(one.logprobs[0]), k
        assert stream[k][0] == pool[k].tokens[0] and _bits32(stream[k][1]) == _bits32(pool[k].logprobs[0]), k
    assert both.tokens == [pool[1].tokens[0], pool[0].tokens[0]]


def test_a_48_khz_recording(tiny):
    _m, c = tiny
    raw = qasr.synth_pcm(7701, 3 * 48000 + 11)
    raw = (raw * (0.05 + np.abs(np.sin(np.arange(len(raw)) * (2 * np.pi / 70000.0))))).astype(f32)
    at16 = qasr.resample_host(raw, 48000)
    segs = c.stage_long([raw], rates=[48000], **PRM)
    assert len(segs) >= 3 and _table(segs) == _table(qasr.segment_host(at16, **PRM))
    a = c.run_staged([1], NTOK, ignore_eos=True)
    b = c.transcribe([at16[segs[1].start:segs[1].start + segs[1].n]], max_tokens=NTOK, ignore_eos=True)
    assert a.tokens == b.tokens and _bits32(a.logprobs[0]) == _bits32(b.logprobs[0])


def test_two_recordings_in_one_call(tiny, rec3):
    _m, c = tiny
    other = qasr.synth_pcm(7702, 160 * 130 + 3)   # its first sample at an odd offset of the buffer (rec3 has 48037)
    short = np.zeros(50, f32)                     # no frame: one segment of 50 samples
    segs = c.stage_long([rec3, short, other], **PRM)
    want = [qasr.segment_host(x, **PRM) for x in (rec3, short, other)]
    assert [s.rec for s in segs] == [0] * len(want[0]) + [1] + [2] * len(want[2])
    for r in range(3):
        mine = [s for s in segs if s.rec == r]
        assert _table(c.get_segments(r)) == _table(mine)
        assert [(s.start, s.n, su.bits(s.peak).item()) for s in mine] == [(s.start, s.n, su.bits(s.peak).item()) for s in want[r]], r
    assert len(want[2]) == 2
    k = len(want[0]) + 1 + 1   # the second segment of the third recording
    a = c.run_staged([k], NTOK, ignore_eos=True)
    b = c.transcribe([other[segs[k].start:segs[k].start + segs[k].n]], max_tokens=NTOK, ignore_eos=True)
    assert a.tokens == b.tokens and _bits32(a.logprobs[0]) == _bits32(b.logprobs[0])


@pytest.fixture(scope="module")
def paused(rec3):
    x = rec3[:48000].copy()
    x[160 * 100:160 * 201] = 0.0   # frames 100 .. 200: both cuts fall on a zero frame, the larger one of equals
    return x


def test_silent_flag_on_the_planted_second_only(tiny, paused):
    _m, c = tiny
    prm = dict(max_frames=100, min_frames=40, smooth_half=0)
    segs = c.stage_long([paused], skip_ratio=0.0, **prm)
    assert [(s.start // 160, s.silent) for s in segs] == [(0, False), (100, True), (200, False)]
    assert _table(segs) == _table(qasr.segment_host(paused, skip_ratio=0.0, **prm))
    assert [s.silent for s in c.stage_long([paused], skip_ratio=-1.0, **prm)] == [False] * 3


def test_transcribe_long_skips_silence_and_joins_the_rest(tiny, paused):
    m, c = tiny
    prm = dict(max_frames=100, min_frames=40, smooth_half=0, skip_ratio=0.0)
    text, parts = c.transcribe_long(paused, max_tokens=NTOK, ignore_eos=True, **prm)
    assert [s.silent for s, _ in parts] == [False, True, False] and parts[1][1] == []
    c.stage_long([paused], **prm)
    for k in (0, 2):
        assert parts[k][1] == c.run_staged([k], NTOK, ignore_eos=True).tokens[0], k
    assert text == " ".join(t for t in (m.detokenize(parts[0][1]), m.detokenize(parts[2][1])) if t)
    # constraints on: the stream refuses them, so the segments go through run_staged in groups
    c.set_constraints(no_repeat_ngram=2)
    try:
        _text, con = c.transcribe_long(paused, max_tokens=NTOK, ignore_eos=True, **prm)
        assert con[1][1] == [] and all(len(con[k][1]) == NTOK for k in (0, 2))
        c.stage_long([paused], **prm)
        assert [con[0][1], con[2][1]] == c.run_staged([0, 2], NTOK, ignore_eos=True).tokens
    finally:
        c.set_constraints()


def test_state_and_argument_errors(tiny, tiny_gguf, rec3):
    m, c = tiny
    L = qasr.lib()
    fresh = qasr.Context(m, max_batch=1, max_ctx=256)
    try:
        assert L.qasr_get_segments(fresh.h, 0, None, None, None, None, 0) == -QASR_ERR_STATE   # before any stage_long
    finally:
        fresh.close()
    segs = c.stage_long([rec3], **PRM)
    assert L.qasr_get_segments(c.h, 0, None, None, None, None, 0) == len(segs)
    assert L.qasr_get_segments(c.h, 1, None, None, None, None, 0) == -QASR_ERR_ARG            # one recording only
    c.stage_audio([rec3[:16000]])
    assert L.qasr_get_segments(c.h, 0, None, None, None, None, 0) == -QASR_ERR_STATE           # a later stage_audio
    c.stage_long([rec3], **PRM)
    c.stage_audio([rec3[:16000]], rates=[16000])
    assert L.qasr_get_segments(c.h, 0, None, None, None, None, 0) == -QASR_ERR_STATE           # ... or stage_audio_rate
    with pytest.raises(qasr.QasrError, match="pool"):
        c.get_segments(0)
    n = np.array([len(rec3)], np.int32)
    ptrs = (C.POINTER(C.c_float) * 1)(qasr._f(rec3))
    for bad, word in ((dict(max_frames=100, min_frames=51), "max_frames"), (dict(min_frames=0), "min_frames"),
                      (dict(smooth_half=65), "smooth_half"), (dict(skip_ratio=float("nan")), "skip_ratio")):
        p = qasr.segment_params(**bad)
        assert L.qasr_stage_long(c.h, ptrs, qasr._i(n), None, 1, C.byref(p)) == -QASR_ERR_ARG
        assert word in L.qasr_last_error().decode()
        with pytest.raises(qasr.QasrError, match=word):
            c.segment([rec3], **bad)
    with pytest.raises(qasr.QasrError, match="44101"):
        c.stage_long([rec3], rates=[44101], **PRM)


def test_an_aligner_model_is_refused(gpu, tmp_path, rec3):
    path = str(tmp_path / "aligner-tiny.gguf")
    qasr.write_synthetic_gguf(path, "aligner-tiny", 42, 1)
    m = qasr.Model(path)
    c = qasr.Context(m, max_batch=1, max_ctx=256)
    try:
        L = qasr.lib()
        n = np.array([len(rec3)], np.int32)
        ptrs = (C.POINTER(C.c_float) * 1)(qasr._f(rec3))
        assert L.qasr_stage_long(c.h, ptrs, qasr._i(n), None, 1, None) == -QASR_ERR_STATE
        assert L.qasr_get_segments(c.h, 0, None, None, None, None, 0) == -QASR_ERR_STATE
    finally:
        c.close()
        m.close()
