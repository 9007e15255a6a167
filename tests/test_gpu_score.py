"""Teacher-forced scoring (qasr_prefill_score, qasr_score) on the tiny model.

Bars:
  oracle / own logits / greedy run / shared prompt: 2 * 1e-2 * max |oracle logits| -- tests/test_gpu_logprobs.py's
      "streams" bar: 1e-2 of the scale is the logit bar test_gpu_parity.py holds for this model, and the target's
      logit and the log-sum-exp each move by at most that.  What was measured against 2 * delta (delta = the same
      prefix's max |logits_gpu - logits_oracle| through qasr_prefill) and against the context's own logits is
      recorded through `parity`.
  Q8_0: twice test_gpu_q8.py's logit bar (Q8_STEP_ABS), read from that file.
  greedy ids: equal to the run's tokens wherever the oracle's top-2 logit gap exceeds twice the bar; with the clips
      below the oracle's gaps are 1.7 .. 10 times that at all 24 positions (checked on the CPU), and at least 3/4
      must qualify.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as op
import qasr

pytestmark = pytest.mark.gpu
SR = 16000
QASR_ERR_ARG, QASR_ERR_STATE = 1, 5
NTOK = 8


def lp64(logits, tok):
    v = np.asarray(logits, np.float64)
    m = v.max()
    return float(v[tok] - (m + np.log(np.exp(v - m).sum())))


def seq_sum(x):
    """float32 sum in order, as qasr_score's"""
    s = np.float32(0)
    for v in np.asarray(x, np.float32):
        s = np.float32(s + v)
    return float(s)


@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=16, max_ctx=640)
    yield m, c
    c.close()
    m.close()


_CLIPS = {}


def clip(oracle, i):
    """tests/test_gpu_logprobs.py's recipe: pcm, the oracle's features and prompt"""
    key = (id(oracle), i)
    if key not in _CLIPS:
        pcm = qasr.synth_pcm(8100 + i, SR + 1733 * i)
        feats = oracle.encode(op.log_mel(pcm))
        _CLIPS[key] = (pcm, feats, oracle.prompt(feats.shape[0]))
    return _CLIPS[key]


def forced_tokens(oracle, feats, ids, seed, n=NTOK):
    """n tokens and the oracle's teacher-forced logit row before each of them and after the last (n + 1 rows):
    even positions take the oracle's argmax, odd ones a random id"""
    rng = np.random.default_rng(seed)
    d = op.OracleDecoder(oracle, 512)
    rows, toks = [d.forward(ids, 0, feats, 9).copy()], []
    for k in range(n):
        toks.append(int(np.argmax(rows[-1])) if k % 2 == 0 else int(rng.integers(0, 151643)))
        rows.append(d.forward([toks[-1]], len(ids) + k).copy())
    return toks, rows


def score_one(c, ids, feats, toks, eos):
    """prefill_score of prompt + toks as one sequence: the last prompt row and every token row scored"""
    seq = list(ids) + list(toks)
    tg = [-1] * (len(ids) - 1) + list(toks) + [eos]
    return c.prefill_score([seq], [tg], feats_list=[feats], audio_pos=[9])[0]


def _against_oracle(m, c, oracle, parity, name, bar_of):
    eos = m.hp.eos_id
    worst = worst_own = ratio = 0.0
    for i in range(2):
        _, feats, ids = clip(oracle, i)
        toks, rows = forced_tokens(oracle, feats, ids, 50 + i)
        sc = score_one(c, ids, feats, toks, eos)
        assert len(sc.logprobs) == NTOK + 1 and (sc.logprobs <= sc.greedy_logprobs).all()
        tg = toks + [eos]
        for k in range(NTOK + 1):
            bar = bar_of(rows[k])
            err = abs(float(sc.logprobs[k]) - lp64(rows[k], tg[k]))
            # the same prefix through the unscored prefill: its logits against the oracle's, and lp against its own
            lg, am = c.prefill([list(ids) + toks[:k]], [feats], [9])
            delta = float(np.abs(lg[0].astype(np.float64) - rows[k]).max())
            own = abs(float(sc.logprobs[k]) - lp64(lg[0], tg[k]))
            print(f"{name} clip {i} row {k}: |lp - oracle| {err:.3g} (bar {bar:.3g}, 2 delta {2 * delta:.3g}), |lp - own logits| {own:.3g}")
            worst, worst_own, ratio = max(worst, err / bar), max(worst_own, own), max(ratio, err / (2 * delta))
            assert err <= bar, (i, k, err, bar)
            assert own <= bar, (i, k, own, bar)
            assert int(sc.greedy_ids[k]) == int(am[0]) or abs(float(lg[0][sc.greedy_ids[k]]) - float(lg[0].max())) <= bar
    parity(name, worst_over_bar=worst, worst_over_2delta=ratio, own_logits_abs=worst_own)


def test_prefill_score_against_oracle_and_own_logits(tiny, tiny_oracle, parity):
    m, c = tiny
    _against_oracle(m, c, tiny_oracle, parity, "tiny_score_oracle", lambda lo: 2 * 1e-2 * float(np.abs(lo).max()))


def test_q8_layers_f16_head(gpu, tiny_q8_gguf, tiny_q8_oracle, parity):
    """the f16 score head behind Q8_0 layers"""
    from test_gpu_q8 import Q8_STEP_ABS
    m = qasr.Model(tiny_q8_gguf)
    c = qasr.Context(m, max_batch=4, max_ctx=640)
    try:
        _against_oracle(m, c, tiny_q8_oracle, parity, "tiny_q8_score_oracle", lambda lo: 2 * Q8_STEP_ABS)
    finally:
        c.close()
        m.close()


def test_score_of_a_greedy_run(tiny, tiny_oracle, parity):
    m, c = tiny
    pcms = [qasr.synth_pcm(8200 + i, SR + 977 * i) for i in range(3)]
    c.set_option("token_logprobs", 1)
    try:
        r = c.transcribe(pcms, max_tokens=NTOK, ignore_eos=True)
    finally:
        c.set_option("token_logprobs", 0)
    sc = c.score([0, 1, 2], r.tokens, include_eos=False)
    qualify = total = 0
    worst = 0.0
    for b in range(3):
        feats = tiny_oracle.encode(op.log_mel(pcms[b]))
        ids = tiny_oracle.prompt(feats.shape[0])
        d = op.OracleDecoder(tiny_oracle, 512)
        lo = d.forward(ids, 0, feats, 9)
        assert len(sc[b].logprobs) == NTOK
        for k in range(NTOK):
            bar = 2 * 1e-2 * float(np.abs(lo).max())
            err = abs(float(sc[b].logprobs[k]) - float(r.logprobs[b][k]))
            worst = max(worst, err / bar)
            assert err <= bar, (b, k, err, bar)
            top = np.sort(lo)[-2:]
            total += 1
            if top[1] - top[0] > 2 * bar:
                qualify += 1
                assert int(sc[b].greedy_ids[k]) == r.tokens[b][k], (b, k)
                assert abs(float(sc[b].greedy_logprobs[k]) - float(sc[b].logprobs[k])) == 0.0
            lo = d.forward([r.tokens[b][k]], len(ids) + k)
    parity("tiny_score_greedy_run", worst_over_bar=worst, qualifying=qualify, positions=total)
    assert 4 * qualify >= 3 * total, (qualify, total)


def test_shared_prompt_equals_independent_sequences(tiny, tiny_oracle, parity):
    """clip A: hypotheses of 8, 3 and 0 tokens; clip B: two; interleaved in the input, EOS scored"""
    m, c = tiny
    eos = m.hp.eos_id
    pcms = [clip(tiny_oracle, 0)[0], clip(tiny_oracle, 1)[0]]
    rng = np.random.default_rng(3)
    hyps = [rng.integers(0, 151643, n).tolist() for n in (8, 5, 3, 2, 0)]
    clips = [0, 1, 0, 1, 0]
    c.stage_audio(pcms)
    a = c.score(clips, hyps, include_eos=True)
    b = c.score(clips, hyps, include_eos=True)
    feats = c.encode(c.mel(pcms))
    worst = 0.0
    for s, (ci, h) in enumerate(zip(clips, hyps)):
        assert len(a[s].logprobs) == len(h) + 1
        for name in ("logprobs", "greedy_ids", "greedy_logprobs"):
            assert getattr(a[s], name).tobytes() == getattr(b[s], name).tobytes(), (s, name)
        assert a[s].sum == b[s].sum == seq_sum(a[s].logprobs), s
        ids, pos = m.build_prompt(feats[ci].shape[0])
        one = score_one(c, ids, feats[ci], h, eos)
        d = op.OracleDecoder(tiny_oracle, 512)
        bar = 2 * 1e-2 * float(np.abs(d.forward(clip(tiny_oracle, ci)[2], 0, clip(tiny_oracle, ci)[1], 9)).max())
        err = float(np.abs(a[s].logprobs - one.logprobs).max())
        print(f"sequence {s} (clip {ci}, {len(h)} tokens): max |shared - independent| {err:.3g} (bar {bar:.3g})")
        worst = max(worst, err / bar)
        assert err <= bar, (s, err, bar)
    parity("tiny_score_shared_prompt", worst_over_bar=worst)
    # without the EOS: the same leading entries, an empty hypothesis yields nothing
    e = c.score(clips, hyps, include_eos=False)
    for s, h in enumerate(hyps):
        assert len(e[s].logprobs) == len(h)
        assert e[s].logprobs.tobytes() == a[s].logprobs[:len(h)].tobytes(), s


def test_score_leaves_transcription_alone_and_ignores_options(tiny):
    m, c = tiny
    pcms = [qasr.synth_pcm(8200 + i, SR + 977 * i) for i in range(2)]
    hyps = [[5, 6, 7], [8, 9]]
    c.set_option("token_logprobs", 1)
    try:
        r0 = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        s0 = c.score([0, 1], hyps)
        r1 = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        assert r0.tokens == r1.tokens and r0.logprobs == r1.logprobs
    finally:
        c.set_option("token_logprobs", 0)
    for name, val in (("beam_width", 4), ("top_k", 3)):
        c.set_option(name, val)
        try:
            s1 = c.score([0, 1], hyps)
        finally:
            c.set_option(name, 0)
        for x, y in zip(s0, s1):
            assert x.logprobs.tobytes() == y.logprobs.tobytes() and x.greedy_ids.tobytes() == y.greedy_ids.tobytes(), name
            assert x.greedy_logprobs.tobytes() == y.greedy_logprobs.tobytes() and x.sum == y.sum, name
    r2 = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
    assert r2.tokens == r0.tokens


def _score_rc(c, clips, hyps, include_eos=1):
    L = qasr.lib()
    idx = np.ascontiguousarray(clips, np.int32)
    nt = np.array([len(h) for h in hyps], np.int32)
    toks = np.ascontiguousarray(np.concatenate([np.asarray(h, np.int32).reshape(-1) for h in hyps] + [np.zeros(1, np.int32)]), np.int32)
    n = int(nt.sum()) + len(hyps) + 1
    lp, gid, glp = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    i = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.qasr_score(c.h, idx.ctypes.data_as(C.POINTER(C.c_int)), i(toks), nt.ctypes.data_as(C.POINTER(C.c_int)), len(hyps),
                      include_eos, f(lp), i(gid), f(glp), None, None)
    return rc, L.qasr_last_error().decode()


def test_score_errors(tiny, gpu, tmp_path):
    m, c = tiny
    pcms = [qasr.synth_pcm(8200 + i, SR) for i in range(3)]
    c.stage_audio(pcms)
    V = m.hp.vocab_size
    assert _score_rc(c, [0], [[V]])[0] == -QASR_ERR_ARG                       # a token >= vocab
    assert _score_rc(c, [3], [[1]])[0] == -QASR_ERR_ARG                       # clip outside the pool
    assert _score_rc(c, [-1], [[1]])[0] == -QASR_ERR_ARG
    assert _score_rc(c, [0] * 9, [[1]] * 9)[0] == -QASR_ERR_ARG               # 9 hypotheses of one clip
    assert _score_rc(c, [0] * 8, [[1]] * 8)[0] == 16                          # 8 are fine: 2 entries each
    assert _score_rc(c, [0] * 6 + [1, 2], [[1]] * 8)[0] == -QASR_ERR_ARG      # D x G = 3 x 6 > 16
    rc, msg = _score_rc(c, [0], [[1] * 640])
    assert rc == -QASR_ERR_ARG and "Context length exceeded" in msg
    assert _score_rc(c, [0], [[]], include_eos=0)[0] == 0                     # nothing to score: valid
    assert _score_rc(c, [0], [[]])[0] == 1                                    # the EOS alone
    c.set_option("fa_exact_prefill", 0)
    try:
        assert _score_rc(c, [0], [[1, 2]])[0] == -QASR_ERR_STATE
    finally:
        c.set_option("fa_exact_prefill", 1)
    with pytest.raises(qasr.QasrError):   # a target >= vocab
        c.prefill_score([[1, 2, 3]], [[-1, V, 1]])
    # a short output buffer
    L = qasr.lib()
    ids, P, tg = np.array([1, 2, 3], np.int32), np.array([3], np.int32), np.array([4, 5, 6], np.int32)
    out = np.zeros(3, np.float32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.qasr_prefill_score(c.h, i32(ids), P.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, None, None, 1, i32(tg), f32(out),
                                i32(np.zeros(3, np.int32)), f32(np.zeros(3, np.float32)), 2) == -QASR_ERR_ARG
    # no staged audio, and an aligner model
    c2 = qasr.Context(m, max_batch=2, max_ctx=128)
    try:
        assert _score_rc(c2, [0], [[1]])[0] == -QASR_ERR_STATE
    finally:
        c2.close()
    p = str(tmp_path / "aligner-tiny.gguf")
    qasr.write_synthetic_gguf(p, "aligner-tiny", 42, 1)
    ma = qasr.Model(p)
    ca = qasr.Context(ma, max_batch=2, max_ctx=256)
    try:
        ca.stage_audio(pcms[:1])
        assert _score_rc(ca, [0], [[1]])[0] == -QASR_ERR_STATE
        with pytest.raises(qasr.QasrError):
            ca.prefill_score([[1, 2, 3]], [[-1, 2, 1]])
    finally:
        ca.close()
        ma.close()
