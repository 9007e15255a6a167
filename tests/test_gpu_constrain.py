"""Decoding constraints (Context.set_constraints) on the tiny model: the device loop against a host loop over the
stage calls, every step's edited logits and token against the normative rule (tests/constrain_util.py) applied to
the raw logits, the loop the tiny model falls into and its end under a no-repeat rule, sampling on top, the captured
steps serving any values, the refusals, and the greedy paths left as they were.

A decode output row depends only on its own inputs, bit for bit (tests/test_gpu_batch.py), so the raw logits of a
constrained run are those of teacher-forcing its tokens with constraints off, and everything here is exact: tokens
and the bits of every logit, log-probability and alternative.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import constrain_util as cu
import qasr
import sample_util as su
from beam_util import prompts

pytestmark = pytest.mark.gpu
SR = 16000
QASR_ERR_ARG, QASR_ERR_STATE = 1, 5
SEED = 0xA5A5F00D0BADC0DE
f32 = np.float32
NEUTRAL = dict(bias={0: -0.0})
RULES = [dict(n=2), dict(n=3), dict(p=1.3, w=4), dict(n=3, p=1.1, bias={0: 5.0})]


@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=12, max_ctx=640)
    yield m, c
    c.close()
    m.close()


def clips(n, seed=9100):
    return [qasr.synth_pcm(seed + i, SR + 4000 * (i % 5)) for i in range(n)]


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


def turn_on(c, n=0, p=1.0, w=0, bias=None, suppress=None):
    c.set_constraints(no_repeat_ngram=n, repetition_penalty=p, penalty_last_n=w, bias=bias, suppress=suppress)


def stage_loop(c, pcms, max_tokens, feed=None):
    """prefill + decode steps over the stage calls -> (tokens [B][max_tokens], the logits every call returned); feed:
    the tokens fed back (teacher forcing), else each call's own"""
    B = len(pcms)
    feats, ids, pos = prompts(c, pcms)
    P = [len(x) for x in ids]
    toks, logits = [[] for _ in range(B)], []
    for k in range(max_tokens):
        if k == 0:
            lg, tok = c.prefill(ids, feats, pos)
        else:
            src = feed if feed is not None else toks
            lg, tok = c.decode_step([t[k - 1] for t in src], [P[b] + k - 1 for b in range(B)])
        logits.append(lg)
        for b in range(B):
            toks[b].append(int(tok[b]))
    return toks, logits


def check_against_rule(c, pcms, toks, edited, rule, hist=None):
    """every step's returned logits and token (None: not the rule's choice, a draw) against the rule on the raw logits
    of teacher-forcing the same tokens with constraints off; returns per step how many rows had their raw argmax edited"""
    c.set_constraints()
    _, raw = stage_loop(c, pcms, len(edited), feed=toks)
    in_E = []
    for k, (lr, le) in enumerate(zip(raw, edited)):
        n_in = 0
        for b in range(len(pcms)):
            want, wtok, E = cu.apply(lr[b], toks[b][:k], **rule)
            assert np.array_equal(bits(le[b]), bits(want)), (k, b, np.flatnonzero(bits(le[b]) != bits(want))[:8])
            if hist is None:
                assert toks[b][k] == wtok, (k, b, toks[b][k], wtok)
            n_in += cu.select(lr[b]) in E
        in_E.append(n_in)
    return in_E


# ------------------------------------------------------- neutral when on
@pytest.mark.parametrize("B", [1, 3, 9])
def test_neutral_constraints_change_no_bit(tiny, B):
    """a bias of -0.0 on one token edits nothing, whichever path the stage takes: tokens, log-probabilities and
    alternatives as with constraints off (1, 3, 9 rows: the fused batch-1 launches, the GEMV path, the decode-batch path)"""
    _, c = tiny
    pcms = clips(B)
    c.set_option("token_logprobs", 1)
    c.set_option("top_k", 3)
    try:
        off = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        turn_on(c, **NEUTRAL)
        assert c.get_constraints()["bias"] == {0: 0.0} and np.signbit(f32(c.get_constraints()["bias"][0]))
        on = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
    finally:
        c.set_constraints()
        c.set_option("token_logprobs", 0)
        c.set_option("top_k", 0)
    assert on.tokens == off.tokens
    assert np.array_equal(bits(on.logprobs), bits(off.logprobs))
    for b in range(B):
        assert np.array_equal(on.topk[b][0], off.topk[b][0]) and np.array_equal(bits(on.topk[b][1]), bits(off.topk[b][1]))


# ------------------------------------------------- device loop vs host loop
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(f"{k}{v}" for k, v in r.items() if k != "bias") + ("-bias" if "bias" in r else ""))
@pytest.mark.parametrize("B", [1, 3, 9])
def test_device_loop_equals_host_loop_equals_rule(tiny, B, rule):
    _, c = tiny
    pcms = clips(B)
    try:
        turn_on(c, **rule)
        toks, edited = stage_loop(c, pcms, 16)
        r = c.transcribe(pcms, max_tokens=16, ignore_eos=True)
        assert r.tokens == toks
        in_E = check_against_rule(c, pcms, toks, edited, rule)
        print(f"B={B} {rule}: rows with the raw argmax edited per step {in_E}")
        assert any(in_E) and not all(x == B for x in in_E)      # both paths of the stage ran
    finally:
        c.set_constraints()


def test_logprobs_and_topk_are_the_edited_rows(tiny):
    """option token_logprobs: log softmax(l')[token]; option top_k: entry 0 the constrained token, the values l''s"""
    _, c = tiny
    pcms = clips(3)
    c.set_option("token_logprobs", 1)
    c.set_option("top_k", 4)
    try:
        turn_on(c, n=2, p=1.3)
        feats, ids, pos = prompts(c, pcms)
        lg, tok = c.prefill(ids, feats, pos)
        seen = [[int(t)] for t in tok]
        for k in range(1, 6):
            lg, tok = c.decode_step([s[-1] for s in seen], [len(ids[b]) + k - 1 for b in range(3)])
            lp, (tid, tlp) = c.step_logprobs(3), c.step_topk(3)
            for b in range(3):
                assert tid[b, 0] == tok[b] and bits(tlp[b, 0]) == bits(lp[b])
                assert abs(float(lp[b]) - su.logsoftmax64(lg[b], int(tok[b]))) <= 2e-5
                order = np.argsort(cu.argmax_key(lg[b], np.arange(lg.shape[1])))[::-1][:4]      # (the keys are distinct)
                assert tid[b].tolist() == order.tolist()
                seen[b].append(int(tok[b]))
        r = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        assert r.tokens == seen and all(r.topk[b][0][:, 0].tolist() == seen[b] for b in range(3))
    finally:
        c.set_constraints()
        c.set_option("token_logprobs", 0)
        c.set_option("top_k", 0)


# -------------------------------------------------------- the effect is real
def test_no_repeat_ends_the_loop_and_suppress_removes_a_token(tiny):
    _, c = tiny
    pcms = clips(3)
    try:
        free = c.transcribe(pcms, max_tokens=16, ignore_eos=True).tokens
        assert all(cu.repeats_ngram(t, 2) for t in free), free
        turn_on(c, n=2)
        held = c.transcribe(pcms, max_tokens=16, ignore_eos=True).tokens
        assert not any(cu.repeats_ngram(t, 2) for t in held), held
        assert all(a[0] == b[0] for a, b in zip(free, held))          # an empty history bans nothing
        assert all(len(set(t)) > len(set(f)) for t, f in zip(held, free))
        turn_on(c, n=1)
        assert all(len(set(t)) == 16 for t in c.transcribe(pcms, max_tokens=16, ignore_eos=True).tokens)
        first = [t[0] for t in free]
        turn_on(c, suppress=first)
        gone = c.transcribe(pcms, max_tokens=16, ignore_eos=True).tokens
        assert not any(set(t) & set(first) for t in gone), (first, gone)
        assert c.get_constraints()["bias"] == {t: -np.inf for t in first}
    finally:
        c.set_constraints()
    assert c.transcribe(pcms, max_tokens=16, ignore_eos=True).tokens == free


# ----------------------------------------------------------- sampling on top
@pytest.mark.parametrize("min_p, N", [(0.0, 1), (0.2, 1), (0.0, 3), (0.2, 3)])
def test_sampling_draws_from_the_edited_rows(tiny, min_p, N):
    """T = 5: every draw a candidate of l' within sample_util's band, the run the host loop's; n_best = N: every (clip,
    sample) against a row decoded from scratch under its identity"""
    _, c = tiny
    pcms, T, rule = clips(2), 5.0, dict(n=2, p=1.3, bias={0: 5.0})
    rows = [pcms[g] for g in range(2) for _ in range(N)]
    clip, sample = [g for g in range(2) for _ in range(N)], list(range(N)) * 2
    try:
        turn_on(c, **rule)
        c.set_sampling(T, min_p, SEED, 1)
        c.set_sample_streams(clip, sample, [0] * len(rows))
        toks, edited = stage_loop(c, rows, 8)
        und = n = 0
        for k, le in enumerate(edited):
            for b in range(len(rows)):
                assert le[b][toks[b][k]] > -np.inf                      # a banned column is never drawn
                und += not su.check_draw(le[b], toks[b][k], None, T, min_p, SEED, clip[b], sample[b], k, what=f"step {k} row {b}")
                n += 1
        assert und <= n // 100, (und, n)
        c.set_sampling(T, min_p, SEED, N)
        r = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert [[s.tokens for s in g] for g in r.samples] == [toks[g * N:(g + 1) * N] for g in range(2)]
        c.set_sampling(0)
        check_against_rule(c, rows, toks, edited, rule, hist="drawn")
    finally:
        c.set_sampling(0)
        c.set_constraints()


# ------------------------------------------------------------ graph captures
def test_value_changes_capture_no_graph(tiny):
    _, c = tiny
    pcms = clips(3)
    try:
        turn_on(c, n=2)
        a = c.transcribe(pcms, max_tokens=8, ignore_eos=True).tokens
        caps = c.get_option("graph_captures")
        outs = []
        for rule in (dict(n=3), dict(p=1.3, w=4), dict(n=8, p=0.7, bias={i: 0.5 for i in range(1024)}), dict(suppress=[a[0][0]]), dict(n=2)):
            turn_on(c, **rule)
            outs.append(c.transcribe(pcms, max_tokens=8, ignore_eos=True).tokens)
        assert c.get_option("graph_captures") == caps
        assert outs[-1] == a and outs[0] != a and outs[3][0][0] != a[0][0]
        c.set_constraints()
        c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        off_caps = c.get_option("graph_captures")
        turn_on(c, n=2)
        c.set_constraints()
        c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert c.get_option("graph_captures") == off_caps         # the greedy graphs were kept beside the constrained ones
    finally:
        c.set_constraints()


# --------------------------------------------- greedy around a constrained run
def test_greedy_bit_identical_around_a_constrained_run(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=9, max_ctx=640)
    try:
        c.set_option("token_logprobs", 1)
        c.set_option("top_k", 3)
        for pcms in (clips(1, 9600), clips(9, 9600)):
            before = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            turn_on(c, n=2, p=1.3)
            con = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            c.set_constraints()
            after = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            assert con.tokens != before.tokens and after.tokens == before.tokens
            assert np.array_equal(bits(after.logprobs), bits(before.logprobs))
            for b in range(len(pcms)):
                assert np.array_equal(after.topk[b][0], before.topk[b][0]) and np.array_equal(bits(after.topk[b][1]), bits(before.topk[b][1]))
                assert con.topk[b][0][:, 0].tolist() == con.tokens[b]
    finally:
        c.close()
        m.close()


# ------------------------------------------------------------------- errors
def _queue(items):
    it = iter(items)
    return lambda: next(it, None)


def test_argument_ranges_and_refusals(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=4, max_ctx=640)
    try:
        lib = qasr.lib()
        V = m.hp.vocab_size
        off = {"no_repeat_ngram": 0, "repetition_penalty": 1.0, "penalty_last_n": 0, "bias": {}}
        assert c.get_constraints() == off
        for kw in (dict(no_repeat_ngram=9), dict(no_repeat_ngram=-1), dict(repetition_penalty=0.0), dict(repetition_penalty=10.5),
                   dict(repetition_penalty=float("nan")), dict(penalty_last_n=-1), dict(bias={V: 1.0}), dict(bias={-1: 1.0}),
                   dict(bias={3: float("inf")}), dict(bias={3: float("nan")}), dict(bias={i: 0.0 for i in range(1025)})):
            with pytest.raises(qasr.QasrError):
                c.set_constraints(**kw)
            assert c.get_constraints() == off, kw
        ids, val = np.array([3, 3], np.int32), np.zeros(2, f32)
        k = qasr.Constraints(0, 1.0, 0, 2, ids.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_float)))
        assert lib.qasr_set_constraints(c.h, C.byref(k)) == QASR_ERR_ARG
        c.set_constraints(8, 10.0, 2 ** 31 - 1, bias={V - 1: -1.5}, suppress=[0])
        assert c.get_constraints() == {"no_repeat_ngram": 8, "repetition_penalty": 10.0, "penalty_last_n": 2 ** 31 - 1,
                                       "bias": {V - 1: -1.5, 0: -np.inf}}
        out = qasr.Constraints()
        assert lib.qasr_get_constraints(c.h, C.byref(out), ids.ctypes.data_as(C.POINTER(C.c_int32)), None, 1) == QASR_ERR_ARG
        assert lib.qasr_get_constraints(c.h, C.byref(out), None, None, 0) == 0 and out.n_bias == 2
        c.set_constraints(penalty_last_n=5)           # the neutral values: off, whatever the window says
        assert c.get_constraints() == off
        assert lib.qasr_set_constraints(c.h, None) == 0
        pcms = clips(3, 9700)
        g = c.transcribe(pcms[:1], max_tokens=4, ignore_eos=True)
        turn_on(c, n=2)
        with pytest.raises(qasr.QasrError, match="stream"):
            c.run_stream(_queue([(0, pcms[0], 3)]), max_tokens=4, ignore_eos=True)
        c.stage_audio(pcms)
        with pytest.raises(qasr.QasrError, match="stream"):
            c.run_stream_staged(_queue([0]), max_tokens=4, ignore_eos=True)
        toks, nt = np.zeros((4, 4), np.int32), np.zeros(4, np.int32)
        c.stage_audio(pcms[:1])
        c.set_option("beam_width", 2)
        assert lib.qasr_run(c.h, 4, 1, toks.ctypes.data_as(C.POINTER(C.c_int32)), nt.ctypes.data_as(C.POINTER(C.c_int)), None) == QASR_ERR_STATE
        assert "beam" in lib.qasr_last_error().decode()
        c.set_option("beam_width", 0)
        seen = []
        c.set_token_callback(lambda seq, k, t: seen.append((seq, k, t)))       # a token callback sees the constrained tokens
        r = c.transcribe(pcms[:1], max_tokens=6, ignore_eos=True)
        c.set_token_callback(None)
        assert [t for _, _, t in seen] == r.tokens[0] and not cu.repeats_ngram(r.tokens[0], 2)
        c.stage_audio(pcms)                                                     # run_staged: a subset of the pool
        sub = c.run_staged([2, 0], max_tokens=6, ignore_eos=True)
        assert sub.tokens[1] == r.tokens[0] and not cu.repeats_ngram(sub.tokens[0], 2)
        # scoring is unaffected
        a = c.score([0], [g.tokens[0]])[0]
        c.set_constraints()
        b = c.score([0], [g.tokens[0]])[0]
        assert np.array_equal(bits(a.logprobs), bits(b.logprobs)) and np.array_equal(a.greedy_ids, b.greedy_ids)
        assert c.transcribe(pcms[:1], max_tokens=4, ignore_eos=True).tokens == g.tokens
    finally:
        c.close()
        m.close()


# --------------------------------------------------------------------- Q8_0
def test_q8_device_loop_equals_host_loop_equals_rule(gpu, tiny_q8_gguf):
    m = qasr.Model(tiny_q8_gguf)
    c = qasr.Context(m, max_batch=3, max_ctx=640)
    try:
        pcms, rule = clips(3, 9200), dict(n=2, p=1.3, w=4)
        turn_on(c, **rule)
        toks, edited = stage_loop(c, pcms, 8)
        assert c.transcribe(pcms, max_tokens=8, ignore_eos=True).tokens == toks
        check_against_rule(c, pcms, toks, edited, rule)
    finally:
        c.close()
        m.close()


# ---------------------------------------------------------------------- CLI
def test_cli_constraint_flags(tiny, tiny_gguf, tmp_path):
    """qwen3-asr-cli --no-repeat-ngram --repetition-penalty --penalty-last-n --suppress-tokens --token-bias: the text
    Context.transcribe gives under the same constraints"""
    m, c = tiny
    cli = os.path.join(os.path.dirname(qasr.LIB_PATH), "qwen3-asr-cli")
    wav = str(tmp_path / "clip.wav")
    qasr.write_wav(wav, clips(1)[0])
    pcm16, _ = qasr.load_wav(wav)   # (the file's 16-bit samples)
    free = c.transcribe([pcm16], max_tokens=12, ignore_eos=False).tokens[0]
    try:
        turn_on(c, n=2, p=1.3, w=4, bias={0: 0.5, 7: -1.0}, suppress=[free[0]])
        want = c.transcribe([pcm16], max_tokens=12, ignore_eos=False).tokens[0]
    finally:
        c.set_constraints()
    assert want != free and free[0] not in want
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(cli))
    base = [cli, "-m", tiny_gguf, "-f", wav, "--max-tokens", "12", "--no-timing"]
    r = subprocess.run(base + ["--no-repeat-ngram", "2", "--repetition-penalty", "1.3", "--penalty-last-n", "4", "--suppress-tokens",
                               str(free[0]), "--token-bias", "0:0.5,7:-1"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == m.detokenize(want) + "\n", (r.stdout, want)
    for flags, msg in ((["--no-repeat-ngram", "9"], "--no-repeat-ngram takes 0..8"), (["--repetition-penalty", "0"], "--repetition-penalty takes 0 < p <= 10"),
                       (["--penalty-last-n", "-1"], "--penalty-last-n takes 0 or more"), (["--suppress-tokens", "3,x"], "--suppress-tokens takes id,id,..."),
                       (["--token-bias", "3"], "--token-bias takes id:val,..."), (["--token-bias", "3:inf"], "--token-bias takes id:val,...")):
        bad = subprocess.run(base + flags, capture_output=True, text=True, env=env, timeout=120)
        assert bad.returncode != 0 and msg in bad.stderr, (flags, bad.stderr)
