"""Hotword boosting (Context.set_phrases) on the tiny model: the device loop against a host loop over
the stage calls, every step's edited logits and token against the normative rule (tests/phrase_util.py) applied to the
raw logits, phrases together with the other constraints, the log-probabilities, alternatives and the sampler reading
the boosted row, the captured steps serving any list, the refusals, and the greedy paths left as they were.

As in tests/test_gpu_constrain.py a decode output row depends only on its own inputs, bit for bit, so the raw logits of
a boosted run are those of teacher-forcing its tokens with everything off, and everything here is exact.

The phrases are built from a plain greedy run: 3 and 4 tokens long, each starting with a token no clip emits by itself
and going on with tokens the clips do emit.  BOOST is the smallest of 25, 50 and 100 (the tiny model's logits have a
scale of about 20) at which, in every parametrisation of the first test, the phrases are spelled out to a depth of at
least 2 and the raw argmax is boosted in some rows and steps and not in others: 25 (at 1, 3 and 9 rows the second phrase
is spelled out to depth 3, and the raw argmax is a boosted token at the steps of depth 2 and 3 only).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import constrain_util as cu
import phrase_util as pu
import qasr
import sample_util as su
from beam_util import prompts

pytestmark = pytest.mark.gpu
SR = 16000
QASR_ERR_ARG, QASR_ERR_STATE = 1, 5
SEED = 0xA5A5F00D0BADC0DE
f32 = np.float32
BOOST = 25.0
STEPS = 16


@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=12, max_ctx=640)
    yield m, c
    c.close()
    m.close()


def clips(n, seed=9100):
    return [qasr.synth_pcm(seed + i, SR + 4000 * (i % 5)) for i in range(n)]


def clips_of(B):
    """B clips; alone, the clip of seed 9100 answers a boosted phrase start by emitting it for ever (its raw logits put
    the start above the phrase's second token), so a single row is the next clip"""
    return clips(B) if B > 1 else clips(1, 9101)


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


def all_off(c):
    c.set_phrases()
    c.set_constraints()


def turn_on(c, n=0, p=1.0, w=0, bias=None):
    c.set_constraints(no_repeat_ngram=n, repetition_penalty=p, penalty_last_n=w, bias=bias)


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


def build_phrases(c, pcms, boost=BOOST):
    """from a plain greedy run: [X1, a, b] and [X2, d, e, f], X1 / X2 tokens no clip emits, the rest tokens of the first
    and the last clip's transcripts"""
    all_off(c)
    free = c.transcribe(pcms, max_tokens=STEPS, ignore_eos=True).tokens
    emitted = {t for row in free for t in row}
    fresh = [x for x in range(1000, 1100) if x not in emitted][:2]
    first, last = free[0], free[-1]
    return [([fresh[0]] + first[1:3], boost), ([fresh[1]] + last[2:5], boost)], free


def check_against_rule(c, pcms, toks, edited, phrases, rule, drawn=False):
    """every step's returned logits and token (drawn: not the rule's choice) against the rule on the raw logits of
    teacher-forcing the same tokens with everything off; returns per step how many rows had their raw argmax edited, and
    the deepest phrase position matched at that step"""
    all_off(c)
    _, raw = stage_loop(c, pcms, len(edited), feed=toks)
    in_E, depth = [], []
    for k, (lr, le) in enumerate(zip(raw, edited)):
        n_in, deep = 0, 0
        for b in range(len(pcms)):
            want, wtok, E = pu.apply(lr[b], toks[b][:k], phrases, **rule)
            assert np.array_equal(bits(le[b]), bits(want)), (k, b, np.flatnonzero(bits(le[b]) != bits(want))[:8])
            if not drawn:
                assert toks[b][k] == wtok, (k, b, toks[b][k], wtok)
            n_in += cu.select(lr[b]) in E
            deep = max(deep, pu.bonuses(phrases, toks[b][:k])[1])
        in_E.append(n_in)
        depth.append(deep)
    return in_E, depth


def run_three_ways(c, pcms, phrases, rule):
    """phrases and rule on: the host loop's tokens and edited logits, asserted equal to the device loop's tokens"""
    turn_on(c, **rule) if rule else c.set_constraints()
    c.set_phrases(phrases)
    toks, edited = stage_loop(c, pcms, STEPS)
    r = c.transcribe(pcms, max_tokens=STEPS, ignore_eos=True)
    assert r.tokens == toks
    return toks, edited


# ------------------------------------------------------------ phrases alone
@pytest.mark.parametrize("B", [1, 3, 9])
def test_device_loop_equals_host_loop_equals_rule(tiny, B):
    """fails without the feature: Context.set_phrases is what it adds"""
    _, c = tiny
    pcms = clips_of(B)
    try:
        phrases, free = build_phrases(c, pcms)
        assert sorted(len(i) for i, _ in phrases) == [3, 4]
        toks, edited = run_three_ways(c, pcms, phrases, {})
        in_E, depth = check_against_rule(c, pcms, toks, edited, phrases, {})
        print(f"B={B} boost {BOOST}: rows with the raw argmax boosted per step {in_E}, deepest match per step {depth}")
        print(f"B={B} phrases {phrases}\n free {free}\n with {toks}")
        assert toks != free
        assert max(depth) >= 2                                      # a phrase was spelled out two tokens deep at least
        assert any(in_E) and not all(x == B for x in in_E)          # both paths of the stage ran
        if B > 1:
            assert any(0 < x < B for x in in_E)                     # ... at some step side by side in one launch
        starts = {i[0] for i, _ in phrases}
        assert all(set(t) & starts for t in toks)                   # every row emitted a token it never emits by itself
    finally:
        all_off(c)


def test_q8_device_loop_equals_host_loop_equals_rule(gpu, tiny_q8_gguf):
    m = qasr.Model(tiny_q8_gguf)
    c = qasr.Context(m, max_batch=3, max_ctx=640)
    try:
        pcms = clips(3, 9200)
        phrases, free = build_phrases(c, pcms)
        toks, edited = run_three_ways(c, pcms, phrases, {})
        _, depth = check_against_rule(c, pcms, toks, edited, phrases, {})
        assert toks != free and max(depth) >= 2
    finally:
        c.close()
        m.close()


# ------------------------------------------- together with the other constraints
@pytest.mark.parametrize("B", [1, 3, 9])
def test_phrases_with_ban_penalty_and_bias(tiny, B):
    _, c = tiny
    pcms = clips_of(B)
    try:
        phrases, free = build_phrases(c, pcms)
        # the bias list holds a phrase token (biased and boosted), the penalty reaches the phrase tokens once emitted
        # (penalised, biased and boosted), and the bigram ban stops a phrase from being spelled a second time
        rule = dict(n=2, p=1.3, bias={phrases[0][0][1]: -1.5, phrases[1][0][0]: 0.75, 0: 5.0})
        toks, edited = run_three_ways(c, pcms, phrases, rule)
        assert not any(cu.repeats_ngram(t, 2) for t in toks)
        in_E, depth = check_against_rule(c, pcms, toks, edited, phrases, rule)
        assert max(depth) >= 2
        banned_boosted = 0
        for b in range(B):
            for k in range(STEPS):
                bon, _ = pu.bonuses(phrases, toks[b][:k])
                banned_boosted += len(set(bon) & cu.banned(toks[b][:k], 2))
        assert banned_boosted > 0                                   # some boosted column was banned, and stayed -inf
    finally:
        all_off(c)


def test_logprobs_and_topk_are_the_boosted_rows(tiny):
    """option token_logprobs: log softmax(l')[token]; option top_k: entry 0 the chosen token, the values l''s"""
    _, c = tiny
    pcms = clips(3)
    c.set_option("token_logprobs", 1)
    c.set_option("top_k", 4)
    try:
        phrases, free = build_phrases(c, pcms)
        c.set_phrases(phrases)
        feats, ids, pos = prompts(c, pcms)
        lg, tok = c.prefill(ids, feats, pos)
        seen = [[int(t)] for t in tok]
        for k in range(1, 7):
            lg, tok = c.decode_step([s[-1] for s in seen], [len(ids[b]) + k - 1 for b in range(3)])
            lp, (tid, tlp) = c.step_logprobs(3), c.step_topk(3)
            for b in range(3):
                assert tid[b, 0] == tok[b] and bits(tlp[b, 0]) == bits(lp[b])
                assert abs(float(lp[b]) - su.logsoftmax64(lg[b], int(tok[b]))) <= 2e-5
                order = np.argsort(cu.argmax_key(lg[b], np.arange(lg.shape[1])))[::-1][:4]      # (the keys are distinct)
                assert tid[b].tolist() == order.tolist()
                seen[b].append(int(tok[b]))
        r = c.transcribe(pcms, max_tokens=7, ignore_eos=True)
        assert r.tokens == seen and all(r.topk[b][0][:, 0].tolist() == seen[b] for b in range(3))
        assert seen != [t[:7] for t in free]
    finally:
        all_off(c)
        c.set_option("token_logprobs", 0)
        c.set_option("top_k", 0)


@pytest.mark.parametrize("N", [1, 3])
def test_sampling_draws_from_the_boosted_rows(tiny, N):
    """T = 5: every draw a candidate of l' within sample_util's band, the run the host loop's; n_best = N: every (clip,
    sample) against a row decoded from scratch under its identity"""
    _, c = tiny
    pcms, T, min_p = clips(2), 5.0, 0.0
    rule = dict(n=2, p=1.3, bias={0: 5.0})
    rows = [pcms[g] for g in range(2) for _ in range(N)]
    clip, sample = [g for g in range(2) for _ in range(N)], list(range(N)) * 2
    try:
        phrases, _ = build_phrases(c, pcms)
        turn_on(c, **rule)
        c.set_phrases(phrases)
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
        check_against_rule(c, rows, toks, edited, phrases, rule, drawn=True)
    finally:
        c.set_sampling(0)
        all_off(c)


# ------------------------------------------------------------ graph captures
def test_list_changes_capture_no_graph(tiny):
    _, c = tiny
    pcms = clips(3)
    try:
        phrases, free = build_phrases(c, pcms)
        # a constraint that edits nothing keeps the stage on throughout (a graph captured before any list was set)
        turn_on(c, bias={0: -0.0})
        assert c.transcribe(pcms, max_tokens=8, ignore_eos=True).tokens == [t[:8] for t in free]
        caps = c.get_option("graph_captures")
        outs = []
        big = [([int(x) for x in 2000 + np.arange(16) + 16 * k], 1.0) for k in range(4096)]
        for ph in (phrases, phrases[:1], big, phrases[1:], None, phrases):
            c.set_phrases(ph)
            outs.append(c.transcribe(pcms, max_tokens=8, ignore_eos=True).tokens)
        assert c.get_option("graph_captures") == caps
        assert outs[0] == outs[5] and outs[0] != outs[4] and outs[4] == [t[:8] for t in free] and outs[1] != outs[3]
        # phrases alone keep the stage on: turning the other constraint off captures nothing either
        c.set_constraints()
        assert c.transcribe(pcms, max_tokens=8, ignore_eos=True).tokens == outs[0]
        turn_on(c, n=2)
        c.set_phrases()
        c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert c.get_option("graph_captures") == caps
        # everything off: the greedy graphs were kept beside the stage's
        all_off(c)
        c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        off_caps = c.get_option("graph_captures")
        c.set_phrases(phrases)
        all_off(c)
        assert c.transcribe(pcms, max_tokens=8, ignore_eos=True).tokens == [t[:8] for t in free]
        assert c.get_option("graph_captures") == off_caps
    finally:
        all_off(c)


# --------------------------------------------- greedy around a phrase run
def test_greedy_bit_identical_around_a_phrase_run(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=9, max_ctx=640)
    try:
        c.set_option("token_logprobs", 1)
        c.set_option("top_k", 3)
        for pcms in (clips(1, 9600), clips(9, 9600)):
            before = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            c.set_phrases([([1000, 1001, 1002], 100.0)])
            con = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            c.set_phrases()
            after = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            assert con.tokens != before.tokens and after.tokens == before.tokens
            assert all(1000 in t for t in con.tokens)
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
        assert c.get_phrases() == []
        for ph in ([[V]], [[-1]], [[1] * 17], [[]], [([3], 0.0)], [([3], 100.5)], [([3], float("nan"))], [([3], float("inf"))],
                   [[k % 100] for k in range(4097)]):
            with pytest.raises(qasr.QasrError):
                c.set_phrases(ph)
            assert c.get_phrases() == [], ph
        p, _keep = qasr.make_phrases([[1, 2]])
        p.ids = None
        assert lib.qasr_set_phrases(c.h, C.byref(p)) == QASR_ERR_ARG
        c.set_phrases([[V - 1], ([0, 1, 2], 100.0), [5] * 16, [5] * 16], boost=2.5)
        assert c.get_phrases() == [([V - 1], 2.5), ([0, 1, 2], 100.0), ([5] * 16, 2.5), ([5] * 16, 2.5)]
        out, ids = qasr.Phrases(), np.zeros(4, np.int32)
        i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        assert lib.qasr_get_phrases(c.h, C.byref(out), i32p(ids), None, None, 4, 0) == QASR_ERR_ARG
        assert lib.qasr_get_phrases(c.h, C.byref(out), None, i32p(ids), None, 0, 3) == QASR_ERR_ARG
        assert lib.qasr_get_phrases(c.h, C.byref(out), None, None, None, 0, 0) == 0 and out.n_phrases == 4
        c.set_phrases([])
        assert c.get_phrases() == []
        assert lib.qasr_set_phrases(c.h, None) == 0
        pcms = clips(3, 9700)
        g = c.transcribe(pcms[:1], max_tokens=4, ignore_eos=True)
        c.set_phrases([([1000, 1001], 100.0)])
        with pytest.raises(qasr.QasrError, match="stream"):
            c.run_stream(_queue([(0, pcms[0], 3)]), max_tokens=4, ignore_eos=True)
        c.stage_audio(pcms)
        with pytest.raises(qasr.QasrError, match="stream"):
            c.run_stream_staged(_queue([0]), max_tokens=4, ignore_eos=True)
        toks, nt = np.zeros((4, 4), np.int32), np.zeros(4, np.int32)
        c.stage_audio(pcms[:1])
        c.set_option("beam_width", 2)
        assert lib.qasr_run(c.h, 4, 1, i32p(toks), nt.ctypes.data_as(C.POINTER(C.c_int)), None) == QASR_ERR_STATE
        assert "beam" in lib.qasr_last_error().decode()
        c.set_option("beam_width", 0)
        seen = []
        c.set_token_callback(lambda seq, k, t: seen.append((seq, k, t)))       # a token callback sees the boosted tokens
        r = c.transcribe(pcms[:1], max_tokens=6, ignore_eos=True)
        c.set_token_callback(None)
        assert [t for _, _, t in seen] == r.tokens[0] and r.tokens[0][0] == 1000 and r.tokens[0][:4] != g.tokens[0]
        c.stage_audio(pcms)                                                     # run_staged: a subset of the pool
        sub = c.run_staged([2, 0], max_tokens=6, ignore_eos=True)
        assert sub.tokens[1] == r.tokens[0] and sub.tokens[0][0] == 1000
        # scoring is unaffected
        a = c.score([0], [g.tokens[0]])[0]
        c.set_phrases()
        b = c.score([0], [g.tokens[0]])[0]
        assert np.array_equal(bits(a.logprobs), bits(b.logprobs)) and np.array_equal(a.greedy_ids, b.greedy_ids)
        assert c.transcribe(pcms[:1], max_tokens=4, ignore_eos=True).tokens == g.tokens
    finally:
        c.close()
        m.close()


def test_aligner_models_ignore_phrases(gpu, tmp_path):
    path = str(tmp_path / "al-tiny.gguf")
    qasr.write_synthetic_gguf(path, "aligner-tiny", 42, 1)
    m = qasr.Model(path)
    c = qasr.Context(m, max_batch=1, max_ctx=2048)
    try:
        assert m.is_aligner
        pcm = qasr.synth_pcm(9800, SR)
        ids, _ = m.align_tokenize("ab cd ef")
        before = c.align(pcm, ids)
        c.set_phrases([([1000, 1001], 100.0), ([int(ids[0])], 100.0)])
        assert c.get_phrases() == [([1000, 1001], 100.0), ([int(ids[0])], 100.0)]
        after = c.align(pcm, ids)
        assert before[0] == after[0] and len(before[0]) > 0
    finally:
        c.close()
        m.close()


# ------------------------------------------------------------- text and CLI
def test_string_phrases_install_both_tokenisations(tiny):
    m, c = tiny
    try:
        c.set_phrases(["ab cd", ("Hi", 7.5), [3, 4]], boost=2.0)
        ab = m.tokenize("ab cd")
        hi = m.tokenize("Hi")
        sp = m.phrase_tokenize("x")[1][0]
        assert m.phrase_tokenize("ab cd") == [ab, [sp] + ab]
        assert c.get_phrases() == [(ab, 2.0), ([sp] + ab, 2.0), (hi, 7.5), ([sp] + hi, 7.5), ([3, 4], 2.0)]
        with pytest.raises(qasr.QasrError, match="empty"):
            c.set_phrases(["  "])
    finally:
        all_off(c)


def test_cli_hotword_flags(tiny, tiny_gguf, tmp_path):
    """qwen3-asr-cli --hotword --hotwords-file --hotword-boost: the text Context.transcribe gives under the same phrases"""
    m, c = tiny
    cli = os.path.join(os.path.dirname(qasr.LIB_PATH), "qwen3-asr-cli")
    wav = str(tmp_path / "clip.wav")
    qasr.write_wav(wav, clips(1)[0])
    pcm16, _ = qasr.load_wav(wav)   # (the file's 16-bit samples)
    free = c.transcribe([pcm16], max_tokens=12, ignore_eos=False).tokens[0]
    try:
        c.set_phrases(["zq xj", ("Hi there", 90.0), "kw"], boost=100.0)
        want = c.transcribe([pcm16], max_tokens=12, ignore_eos=False).tokens[0]
    finally:
        all_off(c)
    assert want != free
    words = tmp_path / "words.txt"
    words.write_text("# two hotwords, the first with its own boost\nHi there\t90\n\nkw\n")
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(cli))
    base = [cli, "-m", tiny_gguf, "-f", wav, "--max-tokens", "12", "--no-timing"]
    r = subprocess.run(base + ["--hotword", "zq xj", "--hotwords-file", str(words), "--hotword-boost", "100"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == m.detokenize(want) + "\n", (r.stdout, want)
    bad = subprocess.run(base + ["--hotword", "a b c d e f g h i"], capture_output=True, text=True, env=env, timeout=120)
    assert bad.returncode != 0 and "1..16" in bad.stderr, bad.stderr
