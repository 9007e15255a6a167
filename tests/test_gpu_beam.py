"""Beam search (context option "beam_width") on the tiny model: the beam step
kernel against the numpy rule, the device loop against a host loop over the
stage calls, the fork against decoding from scratch, the oracle's view of the
returned sums, EOS handling, and the greedy path left as it was.

A decode output row depends only on its own inputs, bit for bit
(tests/test_gpu_batch.py), and the rule's arithmetic is one fp32 add a
candidate, so everything but the oracle comparison is exact: tokens, flags and
the bits of every log-probability and sum.
"""
import ctypes as C
import shutil

import numpy as np
import pytest

import oracle_py as op
import qasr
from beam_util import GroupState, backtrack, check_select, host_beam, prompts, same_hyps
from test_beam_host import EOS
from topk_util import gguf_tensor, logsoftmax64

pytestmark = pytest.mark.gpu
SR = 16000
QASR_ERR_ARG, QASR_ERR_STATE = 1, 5


# ------------------------------------------------------------ select kernel
def rows(ids, lps):
    return np.array(ids, np.int32), np.array(lps, np.float32)


def test_select_kernel_on_the_hand_made_steps(gpu):
    """the cases of tests/test_beam_host.py, two groups a launch where the states allow"""
    # first step; first step with an EOS (a dead row)
    st = [GroupState(3), GroupState(3)]
    check_select(3, st, *rows([[5, 6, 7], [EOS, 8, 9]] + [[0, 0, 0]] * 4, [[-0.5, -1.0, -2.0], [-0.1, -3.0, -4.0]] + [[0, 0, 0]] * 4), EOS, [20, 31])
    assert len(st[1].fin) == 1 and np.isneginf(st[1].cum[2])
    # ... and the step after it: the dead row's candidates sort last
    check_select(3, st, *rows([[1, 2, 3]] * 6, [[-1.0, -1.5, -2.0]] * 6), EOS, [20, 31])
    # score ties across rows and across ranks, either row order
    def at(cum, t):
        s = GroupState(2, cum=np.array(cum, np.float32), t=t)
        s.hist = [None] * t
        return s
    st = [at([-1.0, -1.5], 3), at([-1.5, -1.0], 3)]
    check_select(2, st, *rows([[10, 11], [12, 13], [12, 13], [10, 11]], [[-1.0, -1.0], [-0.5, -0.75], [-0.5, -0.75], [-1.0, -1.25]]), EOS, [20, 20])
    # EOS at index < W and >= W; a table that fills, then the frozen group beside a live one
    st = [at([-1.0, -2.0], 1), at([-1.0, -1.0], 1)]
    st[1].fin = [{"row": 1, "t": 0, "sum": np.float32(-0.7), "lp": np.float32(-0.7)}]
    o = check_select(2, st, *rows([[4, EOS], [EOS, 6], [EOS, 4], [EOS, 5]], [[-0.1, -0.2], [-0.1, -0.5], [-0.1, -0.3], [-0.1, -0.4]]), EOS, [20, 25])
    assert len(st[0].fin) == 1 and st[1].done == 2 and o["done"].tolist() == [0, 2]
    check_select(2, st, *rows([[1, 2], [3, 4]] * 2, [[-0.1, -0.3], [-0.1, -0.4]] * 2), EOS, [20, 25])
    assert st[1].t == 2 and st[0].t == 3
    # ignore_eos
    st = [GroupState(2)]
    check_select(2, st, *rows([[EOS, 3], [0, 0]], [[-0.1, -0.2], [0, 0]]), -1, [20])
    assert not st[0].fin


@pytest.mark.parametrize("W", [2, 3, 8])
def test_select_kernel_random_steps(gpu, W):
    """50 seeded steps of 3 groups: coarse log-probabilities (equal scores happen) and a random EOS rate,
    the states carried from step to step; a group that fills its table stays in the launch, frozen"""
    rng = np.random.default_rng(1000 + W)
    G, P = 3, [17, 40, 23]
    states = [GroupState(W) for _ in range(G)]
    seen_tie = seen_fin = seen_frozen = 0
    for step in range(50):
        if all(s.done for s in states) or step % 17 == 16:   # start over: first steps more than once
            states = [GroupState(W) for _ in range(G)]
        if any(s.t != states[0].t for s in states):
            states = [GroupState(W) for _ in range(G)]
        ids = np.stack([rng.permutation(40)[:W] for _ in range(G * W)]).astype(np.int32)
        eos_at = rng.random(G * W) < 0.5   # (an EOS in half the rows: at W = 8 a table fills within the 16 steps of a stretch)
        ids[eos_at, rng.integers(0, W, int(eos_at.sum()))] = EOS
        lps = (-np.sort(rng.integers(1, 9, (G * W, W)), axis=1) / 8).astype(np.float32)
        if step % 3 == 0:
            lps = (lps - np.abs(rng.standard_normal((G * W, 1))).astype(np.float32)).astype(np.float32)   # fine-grained rows too
        seen_frozen += sum(1 for s in states if s.done)
        check_select(W, states, ids, lps, EOS, P)
        seen_fin += sum(len(s.fin) for s in states)
        for s in states:
            seen_tie += len(set(s.cum.tolist())) < W
    assert seen_tie and seen_fin and seen_frozen, (seen_tie, seen_fin, seen_frozen)


# --------------------------------------------------- device loop, host loop
@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=12, max_ctx=640)
    yield m, c
    c.close()
    m.close()


def clips(n, seed=9300):
    return [qasr.synth_pcm(seed + i, SR + 4000 * (i % 5)) for i in range(n)]


def device_equals_host(c, pcms, W, max_tokens=10, ignore_eos=True):
    want = host_beam(c, pcms, W, max_tokens, ignore_eos)
    c.set_option("beam_width", W)
    try:
        r = c.transcribe(pcms, max_tokens=max_tokens, ignore_eos=ignore_eos)
    finally:
        c.set_option("beam_width", 0)
    assert r.logprobs is None and r.topk is None and len(r.beams) == len(pcms)
    for g, (hyps, _) in enumerate(want):
        same_hyps(r.beams[g], hyps)
        assert r.tokens[g] == hyps[0].tokens
        assert 1 <= len(hyps) <= W
    return r, want


@pytest.mark.parametrize("W", [2, 4, 8])
def test_device_loop_equals_host_loop_one_clip(tiny, W):
    _, c = tiny
    r, want = device_equals_host(c, clips(1), W)
    assert len(r.beams[0]) == W and all(len(b.tokens) == 10 and not b.finished for b in r.beams[0])
    assert len({tuple(b.tokens) for b in r.beams[0]}) == W   # W different hypotheses
    means = [np.float32(b.sum_logprob) / np.float32(10) for b in r.beams[0]]
    assert means == sorted(means, reverse=True)
    for b in r.beams[0]:   # the sum is the running fp32 sum of the per-token values, in order
        acc = np.float32(0)
        for v in b.logprobs:
            acc = np.float32(acc + np.float32(v))
        assert acc.view(np.uint32) == np.float32(b.sum_logprob).view(np.uint32)


def test_device_loop_equals_host_loop_three_ragged_clips(tiny):
    """12 rows: the decode-batch path"""
    _, c = tiny
    pcms = clips(3)
    r, _ = device_equals_host(c, pcms, 4)
    assert len({len(x) for x in prompts(c, pcms)[1]}) == 3   # ragged prompts


def test_device_loop_equals_host_loop_q8(gpu, tiny_q8_gguf):
    m = qasr.Model(tiny_q8_gguf)
    c = qasr.Context(m, max_batch=3, max_ctx=640)
    try:
        device_equals_host(c, clips(1, 9400), 3)
    finally:
        c.close()
        m.close()


def test_run_staged_and_max_tokens_one(tiny):
    _, c = tiny
    pcms = clips(3)
    c.set_option("beam_width", 2)
    try:
        full = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        c.stage_audio(pcms)
        sub = c.run_staged([2, 0], max_tokens=6, ignore_eos=True)
        assert sub.tokens == [full.tokens[2], full.tokens[0]]
        one = c.transcribe(pcms[:1], max_tokens=1, ignore_eos=True)   # the prefill's step alone: its two best tokens
        assert one.timings.n_decode_steps == 0 and [len(b.tokens) for b in one.beams[0]] == [1, 1]
        assert one.beams[0][0].tokens != one.beams[0][1].tokens and one.beams[0][0].logprobs[0] >= one.beams[0][1].logprobs[0]
    finally:
        c.set_option("beam_width", 0)


# ------------------------------------------------------ fork, from scratch
def test_fork_equals_decoding_from_scratch(tiny):
    """W identical prefilled rows: row r fed hypothesis r's whole sequence with no fork gives the last-step
    logits of the same prefill decoded along the recorded parents with kv_fork, bit for bit"""
    _, c = tiny
    W, T = 4, 6
    pcm = clips(1, 9500)
    (hyps, st), = host_beam(c, pcm, W, T, True)
    seqs = [backtrack(st, r, T - 1)[0] for r in range(W)]
    assert len({tuple(s) for s in seqs}) == W and any((st.hist[k][0] != np.arange(W)).any() for k in range(1, T))
    feats, ids, pos = prompts(c, pcm * W)
    P = len(ids[0])
    c.prefill(ids, feats, pos)
    for k in range(T):
        scratch, _ = c.decode_step([s[k] for s in seqs], [P + k] * W)
    c.prefill(ids, feats, pos)
    for k in range(T):
        par, tok, _ = st.hist[k]
        if k:
            c.kv_fork(par, [P] * W, [P + k] * W, W)
        forked, _ = c.decode_step(tok, [P + k] * W)
    assert np.array_equal(forked.view(np.uint32), scratch.view(np.uint32))
    assert len({forked[r].tobytes() for r in range(W)}) == W


# ------------------------------------------------------------------ oracle
@pytest.fixture(scope="module")
def oracle_rows(tiny_oracle):
    """the oracle's teacher-forced log softmax rows along a token sequence of one clip: rows(tokens) ->
    (per step float64 row, max |logits|).  One decoder: a sequence re-decodes only from where it leaves the
    previous one (forward rewrites the cache from that position on), so the hypotheses of both widths share
    their common prefixes' work."""
    pcm = clips(1, 9600)[0]
    feats = tiny_oracle.encode(op.log_mel(pcm))
    ids = tiny_oracle.prompt(feats.shape[0])
    d = op.OracleDecoder(tiny_oracle, 512)
    state = {"tokens": [], "lo": [d.forward(ids, 0, feats, 9)]}

    def rows(tokens):
        prev, lo = state["tokens"], state["lo"]
        keep = 0
        while keep < min(len(prev), len(tokens)) and prev[keep] == tokens[keep]:
            keep += 1
        keep = min(keep, len(lo) - 1)   # lo[k] is the row after tokens[:k]
        del lo[keep + 1:]
        for k in range(keep, len(tokens) - 1):
            lo.append(d.forward([tokens[k]], len(ids) + k))
        state["tokens"] = list(tokens)
        return [logsoftmax64(x) for x in lo[:len(tokens)]], max(float(np.abs(x).max()) for x in lo[:len(tokens)])
    return pcm, rows


@pytest.mark.parametrize("W", [2, 4])
def test_oracle_teacher_forced_sums(tiny, oracle_rows, parity, W):
    """every hypothesis' sum_logprob against the oracle's teacher-forced sum of log softmax at its tokens:
    within n x the per-token bar of the stream tests (2 * 1e-2 * max |oracle logits|)"""
    _, c = tiny
    pcm, rows = oracle_rows
    c.set_option("beam_width", W)
    try:
        r = c.transcribe([pcm], max_tokens=8, ignore_eos=True)
    finally:
        c.set_option("beam_width", 0)
    worst = 0.0
    assert len(r.beams[0]) == W
    for b in r.beams[0]:
        ls, scale = rows(b.tokens)
        n = len(b.tokens)
        total = sum(float(ls[k][t]) for k, t in enumerate(b.tokens))
        err = abs(total - float(b.sum_logprob))
        print(f"W={W} n={n} sum={b.sum_logprob:.6f} oracle={total:.6f} err={err:.3g} bar={n * 2e-2 * scale:.3g}")
        worst = max(worst, err / (n * 2e-2 * scale))
        assert err <= n * 2e-2 * scale, (err, n, scale)
    parity(f"tiny_beam_oracle_W{W}", worst_over_bound=worst)


# --------------------------------------------------------------------- EOS
@pytest.fixture(scope="module")
def eos_model(tiny, tiny_gguf, tmp_path_factory):
    """the tiny model with the EOS row of the embedding a copy of row t, t the token a greedy run of a fixed
    clip emits most often: wherever t leads a row's alternatives, EOS follows it at the same logit"""
    m0, c = tiny
    pcm = qasr.synth_pcm(9700, SR + 900)
    greedy = c.transcribe([pcm], max_tokens=12, ignore_eos=True).tokens[0]
    vals, counts = np.unique(greedy, return_counts=True)
    t, eos = int(vals[np.argmax(counts)]), int(m0.hp.eos_id)
    path = str(tmp_path_factory.mktemp("eos") / "tiny-eos.gguf")
    off, dims, typ = gguf_tensor(tiny_gguf, "token_embd.weight")
    assert typ == 1 and t != eos
    hidden = int(dims[0])
    shutil.copyfile(tiny_gguf, path)
    with open(path, "r+b") as f:
        f.seek(off + t * hidden * 2)
        row = f.read(hidden * 2)
        f.seek(off + eos * hidden * 2)
        f.write(row)
    m = qasr.Model(path)
    yield m, pcm, t, greedy
    m.close()


def test_eos_finishes_hypotheses_and_stops_early(eos_model):
    m, pcm, t, greedy = eos_model
    W, T = 2, 40
    c = qasr.Context(m, max_batch=W, max_ctx=640)
    try:
        r, want = device_equals_host(c, [pcm], W, max_tokens=T, ignore_eos=False)
        hyps, st = want[0]
        eos = int(m.hp.eos_id)
        print("greedy", greedy, "t", t, "done", st.done, "steps", r.timings.n_decode_steps, [(b.tokens, b.finished) for b in r.beams[0]])
        assert st.done and len(r.beams[0]) == W and all(b.finished for b in r.beams[0])
        assert r.timings.n_decode_steps < T - 1 and r.timings.n_decode_steps <= (st.done + 7) // 8 * 8   # stopped at the next look
        best = r.beams[0][0]
        assert eos not in best.tokens and r.tokens[0] == best.tokens
        # the sum counts the popped EOS step: it is below the tokens' own sum by that step's log-probability
        acc = np.float32(0)
        for v in best.logprobs:
            acc = np.float32(acc + np.float32(v))
        assert np.float32(best.sum_logprob) < acc
        f = st.fin[[i for i, x in enumerate(st.fin) if np.float32(x["sum"]) == np.float32(best.sum_logprob)][0]]
        assert np.float32(acc + f["lp"]).view(np.uint32) == np.float32(best.sum_logprob).view(np.uint32)
        full = c.transcribe([pcm], max_tokens=T, ignore_eos=True)   # greedy, EOS ignored: the option is back to 0
        assert len(full.tokens[0]) == T
    finally:
        c.close()


def test_ignore_eos_changes_between_runs_on_one_context(eos_model):
    """ignore_eos is a per-run argument: runs with it on, off and on again, on one context with no option
    touched in between (the captured steps are replayed), each equal the host loop's"""
    m, pcm, _, _ = eos_model
    W, T = 2, 24
    c = qasr.Context(m, max_batch=W, max_ctx=640)
    try:
        (want_ign, _), = host_beam(c, [pcm], W, T, True)
        (want_eos, st), = host_beam(c, [pcm], W, T, False)
        assert st.done and any(f["t"] > 0 for f in st.fin)   # a hypothesis finishes in a replayed decode step
        c.set_option("beam_width", W)
        runs = [c.transcribe([pcm], max_tokens=T, ignore_eos=ign) for ign in (True, False, True, False)]
    finally:
        c.close()
    for r, want in zip(runs, (want_ign, want_eos, want_ign, want_eos)):
        same_hyps(r.beams[0], want)
    assert not any(b.finished for b in runs[0].beams[0]) and all(b.finished for b in runs[1].beams[0])
    assert runs[0].timings.n_decode_steps == T - 1 and runs[1].timings.n_decode_steps < T - 1


# ---------------------------------------------------------- greedy untouched
def test_greedy_bit_identical_around_a_beam_run(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=8, max_ctx=640)
    try:
        c.set_option("token_logprobs", 1)
        pcms = clips(2, 9800)
        before = c.transcribe(pcms, max_tokens=10, ignore_eos=True)
        c.set_option("beam_width", 4)
        beam = c.transcribe(pcms, max_tokens=10, ignore_eos=True)
        assert beam.beams is not None and beam.logprobs is None
        c.set_option("beam_width", 0)
        after = c.transcribe(pcms, max_tokens=10, ignore_eos=True)
        c.set_option("beam_width", 1)
        one = c.transcribe(pcms, max_tokens=10, ignore_eos=True)
        for r in (after, one):
            assert r.beams is None and r.tokens == before.tokens
            assert np.array_equal(np.array(r.logprobs, np.float32).view(np.uint32), np.array(before.logprobs, np.float32).view(np.uint32))
    finally:
        c.close()
        m.close()


# ------------------------------------------------------------------- errors
def _queue(items):
    it = iter(items)
    return lambda: next(it, None)


def test_option_range_and_refusals(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=4, max_ctx=640)
    try:
        lib = qasr.lib()
        tok, lp, s = (C.c_int32 * (8 * 640))(), (C.c_float * (8 * 640))(), (C.c_float * 8)()
        n, fin = (C.c_int * 8)(), (C.c_int * 8)()
        for bad in (9, -1):
            assert lib.qasr_ctx_set_option(c.h, b"beam_width", bad) == QASR_ERR_ARG
        assert c.get_option("beam_width") == 0
        assert lib.qasr_get_beams(c.h, 0, tok, lp, n, s, fin, 8, 640) == -QASR_ERR_STATE   # nothing has run
        pcms = clips(3, 9900)
        c.set_option("top_k", 3)
        c.set_option("token_logprobs", 1)
        c.set_option("beam_width", 2)
        with pytest.raises(qasr.QasrError):   # 3 clips x 2 rows > max_batch 4
            c.transcribe(pcms, max_tokens=4, ignore_eos=True)
        r = c.transcribe(pcms[:2], max_tokens=4, ignore_eos=True)
        assert c.get_option("top_k") == 3 and len(r.beams) == 2   # the user's top_k is left alone
        assert lib.qasr_get_beams(c.h, 1, tok, None, n, s, fin, 8, 640) == 2
        assert lib.qasr_get_beams(c.h, 2, tok, lp, n, s, fin, 8, 640) == -QASR_ERR_ARG     # no such clip
        assert lib.qasr_get_beams(c.h, 0, tok, lp, n, s, fin, 1, 640) == -QASR_ERR_ARG     # room for one hypothesis
        assert lib.qasr_get_beams(c.h, 0, tok, lp, n, s, fin, 8, 3) == -QASR_ERR_ARG       # rows shorter than the tokens
        assert lib.qasr_get_logprobs(c.h, lp, 4, 4) == QASR_ERR_STATE and lib.qasr_get_topk(c.h, tok, lp, 4, 4, 3) == QASR_ERR_STATE
        with pytest.raises(qasr.QasrError):
            c.run_stream(_queue([(0, pcms[0], 3)]), max_tokens=4, ignore_eos=True)
        c.stage_audio(pcms)
        with pytest.raises(qasr.QasrError):
            c.run_stream_staged(_queue([0]), max_tokens=4, ignore_eos=True)
        c.set_token_callback(lambda *a: None)
        with pytest.raises(qasr.QasrError):
            c.transcribe(pcms[:1], max_tokens=4, ignore_eos=True)
        c.set_token_callback(None)
        c.set_option("beam_width", 0)
        assert lib.qasr_get_beams(c.h, 0, tok, lp, n, s, fin, 8, 640) == -QASR_ERR_STATE   # the option change drops the run
        g = c.transcribe(pcms, max_tokens=4, ignore_eos=True)   # greedy again, with its values
        assert g.beams is None and g.topk is not None and g.logprobs is not None
    finally:
        c.close()
        m.close()


# ---------------------------------------------------------------------- CLI
def test_cli_beam_width_and_beams(tiny, tiny_gguf, tmp_path):
    """qwen3-asr-cli --beam-width 2 --beams: the best hypothesis' text on stdout, every hypothesis with its
    sum on stderr, as Context.transcribe gives them (the C++ API's transcribe_params::beam_width underneath)"""
    import os
    import subprocess
    m, c = tiny
    cli = os.path.join(os.path.dirname(qasr.LIB_PATH), "qwen3-asr-cli")
    pcm = clips(1, 9950)[0]
    wav = str(tmp_path / "clip.wav")
    qasr.write_wav(wav, pcm)
    pcm16, _ = qasr.load_wav(wav)   # (the file's 16-bit samples)
    c.set_option("beam_width", 2)
    try:
        want = c.transcribe([pcm16], max_tokens=6, ignore_eos=False)
    finally:
        c.set_option("beam_width", 0)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(cli))
    r = subprocess.run([cli, "-m", tiny_gguf, "-f", wav, "--max-tokens", "6", "--no-timing", "--beam-width", "2", "--beams"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == m.detokenize(want.tokens[0]) + "\n", (r.stdout, want.tokens[0])
    assert f"{len(want.beams[0])} hypotheses" in r.stderr
    for i, b in enumerate(want.beams[0]):
        assert f"[{i}] {b.sum_logprob:.4f}  {len(b.tokens)} tokens" in r.stderr, (i, r.stderr)
    bad = subprocess.run([cli, "-m", tiny_gguf, "-f", wav, "--beam-width", "9"], capture_output=True, text=True, env=env, timeout=120)
    assert bad.returncode != 0 and "--beam-width takes 2..8" in bad.stderr
