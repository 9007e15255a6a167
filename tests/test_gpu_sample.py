"""Temperature sampling (Context.set_sampling) on the tiny model: the device loop against a host loop over
the stage calls, every drawn token against the normative rule on the logits the same call returned
(tests/sample_util.py's band), the n_best fork against decoding every (clip, sample) from scratch, EOS
handling, the captured steps serving any temperature, and the greedy paths left as they were.

A decode output row depends only on its own inputs, bit for bit (tests/test_gpu_batch.py), and a draw only
on (seed, clip, sample, t) and its row's logits, so everything but the band is exact: tokens and the bits of
every log-probability and sum.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import qasr
import sample_util as su
from beam_util import prompts
from topk_util import gguf_tensor

pytestmark = pytest.mark.gpu
SR = 16000
QASR_ERR_ARG, QASR_ERR_STATE = 1, 5
LP_BAR = 2e-5   # tests/test_gpu_logprobs.py's bar for the fp32 log-sum-exp over 151,936 columns
SEED = 0xA5A5F00D0BADC0DE
f32 = np.float32


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


def host_loop(c, pcms, T, min_p, seed, clip, sample, max_tokens, stats=None):
    """sampling over prefill / set_sample_streams / decode_step (n_best plays no part at stage level): per row the
    tokens and their log-probabilities; every draw checked against the logits its call returned"""
    B = len(pcms)
    c.set_sampling(T, min_p, seed, 1)
    keep = c.get_option("token_logprobs")
    c.set_option("token_logprobs", 1)
    try:
        feats, ids, pos = prompts(c, pcms)
        P = [len(x) for x in ids]
        c.set_sample_streams(clip, sample, [0] * B)
        toks, lps = [[] for _ in range(B)], [[] for _ in range(B)]
        und = n = 0
        for k in range(max_tokens):
            if k == 0:
                logits, tok = c.prefill(ids, feats, pos)
            else:
                logits, tok = c.decode_step([t[-1] for t in toks], [P[b] + k - 1 for b in range(B)])
            lp = c.step_logprobs(B)
            for b in range(B):
                und += not su.check_draw(logits[b], int(tok[b]), None, T, min_p, seed, clip[b], sample[b], k, what=f"step {k} row {b}")
                n += 1
                want = su.logsoftmax64(logits[b], int(tok[b]))
                assert abs(float(lp[b]) - want) <= LP_BAR, (k, b, float(lp[b]), want)
                toks[b].append(int(tok[b]))
                lps[b].append(f32(lp[b]))
        assert und <= n // 100, (und, n)
        if stats is not None:
            stats.update(undecided=und, draws=n)
    finally:
        c.set_option("token_logprobs", keep)
    return toks, lps


def cut_at_eos(toks, lps, eos):
    """a hypothesis as the run returns it: (tokens, logprobs, fp32 in-order sum counting a popped EOS)"""
    acc, out_t, out_l = f32(0), [], []
    for t, l in zip(toks, lps):
        acc = f32(acc + f32(l))
        if t == eos:
            break
        out_t.append(t)
        out_l.append(l)
    return out_t, out_l, acc


@pytest.mark.parametrize("B", [1, 3, 9])
def test_transcribe_equals_host_loop(tiny, B):
    """1, 3 and 9 rows: the fused batch-1 launches, the GEMV path and the decode-batch path"""
    _, c = tiny
    pcms, T, mp = clips(B), 5.0, 0.0   # (the tiny model's rows are peaked: a high temperature, so that draws leave the argmax)
    want_t, want_l = host_loop(c, pcms, T, mp, SEED, list(range(B)), [0] * B, 8)
    c.set_sampling(T, mp, SEED, 1)
    c.set_option("token_logprobs", 1)
    try:
        r = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        again = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        c.set_sampling(T, mp, SEED + 1, 1)
        other = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
    finally:
        c.set_option("token_logprobs", 0)
        c.set_sampling(0)
    assert r.tokens == want_t and again.tokens == r.tokens and other.tokens != r.tokens
    assert np.array_equal(bits(r.logprobs), bits(want_l)) and np.array_equal(bits(again.logprobs), bits(r.logprobs))
    assert [s[0].tokens for s in r.samples] == r.tokens and all(len(s) == 1 for s in r.samples)
    assert np.array_equal(bits([s[0].logprobs for s in r.samples]), bits(r.logprobs))
    greedy = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
    assert greedy.samples is None and greedy.tokens != r.tokens


def test_transcribe_equals_host_loop_q8_with_min_p(gpu, tiny_q8_gguf):
    m = qasr.Model(tiny_q8_gguf)
    c = qasr.Context(m, max_batch=3, max_ctx=640)
    try:
        pcms = clips(3, 9200)
        want_t, _ = host_loop(c, pcms, 1.5, 0.2, SEED, [0, 1, 2], [0] * 3, 6)
        c.set_sampling(1.5, 0.2, SEED, 1)
        assert c.transcribe(pcms, max_tokens=6, ignore_eos=True).tokens == want_t
    finally:
        c.close()
        m.close()


def test_one_clip_at_two_pool_positions_under_one_identity(tiny):
    _, c = tiny
    pcm = clips(1, 9300)[0]
    try:
        same, _ = host_loop(c, [pcm, pcm, pcm], 5.0, 0.0, SEED, [5, 5, 6], [0, 0, 0], 6)
        assert same[0] == same[1] and same[2] != same[0]
        c.stage_audio([pcm, pcm, pcm])   # run_staged keys its draws by the pool index, not by the row
        c.set_sampling(5.0, 0.0, SEED, 1)
        a = c.run_staged([0, 2], max_tokens=6, ignore_eos=True)
        b = c.run_staged([2, 1, 0], max_tokens=6, ignore_eos=True)
        assert a.tokens[0] == b.tokens[2] and a.tokens[1] == b.tokens[0] and b.tokens[0] != b.tokens[1]
    finally:
        c.set_sampling(0)


def test_n_best_equals_every_sample_decoded_from_scratch(tiny):
    """n_best = 4, two ragged clips: one prefill a clip and one fork, against eight rows prefilled one by one"""
    _, c = tiny
    pcms, N, T = clips(2, 9400), 4, 5.0
    assert len({len(x) for x in prompts(c, pcms)[1]}) == 2
    rows = [pcms[0]] * N + [pcms[1]] * N
    want_t, want_l = host_loop(c, rows, T, 0.0, SEED, [0] * N + [1] * N, list(range(N)) * 2, 8)
    try:
        c.set_sampling(T, 0.0, SEED, N)
        r = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
        assert r.logprobs is None and r.topk is None and [len(s) for s in r.samples] == [N, N]
        for g in range(2):
            for i in range(N):
                s = r.samples[g][i]
                assert s.tokens == want_t[g * N + i], (g, i)
                assert np.array_equal(bits(s.logprobs), bits(want_l[g * N + i]))
                assert bits(s.sum_logprob) == bits(cut_at_eos(s.tokens, s.logprobs, -1)[2])
            assert r.tokens[g] == r.samples[g][0].tokens
            assert len({tuple(s.tokens) for s in r.samples[g]}) == N
        c.set_sampling(T, 0.0, SEED, 1)
        assert c.transcribe(pcms, max_tokens=8, ignore_eos=True).tokens == r.tokens   # sample 0 is the n_best = 1 run
    finally:
        c.set_sampling(0)


def test_slice_count_option_changes_no_draw(tiny):
    """option sample_slices (the workgroups a row's key kernel is spread over; 0 = the launcher's choice):
    the draws, their log-probabilities and the greedy run are bit-identical at any value"""
    _, c = tiny
    pcms = clips(3, 9450)
    try:
        c.set_option("token_logprobs", 1)
        greedy = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        c.set_sampling(5.0, 0.0, SEED, 1)
        want = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        for slices in (1, 7, 1000):
            c.set_option("sample_slices", slices)
            r = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
            assert r.tokens == want.tokens and np.array_equal(bits(r.logprobs), bits(want.logprobs)), slices
        c.set_sampling(0)
        g = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        assert g.tokens == greedy.tokens and np.array_equal(bits(g.logprobs), bits(greedy.logprobs))
        assert qasr.lib().qasr_ctx_set_option(c.h, b"sample_slices", -1) == QASR_ERR_ARG
    finally:
        c.set_option("sample_slices", 0)
        c.set_option("token_logprobs", 0)
        c.set_sampling(0)


# --------------------------------------------------------------------- EOS
@pytest.fixture(scope="module")
def eos_model(tiny, tiny_gguf, tmp_path_factory):
    """tests/test_gpu_beam.py's model: the EOS row of the embedding a copy of row t, t the token a greedy run of a
    fixed clip emits most often -- wherever t is a candidate, EOS is one at the same logit"""
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
    yield m, pcm
    m.close()


def test_eos_ends_samples_and_counts_in_their_sums(eos_model):
    """min_p = 0.5 at a low temperature keeps the draws near the greedy token, so EOS (its exact tie) is drawn
    within a few steps; ignore_eos on, off and on again on one context replays the captured steps"""
    m, pcm = eos_model
    N, T, mp, MT = 4, 0.3, 0.5, 24
    eos = int(m.hp.eos_id)
    c = qasr.Context(m, max_batch=N, max_ctx=640)
    try:
        full_t, full_l = host_loop(c, [pcm] * N, T, mp, SEED, [0] * N, list(range(N)), MT)
        assert any(eos in t for t in full_t), full_t
        c.set_sampling(T, mp, SEED, N)
        runs = [c.transcribe([pcm], max_tokens=MT, ignore_eos=ign) for ign in (True, False, True)]
        for i in range(N):
            assert runs[0].samples[0][i].tokens == full_t[i] and runs[2].samples[0][i].tokens == full_t[i]
            tk, lp, acc = cut_at_eos(full_t[i], full_l[i], eos)
            s = runs[1].samples[0][i]
            assert s.tokens == tk and np.array_equal(bits(s.logprobs), bits(lp)) and bits(s.sum_logprob) == bits(acc)
            if eos in full_t[i]:   # the sum counts the popped EOS step
                own = cut_at_eos(tk, lp, -1)[2]
                assert eos not in s.tokens and f32(s.sum_logprob) < own
        assert runs[1].tokens[0] == runs[1].samples[0][0].tokens
        if all(eos in t[:8] for t in full_t):
            assert runs[1].timings.n_decode_steps < MT - 1   # every sample ended: the loop stopped at its next look
    finally:
        c.close()


# ------------------------------------------------- graphs, greedy untouched
def test_temperature_change_recaptures_nothing(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    pcms = clips(3, 9500)
    try:
        c = qasr.Context(m, max_batch=3, max_ctx=640)
        c.set_sampling(3.0, 0.0, SEED, 1)
        a = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        caps = c.get_option("graph_captures")
        assert caps >= 1
        c.set_sampling(6.0, 0.001, SEED ^ 0xFFFF, 1)
        b = c.transcribe(pcms, max_tokens=6, ignore_eos=True)
        assert c.get_option("graph_captures") == caps and b.tokens != a.tokens
        sp = c.get_sampling()
        assert (f32(sp.temperature), f32(sp.min_p), sp.seed, sp.n_best) == (f32(6.0), f32(0.001), SEED ^ 0xFFFF, 1)
        c.close()
        c = qasr.Context(m, max_batch=3, max_ctx=640)
        c.set_sampling(6.0, 0.001, SEED ^ 0xFFFF, 1)
        assert c.transcribe(pcms, max_tokens=6, ignore_eos=True).tokens == b.tokens   # a fresh context's result
        c.close()
    finally:
        m.close()


def test_greedy_bit_identical_around_a_sampling_run(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=9, max_ctx=640)
    try:
        c.set_option("token_logprobs", 1)
        c.set_option("top_k", 3)
        for pcms in (clips(1, 9600), clips(9, 9600)):
            before = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            c.set_sampling(5.0, 0.0, SEED, 1)
            smp = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            c.set_sampling(0)
            after = c.transcribe(pcms, max_tokens=8, ignore_eos=True)
            assert smp.samples is not None and smp.tokens != before.tokens
            assert after.samples is None and after.tokens == before.tokens
            assert np.array_equal(bits(after.logprobs), bits(before.logprobs))
            for b in range(len(pcms)):
                assert np.array_equal(after.topk[b][0], before.topk[b][0]) and np.array_equal(bits(after.topk[b][1]), bits(before.topk[b][1]))
                # while sampling, top_k is unchanged: entry 0 is the step's greedy token (the first step's logits are the greedy run's)
                ids, lps = smp.topk[b]
                assert ids[0, 0] == before.tokens[b][0] and bits(lps[0])[0] == bits(before.logprobs[b])[0]
                assert (np.diff(lps, axis=1) <= 0).all()
                # ... and token_logprobs reports the drawn token's value: never above the greedy one
                assert (np.asarray(smp.logprobs[b], f32) <= lps[:, 0]).all()
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
        tok, lp, s, n = (C.c_int32 * (8 * 640))(), (C.c_float * (8 * 640))(), (C.c_float * 8)(), (C.c_int * 8)()
        one = (C.c_int32 * 4)(0, 0, 0, 0)
        assert lib.qasr_set_sample_streams(c.h, one, one, one, 1) == QASR_ERR_STATE     # sampling is off
        assert lib.qasr_get_samples(c.h, 0, tok, lp, n, s, 8, 640) == -QASR_ERR_STATE   # nothing has run
        for T, mp, nb in ((100.5, 0, 1), (float("nan"), 0, 1), (1, -0.1, 1), (1, 1.5, 1), (1, float("nan"), 1), (1, 0, 0), (1, 0, 9)):
            sp = qasr.Sampling(T, mp, 1, nb)
            assert lib.qasr_set_sampling(c.h, C.byref(sp)) == QASR_ERR_ARG, (T, mp, nb)
        assert c.get_sampling().temperature == 0
        c.set_sampling(100.0, 1.0, 2 ** 64 - 1, 8)
        sp = c.get_sampling()
        assert (sp.temperature, sp.min_p, sp.seed, sp.n_best) == (100.0, 1.0, 2 ** 64 - 1, 8)
        assert lib.qasr_set_sampling(c.h, None) == 0 and c.get_sampling().temperature == 0
        pcms = clips(3, 9700)
        g = c.transcribe(pcms[:1], max_tokens=4, ignore_eos=True)
        assert g.samples is None and lib.qasr_get_samples(c.h, 0, tok, lp, n, s, 8, 640) == -QASR_ERR_STATE
        c.set_sampling(0.8, 0.0, 1, 2)
        minus = (C.c_int32 * 4)(0, -1, 0, 0)
        assert lib.qasr_set_sample_streams(c.h, one, minus, one, 2) == QASR_ERR_ARG
        assert lib.qasr_set_sample_streams(c.h, one, one, one, 5) == QASR_ERR_ARG        # more rows than max_batch
        with pytest.raises(qasr.QasrError):   # 3 clips x 2 rows > max_batch 4
            c.transcribe(pcms, max_tokens=4, ignore_eos=True)
        c.set_option("token_logprobs", 1)
        r = c.transcribe(pcms[:2], max_tokens=4, ignore_eos=True)
        assert len(r.samples) == 2 and lib.qasr_get_samples(c.h, 1, tok, None, n, s, 8, 640) == 2
        assert lib.qasr_get_samples(c.h, 2, tok, lp, n, s, 8, 640) == -QASR_ERR_ARG      # no such clip
        assert lib.qasr_get_samples(c.h, 0, tok, lp, n, s, 1, 640) == -QASR_ERR_ARG      # room for one hypothesis
        assert lib.qasr_get_samples(c.h, 0, tok, lp, n, s, 8, 3) == -QASR_ERR_ARG        # rows shorter than the tokens
        assert lib.qasr_get_logprobs(c.h, lp, 4, 4) == QASR_ERR_STATE                     # an n_best >= 2 run: qasr_get_samples'
        with pytest.raises(qasr.QasrError):
            c.run_stream(_queue([(0, pcms[0], 3)]), max_tokens=4, ignore_eos=True)
        c.stage_audio(pcms)
        with pytest.raises(qasr.QasrError):
            c.run_stream_staged(_queue([0]), max_tokens=4, ignore_eos=True)
        toks, nt = np.zeros((4, 4), np.int32), np.zeros(4, np.int32)
        c.stage_audio(pcms[:1])
        c.set_option("beam_width", 2)
        assert lib.qasr_run(c.h, 4, 1, toks.ctypes.data_as(C.POINTER(C.c_int32)), nt.ctypes.data_as(C.POINTER(C.c_int)), None) == QASR_ERR_STATE
        c.set_option("beam_width", 0)
        c.set_token_callback(lambda *a: None)
        assert lib.qasr_run(c.h, 4, 1, toks.ctypes.data_as(C.POINTER(C.c_int32)), nt.ctypes.data_as(C.POINTER(C.c_int)), None) == QASR_ERR_STATE
        seen = []
        c.set_sampling(0.8, 0.0, 1, 1)   # n_best = 1: the ordinary loop, callback included
        c.set_token_callback(lambda seq, k, t: seen.append((seq, k, t)))
        r1 = c.transcribe(pcms[:1], max_tokens=4, ignore_eos=True)
        c.set_token_callback(None)
        assert [t for _, _, t in seen] == r1.tokens[0] and r1.tokens[0] == r.samples[0][0].tokens
        c.set_sampling(0)
        g2 = c.transcribe(pcms[:1], max_tokens=4, ignore_eos=True)
        assert g2.tokens == g.tokens and g2.samples is None and g2.logprobs is not None
    finally:
        c.close()
        m.close()


# ---------------------------------------------------------------------- CLI
def test_cli_sampling_flags(tiny, tiny_gguf, tmp_path):
    """qwen3-asr-cli --temperature --min-p --seed --n-best: sample 0's text on stdout, every sample with its sum on
    stderr in the layout of --beams, as Context.transcribe gives them"""
    m, c = tiny
    cli = os.path.join(os.path.dirname(qasr.LIB_PATH), "qwen3-asr-cli")
    pcm = clips(1, 9950)[0]
    wav = str(tmp_path / "clip.wav")
    qasr.write_wav(wav, pcm)
    pcm16, _ = qasr.load_wav(wav)   # (the file's 16-bit samples)
    try:
        c.set_sampling(0.7, 0.05, 1234, 3)
        want = c.transcribe([pcm16], max_tokens=6, ignore_eos=False)
    finally:
        c.set_sampling(0)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(cli))
    r = subprocess.run([cli, "-m", tiny_gguf, "-f", wav, "--max-tokens", "6", "--no-timing", "--temperature", "0.7", "--min-p", "0.05",
                        "--seed", "1234", "--n-best", "3"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == m.detokenize(want.tokens[0]) + "\n", (r.stdout, want.tokens[0])
    assert f"{len(want.samples[0])} samples" in r.stderr
    for i, s in enumerate(want.samples[0]):
        assert f"[{i}] {s.sum_logprob:.4f}  {len(s.tokens)} tokens" in r.stderr, (i, r.stderr)
    bad = subprocess.run([cli, "-m", tiny_gguf, "-f", wav, "--temperature", "0.7", "--n-best", "9"], capture_output=True, text=True, env=env,
                         timeout=120)
    assert bad.returncode != 0 and "--n-best takes 1..8" in bad.stderr
