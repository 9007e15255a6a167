"""Option kv_fp8 in the engine, tiny synthetic model: wherever the fp16 caches change, "k8" / "v8" equal the rule
(tests/kv_fp8_util.py) of "kc" / "vc" below each slot's n_kv; with the option at 0 nothing exists and nothing moves."""
import ctypes as C

import numpy as np
import pytest

import kv_fp8_util as k8u
import qasr
from beam_util import prompts

pytestmark = pytest.mark.gpu
B, CTX, S = 12, 128, 2


@pytest.fixture(scope="module")
def model(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    yield m
    m.close()


def clips(n):
    return [qasr.synth_pcm(9300 + i, 8000 + 1600 * (i % 5)) for i in range(n)]


def shadow_is_the_rule(c, n_kv, s):
    kc, vc, q8k, q8v = (k8u.read_cache(c, n) for n in ("kc", "vc", "k8", "v8"))
    for b, n in enumerate(n_kv):
        assert n > 0
        assert np.array_equal(q8k[:, b, :, :n], k8u.rule(kc[:, b, :, :n], s)), ("k8", b)
        assert np.array_equal(q8v[:, b, :, :n], k8u.rule(vc[:, b, :, :n], s)), ("v8", b)


def test_shadow_follows_the_cache(model):
    c = qasr.Context(model, max_batch=B, max_ctx=CTX)
    c.set_option("kv_fp8_exp", S)
    c.set_option("kv_fp8", 1)
    feats, ids, apos = prompts(c, clips(B))
    n = np.array([len(x) for x in ids], np.int32)
    _, tok = c.prefill(ids, feats, apos)
    shadow_is_the_rule(c, n, S)
    path = []
    for rows in (B, B, B, 4, 4, B):
        _, tok[:rows] = c.decode_step(tok[:rows].copy(), n[:rows].copy())
        n[:rows] += 1
        path.append(c.get_option("kv_fp8_path"))
        if rows != B or len(path) in (3, 6):   # after each phase (and each 4-row step)
            shadow_is_the_rule(c, n, S)
    assert path == [1, 1, 1, 0, 0, 1]
    # a fork with a swap (rows 0, 1) and a shared parent (rows 1, 2 <- 0), then the range of row 3 alone
    top = int(n[:4].min())
    c.kv_fork([1, 0, 0, 3], [0, 2, 0, 0], [top, top, top - 1, 0], 4)
    shadow_is_the_rule(c, [top] * 3 + [int(n[3])] + list(n[4:]), S)
    c.set_option("kv_fp8_exp", 0)   # the exponent changing under the option re-derives the whole shadow
    shadow_is_the_rule(c, [top] * 3 + [int(n[3])] + list(n[4:]), 0)
    c.close()


def test_shadow_after_a_beam_run(model):
    c = qasr.Context(model, max_batch=B, max_ctx=CTX, kv_fp8=1)
    c.set_option("beam_width", 4)
    pcms, T = clips(3), 6
    P = [len(x) for x in prompts(c, pcms)[1]]
    c.transcribe(pcms, max_tokens=T, ignore_eos=True)
    assert c.get_option("kv_fp8_path") == 1   # 4 x 3 rows a step
    shadow_is_the_rule(c, [P[b // 4] + T - 1 for b in range(B)], 0)
    c.close()


def test_option_off_changes_nothing_and_bad_values(model):
    plain, off = qasr.Context(model, max_batch=B, max_ctx=CTX), qasr.Context(model, max_batch=B, max_ctx=CTX)
    off.set_option("kv_fp8", 0)
    outs = []
    for c in (plain, off):
        feats, ids, apos = prompts(c, clips(B))
        lg0, tok = c.prefill(ids, feats, apos)
        lg1, tok1 = c.decode_step(tok, [len(x) for x in ids])
        outs.append((lg0.view(np.uint32), tok, lg1.view(np.uint32), tok1))
        assert c.get_option("kv_fp8_path") == 0
        k8u.read_cache(c, "k8", expect_rc=k8u.QASR_ERR_STATE)
        k8u.read_cache(c, "v8", expect_rc=k8u.QASR_ERR_STATE)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    L = qasr.lib()
    for name, bad in (("kv_fp8", 2), ("kv_fp8", -1), ("kv_fp8_exp", 9), ("kv_fp8_exp", -9)):
        assert L.qasr_ctx_set_option(off.h, name.encode(), C.c_int(bad)) == k8u.QASR_ERR_ARG
    plain.close()
    off.close()
