"""KV-cache fork (qasr_kv_fork, kv_fork_kernel): the kernel on caller-supplied
caches against numpy, exact uint16 equality over the whole allocations, and
the engine entry through one decode step.

The elements of K, V and V^T count up modulo a prime below 2^16, so no two
slots, layers, heads, keys or dimensions hold the same run of values: a copy
from the wrong place, a write outside the range or a lost blend of a partly
covered V^T block all change some element.  The last
slot(s) of every layer are guard slots no row may touch (0xFF bytes), as is the
V^T read-ahead slack of every slot.
"""
import numpy as np
import pytest

import qasr
from beam_util import fork_ref, prompts, run_fork, vt_ctx

pytestmark = pytest.mark.gpu
LAYERS, HEADS, MAX_CTX = 2, 2, 40


def caches(slots, guard_slots):
    S = slots + guard_slots
    kc = (np.arange(LAYERS * S * HEADS * MAX_CTX * 128, dtype=np.int64) % 65521).astype(np.uint16).reshape(LAYERS, S, HEADS, MAX_CTX, 128)
    vc = ((np.arange(kc.size, dtype=np.int64) * 7 + 3) % 65519).astype(np.uint16).reshape(kc.shape)
    nb = vt_ctx(MAX_CTX) // 8
    vt = ((np.arange(LAYERS * S * HEADS * nb * 128 * 8, dtype=np.int64) * 13 + 5) % 65497).astype(np.uint16).reshape(LAYERS, S, HEADS, nb, 128, 8)
    for a in (kc, vc, vt):
        a[:, slots:] = 0xFFFF
    return kc, vc, vt


# (B, group, slots): slot 4 (slot 8 at B = 8) is never a row; one more guard slot after it
SHAPES = [(4, 4, 5), (4, 2, 5), (3, 3, 5), (8, 8, 9)]
RANGES = {"empty": (9, 9), "all": (0, 40), "blocks": (8, 16), "ragged": (5, 21), "inside_a_block": (7, 9), "per_row": None}


def parents(kind, B, group):
    own = np.arange(B)
    p = own.copy()
    for g0 in range(0, B, group):
        n = group
        if kind == "swap" and n >= 2:
            p[g0], p[g0 + 1] = g0 + 1, g0
        elif kind == "cycle3" and n >= 3:
            p[g0:g0 + 3] = [g0 + 1, g0 + 2, g0]
        elif kind == "cycle3":   # (groups of 2: their only cycle)
            p[g0], p[g0 + 1] = g0 + 1, g0
        elif kind == "one_parent":
            p[g0:g0 + n] = g0 + n - 1
        elif kind == "mix":      # row 0 keeps itself, the others take their left neighbour (a chain through moved rows)
            p[g0 + 1:g0 + n] = own[g0:g0 + n - 1]
    return p


@pytest.mark.parametrize("rng_name", list(RANGES))
@pytest.mark.parametrize("kind", ["identity", "swap", "cycle3", "one_parent", "mix"])
@pytest.mark.parametrize("B,group,slots", SHAPES)
def test_fork_kernel_equals_numpy(gpu, B, group, slots, kind, rng_name):
    kc, vc, vt = caches(slots, 1)
    par = parents(kind, B, group)
    if RANGES[rng_name] is None:
        frm = np.array([(3 * b + 1) % 17 for b in range(B)])
        to = np.array([min(40, frm[b] + 2 + 5 * b) for b in range(B)])
    else:
        frm, to = np.full(B, RANGES[rng_name][0]), np.full(B, RANGES[rng_name][1])
    want = fork_ref(kc.copy(), vc.copy(), vt.copy(), par, frm, to, MAX_CTX)
    got = run_fork(kc, vc, vt, par, frm, to, group, 1)
    for name, g, w in zip(("kc", "vc", "vt"), got, want):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:4])
        assert (g[:, slots:] == 0xFFFF).all(), name      # the guard slot
        assert np.array_equal(g[:, B:slots], w[:, B:slots])   # slots >= B
    assert np.array_equal(got[2][:, :, :, MAX_CTX // 8:], want[2][:, :, :, MAX_CTX // 8:])   # the V^T slack (fork_ref never writes it)
    if kind != "identity" and rng_name != "empty":
        assert not np.array_equal(got[0], caches(slots, 1)[0])   # something moved


def test_fork_grid_smaller_than_the_range_is_the_callers_bound(gpu):
    """blocks bounds the keys a launch can reach (the engine sizes it by the step's bucket): rows past it stay"""
    kc, vc, vt = caches(5, 1)
    par, frm, to = np.array([1, 0, 2, 3]), np.zeros(4, int), np.full(4, 40)
    want = fork_ref(kc.copy(), vc.copy(), vt.copy(), par, frm, np.full(4, 16), MAX_CTX)
    got = run_fork(kc, vc, vt, par, frm, to, 4, 1, blocks=2)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def tiny(gpu, tiny_gguf):
    m = qasr.Model(tiny_gguf)
    c = qasr.Context(m, max_batch=4, max_ctx=640)
    yield m, c
    c.close()
    m.close()


def test_engine_fork_swaps_two_clips(tiny):
    """prefill two clips, swap their cache slots, feed each row the other's token at the other's position:
    the logits rows equal the unforked step's rows, swapped, bit for bit"""
    _, c = tiny
    pcms = [qasr.synth_pcm(9100, 16000), qasr.synth_pcm(9101, 16000 + 4000)]
    feats, ids, pos = prompts(c, pcms)
    P = np.array([len(x) for x in ids], np.int32)
    assert P[0] != P[1]
    _, am = c.prefill(ids, feats, pos)
    plain, _ = c.decode_step(am, P)
    _, am2 = c.prefill(ids, feats, pos)
    assert np.array_equal(am, am2)
    c.kv_fork([1, 0], [0, 0], [int(P.max())] * 2, 2)
    swapped, _ = c.decode_step(am[::-1].copy(), P[::-1].copy())
    assert np.array_equal(swapped.view(np.uint32), plain[::-1].view(np.uint32))
    assert not np.array_equal(plain[0], plain[1])


def test_engine_fork_argument_errors(tiny):
    _, c = tiny
    ok = ([1, 0], [0, 0], [8, 8], 2)
    c.kv_fork(*ok)
    for bad in (([2, 0], [0, 0], [8, 8], 2),          # parent outside B
                ([2, 3, 0, 1], [0] * 4, [8] * 4, 2),  # parent outside the row's group
                ([1, 0], [0, 0], [8, 641], 2),        # past max_ctx
                ([1, 0], [-1, 0], [8, 8], 2),
                ([1, 0, 2], [0] * 3, [8] * 3, 2),     # B no multiple of group
                ([0] * 5, [0] * 5, [8] * 5, 5),       # B > max_batch
                ([1, 0], [0, 0], [8, 8], 9), ([1, 0], [0, 0], [8, 8], 0)):
        with pytest.raises(qasr.QasrError):
            c.kv_fork(*bad)
    c.kv_fork([0, 1], [0, 0], [9999, 9999], 2)   # identity rows: a no-op whatever their range
