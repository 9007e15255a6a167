"""Beam search without a GPU: the numpy rule of beam_util.py on hand-made steps,
the host back-tracking and ranking code (csrc/beam_host.h, through
tools/beam_host_check.cpp) against it, and the argument errors of the new
entry points that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import qasr
from beam_util import NEG_INF, GroupState, beam_step, hypotheses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QASR_ERR_ARG = 1
EOS = 99
f32 = np.float32


def step(st, ids, lps, eos=EOS, P=20):
    return beam_step(st, np.array(ids, np.int32), np.array(lps, np.float32), eos, P)


# ---------------------------------------------------------------- the rule
def test_first_step_only_row_zero_contributes():
    """cum = {0, -inf, ...}: the W best of the one prefilled row, fork [0, P) from row 0"""
    st = GroupState(3)
    assert st.cum.tolist() == [0.0, -np.inf, -np.inf]
    row = [[5, 6, 7]] * 3, [[-0.5, -1.0, -2.0]] * 3
    tok, par, frm, to = step(st, *row)
    assert tok.tolist() == [5, 6, 7] and par.tolist() == [0, 0, 0]
    assert frm.tolist() == [0, 0, 0] and to.tolist() == [20, 20, 20]
    assert st.cum.tolist() == [f32(-0.5), f32(-1.0), f32(-2.0)] and st.t == 1 and not st.fin and not st.done
    assert st.hist[0][0].tolist() == [0, 0, 0]


def test_first_step_eos_leaves_a_dead_row():
    """an EOS among row 0's W: recorded (i < W), and the -inf candidate of row 1 fills the last row"""
    st = GroupState(2)
    tok, par, _, _ = step(st, [[EOS, 8]] * 2, [[-0.1, -3.0]] * 2)
    assert st.fin == [{"row": 0, "t": 0, "sum": f32(-0.1), "lp": f32(-0.1)}]
    assert tok.tolist() == [8, 8] and st.hist[0][0].tolist() == [0, 1] and par.tolist() == [0, 0]
    assert st.cum[0] == f32(-3.0) and st.cum[1] == NEG_INF


def test_score_ties_across_rows_and_ranks():
    """equal scores: lower row first, then lower rank"""
    st = GroupState(2, cum=np.array([-1.0, -1.5], np.float32), t=3)
    st.hist = [None] * 3
    # row 0: -1 + -1 = -2, -1 + -1 = -2 (ranks tie); row 1: -1.5 + -0.5 = -2 (rows tie), -1.5 + -0.75
    tok, par, frm, to = step(st, [[10, 11], [12, 13]], [[-1.0, -1.0], [-0.5, -0.75]])
    assert tok.tolist() == [10, 11] and par.tolist() == [0, 0]
    assert frm.tolist() == [20, 20] and to.tolist() == [23, 23]
    st = GroupState(2, cum=np.array([-1.5, -1.0], np.float32), t=3)
    st.hist = [None] * 3
    tok, par, _, _ = step(st, [[12, 13], [10, 11]], [[-0.5, -0.75], [-1.0, -1.25]])
    assert tok.tolist() == [12, 10] and par.tolist() == [0, 1]   # (-2, row 0), (-2, row 1)


def test_eos_inside_and_outside_the_first_w():
    st = GroupState(2, cum=np.array([-1.0, -2.0], np.float32), t=1)
    st.hist = [None]
    # order: (0,0) -1.1 tok 4; (0,1) -1.2 EOS at i = 1 < W: recorded; (1,0) -2.1 EOS at i = 2 >= W: dropped; (1,1) -2.5
    tok, par, _, _ = step(st, [[4, EOS], [EOS, 6]], [[-0.1, -0.2], [-0.1, -0.5]])
    assert len(st.fin) == 1 and st.fin[0]["row"] == 0 and st.fin[0]["t"] == 1 and st.fin[0]["sum"] == f32(-1.0) + f32(-0.2)
    assert tok.tolist() == [4, 6] and par.tolist() == [0, 1] and not st.done


def test_full_table_sets_done_and_freezes():
    st = GroupState(2, cum=np.array([-1.0, -1.0], np.float32), t=2)
    st.hist = [None] * 2
    st.fin = [{"row": 1, "t": 1, "sum": f32(-0.7), "lp": f32(-0.2)}]
    tok, par, _, _ = step(st, [[EOS, 4], [EOS, 5]], [[-0.1, -0.3], [-0.1, -0.4]])
    # (0,0) EOS recorded (table now full); (1,0) EOS at i = 1 but the table is full: dropped
    assert len(st.fin) == 2 and st.fin[1]["row"] == 0 and st.done == 3 and tok.tolist() == [4, 5]
    before = (st.cum.copy(), len(st.hist), st.t)
    tok, par, frm, to = step(st, [[1, 2], [3, 4]], [[-0.1, -0.3], [-0.1, -0.4]])
    assert tok is None and par.tolist() == [0, 1] and frm.tolist() == to.tolist() == [0, 0]
    assert np.array_equal(st.cum, before[0]) and (len(st.hist), st.t) == before[1:] and len(st.fin) == 2


def test_ignore_eos_never_finishes():
    st = GroupState(2)
    step(st, [[EOS, 3]] * 2, [[-0.1, -0.2]] * 2, eos=-1)
    assert not st.fin and st.hist[0][1].tolist() == [EOS, 3]


def test_ranking_and_its_ties():
    """sum / n in fp32, descending; equal: finished first, then the earlier record / lower row"""
    st = GroupState(2)
    step(st, [[7, 8]] * 2, [[-1.0, -2.0]] * 2)                         # rows: [7] -1, [8] -2
    step(st, [[EOS, 9], [EOS, 9]], [[-1.0, -3.0], [-2.0, -2.0]])       # (0,0) EOS -2 recorded; (1,0) EOS -4 at i = 2 dropped
    assert len(st.fin) == 1 and st.fin[0]["sum"] == f32(-2.0)
    assert st.cum.tolist() == [-4.0, -4.0] and st.hist[1][0].tolist() == [0, 1]
    hy = hypotheses(st)
    # finished {7, EOS}: -2 / 2 = -1; live [7, 9] and [8, 9]: -4 / 2 = -2 each, lower row first; W = 2 kept
    assert [(h.tokens, h.finished, h.n) for h in hy] == [([7], True, 2), ([7, 9], False, 2)]
    assert hy[0].sum == f32(-2.0) and hy[0].logprobs.tolist() == [-1.0]
    st2 = GroupState(2)
    step(st2, [[7, 8]] * 2, [[-1.0, -1.0]] * 2)
    step(st2, [[9, EOS], [5, 6]], [[-1.0, -1.0], [-1.0, -3.0]])        # (0,0) 9 -2; (0,1) EOS -2 at i = 1 recorded; (1,0) 5 -2
    hy = hypotheses(st2)   # all three at -1 a step: the finished one leads, then row 0
    assert [(h.tokens, h.finished) for h in hy] == [([7], True), ([7, 9], False)]


# ------------------------------------------- the C++ host code against the rule
def _hex(a):
    return " ".join(f"{int(x):08x}" for x in np.asarray(a, np.float32).view(np.uint32))


def _case(st, row0, stride, rng):
    """the state the device would leave for group st at rows row0 .. row0 + W - 1 of `stride` rows (the other
    rows hold noise), as beam_host_check's input"""
    W, T, R = st.W, st.t, row0 + st.W
    h_par, h_id = rng.integers(0, stride, (T, stride)), rng.integers(0, 1000, (T, stride))
    h_lp = rng.standard_normal((T, stride)).astype(np.float32)
    for s, (par, ids, lps) in enumerate(st.hist):
        h_par[s, row0:R], h_id[s, row0:R], h_lp[s, row0:R] = par + row0, ids, lps
    cum = rng.standard_normal(R).astype(np.float32)
    cum[row0:] = st.cum
    fin_row, fin_t = rng.integers(0, stride, R), rng.integers(0, 5, R)
    fin_sum, fin_lp = rng.standard_normal(R).astype(np.float32), rng.standard_normal(R).astype(np.float32)
    for e, f in enumerate(st.fin):
        fin_row[row0 + e], fin_t[row0 + e], fin_sum[row0 + e], fin_lp[row0 + e] = row0 + f["row"], f["t"], f["sum"], f["lp"]
    ints = lambda a: " ".join(str(int(x)) for x in np.asarray(a).ravel())
    return "\n".join([f"{W} {row0} {T} {stride} {len(st.fin)} {st.done}", ints(h_par), ints(h_id), _hex(h_lp.ravel()), _hex(cum),
                      ints(fin_row), ints(fin_t), _hex(fin_sum), _hex(fin_lp)]) + "\n"


def _random_group(rng, W, steps, p_eos):
    st = GroupState(W)
    for _ in range(steps):
        ids = np.stack([rng.permutation(50)[:W] for _ in range(W)]).astype(np.int32)
        ids[rng.random((W, W)) < p_eos] = EOS
        for r in range(W):   # a row's ids are distinct: at most one EOS
            e = np.flatnonzero(ids[r] == EOS)
            ids[r, e[1:]] = 60 + e[1:]
        # coarse values: equal scores and equal sum / n happen
        lps = -np.sort(rng.integers(1, 6, (W, W)), axis=1).astype(np.float32) / 4
        if st.t == 0:
            ids, lps = np.repeat(ids[:1], W, 0), np.repeat(lps[:1], W, 0)
        beam_step(st, ids, lps, EOS, 20)
    return st


def test_host_code_equals_the_rule(built, tmp_path):
    exe = str(tmp_path / "beam_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "qwen3-asr.cpp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "beam_host_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(77)
    groups, text = [], ""
    for W in (2, 3, 8):
        for steps, p_eos in ((1, 0.0), (1, 0.5), (4, 0.0), (6, 0.15), (9, 0.3)):
            st = _random_group(rng, W, steps, p_eos)
            groups.append(st)
            text += _case(st, row0=int(rng.integers(0, 3)) * W, stride=3 * W + 1, rng=rng)
    assert any(g.done for g in groups) and any(g.fin and not g.done for g in groups) and any(not g.fin for g in groups)
    path = tmp_path / "cases.txt"
    path.write_text(text)
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    at = 0
    for gi, st in enumerate(groups):
        want = hypotheses(st)
        assert out[at] == f"case {len(want)}", (gi, out[at])
        for i, h in enumerate(want):
            head, toks, lps = out[at + 1 + i].split("|")
            fin, n, s, nt = head.split()
            assert (int(fin), int(n), int(nt)) == (int(h.finished), h.n, len(h.tokens)), (gi, i)
            assert int(s, 16) == int(np.float32(h.sum).view(np.uint32)), (gi, i)
            assert [int(x) for x in toks.split()] == h.tokens, (gi, i)
            assert [int(x, 16) for x in lps.split()] == h.logprobs.view(np.uint32).tolist(), (gi, i)
        at += 1 + len(want)
    assert at == len(out)


# ------------------------------------------------------------ entry points
NAMES = ("qasr_kv_fork", "qasr_get_beams", "qasr_prefill_slots", "qasr_kt_kv_fork", "qasr_kt_beam_select")


def test_beam_symbols_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "qasr_capi.h")).read()
    decl = set(re.findall(r"\b(qasr_[a-z0-9_]+)\s*\(", hdr))
    lib = qasr.lib()
    for n in NAMES:
        assert n in decl and hasattr(lib, n), n
    assert set(NAMES[:3]) <= set(qasr.EXPORTS)
    assert re.search(r"#define\s+QASR_BEAM_MAX\s+8\b", hdr) and qasr.QASR_BEAM_MAX == 8
    assert '"beam_width" [QASR_BEAM_WIDTH]' in hdr


def test_beam_calls_reject_bad_arguments_without_a_device(built):
    """a null context or null arrays: QASR_ERR_ARG before anything touches a device
    (qasr_get_beams returns a count, so its errors are minus the code)"""
    lib = qasr.lib()
    i3 = (C.c_int * 3)(0, 0, 0)
    assert lib.qasr_kv_fork(None, i3, i3, i3, 3, 3) == QASR_ERR_ARG and lib.qasr_last_error()
    tok, lp, s = (C.c_int32 * 8)(), (C.c_float * 8)(), (C.c_float * 1)()
    n, fin = (C.c_int * 1)(), (C.c_int * 1)()
    assert lib.qasr_get_beams(None, 0, tok, lp, n, s, fin, 1, 8) == -QASR_ERR_ARG
    assert lib.qasr_ctx_set_option(None, b"beam_width", 4) == QASR_ERR_ARG
    assert lib.qasr_prefill_slots(None, tok, n, None, None, None, n, 1, None, None) == QASR_ERR_ARG
