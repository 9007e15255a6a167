"""Teacher-forced scoring without a GPU: the entry points' declarations and argument errors, the host
plan of qasr_score (csrc/score_host.h, through tools/score_host_check.cpp), and the float32 restatement
of the score head's reduction order (tests/score_util.py) against float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import qasr
import score_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QASR_ERR_ARG = 1
NAMES = ("qasr_prefill_score", "qasr_score", "qasr_kt_score_head")


def test_score_symbols_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "qasr_capi.h")).read()
    decl = set(re.findall(r"\b(qasr_[a-z0-9_]+)\s*\(", hdr))
    lib = qasr.lib()
    for n in NAMES:
        assert n in decl and hasattr(lib, n), n
    assert set(NAMES[:2]) <= set(qasr.EXPORTS) and NAMES[2] not in qasr.EXPORTS
    assert re.search(r"#define\s+QASR_SCORE_MAX_HYP\s+8\b", hdr)
    assert hasattr(qasr.Context, "score") and hasattr(qasr.Context, "prefill_score")
    assert [f for f in qasr.Score.__dataclass_fields__] == ["logprobs", "greedy_ids", "greedy_logprobs", "sum"]


def test_score_calls_reject_null_arguments_without_a_device(built):
    """a null context or null arrays: minus QASR_ERR_ARG (both return a count) before anything touches a device"""
    lib = qasr.lib()
    i1, t1, f1 = (C.c_int * 1)(1), (C.c_int32 * 1)(0), (C.c_float * 1)()
    assert lib.qasr_score(None, i1, t1, i1, 1, 1, f1, t1, f1, None, None) == -QASR_ERR_ARG and lib.qasr_last_error()
    assert lib.qasr_prefill_score(None, t1, i1, None, None, None, None, None, 1, t1, f1, t1, f1, 1) == -QASR_ERR_ARG
    su.ScoreCall   # (the harness entry: null -> QASR_ERR_ARG, not a count)
    lib.qasr_kt_score_head.argtypes = [C.c_int, C.c_void_p]
    lib.qasr_kt_score_head.restype = C.c_int
    assert lib.qasr_kt_score_head(0, None) == QASR_ERR_ARG


# ------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("score_host") / "score_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "qwen3-asr.cpp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "score_host_check.cpp"), "-o", exe], check=True)
    return exe


def plan(checker, tmp_path, clips, n_tokens, P, eos, max_batch, tokens=None, eos_id=7):
    """one case through the program -> "error ..." or the parsed plan"""
    total = sum(n_tokens)
    tokens = list(range(100, 100 + total)) if tokens is None else tokens
    ints = lambda a: " ".join(str(int(x)) for x in a)
    path = tmp_path / "case.txt"
    path.write_text(f"{len(clips)} {int(eos)} {len(P)} {max_batch} {eos_id}\n{ints(clips)}\n{ints(n_tokens)}\n{ints(P)}\n{ints(tokens)}\n")
    out = subprocess.run([checker, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    if out[0].startswith("error"):
        return out[0]
    res = {"plan": None, "seq": [], "p1": [], "chunk": [], "p2": [], "fork": []}
    for line in out:
        k, *v = line.split()
        v = [int(x) for x in v]
        if k == "plan":
            res["plan"] = v
        else:
            res[k].append(v)
    return res


def test_plan_groups_interleaved_sequences(checker, tmp_path):
    """sequences of one clip not adjacent in the input: groups in order of first appearance, outputs in input order"""
    clips, nt, P = [2, 0, 2, 1, 0, 2], [3, 1, 0, 1, 2, 2], [20, 23, 26]
    r = plan(checker, tmp_path, clips, nt, P, True, 16)
    assert r["plan"] == [3, 3, sum(nt) + 6]
    # seq: s group slot out_off n_out
    assert [x[1] for x in r["seq"]] == [0, 1, 0, 2, 1, 0]
    assert [x[2] for x in r["seq"]] == [0, 3, 1, 6, 4, 2]
    assert [x[3] for x in r["seq"]] == [0, 4, 6, 7, 9, 12] and [x[4] for x in r["seq"]] == [n + 1 for n in nt]
    # pass 1: the last row of each group's prompt (groups: clip 2, 0, 1 -> P 26, 20, 23) against the first token / the EOS
    last = {0: 25, 1: 45, 2: 68}
    toks = list(range(100, 100 + sum(nt)))
    first = [100, 103, 7, 104, 105, 107]
    assert r["p1"] == [[last[g], first[s], o] for s, (g, o) in enumerate(zip([0, 1, 0, 2, 1, 0], [0, 4, 6, 7, 9, 12]))]
    # pass 2: sequence 2 (empty) feeds nothing; every other one its tokens at its clip's prompt length
    assert r["chunk"] == [[0, 3, 0, 26], [1, 1, 3, 20], [3, 1, 6, 23], [4, 2, 4, 20], [5, 2, 2, 26]]
    rows = [x[0] for x in r["p2"]]
    assert rows == list(range(9))
    assert [x[1] for x in r["p2"]] == [101, 102, 7, 7, 7, 106, 7, 108, 7]
    assert [x[2] for x in r["p2"]] == [1, 2, 3, 5, 8, 10, 11, 13, 14]
    outs = sorted([x[2] for x in r["p1"]] + [x[2] for x in r["p2"]])
    assert outs == list(range(sum(nt) + 6))   # every entry exactly once
    # the fork: the group's other used slots take [0, P) of its first
    assert r["fork"] == [[0, 0, 0], [0, 0, 26], [0, 0, 26], [3, 0, 0], [3, 0, 20], [3, 0, 0], [6, 0, 0], [6, 0, 0], [6, 0, 0]]
    assert toks[0] == first[0]


@pytest.mark.parametrize("n_hyp,ok", [(1, True), (8, True), (9, False)])
def test_plan_hypotheses_per_clip(checker, tmp_path, n_hyp, ok):
    r = plan(checker, tmp_path, [0] * n_hyp, [2] * n_hyp, [30], True, 64)
    if not ok:
        assert r == "error more than 8 hypotheses of one clip"
        return
    assert r["plan"] == [1, n_hyp, 3 * n_hyp] and [x[2] for x in r["seq"]] == list(range(n_hyp))
    assert [x[2] for x in r["fork"]] == [0] + [30] * (n_hyp - 1)


def test_plan_slots_against_max_batch(checker, tmp_path):
    """D x G: 2 clips, 3 hypotheses of one -> 6 slots"""
    args = ([0, 1, 0, 0], [1, 1, 1, 1], [30, 31], True)
    assert plan(checker, tmp_path, *args, 6)["plan"][:2] == [2, 3]
    assert plan(checker, tmp_path, *args, 5).startswith("error distinct clips x hypotheses")
    assert plan(checker, tmp_path, [0, 2], [1, 1], [30, 31], True, 8) == "error staged clip index out of range"


def test_plan_empty_hypothesis(checker, tmp_path):
    """with the EOS an empty hypothesis scores the EOS from the prompt's last row; without, it yields nothing --
    and a one-token hypothesis feeds nothing either"""
    r = plan(checker, tmp_path, [0, 0, 0], [0, 3, 1], [30], True, 4)
    assert [x[4] for x in r["seq"]] == [1, 4, 2] and r["p1"][0] == [29, 7, 0]
    assert r["chunk"] == [[1, 3, 1, 30], [2, 1, 2, 30]]
    r = plan(checker, tmp_path, [0, 0, 0], [0, 3, 1], [30], False, 4)
    assert [x[4] for x in r["seq"]] == [0, 3, 1] and [x[2] for x in r["p1"]] == [0, 3]
    assert r["chunk"] == [[1, 2, 1, 30]] and [x[2] for x in r["p2"]] == [1, 2]
    assert plan(checker, tmp_path, [0], [0], [30], False, 1)["plan"] == [1, 1, 0]


def test_randomised_plans(checker):
    """the program's own checks over its fixed cases and 300 random plans: every (row, target) pair exactly once,
    every slot inside its group, output offsets contiguous"""
    out = subprocess.run([checker, "--self", "300"], check=True, capture_output=True, text=True).stdout
    assert "300 random plans clean" in out


# ------------------------------------------------ the reduction order, float32
@pytest.mark.parametrize("R,N,nv,K", [(5, 640, 600, 256), (9, 8960, 8900, 256)])
def test_simulated_order_within_the_bar(R, N, nv, K):
    """the per-tile sums and the merge order of score_head.hip restated in float32 numpy: against float64 the
    error is far inside the 2e-5 bar (full width, 17 x 151,936: 6.2e-7, DESIGN.md "Teacher-forced scoring")"""
    A, W, tg = su.make_case(1000 + R, R, N, K, nv)
    ref, lp, glp, bound = su.reference(A, W, tg, nv)
    lg = np.zeros((R, N), np.float32)
    lg[:, :nv] = ref.astype(np.float32)
    lg[:, nv:] = 1e30   # columns past n_valid must not matter
    sim = su.simulate_lp(lg, tg, nv)
    err = np.abs(sim.astype(np.float64) - lp).max()
    # (the float32 rounding of the logits themselves moves lp by up to 2 * 2^-24 * max |logit|)
    assert err <= su.LSE_BAR / 4 + 2 * 2.0 ** -24 * np.abs(ref).max(), err
    assert sim[0] == np.float32(-np.log(np.float64(nv)))   # the all-zero row: the column count exactly
