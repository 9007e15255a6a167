"""Shared by the beam-search tests (context option "beam_width"): the numpy
restatement of the beam step and of the final ranking (DESIGN.md "Beam search";
the device kernel and the host code are held to it exactly), a host beam search
that drives only prefill, kv_fork, decode_step and step_topk, a numpy
reference of the KV-cache fork, and ctypes bindings of the two test-only
launchers (include/qasr_capi.h, csrc/kernel_harness.hip).

Rows are group-local here (0 .. W - 1); the device uses absolute rows g * W + i.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List

import numpy as np

GUARD = 3
NEG_INF = np.float32(-np.inf)


# ---------------------------------------------------------------- the rule
@dataclass
class GroupState:
    W: int
    cum: np.ndarray = None                     # [W] fp32
    fin: List[dict] = field(default_factory=list)   # {row, t, sum, lp}, at most W
    done: int = 0                              # 0, or the step count at which the table filled
    t: int = 0
    hist: List[tuple] = field(default_factory=list)   # per step (parent [W], id [W], lp [W])

    def __post_init__(self):
        if self.cum is None:
            self.cum = np.full(self.W, NEG_INF, np.float32)
            self.cum[0] = 0.0


def beam_step(st: GroupState, ids, lps, eos, P):
    """One step of one group.  ids / lps: [W][W] (row r's W best, descending); at
    st.t == 0 the caller passes the prefill's one row repeated W times.  eos < 0:
    no token ends a hypothesis.  Returns (tok, fork parent, frm, to), each [W],
    tok None where the group is frozen; updates st."""
    W = st.W
    ids, lps = np.asarray(ids, np.int32), np.asarray(lps, np.float32)
    own = np.arange(W, dtype=np.int32)
    if st.done:   # frozen: identity parents, no records
        return None, own, np.zeros(W, np.int32), np.zeros(W, np.int32)
    first = st.t == 0
    cand = [(np.float32(st.cum[r] + lps[r, j]), r, j) for r in range(W) for j in range(W)]   # one fp32 add each
    cand.sort(key=lambda c: (-float(c[0]), c[1], c[2]))   # score descending; equal: lower row, then lower rank
    tok, par, cum, lp = [], [], [], []
    for i, (score, r, j) in enumerate(cand):
        if len(tok) == W:
            break
        if int(ids[r, j]) == eos:
            if i < W and len(st.fin) < W:
                st.fin.append({"row": r, "t": st.t, "sum": score, "lp": lps[r, j]})
            continue
        tok.append(int(ids[r, j]))
        par.append(r)
        cum.append(score)
        lp.append(lps[r, j])
    assert len(tok) == W, "W * W candidates hold at most W EOS"
    st.cum = np.array(cum, np.float32)
    st.hist.append((np.array(par, np.int32), np.array(tok, np.int32), np.array(lp, np.float32)))
    fork_par = np.zeros(W, np.int32) if first else np.array(par, np.int32)   # first step: every row copies row 0
    frm = np.full(W, 0 if first else P, np.int32)
    to = np.full(W, P + st.t, np.int32)
    if len(st.fin) == W:
        st.done = st.t + 1
    st.t += 1
    return np.array(tok, np.int32), fork_par, frm, to


@dataclass
class Hyp:
    tokens: List[int]
    logprobs: np.ndarray     # fp32, one per token
    sum: np.float32
    n: int
    finished: bool


def backtrack(st: GroupState, row, t):
    """row `row` as it stood after step t: t + 1 tokens, oldest first"""
    tok, lp = [], []
    for s in range(t, -1, -1):
        par, ids, lps = st.hist[s]
        tok.append(int(ids[row]))
        lp.append(lps[row])
        row = int(par[row])
    return tok[::-1], np.array(lp[::-1], np.float32)


def hypotheses(st: GroupState) -> List[Hyp]:
    """finished in record order, then (unless the table filled) the live rows by
    row; ranked by sum / n in fp32, descending, ties in that order; at most W"""
    out = []
    for f in st.fin:
        tok, lp = backtrack(st, f["row"], f["t"] - 1) if f["t"] > 0 else ([], np.zeros(0, np.float32))
        out.append(Hyp(tok, lp, np.float32(f["sum"]), f["t"] + 1, True))   # (the EOS is popped; n and sum count it)
    if not st.done and st.t > 0:
        for b in range(st.W):
            tok, lp = backtrack(st, b, st.t - 1)
            out.append(Hyp(tok, lp, np.float32(st.cum[b]), st.t, False))
    keyed = sorted(range(len(out)), key=lambda i: (-float(np.float32(out[i].sum) / np.float32(out[i].n)), i))
    return [out[i] for i in keyed[:st.W]]


# --------------------------------------------------------- host beam search
def prompts(c, pcms):
    feats = c.encode(c.mel(pcms))
    built = [c.model.build_prompt(f.shape[0]) for f in feats]
    return feats, [b[0] for b in built], [b[1] for b in built]


def host_beam(c, pcms, W, max_tokens, ignore_eos):
    """Beam search on the host over prefill, kv_fork, decode_step and step_topk of
    context c (option top_k = W while it runs, beam_width 0).  Returns, per clip,
    (hypotheses, GroupState)."""
    G, B = len(pcms), len(pcms) * W
    eos = -1 if ignore_eos else int(c.model.hp.eos_id)
    keep = c.get_option("top_k"), c.get_option("beam_width")
    c.set_option("beam_width", 0)
    c.set_option("top_k", W)
    try:
        feats, ids, pos = prompts(c, pcms)
        P = [len(x) for x in ids]
        c.prefill(ids, feats, pos, want_logits=False, slots=[g * W for g in range(G)])
        tk_id, tk_lp = c.step_topk(G)
        states = [GroupState(W) for _ in range(G)]
        tok = np.zeros(B, np.int32)

        def select(first):
            par, frm, to = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
            for g, st in enumerate(states):
                rows = slice(g * W, g * W + W)
                i_g = np.repeat(tk_id[g:g + 1], W, 0) if first else tk_id[rows]
                l_g = np.repeat(tk_lp[g:g + 1], W, 0) if first else tk_lp[rows]
                t_g, p_g, f_g, e_g = beam_step(st, i_g, l_g, eos, P[g])
                if t_g is not None:
                    tok[rows] = t_g
                par[rows], frm[rows], to[rows] = p_g + g * W, f_g, e_g
            c.kv_fork(par, frm, to, W)

        select(True)
        n_past = np.repeat(np.array(P, np.int32), W)
        for k in range(1, max_tokens):
            if all(st.done for st in states):
                break
            _, am = c.decode_step(tok, n_past, want_logits=False)
            for g, st in enumerate(states):   # a frozen group keeps stepping on the greedy token, as on the device
                if st.done:
                    tok[g * W:g * W + W] = am[g * W:g * W + W]
            tk_id, tk_lp = c.step_topk(B)
            select(False)
            n_past = n_past + 1
        return [(hypotheses(st), st) for st in states]
    finally:
        c.set_option("top_k", keep[0])
        c.set_option("beam_width", keep[1])


def same_hyps(got, want):
    """a clip's qasr.Beam list against the host loop's Hyp list, bit for bit"""
    assert len(got) == len(want), (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tokens == b.tokens, (i, a.tokens, b.tokens)
        assert a.finished == b.finished, i
        assert np.float32(a.sum_logprob).view(np.uint32) == np.float32(b.sum).view(np.uint32), (i, a.sum_logprob, b.sum)
        assert np.array_equal(np.array(a.logprobs, np.float32).view(np.uint32), b.logprobs.view(np.uint32)), i


# --------------------------------------------------------- fork reference
def vt_ctx(max_ctx):
    return (max_ctx + 63) // 64 * 64 + 384


def vt_from_v(vt, v):
    """scatter v [..., max_ctx, 128] into the V^T layout [..., vt_ctx / 8, 128, 8] (kernels.h vt_index)"""
    k = np.arange(v.shape[-2])
    vt[..., k >> 3, :, k & 7] = np.moveaxis(v, -2, 0)


def fork_ref(kc, vc, vt, parent, frm, to, max_ctx):
    """kc / vc [layers][slots][heads][max_ctx][128], vt [layers][slots][heads][vt_ctx / 8][128][8]:
    what qasr_kv_fork leaves, from copies taken before any write"""
    k0, v0, t0 = kc.copy(), vc.copy(), vt.copy()
    for b, p in enumerate(parent):
        f, e = max(int(frm[b]), 0), min(int(to[b]), max_ctx)
        if p == b or f >= e:
            continue
        kc[:, b, :, f:e] = k0[:, p, :, f:e]
        vc[:, b, :, f:e] = v0[:, p, :, f:e]
        k = np.arange(f, e)
        vt[:, b, :, k >> 3, :, k & 7] = t0[:, p, :, k >> 3, :, k & 7]
    return kc, vc, vt


# ------------------------------------------------------------------ bindings
_P = C.c_void_p


class ForkCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("layers", "n_kv_head", "max_ctx", "slots", "guard", "B", "group", "blocks")] + [
        (n, _P) for n in ("parent", "frm", "to", "kc", "vc", "vt")] + [("declined", C.c_int32)]


class SelectCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("W", "G", "t", "eos", "guard")] + [(n, _P) for n in (
        "ids", "lps", "P", "cum", "fin_row", "fin_t", "fin_sum", "fin_lp", "n_fin", "done", "t_out",
        "tok", "parent", "frm", "to", "h_par", "h_id", "h_lp")] + [("declined", C.c_int32)]


def _lib():
    import qasr
    L = qasr.lib()
    for name, typ in (("qasr_kt_kv_fork", ForkCall), ("qasr_kt_beam_select", SelectCall)):
        fn = getattr(L, name)
        fn.argtypes = [C.c_int, C.POINTER(typ)]
        fn.restype = C.c_int
    return L


def _ok(L, rc):
    """a HIP error leaves the device in an unknown state: nothing more is launched on it in this session"""
    if rc == 4:   # QASR_ERR_DEVICE
        import pytest
        pytest.exit(f"HIP error in a kernel test: {L.qasr_last_error()}", returncode=3)
    assert rc == 0, (rc, L.qasr_last_error())


def _ptr(a):
    return a.ctypes.data_as(_P)


def run_fork(kc, vc, vt, parent, frm, to, group, guard_slots, blocks=0):
    """kc / vc / vt as fork_ref takes them, the last guard_slots slots of every layer guard slots;
    the arrays are updated in place"""
    L = _lib()
    layers, S, heads, max_ctx = kc.shape[:4]
    par, f, t = (np.ascontiguousarray(x, np.int32) for x in (parent, frm, to))
    assert kc.flags.c_contiguous and vc.flags.c_contiguous and vt.flags.c_contiguous
    c = ForkCall(layers=layers, n_kv_head=heads, max_ctx=max_ctx, slots=S - guard_slots, guard=guard_slots, B=len(par),
                 group=group, blocks=blocks, parent=_ptr(par), frm=_ptr(f), to=_ptr(t), kc=_ptr(kc), vc=_ptr(vc), vt=_ptr(vt))
    _ok(L, L.qasr_kt_kv_fork(0, C.byref(c)))
    assert not c.declined
    return kc, vc, vt


def run_select(W, states, ids, lps, eos, P):
    """beam_select_kernel on G groups in the state of `states` (all at the same step); ids / lps
    [G * W][W] as the kernel reads them (step 0: row g).  Returns the outputs as a dict of arrays,
    the out rows with their guard rows ([1 + 2 GUARD][G * W])."""
    L = _lib()
    G, R = len(states), len(states) * W
    t = states[0].t
    assert all(s.t == t for s in states)
    cum = np.concatenate([s.cum for s in states]).astype(np.float32)
    fin_row, fin_t = np.full(R, -7, np.int32), np.full(R, -7, np.int32)
    fin_sum, fin_lp = np.full(R, -7, np.float32), np.full(R, -7, np.float32)
    for g, s in enumerate(states):
        for e, f in enumerate(s.fin):
            fin_row[g * W + e], fin_t[g * W + e], fin_sum[g * W + e], fin_lp[g * W + e] = g * W + f["row"], f["t"], f["sum"], f["lp"]
    n_fin = np.array([len(s.fin) for s in states], np.int32)
    done = np.array([s.done for s in states], np.int32)
    t_out = np.zeros(G, np.int32)
    Pv = np.ascontiguousarray(P, np.int32)
    ids, lps = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(lps, np.float32)
    outs = {n: np.zeros((1 + 2 * GUARD, R), np.float32 if n == "h_lp" else np.int32)
            for n in ("tok", "parent", "frm", "to", "h_par", "h_id", "h_lp")}
    c = SelectCall(W=W, G=G, t=t, eos=eos, guard=GUARD, ids=_ptr(ids), lps=_ptr(lps), P=_ptr(Pv), cum=_ptr(cum),
                   fin_row=_ptr(fin_row), fin_t=_ptr(fin_t), fin_sum=_ptr(fin_sum), fin_lp=_ptr(fin_lp), n_fin=_ptr(n_fin),
                   done=_ptr(done), t_out=_ptr(t_out), **{n: _ptr(a) for n, a in outs.items()})
    _ok(L, L.qasr_kt_beam_select(0, C.byref(c)))
    assert not c.declined
    outs.update(cum=cum, fin_row=fin_row, fin_t=fin_t, fin_sum=fin_sum, fin_lp=fin_lp, n_fin=n_fin, done=done, t_out=t_out)
    return outs


def check_select(W, states, ids, lps, eos, P):
    """the kernel against beam_step on every group, exactly; advances `states`"""
    G, R = len(states), len(states) * W
    o = run_select(W, states, ids, lps, eos, P)
    ids, lps = np.asarray(ids, np.int32), np.asarray(lps, np.float32)
    first = states[0].t == 0
    for n in ("tok", "parent", "frm", "to", "h_par", "h_id", "h_lp"):
        g_rows = np.r_[o[n][:GUARD], o[n][GUARD + 1:]]
        assert (g_rows.view(np.uint32) == 0xFFFFFFFF).all(), n   # guard rows untouched
    for g, st in enumerate(states):
        rows = slice(g * W, g * W + W)
        i_g = np.repeat(ids[g:g + 1], W, 0) if first else ids[rows]
        l_g = np.repeat(lps[g:g + 1], W, 0) if first else lps[rows]
        was_done, n_before = st.done, len(st.hist)
        tok, par, frm, to = beam_step(st, i_g, l_g, eos, P[g])
        assert np.array_equal(o["parent"][GUARD, rows], par + g * W), (g, o["parent"][GUARD, rows], par)
        assert np.array_equal(o["frm"][GUARD, rows], frm) and np.array_equal(o["to"][GUARD, rows], to), g
        assert np.array_equal(o["cum"][rows].view(np.uint32), st.cum.view(np.uint32)), (g, o["cum"][rows], st.cum)
        assert o["n_fin"][g] == len(st.fin) and o["done"][g] == st.done and o["t_out"][g] == st.t, g
        for e, f in enumerate(st.fin):
            assert (o["fin_row"][g * W + e], o["fin_t"][g * W + e]) == (g * W + f["row"], f["t"]), (g, e)
            assert np.float32(o["fin_sum"][g * W + e]).view(np.uint32) == np.float32(f["sum"]).view(np.uint32), (g, e)
            assert np.float32(o["fin_lp"][g * W + e]).view(np.uint32) == np.float32(f["lp"]).view(np.uint32), (g, e)
        if was_done:   # frozen: nothing but the fork arguments written
            assert (o["tok"][GUARD, rows].view(np.uint32) == 0xFFFFFFFF).all() and len(st.hist) == n_before, g
            continue
        h_par, h_id, h_lp = st.hist[-1]
        assert np.array_equal(o["tok"][GUARD, rows], tok) and np.array_equal(o["h_id"][GUARD, rows], h_id), (g, o["tok"][GUARD, rows], tok)
        assert np.array_equal(o["h_par"][GUARD, rows], h_par + g * W), g
        assert np.array_equal(o["h_lp"][GUARD, rows].view(np.uint32), h_lp.view(np.uint32)), g
    return o
