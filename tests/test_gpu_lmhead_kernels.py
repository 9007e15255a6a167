"""The last step of a decode iteration against references of its own: the one-launch LM heads (csrc/lmhead.hip:
lmhead_batch_kernel<MT, .., LSE, TK> for 1 .. 64 rows, lmhead128_kernel<LSE> for 65 .. 128) through the test-only
entry qasr_kt_lmhead, and token_logprob_kernel, topk_rows_kernel and the small bookkeeping kernels of
csrc/elementwise.hip through qasr_kt_rows (csrc/kernel_harness.hip).  Bindings, input families, references and
comparators: tests/lmhead_util.py (none of it measured); their sharpness: tests/test_lmhead_util_host.py.

LM head.  K = 1024; the vocabulary is sized by G = lmhead_grid() at run time so that half the workgroups hold no
unit, the 128-row ring runs at 0 .. 4 units, wraps, and every batch-kernel wave holds a unit (lu.vocab_sizes).
Every case runs twice, writing its logits and not (production); the second must give the first's tokens,
log-probabilities and alternatives bit for bit.  Asserted: the kernel tag; guard rows and rows >= M untouched; logits
within dense_bound(1024) + tie_slack of float64; the token exact (first index of the maximum of the kernel's own
logits over n_valid); top-K ids exact (key order); log-probabilities within 2e-5 + 2^-24 |lp| of float64 over the
kernel's own logits; the history slots, pos, nkv, step; amax and done zero at rest; logits[0] != logits[1].
Every case holds an all-zero row and a row whose maximum four columns share (the next lane, the next unit, the last
unit); the families `abs` (every logit negative) and `wide` (runner-up log-probability about -220) run beside it.

Row kernels.  Logits are given: rows with -inf columns placed against the thread split (NaN before lse_add let a -inf
value contribute nothing), the float4 and the scalar path, tails, n_valid < 1024 and < K, src_div 3, and one row
that fills topk_rows_kernel's candidate list to 1737 of 2048.  The small kernels are exact.
The worst error over its bar per kernel, the tags seen and the wall time go to the parity record
("lmhead_reference_tests").
"""
import time

import numpy as np
import pytest

import kernel_util as ku
import lmhead_util as lu
from kernel_util import GUARD

pytestmark = pytest.mark.gpu

WORST, TAGS = {}, set()
VAR = {"P": (False, 0), "L": (True, 0), "T1": (True, 1), "T3": (True, 3), "T8": (True, 8)}


@pytest.fixture(scope="module", autouse=True)
def _record(gpu, parity):
    t0 = time.time()
    yield
    parity("lmhead_reference_tests", wall_s=time.time() - t0, grid=lu.lmhead_grid(), tags=sorted(TAGS),
           **{f"{k}_worst_over_bar": v for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module")
def sizes(gpu):
    return lu.vocab_sizes(lu.lmhead_grid())


def worst(name, v):
    WORST[name] = max(WORST.get(name, 0.0), v)


def lm_tag(M, var):
    lse, tk = int(var != "P"), int(var[0] == "T")
    return f"lmhead128<{lse}>" if M > 64 else f"lmhead<{(M + 15) // 16},{lse},{tk}>"


def n_valid_of(kind, N, G):
    return {0: 0, "m5": N - 5, "first": lu.first_range_valid(N, G), 5: 5}[kind]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_outputs(r, M, N, nv, var, logits, what):
    """tokens, log-probabilities and alternatives of one call against the fp32 logits `logits`; returns them"""
    lp, K = VAR[var]
    tok = ku.in_range(r.tok_out, M, 1, what + " tok")[:, 0]
    ku.check_argmax(tok, logits, nv, what)
    out = dict(tok=tok.copy())
    if lp:
        ids, lps = lu.expect_rows(logits, max(K, 1), nv)
        got = ku.in_range(r.lp_out, M, 1, what + " lp")[:, 0]
        worst(r.tag.split("<")[0] + "_lp", lu.check_lp(got, lps[:, 0], what + " lp"))
        out["lp"] = got.copy()
    if K:
        tid, tlp = ku.in_range(r.tk_out, M, K, what + " tk_out"), ku.in_range(r.tk_lp, M, K, what + " tk_lp")
        assert np.array_equal(tid, ids), f"{what}: top-K ids differ, first row {np.argwhere((tid != ids).any(1))[0]}: {tid[(tid != ids).any(1)][0]} want {ids[(tid != ids).any(1)][0]}"
        worst("lmhead_topk_lp", lu.check_lp(tlp, lps, what + " tk_lp"))
        assert np.array_equal(bits(tlp[:, 0]), bits(got)) and np.array_equal(tid[:, 0], tok), f"{what}: entry 0 is not the token"
        out.update(tid=tid.copy(), tlp=tlp.copy())
    return out


def check_book(r, M, o, var, *, step=2, hist_stride=6, launches=1, keep_step=0, nkv=True, hist=True, what=""):
    """history slots step + 1 .. of every launch, pos, nkv, step; everything else as it was; amax / done at rest"""
    lp, K = VAR[var]
    hs = hist_stride
    slots = [step + 1] * launches if keep_step else [step + 1 + i for i in range(launches)]
    rows = np.arange(M)[:, None]
    assert np.array_equal(ku.in_range(r.pos, M, 1, what + " pos"), lu.POS0 + rows + launches), what
    if nkv:
        assert np.array_equal(ku.in_range(r.nkv, M, 1, what + " nkv"), lu.NKV0 + rows + launches), what
    assert int(r.step[0]) == step + (0 if keep_step else launches), (what, r.step)
    assert not ku.in_range(r.amax, 128, 1, what + " amax").any() and int(r.done[0]) == 0, f"{what}: amax / done not zero at rest"

    def slot_check(buf, cols, init, vals, name):
        h = ku.in_range(buf, M, hs * cols, f"{what} {name}").reshape(M, hs, cols)
        want = np.full((M, hs, cols), init, h.dtype)
        for s in slots:
            want[:, s] = vals.reshape(M, cols)
        assert np.array_equal(h.view(np.uint32), want.view(np.uint32)), f"{what}: {name} differs"
    if hist:
        slot_check(r.hist, 1, lu.HIST_INIT, o["tok"], "hist")
    if lp:
        slot_check(r.lp_hist, 1, lu.LPH_INIT, o["lp"], "lp_hist")
    if K:
        slot_check(r.tk_hist, K, lu.HIST_INIT, o["tid"], "tk_hist")
        slot_check(r.tk_lphist, K, lu.LPH_INIT, o["tlp"], "tk_lphist")


def run_case(M, N, G, var, nvkind, family, **kw):
    """the case with logits written and without: the common assertions; returns (result, outputs, logits)"""
    lp, K = VAR[var]
    nv = n_valid_of(nvkind, N, G)
    X, nw, W, ref, bound = lu.reference(N, family)
    what = f"M{M} N{N} {var} nv{nv} {family}"
    r = lu.run_lmhead(M, N, X[:M], nw, W, lp=lp, tk=K, n_valid=nv, **kw)
    assert not r.declined, r.msg
    assert r.tag == lm_tag(M, var) and r.grid == G, (what, r.tag)
    TAGS.add(r.tag)
    logits = ku.in_range(r.out_f32, M, N, what + " logits")
    worst(r.tag.split("<")[0] + "_logits", ku.check_values(logits, ref[:M], bound[:M], what=what + " logits"))
    if M > 1:
        assert not np.array_equal(logits[0], logits[1]), f"{what}: rows 0 and 1 hold the same logits"
    o = check_outputs(r, M, N, nv, var, logits, what)
    check_book(r, M, o, var, what=what, **kw)
    # production: no logits written; the same bits
    p = lu.run_lmhead(M, N, X[:M], nw, W, logits=False, lp=lp, tk=K, n_valid=nv, **kw)
    assert not p.declined and p.tag == r.tag, (what, p.tag, p.msg)
    po = check_outputs(p, M, N, nv, var, logits, what + " (no logits)")
    for k in o:
        assert np.array_equal(bits(o[k]), bits(po[k])), f"{what}: {k} differs when the logits are not written"
    check_book(p, M, po, var, what=what + " (no logits)", **kw)
    return r, o, logits, nv


# ===================================================================== LM heads
# (rows, vocabulary regime, variant, n_valid): every MT at a tile edge and inside a tile x {plain, LSE, TK 1 / 3 / 8},
# the 128-row kernel x {plain, LSE}, each across the regimes and the n_valid kinds
CASES = [
    (1, "half", "P", 0), (9, "g1", "L", "m5"), (16, "g8", "T8", 0), (16, "g3", "P", "first"), (9, "half", "T1", 0),
    (1, "g5", "L", 0), (16, "g1", "T3", "first"), (9, "half", "T8", 5),
    (17, "half", "L", 0), (32, "g8", "P", "m5"), (17, "g3", "T8", 0), (32, "g1", "T1", "m5"), (32, "g5", "L", "first"),
    (17, "g1", "P", 0), (32, "half", "T3", "first"),
    (33, "g1", "P", 0), (48, "g8", "L", 0), (33, "half", "T3", "m5"), (48, "g3", "T8", "first"), (48, "g5", "P", "m5"),
    (33, "g5", "L", 0), (48, "g1", "T1", 0),
    (49, "half", "P", "m5"), (64, "g8", "T8", 0), (49, "g1", "L", "first"), (64, "g3", "T1", 0), (64, "g5", "T3", "m5"),
    (64, "half", "L", 0), (49, "g3", "T8", "m5"),
    (65, "half", "P", 0), (113, "half", "L", "m5"), (128, "g1", "L", 0), (65, "g1", "P", "first"), (113, "g3", "P", 0),
    (128, "g3", "L", "first"), (65, "g5", "L", "m5"), (128, "g5", "P", 0), (128, "g8", "L", 0), (113, "g8", "P", "m5"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_lmhead(sizes, case):
    M, kind, var, nvkind = case
    N, G = sizes[kind], lu.lmhead_grid()
    r, o, logits, nv = run_case(M, N, G, var, nvkind, "normal")
    lp, K = VAR[var]
    nvv = nv or N
    if M > lu.ZERO_ROW:      # every logit +0: the token is column 0, the alternatives 0 .. K - 1, each -log(n_valid)
        assert not logits[lu.ZERO_ROW].any() and not np.signbit(logits[lu.ZERO_ROW]).any() and o["tok"][lu.ZERO_ROW] == 0
        if lp:
            assert abs(float(o["lp"][lu.ZERO_ROW]) + np.log(nvv)) <= lu.LP_BAR
        if K:
            assert o["tid"][lu.ZERO_ROW].tolist() == [i if i < nvv else -1 for i in range(K)]
    if M > lu.TIE_ROW:       # four equal maxima in two lanes of a unit, the next unit and the last unit: ascending ids
        cols = [c for c in lu.tie_columns(N) if c < nvv]
        row = logits[lu.TIE_ROW]
        assert len(set(bits(row[lu.tie_columns(N)]).tolist())) == 1 and (np.delete(row, lu.tie_columns(N)) < row[3]).all()
        assert o["tok"][lu.TIE_ROW] == 3
        if K:
            n = min(K, len(cols))
            assert o["tid"][lu.TIE_ROW][:n].tolist() == cols[:n] and len(set(bits(o["tlp"][lu.TIE_ROW][:n]).tolist())) == 1


@pytest.mark.parametrize("case", [(16, "half", "T8", 0), (33, "half", "T3", "m5"), (64, "g1", "L", 0), (128, "g1", "L", "m5"),
                                  (17, "g1", "P", 0)], ids=lambda c: "-".join(str(x) for x in c))
def test_lmhead_all_negative_logits(sizes, case):
    """W = |normal|, x = -|normal|: the sign branch of argmax_key in every key"""
    M, kind, var, nvkind = case
    r, o, logits, _ = run_case(M, sizes[kind], lu.lmhead_grid(), var, nvkind, "abs")
    assert (logits < 0).all()


@pytest.mark.parametrize("case", [(16, "T8"), (48, "L"), (113, "L")], ids=lambda c: f"{c[0]}-{c[1]}")
def test_lmhead_wide_logits(sizes, case):
    """norm_w x 8: logits span a few hundred, exp underflows for nearly every column, the runner-up's
    log-probability is about -220 (where the 2^-24 |lp| term of the bar is as large as the 2e-5)"""
    M, var = case
    r, o, logits, _ = run_case(M, sizes["g3"], lu.lmhead_grid(), var, 0, "wide")
    assert (logits.max(1) - logits.min(1) > 200).all()
    if "tlp" in o:
        assert (o["tlp"][:, 1] < -150).all() and (o["tlp"][:, 0] > -1e-3).all()


@pytest.mark.parametrize("case", [(9, "T3"), (40, "T8"), (64, "L"), (100, "L"), (48, "P")], ids=lambda c: f"{c[0]}-{c[1]}")
def test_lmhead_two_launches_back_to_back(sizes, case):
    """no host reset between two launches: amax, done, the partials and the LDS lists re-arm themselves; the same
    tokens and values bit for bit in history slots step + 1 and step + 2, pos / nkv / step advanced twice"""
    M, var = case
    run_case(M, sizes["g3"], lu.lmhead_grid(), var, "m5", "normal", launches=2)


@pytest.mark.parametrize("case", [(9, "T3"), (33, "P"), (70, "L")], ids=lambda c: f"{c[0]}-{c[1]}")
def test_lmhead_keep_step_null_nkv_null_hist(sizes, case):
    M, var = case
    G = lu.lmhead_grid()
    run_case(M, sizes["g1"], G, var, 0, "normal", keep_step=1, launches=2)
    run_case(M, sizes["g1"], G, var, 0, "normal", nkv=False, hist=False, step=0, hist_stride=2)


DECLINES = {
    "K-512": dict(K=512), "N-not-16": dict(N=2040), "M-129": dict(M=129), "lp-no-part": dict(lp=True, lp_part=False),
    "lp-no-out": dict(lp=True, drop=("lp_out",)), "lp-no-hist": dict(lp=True, drop=("lp_hist",)),
    "tk-no-part": dict(tk=3, tk_part=False), "tk-no-lphist": dict(tk=3, drop=("tk_lphist",)), "tk-no-lp-group": dict(tk=3, lp_part=False),
    "tk-M65": dict(M=65, tk=3), "tk-k9": dict(tk=8, tk_k=9), "tk-k0": dict(tk=8, tk_k=0),
}


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_lmhead_declines_write_nothing(name):
    kw = dict(DECLINES[name])
    M, N, K = kw.pop("M", 20), kw.pop("N", 2048), kw.pop("K", 1024)
    rng = np.random.default_rng(len(name))
    x = rng.standard_normal((M, K)).astype(np.float32)
    r = lu.run_lmhead(M, N, x, np.ones(K, np.float32), ku.f16_normal(rng, (N, K), 1 / 32), K=K, **kw)
    assert r.declined and r.tag == "" and r.msg, (r.tag, r.msg)
    ku.untouched(r.out_f32, r.tok_out, getattr(r, "lp_out", None), getattr(r, "tk_out", None), getattr(r, "tk_lp", None))
    fresh = lu._io
    assert np.array_equal(r.hist, fresh(M, 6, np.int32, lu.HIST_INIT)) and int(r.step[0]) == 2 and int(r.done[0]) == 0
    assert np.array_equal(r.pos, fresh(M, 1, np.int32, lu.POS0 + np.arange(M)[:, None]))
    assert not ku.in_range(r.amax, 128, 1).any()
    for nm in ("lp_hist", "tk_lphist"):
        if getattr(r, nm, None) is not None:
            assert (getattr(r, nm)[GUARD:GUARD + M] == lu.LPH_INIT).all()


# =================================================================== row kernels
ROW_SHAPES = [(5000, 4999), (5001, 4998), (5000, 0), (700, 700)]      # float4 + a 3-column tail; scalar; whole; n_valid < 1024


def row_logits(ld, nv):
    return lu.inf_rows(np.random.default_rng(ld), ld, nv or ld)


def row_tokens(lg, nv, B, src_div):
    """argmax on even rows, another finite column on odd rows; row 1: the -inf column 0"""
    tok = np.zeros(B, np.int32)
    for b in range(B):
        row = lg[b // src_div, :nv]
        tok[b] = int(np.argmax(row)) if b % 2 == 0 else int(np.flatnonzero(np.isfinite(row))[(7 * b) % 5])
    if src_div == 1 and B > 1:
        tok[1] = 0
    return tok


@pytest.mark.parametrize("src_div", [1, 3])
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: f"ld{s[0]}-nv{s[1]}")
def test_token_logprob(shape, src_div):
    ld, nvk = shape
    nv = nvk or ld
    lg = row_logits(ld, nv)
    for B in (12, 1):
        src = lg[:(B + src_div - 1) // src_div]
        tok = row_tokens(lg, nv, B, src_div)
        hist = lu._io(B, 4, np.float32, lu.LPH_INIT)
        r = lu.run_rows("token_logprob", B, ld=ld, in_rows=len(src), n_valid=nvk, src_div=src_div, hist_stride=4, step=1, f_in=src,
                        i_in=tok, f_out=lu._out(B, 1, np.float32), f_hist=hist)
        assert not r.declined and r.tag == f"token_logprob<{int(src_div > 1)},{int(ld % 4 == 0)}>", (r.tag, r.msg)
        TAGS.add(r.tag)
        got = ku.in_range(r.f_out, B, 1, "lp_out")[:, 0]
        want = np.array([lu.logsoftmax64(lg[b // src_div], nv)[tok[b]] for b in range(B)])
        worst("token_logprob", lu.check_lp(got, want, f"token_logprob ld {ld} nv {nv} B {B} div {src_div}"))
        if src_div == 1 and B == 12:
            assert np.isneginf(got[1])
        h = ku.in_range(r.f_hist, B, 4, "lp_hist")
        assert np.array_equal(bits(h[:, 1]), bits(got)) and (np.delete(h, 1, axis=1) == lu.LPH_INIT).all()


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("shape", ROW_SHAPES + [(8, 5), (9, 5)], ids=lambda s: f"ld{s[0]}-nv{s[1]}")
def test_topk_rows(shape, K):
    """ids exact in key order (-inf columns once the finite ones run out, -1 past n_valid), no NaN, a -inf column's
    value -inf, entry 0's value the bits token_logprob gives the argmax"""
    ld, nvk = shape
    nv = nvk or ld
    lg = row_logits(ld, nv)
    for B in (12, 1):
        hi, hf = lu._io(B, 3 * K, np.int32, lu.HIST_INIT), lu._io(B, 3 * K, np.float32, lu.LPH_INIT)
        r = lu.run_rows("topk_rows", B, ld=ld, in_rows=B, n_valid=nvk, K=K, hist_stride=3, step=2, f_in=lg[:B],
                        i_out=lu._out(B, K, np.int32), f_out=lu._out(B, K, np.float32), i_hist=hi, f_hist=hf)
        assert not r.declined and r.tag == f"topk_rows<{K},{int(ld % 4 == 0)}>", (r.tag, r.msg)
        TAGS.add(r.tag)
        ids, lps = lu.expect_rows(lg[:B], K, nv)
        tid, tlp = ku.in_range(r.i_out, B, K, "tk_ids"), ku.in_range(r.f_out, B, K, "tk_lp")
        assert np.array_equal(tid, ids), (ld, nv, K, tid[(tid != ids).any(1)][:2], ids[(tid != ids).any(1)][:2])
        worst("topk_rows", lu.check_lp(tlp, lps, f"topk_rows ld {ld} nv {nv} K {K}"))
        if B == 12 and K == 8:
            assert np.isneginf(tlp[4, 1:min(K, nv)]).all() and np.isfinite(tlp[4, 0])     # all columns but one are -inf
        assert np.array_equal(ku.in_range(r.i_hist, B, 3 * K).reshape(B, 3, K)[:, 2], tid)
        assert np.array_equal(bits(ku.in_range(r.f_hist, B, 3 * K).reshape(B, 3, K)[:, 2]), bits(tlp))
        assert (r.i_hist[GUARD:GUARD + B].reshape(B, 3, K)[:, :2] == lu.HIST_INIT).all()
        t = lu.run_rows("token_logprob", B, ld=ld, in_rows=B, n_valid=nvk, f_in=lg[:B], i_in=np.maximum(tid[:, 0], 0),
                        f_out=lu._out(B, 1, np.float32))
        assert np.array_equal(bits(ku.in_range(t.f_out, B, 1)[:, 0]), bits(tlp[:, 0]))


def test_topk_rows_at_the_candidate_limit():
    """253952 columns, K = 8: seven threads hold all 248 of their columns above the eighth thread's maximum, so the
    second pass collects 1737 keys of the 2048 the list holds; the result is exact, ties by ascending column"""
    row = lu.pressure_row()[None, :]
    n = lu.PRESSURE_N
    r = lu.run_rows("topk_rows", 1, ld=n, in_rows=1, K=8, step=0, f_in=row, i_out=lu._out(1, 8, np.int32), f_out=lu._out(1, 8, np.float32))
    assert not r.declined and r.tag == "topk_rows<8,1>", (r.tag, r.msg)
    ids, lps = lu.expect_rows(row, 8)
    assert np.array_equal(ku.in_range(r.i_out, 1, 8), ids), (r.i_out[GUARD], ids)
    worst("topk_rows", lu.check_lp(ku.in_range(r.f_out, 1, 8), lps, "candidate limit"))


@pytest.mark.parametrize("n,K", [(lu.PRESSURE_DECLINED_N, 8), (5000, 9), (5000, 0)])
def test_topk_rows_declines_write_nothing(n, K):
    row = np.zeros((1, n), np.float32)
    kk = max(K, 1)
    r = lu.run_rows("topk_rows", 1, ld=n, in_rows=1, K=K, step=0, f_in=row, i_out=lu._out(1, kk, np.int32), f_out=lu._out(1, kk, np.float32))
    assert r.declined and r.tag == "", (r.tag, r.msg)
    ku.untouched(r.i_out, r.f_out)


# ================================================================ small kernels
@pytest.mark.parametrize("hidden", [1024, 2048])
def test_embed(hidden):
    rng = np.random.default_rng(hidden)
    V, A = 37, 5
    embd = ku.f16_normal(rng, (V, hidden))
    audio = rng.standard_normal((A, hidden)).astype(np.float32)
    ids = np.array([0, V - 1, 5, 5, 0, 17, V - 1], np.int32)
    for row_audio in (None, np.array([-1, -1, 4, 0, -1, 2, -1], np.int32)):
        r = lu.run_rows("embed", len(ids), ld=hidden, in_rows=V, in_rows2=A if row_audio is not None else 0, h_in=embd,
                        f_in=audio if row_audio is not None else None, i_in=ids, i_in2=row_audio, f_out=lu._out(len(ids), hidden, np.float32))
        want = embd[ids].astype(np.float32)
        if row_audio is not None:
            want[row_audio >= 0] = audio[row_audio[row_audio >= 0]]
        assert np.array_equal(bits(ku.in_range(r.f_out, len(ids), hidden, "embed")), bits(want))


@pytest.mark.parametrize("B", [1, 12, 256])
def test_argmax_finish(B):
    rng = np.random.default_rng(B)
    vals = -np.abs(rng.standard_normal(B)).astype(np.float32) * (np.arange(B) % 3 > 0)       # negative values and zeros
    idx = rng.integers(0, 151936, B)
    keys = np.array([lu.argmax_keys(np.float32([v]), [i])[0] for v, i in zip(vals, idx)], np.uint64)
    for with_hist in (True, False):
        r = lu.run_rows("argmax_finish", B, hist_stride=5, step=3, u_in=keys, i_out=lu._out(B, 1, np.int32),
                        i_hist=lu._io(B, 5, np.int32, lu.HIST_INIT) if with_hist else None)
        assert np.array_equal(ku.in_range(r.i_out, B, 1)[:, 0], idx)
        if with_hist:
            h = ku.in_range(r.i_hist, B, 5)
            assert np.array_equal(h[:, 3], idx) and (np.delete(h, 3, axis=1) == lu.HIST_INIT).all()


def test_gather_rows():
    rng = np.random.default_rng(4)
    src = rng.standard_normal((9, 1024)).astype(np.float32)
    for idx in ([8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 3, 0, 8, 3], [8]):
        r = lu.run_rows("gather_rows", len(idx), ld=1024, in_rows=9, f_in=src, i_in=idx, f_out=lu._out(len(idx), 1024, np.float32))
        assert np.array_equal(bits(ku.in_range(r.f_out, len(idx), 1024, "gather")), bits(src[idx]))


@pytest.mark.parametrize("B", [1, 256])
def test_step_advance_and_fill_u64(B):
    rows = np.arange(B, dtype=np.int32)[:, None]
    r = lu.run_rows("step_advance", B, step=41, i_out=lu._io(B, 1, np.int32, 10 + rows), i_hist=lu._io(B, 1, np.int32, 500 - rows))
    assert np.array_equal(ku.in_range(r.i_out, B, 1), 11 + rows) and np.array_equal(ku.in_range(r.i_hist, B, 1), 501 - rows)
    assert r.step_out == 42
    for v in (0, 0x0123456789ABCDEF):
        f = lu.run_rows("fill_u64", B, fill=v, u_out=lu._out(B, 1, np.uint64))
        assert (ku.in_range(f.u_out, B, 1) == np.uint64(v)).all()


def test_every_variant_ran():
    """(last in the module) MT 1 .. 4 x {plain, LSE, TK}, the 128-row kernel x {plain, LSE}, both row kernels on the
    float4 and the scalar path"""
    want = {f"lmhead<{mt},{l},{t}>" for mt in (1, 2, 3, 4) for l, t in ((0, 0), (1, 0), (1, 1))} | {"lmhead128<0>", "lmhead128<1>"}
    want |= {f"token_logprob<{m},{v}>" for m in (0, 1) for v in (0, 1)} | {f"topk_rows<{k},{v}>" for k in (1, 3, 8) for v in (0, 1)}
    assert want <= TAGS, sorted(want - TAGS)
