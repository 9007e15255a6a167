"""The score head (csrc/score_head.hip) through its harness entry, against a float64 reference over
the same fp16 operands (tests/score_util.py): the smallest shapes that cross every edge -- one row,
rows and columns short of a tile, n_valid that leaves a wave half and two whole tiles empty
(300 of 640), two row tiles, n_valid inside the last tile, and the full vocabulary
width (every one of the 1187 column tiles and the full merge)."""
import numpy as np
import pytest

from kernel_util import GUARD, bits, untouched
from score_util import body, check_gid, make_case, reference, run_score_head, simulate_lp

pytestmark = pytest.mark.gpu

# (R, N, n_valid, K)
SHAPES = [(1, 640, 0, 256), (5, 640, 600, 256), (5, 640, 300, 256), (128, 640, 0, 1024), (129, 1280, 1279, 256), (17, 151936, 0, 1024)]
_CASES = {}


def case(shape):
    """operands, one float64 reference and one pair of launches a shape, shared by the tests below"""
    if shape not in _CASES:
        R, N, nv, K = shape
        A, W, tg = make_case(1000 + R, R, N, K, nv)
        ref, lp, glp, bound = reference(A, W, tg, nv)
        out = run_score_head(bits(A), bits(W), tg, n_valid=nv, launches=1)
        again = run_score_head(bits(A), bits(W), tg, n_valid=nv, launches=2)
        _CASES[shape] = dict(A=A, W=W, tg=tg, ref=ref, lp=lp, glp=glp, bound=bound, out=out, again=again)
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_score_head_against_float64(gpu, parity, shape):
    R, N, nv, K = shape
    c = case(shape)
    out = c["out"]
    assert not out.declined and out.tag == "score_head<128,128,1,3,0>", (out.declined, out.tag, out.msg)
    lp, gid, glp = body(out.lp, R, "lp"), body(out.gid, R, "gid"), body(out.glp, R, "glp")
    e_lp, e_glp = np.abs(lp - c["lp"]), np.abs(glp - c["glp"])
    print(f"shape {shape}: max |lp - lp64| {e_lp.max():.3e} (worst / bound {(e_lp / c['bound']).max():.3f}), "
          f"max |glp - glp64| {e_glp.max():.3e} (worst / bound {(e_glp / c['bound']).max():.3f}), bound {c['bound'].max():.3e}")
    parity(f"score_head {shape}", lp_err=e_lp.max(), glp_err=e_glp.max(), bound=c["bound"].max(),
           worst_over_bound=max((e_lp / c["bound"]).max(), (e_glp / c["bound"]).max()))
    assert (e_lp <= c["bound"]).all(), (int(np.argmax(e_lp / c["bound"])), e_lp.max())
    assert (e_glp <= c["bound"]).all(), (int(np.argmax(e_glp / c["bound"])), e_glp.max())
    assert ((gid >= 0) & (gid < (nv or N))).all()
    clear = check_gid(gid, c["ref"], c["bound"])
    assert clear >= (R - 1) * 3 // 4   # (the all-zero row ties; a random row's top two may sit inside the bound)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_special_rows(gpu, shape):
    R, N, nv, K = shape
    c = case(shape)
    lp, gid, glp = (b[GUARD:GUARD + R] for b in (c["out"].lp, c["out"].gid, c["out"].glp))
    # all-zero row: every logit +0.0, the sum of exp is the column count exactly
    want = np.float32(-np.log(np.float64(nv or N)))
    assert gid[0] == 0 and lp[0] == glp[0] and abs(float(lp[0]) - float(want)) <= 2e-6, (gid[0], lp[0], glp[0], want)
    if R >= 3:
        # one logit >= 30 above the rest: its log-probability is ~0, and it is the greedy token
        gap = np.sort(c["ref"][1])[-1] - np.sort(c["ref"][1])[-2]
        assert gap >= 30 and gid[1] == c["tg"][1] and -1e-6 <= lp[1] <= 0 and lp[1].tobytes() == glp[1].tobytes(), (gap, lp[1])
        # the target is the row's argmax: the two outputs are the same bits
        assert gid[2] == c["tg"][2] and lp[2].tobytes() == glp[2].tobytes(), (gid[2], c["tg"][2], lp[2], glp[2])
    same = np.flatnonzero(gid == c["tg"])
    assert np.array_equal(lp[same].view(np.uint32), glp[same].view(np.uint32))
    assert (lp <= glp).all()   # no token beats the greedy one


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_launches_bit_identical(gpu, shape):
    c = case(shape)
    for name in ("lp", "gid", "glp"):
        a, b = getattr(c["out"], name), getattr(c["again"], name)
        assert a.tobytes() == b.tobytes(), name


def test_grid_orders_agree(gpu):
    """the column-tiles-first grid (diagnostic) computes the same bits"""
    shape = SHAPES[3]
    c = case(shape)
    other = run_score_head(bits(c["A"]), bits(c["W"]), c["tg"], n_valid=shape[2], cols_fast=1)
    assert not other.declined and other.tag == "score_head<128,128,1,3,1>"
    for name in ("lp", "gid", "glp"):
        assert getattr(other, name).tobytes() == getattr(c["out"], name).tobytes(), name


def test_padded_leading_dimensions(gpu):
    """lda / ldw wider than K: the padding columns (NaN) are never read"""
    from kernel_util import pad_cols
    R, N, nv, K = SHAPES[1]
    c = case(SHAPES[1])
    out = run_score_head(pad_cols(bits(c["A"]), K + 8, 0xFFFF), pad_cols(bits(c["W"]), K + 16, 0xFFFF), c["tg"], n_valid=nv, K=K)
    assert not out.declined
    for name in ("lp", "gid", "glp"):
        assert getattr(out, name).tobytes() == getattr(c["out"], name).tobytes(), name


@pytest.mark.parametrize("R,N,K", [(4, 704, 256), (4, 640, 192), (4, 64, 256)])
def test_declined_shapes(gpu, R, N, K):
    """N = 704 = 64 x 11 (not a multiple of the 128-column tile), K % 128 != 0, N below one tile"""
    rng = np.random.default_rng(5)
    A, W = rng.standard_normal((R, K)).astype(np.float16), rng.standard_normal((N, K)).astype(np.float16)
    out = run_score_head(bits(A), bits(W), np.zeros(R, np.int32))
    assert out.declined and out.msg and out.tag == ""
    untouched(out.lp, out.gid, out.glp)


@pytest.mark.parametrize("R,N,nv", [(7, 1280, 0), (7, 640, 300), (130, 8960, 8900)])
def test_kernel_follows_the_simulated_order(gpu, R, N, nv):
    """Operands whose logits are exact in fp32 whatever the summation order (entries in {-1/4, 0, 1/4}: products and
    sums are multiples of 1/16 below 2^24), so the kernel's logits are the reference's bit for bit and what remains is
    the reduction: the kernel against tests/score_util.py's float32 restatement of its order (simulate_lp).  The two
    differ only in the exp (v_exp_f32 of x log2 e on the device, numpy's expf here).  dev_common.h puts the device
    exp's relative error at ~1e-7 (1 + |x|); with these logits (standard deviation 0.67, the maximum 2 .. 3 above the
    mean) the softmax-weighted |x| is ~2.5, so one level of exps moves a sum by at most 3.5e-7 relative.  A partial is
    rescaled by one more exp whenever a merge raises its maximum: at most once in the tile, twice in a lane's walk
    (<= 70 tiles over 64 lanes) and six times in the butterfly -- with the terms' own exp ten levels, 3.5e-6 on the
    log; a dropped column would move it by 1e-4 or more.  Tolerance: 4e-6 plus two ulps of |lp|."""
    rng = np.random.default_rng(40 + R)
    K = 256
    A = (rng.integers(-1, 2, (R, K)) * 0.25).astype(np.float16)
    W = (rng.integers(-1, 2, (N, K)) * 0.25).astype(np.float16)
    tg = rng.integers(0, nv or N, R).astype(np.int32)
    logits = (A.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)   # exact
    out = run_score_head(bits(A), bits(W), tg, n_valid=nv)
    assert not out.declined
    lp, gid, glp = body(out.lp, R, "lp"), body(out.gid, R, "gid"), body(out.glp, R, "glp")
    lv = logits[:, :nv or N]
    assert np.array_equal(gid, np.argmax(lv, axis=1))   # exact logits: exactly the first maximum
    sim_lp, sim_glp = simulate_lp(logits, tg, nv), simulate_lp(logits, np.argmax(lv, axis=1), nv)
    for name, got, sim in (("lp", lp, sim_lp), ("glp", glp, sim_glp)):
        tol = 4e-6 + 2 * np.spacing(np.abs(sim).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - sim.astype(np.float64))
        print(f"({R}, {N}, {nv}) {name}: max |kernel - simulated| {err.max():.3g} (tolerance {tol.min():.3g} .. {tol.max():.3g})")
        assert (err <= tol).all(), (name, int(np.argmax(err / tol)), err.max())
