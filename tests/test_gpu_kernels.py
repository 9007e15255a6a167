"""Every GEMM, GEMV and Q8_0 kernel variant against a float64 reference.

The launchers of csrc/kernels.h are called directly on seeded arrays through the
test-only entries of csrc/kernel_harness.hip, at the smallest shapes that reach
each branch of their dispatch tables plus each tile's ragged edges.  Every case
asserts the tag of the kernel it meant to reach (kernels.h note_kernel), so a
retuned table cannot silently stop covering a tile, and the buffer state: guard
rows and padding columns untouched, every in-range element written, no NaN
(inputs carry NaN guard rows and NaN padding columns).  References, bounds and
comparators: tests/kernel_util.py; their sharpness: tests/test_kernel_util_host.py.
The worst error / bound ratio per launcher family and the file's wall time go to
the parity record ("kernel_reference_tests"); fp16 outputs are recorded apart
("_f16_out": their bound includes the output's own half ulp, which a correct
kernel uses up, so their ratio sits near 1 by construction).
"""
import functools
import time

import numpy as np
import pytest

import kernel_util as ku
from kernel_util import (EPI_ARGMAX, EPI_F16, EPI_F32, EPI_GELU_F16, EPI_SWIGLU_F16, EPI_SWIGLU_F32, EPI_SWIGLU_Q8, GEMM, GEMM_Q8,
                         SKINNY, SKINNY_Q8)

pytestmark = pytest.mark.gpu

WORST = {}


def note(family, ratio):
    assert ratio <= 1.0, (family, ratio)
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _record(gpu, parity):
    t0 = time.time()
    yield
    parity("kernel_reference_tests", wall_s=time.time() - t0, **{f"{k}_worst_over_bound": v for k, v in sorted(WORST.items())})


@functools.lru_cache(maxsize=None)
def dense_case(M, N, K):
    """seeded fp16 operands with O(1) outputs, their float64 product and |A| |W|^T (computed once, shared, never written)"""
    rng = np.random.default_rng([M, N, K])
    A = ku.f16_normal(rng, (M, K))
    W = ku.f16_normal(rng, (N, K), K ** -0.5)
    ref, mag = ku.dense_terms(A, W)
    for a in (A, W, ref, mag):
        a.setflags(write=False)
    return A, W, ref, mag


def gelu_bias(rng, N):
    """columns past +-10 on both sides (the two clamps) between ordinary ones (the table)"""
    b = rng.standard_normal(N).astype(np.float32)
    b[1::7] = 14.0
    b[4::7] = -14.0
    return b


def dense_call(launcher, epi, M, N, K, *, A=None, W=None, bias=False, res=False, pe=False, **kw):
    """run one dense launcher with strictly larger leading dimensions; returns (result, ref, bound, extras)"""
    if A is None:
        A, W, ref, mag = dense_case(M, N, K)
    else:
        ref, mag = ku.dense_terms(A, W)
    rng = np.random.default_rng([M, N, K, epi])
    swiglu = epi in (EPI_SWIGLU_F16, EPI_SWIGLU_F32)
    NO = N // 2 if swiglu else N
    bv = (gelu_bias(rng, N) if epi == EPI_GELU_F16 else rng.standard_normal(N).astype(np.float32)) if bias else None
    rv = rng.standard_normal((M, N)).astype(np.float32) if res else None
    pev = rng.standard_normal((7, N)).astype(np.float32) if pe else None
    pos = rng.integers(0, 7, M) if pe else None
    f32 = epi in (EPI_F32, EPI_SWIGLU_F32, EPI_ARGMAX)
    r = ku.run_gemm(launcher, epi, M, N, K, A=ku.pad_cols(A, K + 8), W=ku.pad_cols(W, K + 8), bias=bv,
                    res=None if rv is None else ku.pad_cols(rv, N + 4), pe=pev, pe_pos=pos,
                    ldo=NO + 4 if f32 else 0, ldo16=0 if f32 else NO + 4, amax=epi == EPI_ARGMAX, **kw)
    ref, bound = ku.add_terms(ref, ku.dense_bound(K, mag), bv, None if pev is None else pev[pos], rv)
    return r, ref, bound


def check_epilogue(r, epi, M, N, ref, bound, family, n_valid=0):
    """the output of any GEMM-shaped launcher against the reference pre-epilogue values"""
    if epi in (EPI_F32, EPI_ARGMAX):
        out = ku.in_range(r.out_f32, M, N)
        note(family, ku.check_values(out, ref, bound))
        if epi == EPI_ARGMAX:
            keys = ku.in_range(r.amax, M, 1)[:, 0]
            ku.check_argmax(ku.key_index(keys), out, n_valid)
            nv = n_valid or N
            assert np.array_equal(ku.key_value(keys), out[:, :nv].max(1))
    elif epi == EPI_F16:
        note(family + "_f16_out", ku.check_values(ku.in_range(r.out_f16, M, N), ref, bound, fp16=True))
    elif epi == EPI_GELU_F16:
        assert (ref - bound >= 10).any() and (ref + bound <= -10).any() and (np.abs(ref) < 9).any()
        ku.check_gelu(ku.in_range(r.out_f16, M, N), r.gelu_out, ref, bound)
    else:
        gate, up = ku.swiglu_rows(N // 2)
        v, bv = ku.swiglu_terms(ref[:, gate], bound[:, gate], ref[:, up], bound[:, up])
        if epi == EPI_SWIGLU_F16:
            note(family + "_f16_out", ku.check_values(ku.in_range(r.out_f16, M, N // 2), v, bv, fp16=True))
        else:
            note(family, ku.check_values(ku.in_range(r.out_f32, M, N // 2), v, bv))


def same_bits(a, b):
    for name in ("out_f32", "out_f16", "out_q", "out_d", "amax"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name


# ====================================================================== launch_gemm, dense
P8 = "gemm8p"
G256, G128, G128W = "glds<256,256,1,3,4>", "glds<128,128,1,2,2>", "glds<128,128,1,3,4>"
R1, R2 = "gemm<128,128,1>", "gemm<128,128,2>"
# (M, N, K, tag, regs_staged, [(epilogue, bias, res, pe)], tag of the register-staged A/B or None)
PLAIN, BR = (EPI_F32, 0, 0, 0), (EPI_F32, 1, 1, 0)
ALL = [PLAIN, BR, (EPI_GELU_F16, 1, 0, 0), (EPI_F16, 1, 0, 0), (EPI_F16, 0, 0, 0), (EPI_SWIGLU_F16, 0, 0, 0),
       (EPI_SWIGLU_F32, 0, 0, 0)]
SOME = [BR, (EPI_GELU_F16, 1, 0, 0), (EPI_SWIGLU_F16, 0, 0, 0)]
GEMM_CASES = [
    (2048, 256, 128, P8, 0, ALL, R1),
    (2049, 288, 256, P8, 0, [(EPI_F32, 1, 1, 1), (EPI_F32, 0, 0, 1), (EPI_GELU_F16, 1, 0, 0), (EPI_F16, 1, 0, 0),
                             (EPI_SWIGLU_F16, 0, 0, 0), (EPI_SWIGLU_F32, 0, 0, 0)], None),
    (2303, 896, 896, P8, 0, [BR, (EPI_GELU_F16, 1, 0, 0), (EPI_F16, 1, 0, 0), (EPI_SWIGLU_F16, 0, 0, 0), (EPI_SWIGLU_F32, 0, 0, 0)], R1),
    (2049, 256, 192, G256, 0, ALL, R1),
    (2048, 512, 128, G256, 0, [(EPI_ARGMAX, 0, 0, 0)], R1),
    (2050, 384, 192, G128, 0, ALL + [(EPI_ARGMAX, 0, 0, 0)], R1),
    (1, 2048, 32, G128W, 0, SOME, None),
    (129, 2176, 96, G128W, 0, ALL + [(EPI_ARGMAX, 0, 0, 0)], None),
    (2049, 128, 64, R1, 1, ALL + [(EPI_ARGMAX, 0, 0, 0)], None),
    (2049, 128, 1088, R2, 1, SOME, None),
    (65, 64, 2048, "gemm<64,64,4>", 0, ALL + [(EPI_ARGMAX, 0, 0, 0)], None),
    (97, 3136, 64, "gemm<96,64,2>", 0, ALL + [(EPI_ARGMAX, 0, 0, 0)], None),
    (95, 3136, 128, "gemm<96,64,2>", 0, SOME, None),
    (1, 64, 64, "gemm<64,64,2>", 0, SOME, None),
    (63, 64, 64, "gemm<64,64,2>", 0, SOME, None),
    (65, 128, 192, "gemm<64,64,2>", 0, ALL + [(EPI_ARGMAX, 0, 0, 0)], None),
    (1, 64, 32, "gemm<64,64,1>", 0, SOME, None),
    (64, 64, 96, "gemm<64,64,1>", 0, ALL + [(EPI_ARGMAX, 0, 0, 0)], None),
]


@pytest.mark.parametrize("M,N,K,tag,regs,epis,ab", GEMM_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}" for c in GEMM_CASES])
def test_gemm_dense(M, N, K, tag, regs, epis, ab):
    for epi, bias, res, pe in epis:
        r, ref, bound = dense_call(GEMM, epi, M, N, K, bias=bias, res=res, pe=pe, regs_staged=regs)
        assert not r.declined, r.msg
        assert r.tag == tag, (epi, r.tag)
        check_epilogue(r, epi, M, N, ref, bound, "gemm")
        if ab:   # the register-staged tile gives the same bits, and is held to the same bound
            r2, _, _ = dense_call(GEMM, epi, M, N, K, bias=bias, res=res, pe=pe, regs_staged=1)
            assert r2.tag == ab, r2.tag
            check_epilogue(r2, epi, M, N, ref, bound, "gemm")
            same_bits(r, r2)


def _tied(M, N, K, c):
    """operands whose columns c, c + 1, c + 16 and c + N / 2 hold the same, largest logit in every row"""
    A, W, _, _ = dense_case(M, N, K)
    A, W = A.copy(), W.copy()
    A[:, 0] = 8.0
    W[c, 0] = 4.0
    for d in (1, 16, N // 2):
        W[c + d] = W[c]
    return A, W


@pytest.mark.parametrize("M,N,K,tag", [(65, 128, 192, "gemm<64,64,2>"), (2048, 512, 128, G256)])
def test_gemm_argmax_ties_and_padding(M, N, K, tag):
    c = 5
    A, W = _tied(M, N, K, c)
    r, ref, bound = dense_call(GEMM, EPI_ARGMAX, M, N, K, A=A, W=W)
    assert r.tag == tag
    check_epilogue(r, EPI_ARGMAX, M, N, ref, bound, "gemm")
    assert (ku.key_index(ku.in_range(r.amax, M, 1)[:, 0]) == c).all()   # the lowest of the four equal columns
    logits = ku.in_range(r.out_f32, M, N)
    assert (logits[:, c] == logits[:, c + 1]).all() and (logits[:, c] == logits[:, c + N // 2]).all()
    # n_valid < N: the padded columns hold the largest values and never win
    nv = N - 28
    W2 = W.copy()
    W2[nv:, 0] = 8.0
    r, ref, bound = dense_call(GEMM, EPI_ARGMAX, M, N, K, A=A, W=W2, n_valid=nv)
    assert (ku.in_range(r.out_f32, M, N)[:, nv:].min(1) > ku.in_range(r.out_f32, M, N)[:, :nv].max(1)).all()
    check_epilogue(r, EPI_ARGMAX, M, N, ref, bound, "gemm", n_valid=nv)


# ====================================================================== launch_gemm_q8
@functools.lru_cache(maxsize=None)
def q8_case(M, N, K):
    rng = np.random.default_rng([8, M, N, K])
    Aq, Ad = ku.q8_operand(rng, M, K, np.float32, 0.02)
    Wq, Wd = ku.q8_operand(rng, N, K, np.float16, 0.02 * K ** -0.5)
    ref, mag = ku.q8_terms(Aq, Ad, Wq, Wd)
    return Aq, Ad, Wq, Wd, ref, mag


def q8_call(launcher, epi, M, N, K, *, bias=False, res=False, **kw):
    Aq, Ad, Wq, Wd, ref, mag = q8_case(M, N, K)
    rng = np.random.default_rng([8, M, N, K, epi])
    bv = (gelu_bias(rng, N) if epi == EPI_GELU_F16 else rng.standard_normal(N).astype(np.float32)) if bias else None
    rv = rng.standard_normal((M, N)).astype(np.float32) if res else None
    NO = N // 2 if epi in (EPI_SWIGLU_F32, EPI_SWIGLU_Q8) else N
    r = ku.run_gemm(launcher, epi, M, N, K, Aq=ku.pad_cols(Aq, K + 16), Ad=ku.pad_cols(Ad, K // 32 + 4), Wq=ku.pad_cols(Wq, K + 16),
                    Wd=Wd, bias=bv, res=None if rv is None else ku.pad_cols(rv, N + 4),
                    ldo=NO + 4 if epi in (EPI_F32, EPI_SWIGLU_F32) else 0, ldo16=NO + 4 if epi in (EPI_GELU_F16, EPI_F16) else 0,
                    ldoq=NO + 32 if epi == EPI_SWIGLU_Q8 else 0, **kw)
    ref, bound = ku.add_terms(ref, ku.q8_bound(K, mag), bv, rv)
    return r, ref, bound


@pytest.mark.parametrize("M,N,K,tag", [(2049, 128, 128, "gemm_q8<128,64,2>"), (65, 64, 128, "gemm_q8<64,64,4>"),
                                       (63, 64, 96, "gemm_q8<64,64,1>")])
def test_gemm_q8(M, N, K, tag):
    for epi, bias, res in ((EPI_F32, 0, 0), (EPI_F32, 1, 1), (EPI_GELU_F16, 1, 0), (EPI_SWIGLU_F32, 0, 0)):
        r, ref, bound = q8_call(GEMM_Q8, epi, M, N, K, bias=bias, res=res)
        assert not r.declined, r.msg
        assert r.tag == tag, r.tag
        check_epilogue(r, epi, M, N, ref, bound, "gemm_q8")


# ====================================================================== skinny GEMMs
ALL_M = (1, 9, 16, 17, 33, 64, 65, 127, 128)
ALL_K = (128, 256, 512, 640, 1024, 1152, 2048, 3072)


def _mt(M, cap):
    return min((M + 15) // 16, cap)


def _plain_tiling(M, N):
    """launch_gemm_skinny / _q8, EPI_F32 / EPI_F16: (MT, NT, KW) as gemm_skinny.hip states them"""
    if M > 64:
        return (4, 2, 8) if N >= 4096 else (2, 1, 8)
    return (_mt(M, 4), 1, 8) if N >= 4096 else (1, 1, 8)


def _cpw(K, mt, kw, inflight, esz):
    """chunks a wave with all of them in flight: whole chunks per wave, images within 128 KiB of LDS"""
    ch = K // 128
    cpw = ch // kw if inflight and ch % kw == 0 else 0
    return cpw if cpw == 1 or (cpw in (2, 3) and cpw * kw * mt * 16 * 128 * esz <= 131072) else 0


def _skinny_tag(q8, tiling, K, inflight=1, wdef=1, regs=0):
    mt, nt, kw = tiling
    var = 0 if regs else 4 if q8 else (12 if wdef else 4)
    cpw = 0 if regs else _cpw(K, mt, kw, inflight, 1 if q8 else 2)
    return f"{'skinny_q8' if q8 else 'skinny'}<{mt},{nt},{kw},{var},{cpw}>"


# the tags of the per-M sweeps written out: the table above restates the launcher, these pin it
PLAIN_TAGS_N64_K1024 = {1: "<1,1,8,12,1>", 9: "<1,1,8,12,1>", 16: "<1,1,8,12,1>", 17: "<1,1,8,12,1>", 33: "<1,1,8,12,1>",
                        64: "<1,1,8,12,1>", 65: "<2,1,8,12,1>", 127: "<2,1,8,12,1>", 128: "<2,1,8,12,1>"}
PLAIN_TAGS_N4096_K256 = {1: "<1,1,8,12,0>", 9: "<1,1,8,12,0>", 16: "<1,1,8,12,0>", 17: "<2,1,8,12,0>", 33: "<3,1,8,12,0>",
                         64: "<4,1,8,12,0>", 65: "<4,2,8,12,0>", 127: "<4,2,8,12,0>", 128: "<4,2,8,12,0>"}


def _skinny_plain(q8, M, N, K, epi=EPI_F32, **kw):
    call = q8_call if q8 else dense_call
    r, ref, bound = call(SKINNY_Q8 if q8 else SKINNY, epi, M, N, K, bias=True, res=epi == EPI_F32, **kw)
    assert not r.declined, r.msg
    check_epilogue(r, epi, M, N, ref, bound, "skinny_q8" if q8 else "skinny")
    return r


@pytest.mark.parametrize("M", ALL_M)
def test_skinny_every_row_count(M):
    for N, K, tags in ((64, 1024, PLAIN_TAGS_N64_K1024), (4096, 256, PLAIN_TAGS_N4096_K256)):
        r = _skinny_plain(False, M, N, K)
        assert r.tag == "skinny" + tags[M] == _skinny_tag(False, _plain_tiling(M, N), K), r.tag
        r = _skinny_plain(True, M, N, K)
        assert r.tag == "skinny_q8" + tags[M].replace(",12,", ",4,") == _skinny_tag(True, _plain_tiling(M, N), K), r.tag


@pytest.mark.parametrize("M", (17, 65))
@pytest.mark.parametrize("K", ALL_K)
def test_skinny_every_k(M, K):
    """fewer chunks than waves (K = 128), uneven chunk splits, and 0 .. 3 chunks a wave all in flight;
    skinny_inflight 0 / 1 and the register-staged form give the same bits"""
    seen = set()
    for q8 in (False, True):
        N = 64
        r1 = _skinny_plain(q8, M, N, K, inflight=1)
        r0 = _skinny_plain(q8, M, N, K, inflight=0)
        rr = _skinny_plain(q8, M, N, K, regs_staged=1)
        assert r1.tag == _skinny_tag(q8, _plain_tiling(M, N), K), r1.tag
        assert r0.tag == _skinny_tag(q8, _plain_tiling(M, N), K, inflight=0), r0.tag
        assert rr.tag == _skinny_tag(q8, _plain_tiling(M, N), K, regs=1), rr.tag
        same_bits(r1, r0)
        same_bits(r1, rr)
        seen.add(r1.tag)
    if K == 3072 and M == 17:
        assert seen == {"skinny<1,1,8,12,3>", "skinny_q8<1,1,8,4,3>"}
    if K == 2048 and M == 65:
        assert seen == {"skinny<2,1,8,12,2>", "skinny_q8<2,1,8,4,2>"}
    if K == 640:
        assert all(t.endswith(",0>") for t in seen)


@pytest.mark.parametrize("M", (17, 65))
def test_skinny_wide_ragged_columns_and_cache_policy(M):
    r = _skinny_plain(False, M, 4128, 128)
    assert r.tag == ("skinny<2,1,8,12,0>" if M == 17 else "skinny<4,2,8,12,0>")
    r = _skinny_plain(True, M, 4128, 128)
    assert r.tag == ("skinny_q8<2,1,8,4,0>" if M == 17 else "skinny_q8<4,2,8,4,0>")
    a = _skinny_plain(False, M, 64, 1024, EPI_F16, wdef=1)
    b = _skinny_plain(False, M, 64, 1024, EPI_F16, wdef=0)
    assert (a.tag, b.tag) == (("skinny<1,1,8,12,1>", "skinny<1,1,8,4,1>") if M == 17 else ("skinny<2,1,8,12,1>", "skinny<2,1,8,4,1>"))
    same_bits(a, b)


SWIGLU_TAGS = {   # (M, N) -> f16 tiling at K = 1024
    1: "<1,2,4,12,2>", 9: "<1,2,4,12,2>", 16: "<1,2,4,12,2>", 17: "<2,2,4,12,2>", 33: "<4,2,8,12,1>", 64: "<4,2,8,12,1>"}


@pytest.mark.parametrize("M", ALL_M)
@pytest.mark.parametrize("N", (64, 96, 128))
def test_skinny_swiglu(M, N):
    """EPI_SWIGLU_Q8 is held bit for bit to the float32 restatement of q8_scale / q8_quant over the fp32 values of
    a second, EPI_SWIGLU_F32 run: both forms split K over the same 8 waves, so those are the values its epilogue
    quantises.  (With the fp32 form on 4 waves, as it was, one quant of 8192 came out one apart at M = 128, N = 128
    and none of 45,664 in the other cases; a float32 numpy restatement of the two splits gave the same count.)"""
    K = 1024
    for epi in (EPI_SWIGLU_F16, EPI_SWIGLU_F32):
        r, ref, bound = dense_call(SKINNY, epi, M, N, K)
        assert not r.declined, r.msg
        want = SWIGLU_TAGS[M] if M <= 64 else "<4,4,8,12,1>" if N % 64 == 0 else "<2,2,4,12,2>"
        assert r.tag == "skinny" + want, r.tag
        check_epilogue(r, epi, M, N, ref, bound, "skinny")
    # Q8_0: fp32 SwiGLU, and the same quantised in the epilogue -- bit for bit the restatement over the
    # kernel's own fp32 values (kernels.h: "the bits of EPI_SWIGLU_F32 + launch_quantize_q8")
    r, ref, bound = q8_call(SKINNY_Q8, EPI_SWIGLU_F32, M, N, K)
    assert r.tag == f"skinny_q8<{_mt(M, 2)},2,8,4,1>", r.tag
    check_epilogue(r, EPI_SWIGLU_F32, M, N, ref, bound, "skinny_q8")
    rq, _, _ = q8_call(SKINNY_Q8, EPI_SWIGLU_Q8, M, N, K)
    if N % 64:
        assert rq.declined
        ku.untouched(rq.out_q, rq.out_d)
        return
    assert rq.tag == ("skinny_q8<4,4,8,4,1>" if M > 64 else f"skinny_q8<{_mt(M, 2)},4,8,4,1>"), rq.tag
    v = ku.in_range(r.out_f32, M, N // 2)
    q = ku.in_range(rq.out_q, M, N // 2)
    d = ku.in_range(rq.out_d, M, N // 64)
    # dequantised, the quants sit within half a quant step (+ the fp16 rounding of the scale, 2^-11 of
    # up to 127 steps) of the float64 reference
    gate, up = ku.swiglu_rows(N // 2)
    vr, bv = ku.swiglu_terms(ref[:, gate], bound[:, gate], ref[:, up], bound[:, up])
    step = np.repeat(d.astype(np.float64), 32, axis=1)
    note("skinny_q8_dequantised", ku.check_values((q * step).astype(np.float32), vr, bv + (0.5 + 127 * 2.0 ** -11) * step + ku.U * np.abs(vr)))
    q_ref, d_ref = ku.q8_quantize(v)
    print(f"swiglu_q8 M={M} N={N}: {int((q != q_ref).sum())} of {q.size} quants, "
          f"{int((d.view(np.uint32) != d_ref.view(np.uint32)).sum())} of {d.size} scales differ from the restatement")
    ku.check_q8(q, d, q_ref, d_ref, "EPI_SWIGLU_Q8 against q8_quantize(EPI_SWIGLU_F32 output)")


# ====================================================================== launch_gemv
def _gemv_x(rng, M, K, src, n_embd=11):
    """the activation source and the fp16 rows the kernel multiplies: (kwargs, xh fp16 [M][K], tie mask or None)"""
    if src == "x":
        x = ku.f16_normal(rng, (M, K))
        return dict(x=ku.pad_cols(x.astype(np.float32), K + 4)), x, None
    if src == "xh":
        x = ku.f16_normal(rng, (M, K))
        return dict(xh=ku.pad_cols(x, K + 8)), x, None
    if src == "norm":
        x = (ku.f16_normal(rng, (M, K)).astype(np.float32) * 3).astype(np.float32)
        w = (1 + 0.25 * rng.standard_normal(K)).astype(np.float32)
        h, _, tie = ku.rms_prologue(x, w, 1e-6)
        assert tie.mean(1).max() <= 0.01, tie.mean(1)   # near-tie elements: at most 1 % of a row
        return dict(x=ku.pad_cols(x, K + 4), norm_w=w, eps=1e-6), h, tie
    embd = ku.f16_normal(rng, (n_embd, K))
    ids = rng.integers(0, n_embd, M)
    return dict(embd=embd, embd_ids=ids, x_store_ld=K + 4), embd[ids], None


# chosen on the CPU so that every RMS-norm case below has at most 1 % of a row's elements near an fp16
# rounding tie (asserted in _gemv_x; the near-tie elements are the only ones a bound gets slack for)
GEMV_SEED = 4


def gemv_call(epi, M, N, K, tag, *, src="x", bias=False, res=False, q8=False, book=None, launches=1, W=None, xfix=None):
    rng = np.random.default_rng([GEMV_SEED, M, N, K, epi, q8])
    swiglu = epi in (EPI_SWIGLU_F16, EPI_SWIGLU_F32)
    wrows = 2 * N if swiglu else N
    xkw, xh, tie = _gemv_x(rng, M, K, src)
    if xfix is not None:
        xkw, xh = xfix(xkw, xh)
    bv = rng.standard_normal(N).astype(np.float32) if bias else None
    rv = rng.standard_normal((M, N)).astype(np.float32) if res else None
    f32 = epi in (EPI_F32, EPI_SWIGLU_F32, EPI_ARGMAX)
    if q8:
        Wq, Wd = ku.q8_operand(rng, wrows, K, np.float16, 0.02 * K ** -0.5)
        wkw = dict(Wq=Wq, Wd=Wd)
        Aq, Ad = ku.q8_quantize(xh.astype(np.float32))   # the prologue: bit for bit the restatement, or the product is off
        ref, mag = ku.q8_terms(Aq, Ad, Wq, Wd)
        bound = ku.q8_bound(K, mag)
    else:
        if W is None:
            W = ku.f16_normal(rng, (wrows, K), K ** -0.5)
        wkw = dict(W=W)
        ref, mag = ku.dense_terms(xh, W)
        bound = ku.dense_bound(K, mag) + (ku.tie_slack(xh, tie, W) if tie is not None else 0.0)
    r = ku.run_gemv(epi, M, N, K, wrows=wrows, bias=bv, res=None if rv is None else ku.pad_cols(rv, N + 4),
                    ldo=N + 4 if f32 else 0, ldo16=0 if f32 else N + 4, amax=epi == EPI_ARGMAX, book=book, launches=launches,
                    **xkw, **wkw)
    assert not r.declined, r.msg
    assert r.tag == tag, r.tag
    family = "gemv_q8" if q8 else "gemv"
    if src == "embd":
        xs = ku.in_range(r.x_store, M, K)
        assert np.array_equal(xs, xh.astype(np.float32))
    if swiglu:
        gate, up = ku.swiglu_rows(N)
        v, bvv = ku.swiglu_terms(ref[:, gate], bound[:, gate], ref[:, up], bound[:, up])
        if epi == EPI_SWIGLU_F16:
            note(family + "_f16_out", ku.check_values(ku.in_range(r.out_f16, M, N), v, bvv, fp16=True))
        else:
            note(family, ku.check_values(ku.in_range(r.out_f32, M, N), v, bvv))
        return r
    ref, bound = ku.add_terms(ref, bound, bv, rv)
    if epi == EPI_F16:
        note(family + "_f16_out", ku.check_values(ku.in_range(r.out_f16, M, N), ref, bound, fp16=True))
    else:
        note(family, ku.check_values(ku.in_range(r.out_f32, M, N), ref, bound))
    return r


# every MR x CPW once at K = 1024 (M = 1 reaches the generic kernel through EPI_ARGMAX, which gemv1 does not take)
@pytest.mark.parametrize("M,N,tag", [
    (2, 5, "gemv<1,2,2>"), (2, 2050, "gemv<2,2,2>"), (2, 16424, "gemv<4,2,2>"),
    (3, 1, "gemv<1,4,2>"), (3, 2048, "gemv<2,4,2>"), (3, 8192, "gemv<4,4,2>"), (4, 2050, "gemv<2,4,2>"),
    (5, 5, "gemv<1,8,2>"), (5, 2050, "gemv<2,8,2>"), (5, 16424, "gemv<4,8,2>"), (8, 8192, "gemv<4,8,2>"), (8, 16424, "gemv<4,8,2>")])
def test_gemv_rows_and_columns(M, N, tag):
    gemv_call(EPI_F32, M, N, 1024, tag, bias=True, res=True)


@pytest.mark.parametrize("K,nk", [(256, 1), (1024, 2), (1536, 4), (2560, 6), (3072, 6), (3584, 8), (4096, 8)])
def test_gemv_every_nk(K, nk):
    gemv_call(EPI_F32, 2, 2050, K, f"gemv<2,2,{nk}>", bias=True, res=True)
    gemv_call(EPI_F16, 2, 2050, K, f"gemv<2,2,{nk}>", src="xh", bias=True)


@pytest.mark.parametrize("K", (256, 512, 1024, 1536, 2048, 3072))
def test_gemv_one_row(K):
    """M = 1: the gemv1 fast path at its five widths, the generic kernel otherwise"""
    fast = K != 1536
    nk = {256: 1, 512: 1, 1024: 2, 1536: 4, 2048: 4, 3072: 6}[K]
    gemv_call(EPI_F32, 1, 2050, K, f"gemv1<{K},1>" if fast else f"gemv<2,1,{nk}>", src="norm", bias=True, res=True)
    gemv_call(EPI_F32, 1, 8192, K, f"gemv1<{K},2>" if fast else f"gemv<4,1,{nk}>", bias=True)
    gemv_call(EPI_F16, 1, 5, K, f"gemv1<{K},1>" if fast else f"gemv<1,1,{nk}>", src="xh", bias=True)
    gemv_call(EPI_SWIGLU_F16, 1, 4096, K, f"gemv1<{K},1>" if fast else f"gemv<2,1,{nk}>", src="norm")
    gemv_call(EPI_F32, 1, 2050, K, f"gemv1<{K},1>" if fast else f"gemv<2,1,{nk}>", src="embd", res=True)


@pytest.mark.parametrize("M", (2, 3, 8))
def test_gemv_epilogues_and_sources(M):
    mr = {2: 2, 3: 4, 8: 8}[M]
    gemv_call(EPI_F32, M, 2050, 1024, f"gemv<2,{mr},2>", src="norm", bias=True, res=True)
    gemv_call(EPI_F32, M, 16424, 1024, f"gemv<4,{mr},2>", src="embd", res=True)
    gemv_call(EPI_F16, M, 2050, 1024, f"gemv<2,{mr},2>", src="embd", bias=True)
    gemv_call(EPI_F16, M, 5, 1536, f"gemv<1,{mr},4>", src="norm")
    gemv_call(EPI_SWIGLU_F16, M, 2048, 1024, f"gemv<2,{mr},2>", src="norm")
    gemv_call(EPI_SWIGLU_F16, M, 8192, 256, f"gemv<4,{mr},1>", src="embd")
    gemv_call(EPI_SWIGLU_F16, M, 16, 3072, f"gemv<1,{mr},6>", src="xh")


def _check_gemv_argmax(r, M, N):
    logits = ku.in_range(r.out_f32, M, N)
    idx = ku.key_index(r.amax[:M])
    ku.check_argmax(idx, logits)
    assert np.array_equal(ku.key_value(r.amax[:M]), logits.max(1))
    return idx


@pytest.mark.parametrize("M,N,tag", [(1, 5, "gemv<1,1,2>"), (1, 2050, "gemv<2,1,2>"), (1, 16424, "gemv<4,1,2>"), (3, 2050, "gemv<2,4,2>"),
                                     (8, 16424, "gemv<4,8,2>")])
def test_gemv_argmax(M, N, tag):
    r = gemv_call(EPI_ARGMAX, M, N, 1024, tag, src="norm")
    _check_gemv_argmax(r, M, N)
    r = gemv_call(EPI_ARGMAX, M, N, 1024, tag, src="embd")
    _check_gemv_argmax(r, M, N)


@pytest.mark.parametrize("M,N", [(3, 2050), (5, 16424)])
def test_gemv_argmax_ties_and_bookkeeping(M, N):
    K, c, step0, stride = 1024, 7, 4, 12
    rng = np.random.default_rng([5, M, N])
    W = ku.f16_normal(rng, (N, K), K ** -0.5)
    W[c, 0] = 4.0
    for d in (1, 16, N // 2):
        W[c + d] = W[c]

    def xfix(xkw, xh):
        xh = xh.copy()
        xh[:, 0] = 8.0
        return dict(x=ku.pad_cols(xh.astype(np.float32), K + 4)), xh

    tag = f"gemv<{2 if N < 8192 else 4},{4 if M == 3 else 8},2>"
    r = gemv_call(EPI_ARGMAX, M, N, K, tag, W=W, xfix=xfix)
    assert (_check_gemv_argmax(r, M, N) == c).all()   # the lowest of the four equal columns
    pos0 = np.arange(M) * 3 + 20
    r = gemv_call(EPI_ARGMAX, M, N, K, tag, W=W, xfix=xfix, book=dict(step=step0, pos=pos0, hist_stride=stride), launches=2)
    logits = ku.in_range(r.out_f32, M, N)
    want = np.argmax(logits, 1)
    assert (want == c).all()
    assert np.array_equal(r.tok_out[:M], want) and (r.tok_out[M:] == -7).all()
    hist = np.full((M, stride), -7)
    hist[:, step0 + 1] = want
    hist[:, step0 + 2] = want   # the second launch on the same state: the first re-armed it
    assert np.array_equal(r.hist, hist)
    assert np.array_equal(r.pos[:M], pos0 + 2) and not r.pos[M:].any() and r.step[0] == step0 + 2
    assert not r.amax.any() and r.done[0] == 0   # zero at rest


@pytest.mark.parametrize("K,nk", [(256, 1), (1024, 1), (2048, 2), (3072, 3), (4096, 4)])
def test_gemv_q8(K, nk):
    gemv_call(EPI_F32, 2, 2050, K, f"gemv_q8<2,2,{nk}>", q8=True, bias=True, res=True)
    gemv_call(EPI_F32, 1, 5, K, f"gemv_q8<1,1,{nk}>", q8=True, src="embd", res=True)
    gemv_call(EPI_SWIGLU_F32, 3, 2048, K, f"gemv_q8<2,4,{nk}>", q8=True)
    gemv_call(EPI_SWIGLU_F32, 8, 16, K, f"gemv_q8<1,8,{nk}>", q8=True, src="embd")
    gemv_call(EPI_F32, 5, 16424, K, f"gemv_q8<2,8,{nk}>", q8=True, bias=True)


# ====================================================================== launch_quantize_q8
@pytest.mark.parametrize("M,K,gC", [(5, 512, 0), (3, 96, 0), (2049, 256, 0), (7, 96, 6), (65, 7680, 480)])
@pytest.mark.parametrize("half", (False, True))
def test_quantize_q8(M, K, gC, half):
    rng = np.random.default_rng([4, M, K, gC, half])
    src = ku.f16_normal(rng, (M, K)) if half else (rng.standard_normal((M, K)) * 3).astype(np.float32)
    src[min(2, M - 1), 32:64] = 0   # an all-zero block
    ld = K + 4
    q, d = ku.run_quantize(M, K, gather_C=gC, **{"x16" if half else "x32": ku.pad_cols(src, ld)})
    j = np.arange(K)
    v = src[:, (j & 15) * gC + (j >> 4)] if gC else src
    q_ref, d_ref = ku.q8_quantize(v.astype(np.float32))
    ku.check_q8(ku.in_range(q, M, K), ku.in_range(d, M, K // 32), q_ref, d_ref)


# ====================================================================== contract: declined, nothing written
def _declined(r):
    assert r.declined and r.msg and not r.tag, (r.declined, r.msg, r.tag)
    ku.untouched(r.out_f32, r.out_f16, r.out_q, r.out_d)


@pytest.mark.parametrize("M,N,K,kw", [(65, 96, 64, {}), (129, 2080, 96, {}), (2049, 2080, 96, {}), (65, 64, 40, {}),
                                      (2049, 256, 40, {}), (2049, 384, 40, {}), (2049, 288, 256, dict(regs_staged=1))])
def test_gemm_declines_shapes_it_would_run_short(M, N, K, kw):
    """N % 64 != 0 left the last columns unwritten and K % 32 != 0 dropped the last terms before the launcher checked"""
    for epi in (EPI_F32, EPI_F16, EPI_ARGMAX):
        _declined(dense_call(GEMM, epi, M, N, K, **kw)[0])


def test_gemm_q8_declines():
    _declined(q8_call(GEMM_Q8, EPI_F16, 65, 64, 128)[0])     # an epilogue it does not instantiate
    _declined(q8_call(GEMM_Q8, EPI_ARGMAX, 65, 64, 128)[0])
    _declined(q8_call(GEMM_Q8, EPI_F32, 65, 64, 48)[0])      # half a block
    _declined(q8_call(GEMM_Q8, EPI_F32, 65, 96, 128)[0])


def test_skinny_declines():
    _declined(dense_call(SKINNY, EPI_F32, 129, 64, 128)[0])
    _declined(dense_call(SKINNY, EPI_F32, 17, 64, 192)[0])
    _declined(q8_call(SKINNY_Q8, EPI_F32, 129, 64, 128)[0])
    _declined(q8_call(SKINNY_Q8, EPI_GELU_F16, 17, 64, 128)[0])


@pytest.mark.parametrize("M,N,K,epi,q8", [(2, 2050, 4608, EPI_F32, False), (2, 2050, 260, EPI_F32, False), (1, 2050, 260, EPI_F16, False),
                                          (2, 5, 1024, EPI_SWIGLU_F16, False), (2, 64, 1024, EPI_SWIGLU_F32, False),
                                          (2, 2050, 8704, EPI_F32, True), (2, 2050, 272, EPI_F32, True),
                                          (2, 64, 1024, EPI_F16, True)])
def test_gemv_declines(M, N, K, epi, q8):
    """K > 4096 was summed over its first 4096 terms only; K % 8 != 0 read past the row"""
    rng = np.random.default_rng([6, K])
    wrows = 2 * N if epi in (EPI_SWIGLU_F16, EPI_SWIGLU_F32) else N
    wq, wd = ku.q8_operand(rng, wrows, K - K % 32, np.float16)
    wkw = dict(Wq=ku.pad_cols(wq, K, 1), Wd=wd) if q8 else dict(W=ku.f16_normal(rng, (wrows, K)))
    f32 = epi in (EPI_F32, EPI_SWIGLU_F32)
    r = ku.run_gemv(epi, M, N, K, wrows=wrows, x=ku.pad_cols(ku.f16_normal(rng, (M, K)).astype(np.float32), K + 4),
                    ldo=N + 4 if f32 else 0, ldo16=0 if f32 else N + 4, **wkw)
    assert r.declined and r.msg and not r.tag, (r.declined, r.msg, r.tag)
    ku.untouched(r.out_f32, r.out_f16)
