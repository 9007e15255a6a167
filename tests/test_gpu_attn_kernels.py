"""The norm, RoPE and prefill / encoder attention launchers against float64 references.

launch_layernorm_f16, launch_rmsnorm_f16 / _q8, launch_qkv_post, launch_enc_attention (split-fp16 and fp32-MFMA
forms), launch_prefill_attention and launch_prefill_attention_exact (fp16 scores and the aligner's fp32 scores) are
called directly through the test-only entries qasr_kt_norm / _qkv_post / _enc_attention / _prefill_attention
(csrc/kernel_harness.hip), at the smallest shapes at which each can still go wrong: every row count around the
four-rows-a-block seam, every tile seam of the attention kernels (16 / 32 / 64 / 128 keys, one to four tiles for
the encoder's alternating wave groups), cached prefixes, both ends of an 8-key V^T block.  Inputs carry NaN guard
rows, NaN rows between segments / sequences and NaN in every cache row at or past a sequence's key count (and in
the kKvPadRows rows the exact kernel stages past the last cache region): no output may be NaN, so none of them
enters an output.  Outputs sit between 0xFF sentinels; rows no segment owns and cache rows no token owns keep
them.  References, bounds (derived, none measured) and comparators: tests/attn_util.py; their sharpness:
tests/test_kernel_util_host.py.  The exact prefill kernel with fp16 scores is held to a numpy restatement of
ggml's chain to the last bit of the accumulator outside a near-tie mask (capped at 5 % of a case); with q32 / k32
its scores are fp32 sums whose order is not pinned, so there the float64 reference with the chain's bound term
applies and the bit-level rule does not.  The worst error / bound per family, the near-tie shares and the file's
wall time go to the parity record ("attention_reference_tests").
"""
import functools
import time

import numpy as np
import pytest

import attn_util as au
import kernel_util as ku

pytestmark = pytest.mark.gpu

WORST, SHARE = {}, {}


def note(family, ratio):
    assert ratio <= 1.0, (family, ratio)
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))


def note_share(family, share):
    assert share <= 0.05, (family, share)
    SHARE[family] = max(SHARE.get(family, 0.0), float(share))


@pytest.fixture(scope="module", autouse=True)
def _record(gpu, parity):
    t0 = time.time()
    yield
    parity("attention_reference_tests", wall_s=time.time() - t0, **{f"{k}_worst_over_bound": v for k, v in sorted(WORST.items())},
           **{f"{k}_near_tie_share": v for k, v in sorted(SHARE.items())})


MS = (1, 4, 5, 9)   # four rows a block: one row, a full block, one row into the next, two blocks and one


# ==================================================================== norms
@pytest.mark.parametrize("D", [256, 896, 1024, 2048])
def test_layernorm(D):
    rng = np.random.default_rng([D, 1])
    w = (1 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    for M in MS:
        x = au.norm_rows(rng, M, D)
        for wv, bv in ((w, b), (None, None), (w, None)):
            ref, bound = au.layernorm_ref(x, wv, bv, 1e-5)
            for f32 in (False, True):
                r = au.run_norm(au.LN, x, M, D, w=wv, b=bv, eps=1e-5, f32=f32)
                assert not r.declined, r.msg
                out = ku.in_range(r.y32 if f32 else r.y, M, D, "layernorm")
                note("layernorm" if f32 else "layernorm_f16_out", ku.check_values(out, ref, bound, fp16=not f32, what=f"layernorm D {D} M {M}"))


@pytest.mark.parametrize("D", [256, 1024, 2048])
def test_rmsnorm(D):
    rng = np.random.default_rng([D, 2])
    w = (1 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    for M in MS:
        xs = au.norm_rows(rng, M + 2, D)
        # in order, and gathered: reversed with a repeat
        idx = (M + 1 - np.arange(M)).astype(np.int32)
        idx[-1] = idx[0]
        for row_idx in (None, idx):
            x = xs[:M] if row_idx is None else xs[row_idx]
            ref, bound = au.rmsnorm_ref(x, w, 1e-6)
            for f32 in (False, True):
                r = au.run_norm(au.RMS, ku.pad_cols(xs, D + 4), M, D, w=w, eps=1e-6, row_idx=row_idx, f32=f32)
                assert not r.declined, r.msg
                out = ku.in_range(r.y32 if f32 else r.y, M, D, "rmsnorm")
                note("rmsnorm" if f32 else "rmsnorm_f16_out", ku.check_values(out, ref, bound, fp16=not f32, what=f"rmsnorm D {D} M {M}"))
                if not f32:
                    note_share("rmsnorm", au.check_rms_bits(out, x, w, 1e-6))
        # Q8_0 output: the restated fp32 values, quantised
        r = au.run_norm(au.RMS_Q8, ku.pad_cols(xs, D + 4), M, D, w=w, eps=1e-6)
        assert not r.declined, r.msg
        q_ref, d_ref = ku.q8_quantize(ku.rms_prologue(xs[:M], w, 1e-6)[1])
        ku.check_q8(ku.in_range(r.yq, M, D, "yq"), ku.in_range(r.yd, M, D // 32, "yd"), q_ref, d_ref, what=f"rmsnorm_q8 D {D} M {M}")


# ================================================================= qkv_post
@pytest.mark.parametrize("heads", [(16, 8), (8, 4), (2, 1), (3, 1)])
def test_qkv_post(heads):
    for rows in (1, 3, 5):
        case = au.qkv_case(heads[0], heads[1], rows)
        q, bq, k, bk, v = au.qkv_post_ref(case)
        want_vt = au.vt_expected(case, v)
        for f32 in (False, True):
            r = au.run_qkv_post(case, f32)
            assert not r.declined, r.msg
            what = f"qkv_post {heads} rows {rows}"
            note("qkv_post_f16_out", ku.check_values(ku.in_range(r.q_out, rows, heads[0] * 128, "q_out"), q, bq, fp16=True, what=what + " q"))
            note("qkv_post_f16_out", au.check_cache_rows(r.kc, case, k, bk, what + " kc"))
            au.check_cache_rows(r.vc, case, v, None, what + " vc")
            au.check_vt(r.vt, want_vt)
            if f32:
                note("qkv_post", ku.check_values(ku.in_range(r.q32, rows, heads[0] * 128, "q32"), q, bq, what=what + " q32"))
                note("qkv_post", ku.check_values(ku.in_range(r.k32, rows, heads[1] * 128, "k32"), k, bk, what=what + " k32"))


# ======================================================== encoder attention
@functools.lru_cache(maxsize=None)
def enc_ref(H, scale_log2, spike, f32_mfma):
    return au.enc_reference(au.enc_case(H, scale_log2, spike), f32_mfma)


def enc_check(H, scale_log2, spike, f32_mfma, f32_out):
    case = au.enc_case(H, scale_log2, spike)
    ref, bound, valid = enc_ref(H, scale_log2, spike, f32_mfma)
    r = au.run_enc_attention(case, f32_mfma, f32_out)
    assert not r.declined, r.msg
    fam = ("enc_attention_f32mfma" if f32_mfma else "enc_attention_split") + ("" if f32_out else "_f16_out")
    note(fam, au.check_rows(r.out32 if f32_out else r.out, valid, ref, bound, not f32_out, f"{fam} H {H} scale 2^{scale_log2} spike {spike}"))


@pytest.mark.parametrize("f32_mfma", [False, True])
@pytest.mark.parametrize("H", [1, 2, 14])
def test_enc_attention(H, f32_mfma):
    for f32_out in (False, True):
        enc_check(H, 0, False, f32_mfma, f32_out)


@pytest.mark.parametrize("f32_mfma", [False, True])
def test_enc_attention_operand_scales_and_spike(f32_mfma):
    for scale_log2 in (-6, 3):
        for f32_out in (False, True):
            enc_check(2, scale_log2, False, f32_mfma, f32_out)
    enc_check(2, 0, True, f32_mfma, True)   # one key 40 above the rest


# ======================================================== prefill attention
FRESH = tuple((0, L) for L in au.PREFILL_L)
HEADS = [(2, 1), (16, 8)]


@functools.lru_cache(maxsize=None)
def plain_ref(heads, seqs):
    case = au.prefill_case(heads[0], heads[1], seqs, 11, False)
    return case, au.prefill_reference(case)


@functools.lru_cache(maxsize=None)
def chain_ref(heads, seqs):
    case = au.prefill_case(heads[0], heads[1], seqs, au.EXACT_SEED if seqs == FRESH else au.EXACT_SEED_CACHED, True)
    return case, au.exact_chain(case)


@pytest.mark.parametrize("seqs", [FRESH, au.PREFILL_CACHED], ids=["fresh", "cached"])
@pytest.mark.parametrize("heads", HEADS)
def test_prefill_attention(heads, seqs):
    case, (ref, bound) = plain_ref(heads, seqs)
    for f32_out in (False, True):
        r = au.run_prefill(case, False, f32_out)
        assert not r.declined, r.msg
        fam = "prefill_attention" + ("" if f32_out else "_f16_out")
        note(fam, au.check_rows(r.out32 if f32_out else r.out, au.prefill_valid(case), ref, bound, not f32_out, f"{fam} {heads}"))


@pytest.mark.parametrize("seqs", [FRESH, au.PREFILL_CACHED], ids=["fresh", "cached"])
@pytest.mark.parametrize("heads", HEADS)
def test_prefill_attention_exact(heads, seqs):
    case, chain = chain_ref(heads, seqs)
    for f32_out in (False, True):
        r = au.run_prefill(case, True, f32_out)
        assert not r.declined, r.msg
        fam = "prefill_exact" + ("" if f32_out else "_f16_out")
        ratio, share = au.check_exact(r.out32 if f32_out else r.out, case, chain, not f32_out, f"{fam} {heads}")
        note(fam, ratio)
        note_share("prefill_exact", share)


@pytest.mark.parametrize("heads", HEADS)
def test_prefill_attention_exact_fp32_scores(heads):
    """q32 / k32 (the aligner): the scores are fp32 sums of fp32 products in the MFMA's order, so the chain's inputs
    are not pinned to the bit and the restatement's bit-level rule does not apply; the float64 reference with one
    fp16 rounding of the accumulator per key in its bound (au.prefill_reference) does"""
    case = au.prefill_case(heads[0], heads[1], FRESH, 13, False, True)
    ref, bound = au.prefill_reference(case, fp32_scores=True)
    for f32_out in (False, True):
        r = au.run_prefill(case, True, f32_out)
        assert not r.declined, r.msg
        fam = "prefill_exact_fp32_scores" + ("" if f32_out else "_f16_out")
        note(fam, au.check_rows(r.out32 if f32_out else r.out, au.prefill_valid(case), ref, bound, not f32_out, f"{fam} {heads}"))


# ================================================================= declines
def test_declined_shapes_write_nothing():
    rng = np.random.default_rng(5)
    for D, ldx in ((512, 516), (4096, 4100), (256, 258)):   # a width without an instance (below and above 2048); rows not 16-B aligned
        x = rng.standard_normal((3, ldx)).astype(np.float32)
        w = np.ones(D, np.float32)
        for f32 in (False, True):
            r = au.run_norm(au.RMS, x, 3, D, w=w, f32=f32)
            assert r.declined and "launch_rmsnorm_f16 has no kernel" in r.msg, r.msg
            ku.untouched(r.y32 if f32 else r.y)
        r = au.run_norm(au.RMS_Q8, x, 3, D, w=w)
        assert r.declined and "launch_rmsnorm_q8 has no kernel" in r.msg, r.msg
        ku.untouched(r.yq, r.yd)
    for D in (2049, 2304, 4096):
        x = rng.standard_normal((3, D)).astype(np.float32)
        for f32 in (False, True):
            r = au.run_norm(au.LN, x, 3, D, f32=f32)
            assert r.declined and "launch_layernorm_f16 has no kernel" in r.msg, r.msg
            ku.untouched(r.y32 if f32 else r.y)
    for heads in ((3, 1), (1, 1), (4, 1)):
        case = au.prefill_case(heads[0], heads[1], ((0, 5), (0, 17)), 1, False)
        for f32_out in (False, True):
            r = au.run_prefill(case, False, f32_out)
            assert r.declined and "launch_prefill_attention has no kernel" in r.msg, r.msg
            ku.untouched(r.out32 if f32_out else r.out)


def test_enc_attention_rejects_other_head_dims():
    case = au.enc_case(2, lens=(5, 17))
    assert au.run_enc_attention(case, False, True, expect_rc=au.QASR_ERR_ARG, H=3) is None
    assert au.run_enc_attention(case, True, False, expect_rc=au.QASR_ERR_ARG, H=1) is None
