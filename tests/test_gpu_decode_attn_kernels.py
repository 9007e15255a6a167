"""The decode attention launchers that do not wait in-launch, against references of their own.

launch_decode_attention (every dispatch branch: 64 / 128 / 256-key splits, the per-sequence kernel, scores mode),
launch_decode_attention_exact (single-head and pair kernels) and launch_decode_attention_exact_seq are called through
the test-only entry qasr_kt_decode_attention (csrc/kernel_harness.hip); the fused batch-1 launch stays with its
bit-identity tests against these kernels.  Cases, references, bounds (derived, none measured) and comparators:
tests/decode_attn_util.py; their sharpness: tests/test_kernel_util_host.py.  Every case asserts the kernel tag the
launchers recorded.  Inputs follow the cache contract of csrc/kernels.h (above DecodeAttnArgs): NaN in every K / V
row above pos and every V^T key block after pos's, +-65504 junk in row pos and in the rest of pos's V^T block -- no
output may be NaN or show the junk; after each call the caches equal the input except row / column pos.  Batches mix
lengths, so short sequences meet empty splits of a grid sized for the longest.  The harness checks the split counters
zero after every launch and, with repeat 2, launches twice on the same part and counter: the two outputs must be
bit-identical (the counter re-arm and the index-ordered combine).  The worst error / bound per family and the
near-tie shares go to the parity record ("decode_attention_reference_tests").
"""
import functools
import time

import numpy as np
import pytest

import decode_attn_util as du
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
    parity("decode_attention_reference_tests", wall_s=time.time() - t0, **{f"{k}_worst_over_bound": v for k, v in sorted(WORST.items())},
           **{f"{k}_near_tie_share": v for k, v in sorted(SHARE.items())})


SHORT = (0, 1, 15, 16, 31, 32, 33, 62)           # one 64-key split
MID = (63, 64, 65, 127, 128, 129, 255, 256)      # both sides of the 64 / 128 / 256-key seams
TOP = (257, 319, 0)                              # ... and max_ctx - 1 = 319
NINE = (0, 63, 64, 65, 127, 128, 129, 192, 257)  # a batch of 9: the chunk seams of both register sets
CTX = 320


@functools.lru_cache(maxsize=None)
def generic_ref(pos, nkv, max_ctx, spl, grid_splits, kscale_log2=0, spike=False):
    case = du.decode_case(pos, nkv, max_ctx, 11, False, kscale_log2, spike)
    return case, du.decode_reference(case, spl, grid_splits)


def outputs(r, kind, sfx=""):
    return (getattr(r, "outq" + sfx), getattr(r, "outd" + sfx)) if kind == "q8" else (getattr(r, ("out32" if kind == "f32" else "out") + sfx),)


def plain_check(pos, nkv, max_ctx, tag, *, kind="f32", grid_splits=None, repeat=1, kscale_log2=0, spike=False, **call):
    gs = grid_splits or max(pos) // 64 + 1
    spl = du.split_of(dict(B=len(pos), n_kv_head=nkv), dict(call, grid_splits=gs))
    case, (ref, bound) = generic_ref(pos, nkv, max_ctx, spl, gs, kscale_log2, spike)
    r = du.run_decode(case, du.PLAIN, kind, grid_splits=gs, repeat=repeat, **call)
    assert not r.declined, r.msg
    assert r.tag == tag, r.tag
    fam = ("decode_split" if spl else "decode_seq") + ("_f16_out" if kind == "f16" else "")
    what = f"{tag} pos {pos} {kind}"
    B, QD = case["B"], case["n_head"] * 128
    if kind == "q8":   # the same case's fp32 output, quantised: bit for bit
        r32 = du.run_decode(case, du.PLAIN, "f32", grid_splits=gs, **call)
        q_ref, d_ref = ku.q8_quantize(ku.in_range(r32.out32, B, QD, what))
        ku.check_q8(ku.in_range(r.outq, B, QD, "outq"), ku.in_range(r.outd, B, QD // 32, "outd"), q_ref, d_ref, what=what)
    else:
        note(fam, ku.check_values(ku.in_range(outputs(r, kind)[0], B, QD, what), ref, bound, fp16=kind == "f16", what=what))
    note("decode_new_k_row", du.check_caches(r, case, what))
    if repeat == 2:
        for a, b in zip(outputs(r, kind), outputs(r, kind, "_b")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: the second launch on the same part / counter differs"
    return r


# ============================================================ split kernels
@pytest.mark.parametrize("pos,gs", [(SHORT, 1), (MID, 5), (TOP, 5)], ids=["short", "mid", "top"])
def test_split_64_and_128(pos, gs):
    nkv = 2 if pos is TOP else 1
    plain_check(pos, nkv, CTX, "decode_split<64>", spl1=64, grid_splits=gs, repeat=2)
    plain_check(pos, nkv, CTX, "decode_split<128>", spl1=128, grid_splits=gs, repeat=2)


def test_split_auto_on_both_sides_of_30_splits():
    plain_check(MID, 1, CTX, "decode_split<64>", grid_splits=29)     # 29 64-key splits, 24 of them empty for every sequence
    plain_check(MID, 1, CTX, "decode_split<128>", grid_splits=30)    # 15 128-key splits


def test_split_combiner_passes():
    """1 split (above), 16 and 17: the combiner's second pass of 16, and a pos = 0 sequence in the 17-split grid"""
    plain_check((1023, 700), 1, 1100, "decode_split<64>", spl1=64, grid_splits=16, repeat=2)
    plain_check((1087, 0), 1, 1100, "decode_split<64>", spl1=64, grid_splits=17, repeat=2)


def test_split_outputs_f16_and_q8():
    for kind in ("f16", "q8"):
        plain_check(MID, 1, CTX, "decode_split<64>", kind=kind, spl1=64, grid_splits=5, repeat=2)
        plain_check(NINE, 1, CTX, "decode_split<256>", kind=kind, grid_splits=5, spl_batch=256)


def test_split_operand_scales_and_spike():
    for ks in (-6, 3):
        plain_check(MID, 1, CTX, "decode_split<64>", spl1=64, grid_splits=5, kscale_log2=ks)
    plain_check(MID, 1, CTX, "decode_split<128>", spl1=128, grid_splits=5, spike=True)
    plain_check(NINE, 1, CTX, "decode_seq<0>", grid_splits=5, stream_blocks=2, spike=True)


@pytest.mark.parametrize("spl", [128, 256])
def test_batch_of_nine_split(spl):
    plain_check(NINE, 1, CTX, f"decode_split<{spl}>", grid_splits=5, spl_batch=spl, stream_blocks=0, repeat=2)


# ===================================================== per-sequence kernel
def test_batch_of_nine_per_sequence():
    for kind in ("f32", "f16", "q8"):
        plain_check(NINE, 1, CTX, "decode_seq<0>", kind=kind, grid_splits=5, stream_blocks=2, repeat=2 if kind == "f32" else 1)
    plain_check(NINE + TOP, 2, CTX, "decode_seq<0>", grid_splits=5, stream_blocks=8)
    for ks in (-6, 3):
        plain_check(NINE, 1, CTX, "decode_seq<0>", grid_splits=5, stream_blocks=2, kscale_log2=ks)


def test_kv_nt_is_bit_identical():
    for pos, call, tag in ((MID, dict(spl1=64), "decode_split<64>"), (NINE, dict(stream_blocks=2), "decode_seq<0>")):
        case = du.decode_case(pos, 1, CTX, 11)
        a = du.run_decode(case, du.PLAIN, "f32", grid_splits=5, kv_nt=0, **call)
        b = du.run_decode(case, du.PLAIN, "f32", grid_splits=5, kv_nt=1, **call)
        assert a.tag == b.tag == tag
        assert np.array_equal(a.out32.view(np.uint32), b.out32.view(np.uint32)) and np.array_equal(a.kc, b.kc)
    case = du.decode_case(NINE, 1, CTX, 11)
    for mode, tag in ((du.EXACT_SEQ, "decode_seq<1>"), (du.EXACT, "decode_seq<0>+decode_exact<1>")):
        a = du.run_decode(case, mode, "f32", grid_splits=5, stream_blocks=2, kv_nt=0)
        b = du.run_decode(case, mode, "f32", grid_splits=5, stream_blocks=2, kv_nt=1)
        assert a.tag == b.tag == tag
        assert np.array_equal(a.out32.view(np.uint32), b.out32.view(np.uint32)) and np.array_equal(a.vt, b.vt)


# ================================================== lattice family: scores
LAT = (0, 30, 31, 32, 62, 63, 64, 129)   # key counts 1, 31, 32, 33, 63, 64, 65 and three 64-key chunks
LAT9 = LAT + (257,)


@pytest.mark.parametrize("pos,call,tag", [
    (LAT, dict(spl1=64), "decode_split<64>"), (LAT, dict(spl1=128), "decode_split<128>"),
    (LAT9, dict(spl_batch=128), "decode_split<128>"), (LAT9, dict(spl_batch=256), "decode_split<256>"),
    (LAT9, dict(stream_blocks=2), "decode_seq<0>")], ids=["s64", "s128", "b128", "b256", "seq"])
def test_scores_bit_exact(pos, call, tag):
    case = du.decode_case(pos, 1, CTX, du.LATTICE_SEED, True)
    want = du.lattice_scores(case).astype(np.float32)
    r = du.run_decode(case, du.SCORES, grid_splits=5, **call)
    assert not r.declined and r.tag == tag, (r.tag, r.msg)
    raw = r.scores.view(np.uint32)
    assert (raw[:du.GUARD] == 0xFFFFFFFF).all() and (raw[-du.GUARD:] == 0xFFFFFFFF).all(), "guard rows overwritten"
    body = raw[du.GUARD:-du.GUARD].reshape(want.shape)
    masked = np.isnan(want)
    assert (body[masked] == 0xFFFFFFFF).all(), "a masked position of the scores buffer was written"
    assert np.array_equal(body[~masked], want[~masked].view(np.uint32)), "scores differ from the float64 reference's bits"
    du.check_caches(r, case, tag + " scores mode")


# =================================================== lattice family: chain
@functools.lru_cache(maxsize=None)
def lattice_ref(pos, max_ctx, wmax):
    case = du.decode_case(pos, 1, max_ctx, du.LATTICE_SEED, True, wmax=wmax)
    return case, du.lattice_chain(case)


def exact_check(case, chain, mode, tag, kind="f32", **call):
    r = du.run_decode(case, mode, kind, **call)
    assert not r.declined, r.msg
    assert r.tag == tag, r.tag
    fam = "decode_exact" + ("_f16_out" if kind == "f16" else "")
    if kind == "q8":
        r32 = du.run_decode(case, mode, "f32", **call)
        B, QD = case["B"], case["n_head"] * 128
        q_ref, d_ref = ku.q8_quantize(ku.in_range(r32.out32, B, QD, tag))
        ku.check_q8(ku.in_range(r.outq, B, QD, "outq"), ku.in_range(r.outd, B, QD // 32, "outd"), q_ref, d_ref, what=tag)
    else:
        ratio, share = du.check_chain(outputs(r, kind)[0], chain, kind == "f16", f"{tag} pos {tuple(case['pos'])}")
        note(fam, ratio)
        note_share("decode_exact", share)
    if mode != du.CHAIN:
        du.check_caches(r, case, tag)
    return r


def test_exact_two_launches_short():
    case, chain = lattice_ref(LAT, CTX, 12)
    for kind in ("f32", "f16", "q8"):
        exact_check(case, chain, du.EXACT, "decode_split<64>+decode_exact<1>", kind, grid_splits=5, spl1=64, repeat=2 if kind == "f32" else 1)


@pytest.mark.parametrize("pos", [(2046, 2047), (2048, 32)], ids=["2047_2048", "2049"])
def test_exact_two_launches_two_weight_chunks(pos):
    case, chain = lattice_ref(pos, 2112, 32)
    exact_check(case, chain, du.EXACT, "decode_split<128>+decode_exact<1>", grid_splits=33)


def test_exact_one_launch_matches_two():
    """decode_attn_seq_kernel<1> against the scores launch followed by the pair kernel: bit-identical (the comment
    above the kernel claims it), and both against the restatement"""
    case, chain = lattice_ref(LAT9, CTX, 12)
    call = dict(grid_splits=5, stream_blocks=2, fx_seq=1)
    for kind in ("f32", "f16", "q8"):
        one = exact_check(case, chain, du.EXACT_SEQ, "decode_seq<1>", kind, **call)
        two = exact_check(case, chain, du.EXACT, "decode_seq<0>+decode_exact<1>", kind, **call)
        for a, b in zip(outputs(one, kind), outputs(two, kind)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{kind}: one launch and two launches differ"
        assert np.array_equal(one.kc, two.kc) and np.array_equal(one.vc, two.vc) and np.array_equal(one.vt, two.vt)
    case, chain = lattice_ref((2048, 2047, 2046, 64, 63, 0, 1, 500, 1000), 2112, 32)
    call = dict(grid_splits=33, stream_blocks=2, fx_seq=1)
    one = exact_check(case, chain, du.EXACT_SEQ, "decode_seq<1>", **call)
    two = exact_check(case, chain, du.EXACT, "decode_seq<0>+decode_exact<1>", **call)
    assert np.array_equal(one.out32.view(np.uint32), two.out32.view(np.uint32))


@pytest.mark.parametrize("rise", ["late", "early"])
def test_chain_alone_pair_against_single_head(rise):
    """mode 4 on supplied scores: the maximum rises in the second weights chunk (late) or never does (early); the pair
    kernel (n_head 2, n_kv_head 1) against the single-head kernel (n_head = n_kv_head = 2, V^T duplicated)"""
    pair = du.chain_case((2048, 2047), 2, 1, 2112, du.CHAIN_SEED, rise, 4.0)
    chain = du.chain_case_reference(pair)
    single = dict(pair, n_kv_head=2, ratio=1, vt=np.repeat(pair["vt"], 2, 1), V=np.repeat(pair["V"], 2, 1))
    a = exact_check(pair, chain, du.CHAIN, "decode_exact<1>")
    b = exact_check(single, chain, du.CHAIN, "decode_exact<0>")
    assert np.array_equal(a.out32.view(np.uint32), b.out32.view(np.uint32)), "pair and single-head kernels differ"
    assert np.array_equal(a.vt, ku.bits(pair["vt"])) and np.array_equal(b.vt, ku.bits(single["vt"])), "the chain wrote V^T"


def test_chain_alone_short_and_other_ratios():
    for ratio, nkv, tag in ((2, 1, "decode_exact<1>"), (3, 1, "decode_exact<0>"), (4, 2, "decode_exact<1>"), (1, 1, "decode_exact<0>")):
        case = du.chain_case((0, 30, 31, 32, 62, 63, 64), ratio, nkv, 96, du.CHAIN_SEED)
        for kind in ("f32", "f16"):
            exact_check(case, du.chain_case_reference(case), du.CHAIN, tag, kind)


# ================================================================= declines
def _untouched(r, case):
    ku.untouched(*[v for k, v in vars(r).items() if k.startswith(("out", "scores"))])
    assert np.array_equal(r.vt, ku.bits(case["vt"])), "a declined launcher wrote V^T"
    if hasattr(r, "kc"):
        assert np.array_equal(r.kc, ku.bits(case["kc"])) and np.array_equal(r.vc, ku.bits(case["vc"]))


def test_declined_head_ratios_write_nothing():
    case = du.decode_case(NINE, 2, CTX, 11)   # holds 4 + 2 heads: the overrides below never read past it
    for nh, nkv in ((1, 1), (3, 1), (3, 2), (4, 1)):
        for mode in (du.PLAIN, du.SCORES, du.EXACT, du.EXACT_SEQ):
            for B8 in (False, True):
                c = case if not B8 else du.decode_case(SHORT, 2, CTX, 11)
                if B8 and mode == du.EXACT_SEQ:
                    continue
                r = du.run_decode(c, mode, n_head=nh, n_kv_head=nkv, grid_splits=5, stream_blocks=2)
                assert r.declined and r.tag == "", (r.tag, r.msg)
                if mode != du.EXACT_SEQ:
                    assert "launch_decode_attention has no kernel" in r.msg, r.msg
                _untouched(r, c)
    chain = du.chain_case((5, 17), 3, 2, 96, du.CHAIN_SEED)
    r = du.run_decode(chain, du.CHAIN, n_head=5)   # 5 heads over 2 kv heads
    assert r.declined and "launch_decode_attention_exact has no kernel" in r.msg, r.msg
    _untouched(r, chain)


def test_one_launch_exact_declines():
    nine, eight = du.decode_case(NINE, 1, CTX, 11), du.decode_case(MID, 1, CTX, 11)
    for case, call in ((eight, dict(stream_blocks=2)), (nine, dict(stream_blocks=2, fx_seq=0)), (nine, dict(stream_blocks=0)),
                       (du.decode_case(NINE, 1, 4160, 11), dict(stream_blocks=2))):
        r = du.run_decode(case, du.EXACT_SEQ, grid_splits=5, **call)
        assert r.declined and r.tag == "", (r.tag, r.msg)
        _untouched(r, case)
    r = du.run_decode(du.decode_case(NINE, 1, 4096, 11), du.EXACT_SEQ, grid_splits=5, stream_blocks=2)   # exactly 32 KiB: taken
    assert not r.declined and r.tag == "decode_seq<1>"


def test_arguments_rejected_before_any_launch():
    case = du.decode_case(MID, 1, CTX, 11)
    E = du.au.QASR_ERR_ARG
    assert du.run_decode(case, du.PLAIN, grid_splits=4, expect_rc=E) is None            # 4 * 64 = 256 does not exceed pos 256
    assert du.run_decode(case, du.PLAIN, grid_splits=257, spl1=64, expect_rc=E) is None  # more splits than part holds
    assert du.run_decode(case, du.PLAIN, grid_splits=5, max_ctx=256, expect_rc=E) is None   # pos 256 outside the cache
    assert du.run_decode(case, du.SCORES, grid_splits=5, repeat=2, expect_rc=E) is None
    r = du.run_decode(case, du.PLAIN, grid_splits=512, spl1=128)   # 256 128-key splits: exactly what part holds
    assert not r.declined and r.tag == "decode_split<128>"
