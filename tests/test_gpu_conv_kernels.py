"""The audio encoder's conv subsampler against references of its own.

launch_conv1 and launch_gemm in the modes AM_CONV2 / AM_CONV3 -- the implicit im2col as gemm_kernel, glds_mainloop and
the 8-phase tile each write it -- are called through the test-only entry qasr_kt_conv (csrc/kernel_harness.hip) on
chunk tables the tests fill.  References, input families and comparators: tests/conv_util.py (geometry stated as
nine strided slices of a zero-padded NCHW image, none of it measured); their sharpness: tests/test_kernel_util_host.py.

Every case asserts the kernel tag, the buffer state (guard rows keep the sentinel, every in-range element written,
no NaN) and the values.  The input sits between guard rows of NaN on both sides and the weights' padding columns
are NaN wherever the 8-phase tile (whose contract is zeros there) is not expected, so a tap that should be padding
shows as NaN at the first and last chunk and as a wrong exact value everywhere else: conv1 is held bit for bit to
its stated arithmetic, conv2 / conv3 bit for bit on lattice inputs whose fp32 sums are exact in any order, and
within the dense bound on normal inputs (one case a tile family).  Chunk lists mix lengths, so tiles straddle
chunks and the chunk search meets unequal ones.  The worst error / bound per tile, the widest GELU candidate set
and the wall time go to the parity record ("conv_reference_tests").
"""
import time

import numpy as np
import pytest

import conv_util as cu
import kernel_util as ku

pytestmark = pytest.mark.gpu

WORST, WIDEST = {}, [0]


@pytest.fixture(scope="module", autouse=True)
def _record(gpu, parity):
    t0 = time.time()
    yield
    parity("conv_reference_tests", wall_s=time.time() - t0, widest_gelu_set=WIDEST[0],
           **{f"{k}_worst_over_bound": v for k, v in sorted(WORST.items())})


def ran(r, tag, rows, Cc, what):
    assert not r.declined, r.msg
    assert r.tag == tag, (what, r.tag)
    return ku.in_range(r.out, rows, Cc, what)


def check_normal(out, table, ref, bound, tile, what):
    """set membership within the bound is the assertion; the error over the bound is recorded"""
    WIDEST[0] = max(WIDEST[0], ku.check_gelu(out, table, ref, bound, what))
    WORST[tile] = max(WORST.get(tile, 0.0), cu.gelu_error_over_bound(out, table, ref, bound))


# ======================================================================= conv1
@pytest.mark.parametrize("Cc", [96, 480, 512])
def test_conv1(Cc):
    """12, 60 and all 64 lanes active.  One call: a clip of chunks 100 / 100 / 57 (the left tap of chunks 2 and 3 is
    padding though frame 99 of the chunk before lies there; the right tap of an odd length), clips of 1 and 2 frames
    (W1 = 1: a partly filled last wave, chunks that leave a grid sized by a wider neighbour early), an aligner chunk
    of 100 frames with 37 read (the mel's next bin lies past frame 37; all 50 output columns are written) and an
    unchunked chunk of 257 frames (W1 = 129, the max_w1 grid)"""
    rng = np.random.default_rng(Cc)
    chunks = cu.make_chunks(cu.CONV1_CLIPS)
    assert [c["L"] for c in chunks] == [100, 100, 57, 1, 2, 100, 257] and chunks[5]["Lv"] == 37 and chunks[6]["W1"] == 129
    mel = (rng.standard_normal(cu.mel_len(chunks)) * 0.7 + 0.3).astype(np.float32)
    w = ku.f16_normal(rng, (Cc, 1, 3, 3), 0.5)
    bias = rng.standard_normal(Cc).astype(np.float32)
    bias[[0, Cc - 1]] = 14.0, -14.0
    r = cu.run_conv(1, Cc, chunks, w.reshape(Cc, 9), bias, mel=mel)
    out = ran(r, "conv1<7>", cu.total_rows(1, chunks), Cc, f"conv1 C {Cc}")
    cu.check_exact(out, cu.conv1_reference(chunks, mel, w, bias, r.gelu_out), f"conv1 C {Cc}")


# ================================================================ conv2 / conv3
@pytest.mark.parametrize("case", cu.CASES, ids=cu.case_id)
def test_conv_gemm(case):
    layer, Cc, lengths, tag, twin, normal = case
    chunks = cu.make_chunks(lengths)
    rows = cu.total_rows(layer, chunks)
    rng = cu.case_rng(case)
    pad = 0.0 if tag == "gemm8p" else np.nan
    what = cu.case_id(case)
    # lattice inputs: exact, so one wrong tap anywhere is one wrong output
    act, w, bias = cu.lattice_inputs(rng, layer, Cc, chunks)
    cu.lattice_exact(act, w, bias)
    r = cu.run_conv(layer, Cc, chunks, cu.pack_weights(w, pad), bias, act=act)
    out = ran(r, tag, rows, Cc, what)
    cu.check_exact(out, cu.lattice_expect(layer, chunks, act, w, bias, r.gelu_out), what + " lattice")
    if twin:   # the register-staged tile: never reads the padding columns, the same bits
        r2 = cu.run_conv(layer, Cc, chunks, cu.pack_weights(w, np.nan), bias, act=act, regs_staged=1)
        assert np.array_equal(ran(r2, twin, rows, Cc, what + " regs_staged"), out), f"{what}: regs_staged differs"
    if normal:
        act, w, bias = cu.normal_inputs(rng, layer, Cc, chunks)
        ref, bound = cu.normal_expect(layer, chunks, act, w, bias)
        r = cu.run_conv(layer, Cc, chunks, cu.pack_weights(w, pad), bias, act=act)
        check_normal(ran(r, tag, rows, Cc, what), r.gelu_out, ref, bound, f"conv{layer}_{tag}", what + " normal")
        if twin:
            r2 = cu.run_conv(layer, Cc, chunks, cu.pack_weights(w, np.nan), bias, act=act, regs_staged=1)
            out2 = ran(r2, twin, rows, Cc, what + " regs_staged")
            assert np.array_equal(out2, ku.in_range(r.out, rows, Cc)), f"{what}: regs_staged differs on normal inputs"
            check_normal(out2, r2.gelu_out, ref, bound, f"conv{layer}_{twin}", what + " normal regs_staged")


def test_conv3_row_order_is_frame_major():
    """the (chunk, ow, oh) order of act3, stated without the reference's map: output frame ow of a chunk is the 16
    consecutive rows row3 + 16 ow .. + 15, one per image row"""
    case = cu.CASES[7]
    layer, Cc, lengths, tag = case[:4]
    chunks = cu.make_chunks(lengths)
    act, w, bias = cu.lattice_inputs(cu.case_rng(case), layer, Cc, chunks)
    r = cu.run_conv(layer, Cc, chunks, cu.pack_weights(w, np.nan), bias, act=act)
    out = ran(r, tag, cu.total_rows(3, chunks), Cc, "conv3 row order")
    a64, w64 = act.astype(np.float64), w.astype(np.float64)
    for ch in chunks:
        y, _ = cu.conv_ref(cu.from_rows(2, cu.chunk_rows(2, ch, a64), ch), w64)      # [C][16][W3]
        want = cu.gelu_bits((y + bias[:, None, None].astype(np.float64)).astype(np.float32), r.gelu_out)
        for ow in range(ch["W3"]):
            for oh in range(16):
                assert np.array_equal(out[ch["row3"] + 16 * ow + oh], want[:, oh, ow]), (ch["row3"], ow, oh)


# ================================================================ chained
def test_conv1_conv2_conv3_chained():
    """two ragged clips at C = 96 through all three layers on the device's own outputs: each stage against its
    reference computed from the device output of the stage before, so the three row tables agree with one another"""
    Cc = 96
    rng = np.random.default_rng(96)
    chunks = cu.make_chunks((257, 163))
    mel = (rng.standard_normal(cu.mel_len(chunks)) * 0.7 + 0.3).astype(np.float32)
    w1 = ku.f16_normal(rng, (Cc, 1, 3, 3), 0.5)
    b1 = rng.standard_normal(Cc).astype(np.float32)
    r1 = cu.run_conv(1, Cc, chunks, w1.reshape(Cc, 9), b1, mel=mel)
    act = ran(r1, "conv1<7>", cu.total_rows(1, chunks), Cc, "chain conv1")
    cu.check_exact(act, cu.conv1_reference(chunks, mel, w1, b1, r1.gelu_out), "chain conv1")
    for layer in (2, 3):
        w = ku.f16_normal(rng, (Cc, Cc, 3, 3), (9 * Cc) ** -0.5 * 2)
        b = rng.standard_normal(Cc).astype(np.float32)
        r = cu.run_conv(layer, Cc, chunks, cu.pack_weights(w, np.nan), b, act=np.ascontiguousarray(act))
        nxt = ran(r, "gemm<64,96,3>", cu.total_rows(layer, chunks), Cc, f"chain conv{layer}")
        ref, bound = cu.normal_expect(layer, chunks, np.ascontiguousarray(act), w, b)
        check_normal(nxt, r.gelu_out, ref, bound, f"chain_conv{layer}", f"chain conv{layer}")
        act = nxt


# ================================================================ declines
@pytest.mark.parametrize("layer", [2, 3])
@pytest.mark.parametrize("Cc", [32, 160, 224])
def test_conv_gemm_declines_widths_no_tile_covers(layer, Cc):
    """below 2048 rows no tile family covers all N columns of these widths: declined, nothing written"""
    chunks = cu.make_chunks((7, 57))
    act, w, bias = cu.lattice_inputs(np.random.default_rng(Cc), layer, Cc, chunks)
    r = cu.run_conv(layer, Cc, chunks, cu.pack_weights(w, np.nan), bias, act=act)
    assert r.declined and "no kernel for shape" in r.msg, (r.tag, r.msg)
    ku.untouched(r.out)


def test_conv1_declines_more_than_512_channels():
    Cc = 576
    rng = np.random.default_rng(Cc)
    chunks = cu.make_chunks((7, 57))
    mel = rng.standard_normal(cu.mel_len(chunks)).astype(np.float32)
    r = cu.run_conv(1, Cc, chunks, ku.f16_normal(rng, (Cc, 9), 0.5), rng.standard_normal(Cc).astype(np.float32), mel=mel)
    assert r.declined and "launch_conv1" in r.msg, (r.tag, r.msg)
    ku.untouched(r.out)
