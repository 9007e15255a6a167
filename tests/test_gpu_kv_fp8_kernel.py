"""The FP8 shadow KV cache's two kernels (csrc/kv_fp8.hip) through their test-only entries.

Conversion: bit for bit against the rule as torch states it on the CPU (clamp, then .to(float8_e4m3fn)).
Attention: against float64 softmax(q K^T scale) V over the dequantised shadow as the launch left it, under the bound
tests/decode_attn_util.py derives for the fa_exact_decode = 0 per-sequence kernel (the operands are exact fp16 values;
its 64-key chunk counts bound this kernel's 128-key ones from above), on decode_attn_util's poisoned cases.
"""
import numpy as np
import pytest

import decode_attn_util as du
import kernel_util as ku
import kv_fp8_util as k8u
from kernel_util import GUARD

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ conversion
L, SLOTS, H, CTX = 2, 3, 2, 40
RANGES = {"empty": (0, 0), "one": (0, 1), "ragged": (5, 21), "all": (0, CTX)}


def values(s):
    """fp16 inputs x whose x 2^s are: every E4M3 code, every midpoint of adjacent codes (the smallest subnormal 2^-9
    and half of it, the tie with zero, among them), +-0; then x itself +-448, +-449, +-65504 and 300 seeded normals"""
    codes = np.array([b for b in range(256) if b & 0x7f != 0x7f], np.uint8)
    pos = np.sort(k8u.dequant(codes[codes < 0x80], 0).astype(np.float64))
    mids = (pos[:-1] + pos[1:]) / 2
    y = np.concatenate([pos, -pos, mids, -mids]) * 2.0 ** -s
    x = np.concatenate([y, [448, -448, 449, -449, 65504, -65504], np.random.default_rng(8).standard_normal(300) * 3])
    h = x.astype(np.float16)
    assert np.array_equal(h[:len(y)].astype(np.float64), y), "a code or a tie is no fp16 value at this exponent"
    return h


@pytest.mark.parametrize("name", list(RANGES))
@pytest.mark.parametrize("s", [-3, 0, 4])
def test_convert_equals_the_rule(gpu, s, name):
    shape = (L, SLOTS + 1, H, CTX, 128)
    n = int(np.prod(shape))
    v = values(s)
    kc = v[np.arange(n) % len(v)].reshape(shape).copy()
    vc = v[(np.arange(n) * 7 + 3) % len(v)].reshape(shape).copy()
    rng = np.random.default_rng(5)
    k8, v8 = rng.integers(0, 256, shape, np.uint8), rng.integers(0, 256, shape, np.uint8)
    for a in (kc.view(np.uint16), vc.view(np.uint16), k8, v8):
        a[:, SLOTS:] = np.iinfo(a.dtype).max   # the guard slot
    f, t = RANGES[name]
    gk, gv = k8u.run_convert(kc.view(np.uint16), vc.view(np.uint16), k8, v8, [0, 2], [f, f], [t, t], s, 1)
    wk, wv = k8.copy(), v8.copy()
    for slot in (0, 2):
        wk[:, slot, :, f:t] = k8u.rule(kc[:, slot, :, f:t], s)
        wv[:, slot, :, f:t] = k8u.rule(vc[:, slot, :, f:t], s)
    assert np.array_equal(gk, wk), ("k8", np.argwhere(gk != wk)[:4])
    assert np.array_equal(gv, wv), ("v8", np.argwhere(gv != wv)[:4])


# ------------------------------------------------------------------- attention
POS9 = (300, 0, 127, 128, 129, 1, 64, 65, 16)
POS12 = (128, 15, 300, 0, 63, 64, 1, 65, 127, 16, 129, 300)
NKV, ACTX = 2, 384


def shadows(case, s, beyond=None):
    """the rule of the case's fp16 caches (NaN above pos -> the NaN codes), guard slots 0xFF; beyond: that byte in every
    row above pos instead"""
    out = []
    for c in (case["kc"], case["vc"]):
        q = np.full((case["B"] + GUARD,) + c.shape[1:], 0xFF, np.uint8)
        q[:case["B"]] = k8u.rule(c, s)
        if beyond is not None:
            for b, p in enumerate(case["pos"]):
                q[b, :, p + 1:] = beyond
        out.append(q)
    return out


@pytest.mark.parametrize("pos,s,kind", [(POS9, 0, "f32"), (POS12, 3, "f16"), (POS9, -2, "q8")], ids=["b9_f32", "b12_f16", "b9_q8"])
def test_attention_against_float64_over_the_shadow(gpu, pos, s, kind):
    case = du.decode_case(pos, NKV, ACTX, 11)
    B, QD, gs = case["B"], case["n_head"] * 128, max(pos) // 64 + 1
    k8, v8 = shadows(case, s)
    r = k8u.run_attn(case, k8, v8, s, kind, repeat=2)   # (the harness requires both launches to leave equal caches)
    assert not r.declined and r.tag == "decode_seq_fp8<128>", (r.msg, r.tag)
    # the fp16 rows: decode_attn_seq_kernel<0>'s bits, everything else as given
    f16 = du.run_decode(case, du.PLAIN, "f32", grid_splits=gs, stream_blocks=2)
    assert f16.tag == "decode_seq<0>"
    for name in ("kc", "vc", "vt"):
        assert np.array_equal(getattr(r, name), getattr(f16, name)), name
    # the shadow: the rule of the new fp16 rows at pos, every other byte (guard slots too) unchanged
    bi = np.arange(B)
    for got, given, new16 in ((r.k8, k8, r.kc), (r.v8, v8, r.vc)):
        want = given.copy()
        want[bi, :, case["pos"]] = k8u.rule(new16.view(np.float16).reshape(case["kc"].shape)[bi, :, case["pos"]], s)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    # float64 attention over the dequantised shadow as the launch left it ('stale': row pos as the caches hold it)
    hat = dict(case, kc=k8u.dequant(r.k8[:B], s), vc=k8u.dequant(r.v8[:B], s))
    ref, bound = du.decode_reference(hat, 0, gs, defect="stale")
    what = f"decode_seq_fp8 pos {pos} s {s} {kind}"
    if kind == "q8":   # the same launch's fp32 output, quantised: bit for bit
        r32 = k8u.run_attn(case, k8, v8, s, "f32")
        q_ref, d_ref = ku.q8_quantize(ku.in_range(r32.out32, B, QD, what))
        ku.check_q8(ku.in_range(r.outq, B, QD, "outq"), ku.in_range(r.outd, B, QD // 32, "outd"), q_ref, d_ref, what=what)
        outs = [("outq", "outq_b"), ("outd", "outd_b")]
    else:
        name = "out32" if kind == "f32" else "out"
        worst = ku.check_values(ku.in_range(getattr(r, name), B, QD, what), ref, bound, fp16=kind == "f16", what=what)
        print(f"{what}: worst error / bound {worst:.3f}")
        outs = [(name, name + "_b")]
    for a, b in outs:
        assert np.array_equal(getattr(r, a).view(np.uint8), getattr(r, b).view(np.uint8)), f"{what}: the second launch differs"


def test_attention_ignores_keys_beyond_pos(gpu):
    """1000 in every fp16 key and value above pos (the code of 448 in the shadow): the output keeps its bits"""
    case = du.decode_case(POS9, NKV, ACTX, 11)
    kc, vc = case["kc"].copy(), case["vc"].copy()
    for b, p in enumerate(POS9):
        kc[b, :, p + 1:] = vc[b, :, p + 1:] = 1000
    base = k8u.run_attn(case, *shadows(case, 0), 0)
    loud = k8u.run_attn(dict(case, kc=kc, vc=vc), *shadows(case, 0, beyond=0x7e), 0)
    assert np.array_equal(base.out32.view(np.uint32), loud.out32.view(np.uint32))
