"""Shared by the norm / RoPE / attention kernel tests (tests/test_gpu_attn_kernels.py and the
sharpness cases of tests/test_kernel_util_host.py): ctypes bindings of qasr_kt_norm, qasr_kt_qkv_post,
qasr_kt_enc_attention and qasr_kt_prefill_attention (include/qasr_capi.h, csrc/kernel_harness.hip), seeded cases,
float64 references over the same rounded inputs, first-order bounds derived from the kernels' arithmetic (each
next to its function; none is measured), the numpy restatement of ggml's fp16 chain for the exact prefill
kernel, and the comparators.

Layouts (csrc/kernels.h): K / V cache [slot][kv head][max_ctx][128] fp16; V^T cache per (slot, kv head)
128 * vt_ctx(max_ctx) fp16 with element (key, d) at vt_index; rope [pos][64][2] = (cos, sin); encoder qkv
fp32 [rows][3 D] = q | k | v, head h at columns 64 h.  Outputs come back as their whole allocation, GUARD
sentinel rows on both sides; rows no segment / sequence owns keep the sentinel too.
"""
import ctypes as C
import functools

import numpy as np

import kernel_util as ku
from kernel_util import GUARD, U, ulp16

_P = C.c_void_p
_TAIL = [("declined", C.c_int32), ("msg", C.c_char * 256)]


def _i32(*names):
    return [(n, C.c_int32) for n in names]


def _ptr(*names):
    return [(n, _P) for n in names]


class NormCall(C.Structure):
    _fields_ = _i32("kind", "M", "D", "ldx", "xrows", "guard") + [("eps", C.c_float)] + _ptr(
        "x", "row_idx", "w", "b", "y", "y32", "yq", "yd") + _TAIL


class QkvPostCall(C.Structure):
    _fields_ = _i32("rows", "n_head", "n_kv_head", "max_ctx", "slots", "max_pos", "guard") + [("eps", C.c_float)] + _ptr(
        "qkv", "row_seq", "row_pos", "q_norm", "k_norm", "rope", "q_out", "q32", "k32", "kc", "vc", "vt") + _TAIL


class EncAttnCall(C.Structure):
    _fields_ = _i32("rows", "D", "H", "n_seg", "max_len", "f32_mfma", "guard") + _ptr(
        "qkv", "seg_start", "seg_len", "out", "out32") + _TAIL


class PrefillCall(C.Structure):
    _fields_ = _i32("exact", "rows", "n_head", "n_kv_head", "max_ctx", "slots", "n_seq", "max_len", "guard") + [
        ("scale", C.c_float)] + _ptr("q", "kc", "vc", "seq_row0", "seq_len", "seq_slot", "seq_pos0", "q32", "k32", "out", "out32") + _TAIL


LN, RMS, RMS_Q8 = range(3)
QASR_ERR_ARG = 1


def _call(name, c, keep, expect_rc=0):
    import qasr
    L = qasr.lib()
    fn = getattr(L, name)
    fn.argtypes = [C.c_int, C.POINTER(type(c))]
    fn.restype = C.c_int
    rc = fn(0, C.byref(c))
    del keep
    if expect_rc:
        assert rc == expect_rc, (rc, L.qasr_last_error())
        return rc
    ku._ok(L, rc)
    return rc


class Out:
    def __init__(self, call, outs):
        self.declined = bool(call.declined)
        self.msg = call.msg.decode()
        self.__dict__.update(outs)


def _out(rows, ld, dtype):
    return np.zeros((rows + 2 * GUARD, ld), dtype)


def vt_ctx(max_ctx):
    return (max_ctx + 63) // 64 * 64 + 384


def vt_index(k, d):
    """kernels.h vt_index: 8-key blocks of [128 d][8 keys]"""
    return ((k >> 3) * 128 + d) * 8 + (k & 7)


KV_PAD_ROWS = 256   # kernels.h kKvPadRows: rows the harness appends (NaN) after the last cache region


# ==================================================================== norms
def run_norm(kind, x, M, D, *, w=None, b=None, eps=1e-5, row_idx=None, f32=False):
    """x fp32 [xrows][ldx]; returns Out with y / y32 (kinds LN, RMS) or yq + yd (RMS_Q8)"""
    c = NormCall(kind=kind, M=M, D=D, ldx=x.shape[1], xrows=x.shape[0], guard=GUARD, eps=eps)
    if kind == RMS_Q8:
        outs = dict(yq=_out(M, D, np.int8), yd=_out(M, max(D // 32, 1), np.float32))
    else:
        outs = dict(y32=_out(M, D, np.float32)) if f32 else dict(y=_out(M, D, np.uint16))
    keep = ku._set(c, [], x=x, w=w, b=b, row_idx=None if row_idx is None else np.asarray(row_idx, np.int32), **outs)
    _call("qasr_kt_norm", c, keep)
    return Out(c, outs)


def norm_rows(rng, M, D):
    """fp32 rows cycling through: unit normal, mean 50x the spread, constant (variance 0), all zero, magnitude 1e4"""
    x = rng.standard_normal((M, D))
    for r in range(M):
        kind = r % 5
        if kind == 1:
            x[r] += 50.0
        elif kind == 2:
            x[r] = 3.25
        elif kind == 3:
            x[r] = 0.0
        elif kind == 4:
            x[r] *= 1e4
    return x.astype(np.float32)


LN_ROUNDINGS = 10   # see layernorm_ref
RMS_ROUNDINGS = 8   # see rmsnorm_ref


def layernorm_ref(x, w, b, eps):
    """float64 LayerNorm of fp32 rows and its bound.  layernorm_kernel: mean = fl32(sum / D) (the double sum is
    exact to 2^-53), v = fl(x - mean), var = fl32(sum fl(v v) / D), scale = 1 / sqrtf(var + eps), t = fl(fl(v scale) w)
    + b.  Relative roundings on t: v 1, scale 6.5 (var: 2 from v, 1 the square, 1 the cast, 1 the add, halved by the
    root; root and divide 2 each at <= 1 ulp), the two multiplies 2 -> LN_ROUNDINGS = 10 (rounded up); the mean's own
    rounding shifts every v by <= U |mean|, i.e. the output by U |mean| scale |w| (its effect on var is second
    order); the add of b rounds once more, U |y|."""
    x = np.asarray(x, np.float64)
    mean = x.mean(1, keepdims=True)
    xc = x - mean
    scale = 1.0 / np.sqrt((xc * xc).mean(1, keepdims=True) + eps)
    wv = np.ones(x.shape[1]) if w is None else np.asarray(w, np.float64)
    t = xc * scale * wv
    y = t if b is None else t + np.asarray(b, np.float64)
    bound = LN_ROUNDINGS * U * np.abs(t) + U * np.abs(mean) * scale * np.abs(wv) + U * np.abs(y)
    return y, bound


def layernorm_one_pass(x, w, b, eps):
    """the defect: var = E[x^2] - mean^2 in fp32"""
    x = np.asarray(x, np.float32)
    mean = x.mean(1, keepdims=True, dtype=np.float32)
    var = (x * x).mean(1, keepdims=True, dtype=np.float32) - mean * mean
    t = (x - mean) / np.sqrt(np.maximum(var, 0) + np.float32(eps))
    if w is not None:
        t = t * w
    return (t if b is None else t + b).astype(np.float32)


def rmsnorm_ref(x, w, eps):
    """float64 RMSNorm and its bound.  rms_row: scale = 1 / sqrtf(fl32(sum fl(x x) / D) + eps): the squares, the
    cast and the add are 3 roundings halved by the root, root and divide 2 each -> 5.5; two multiplies -> 7.5, taken
    as RMS_ROUNDINGS = 8 relative roundings of the output."""
    x = np.asarray(x, np.float64)
    y = x / np.sqrt((x * x).mean(1, keepdims=True) + eps) * np.asarray(w, np.float64)
    return y, RMS_ROUNDINGS * U * np.abs(y)


def check_rms_bits(y_bits, x, w, eps):
    """fp16 RMSNorm output against ku.rms_prologue: bit for bit outside the near-tie mask, the neighbouring fp16
    value at most inside it.  Returns the share of near-tie elements"""
    h, v, tie = ku.rms_prologue(x, w, eps)
    got = np.ascontiguousarray(y_bits).view(np.float16)
    diff = ku._f16_index(got) - ku._f16_index(h)
    bad = (diff != 0) & ~tie | (np.abs(diff) > 1)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"rmsnorm: {int(bad.sum())} elements differ from the float32 restatement, first {i}: "
                             f"got {got[i]!r} want {h[i]!r} (near a tie: {bool(tie[i])})")
    return float(tie.mean())


# ================================================================= qkv_post
@functools.lru_cache(maxsize=None)
def qkv_case(n_head, n_kv_head, rows):
    """seeded launch_qkv_post inputs: rows scattered over slots {0, 2} of 3 and positions {0, 1, 7, 8, 63, 64, 71}
    (both ends of an 8-key V^T block and of the 64-key granule, the last position of max_ctx = 72)"""
    rng = np.random.default_rng([n_head, n_kv_head, rows, 41])
    max_ctx, slots, max_pos = 72, 3, 80
    cells = [(s, p) for p in (71, 7, 64, 0, 8, 63, 1) for s in (2, 0)]
    pick = [cells[i] for i in rng.permutation(len(cells))[:rows]]
    if rows >= 3:   # positions 7 and 8 of one slot: neighbours across a V^T block seam
        pick[0], pick[1] = (2, 7), (2, 8)
    W = (n_head + 2 * n_kv_head) * 128
    qkv = (rng.standard_normal((rows, W)) * np.repeat(2.0 ** rng.integers(-3, 4, W // 128), 128)).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, (max_pos, 64))
    rope = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)
    case = dict(n_head=n_head, n_kv_head=n_kv_head, rows=rows, max_ctx=max_ctx, slots=slots, max_pos=max_pos, eps=1e-6,
                qkv=qkv, row_seq=np.array([c[0] for c in pick], np.int32), row_pos=np.array([c[1] for c in pick], np.int32),
                q_norm=(1 + 0.2 * rng.standard_normal(128)).astype(np.float32),
                k_norm=(1 + 0.2 * rng.standard_normal(128)).astype(np.float32), rope=rope)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def run_qkv_post(case, f32):
    c = QkvPostCall(guard=GUARD, **{k: case[k] for k in ("rows", "n_head", "n_kv_head", "max_ctx", "slots", "max_pos", "eps")})
    R, QD, KD = case["rows"], case["n_head"] * 128, case["n_kv_head"] * 128
    cache = case["slots"] * case["n_kv_head"] * case["max_ctx"] * 128
    outs = dict(q_out=_out(R, QD, np.uint16), kc=np.full(cache, 0xFFFF, np.uint16), vc=np.full(cache, 0xFFFF, np.uint16),
                vt=np.full(case["slots"] * case["n_kv_head"] * 128 * vt_ctx(case["max_ctx"]), 0xFFFF, np.uint16))
    if f32:
        outs.update(q32=_out(R, QD, np.float32), k32=_out(R, KD, np.float32))
    keep = ku._set(c, [], **{k: case[k] for k in ("qkv", "row_seq", "row_pos", "q_norm", "k_norm", "rope")}, **outs)
    _call("qasr_kt_qkv_post", c, keep)
    return Out(c, outs)


def qkv_post_ref(case, pair_adjacent=False):
    """float64 q / k rows after RMSNorm and the NEOX rotation, with bounds.  The norm carries RMS_ROUNDINGS relative
    roundings (rmsnorm_ref; the same arithmetic on 128 values); the rotation y0 = fl(fl(n0 c) - fl(n1 s)) with the
    table's fp32 (c, s) as exact inputs adds one rounding per product and one for the difference:
    (RMS_ROUNDINGS + 1) U (|n0 c| + |n1 s|) + U |y0|, likewise y1.  Returns (q, bq, k, bk) as [rows][heads * 128]
    and v as the exact fp16 rows (ggml_cpy f32 -> f16: one conversion, compared bit for bit).
    pair_adjacent: the defect -- element i rotated with i + 1 (GPT-J pairs) instead of i + 64"""
    nh, nkv, R = case["n_head"], case["n_kv_head"], case["rows"]
    x = case["qkv"].astype(np.float64).reshape(R, nh + 2 * nkv, 128)
    cs = case["rope"].astype(np.float64)[case["row_pos"]]   # [R][64][2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    res = []
    for heads, w in ((x[:, :nh], case["q_norm"]), (x[:, nh:nh + nkv], case["k_norm"])):
        n = heads / np.sqrt((heads * heads).mean(-1, keepdims=True) + case["eps"]) * w.astype(np.float64)
        n0, n1 = (n[..., 0::2], n[..., 1::2]) if pair_adjacent else (n[..., :64], n[..., 64:])
        y0, y1 = n0 * c - n1 * s, n0 * s + n1 * c
        b0 = (RMS_ROUNDINGS + 1) * U * (np.abs(n0 * c) + np.abs(n1 * s)) + U * np.abs(y0)
        b1 = (RMS_ROUNDINGS + 1) * U * (np.abs(n0 * s) + np.abs(n1 * c)) + U * np.abs(y1)
        y, b = np.empty_like(n), np.empty_like(n)
        if pair_adjacent:
            y[..., 0::2], y[..., 1::2], b[..., 0::2], b[..., 1::2] = y0, y1, b0, b1
        else:
            y[..., :64], y[..., 64:], b[..., :64], b[..., 64:] = y0, y1, b0, b1
        res += [y.reshape(R, -1), b.reshape(R, -1)]
    v = case["qkv"].reshape(R, nh + 2 * nkv, 128)[:, nh + nkv:].astype(np.float16)
    return res[0], res[1], res[2], res[3], v


def check_cache_rows(cache, case, ref, bound, what):
    """kc / vc [slot][kv head][max_ctx][128]: the rows (row_seq, row_pos) hold ref (bound None: the fp16 bits of
    ref), every other element the sentinel.  Returns the worst error / bound"""
    nkv, mc = case["n_kv_head"], case["max_ctx"]
    c = cache.reshape(case["slots"], nkv, mc, 128)
    seq, pos = case["row_seq"], case["row_pos"]
    rest = np.ones(c.shape[:3], bool)
    rest[seq, :, pos] = False
    assert (c[rest] == 0xFFFF).all(), f"{what}: a cache row outside (row_seq, row_pos) was written"
    got = c[seq, :, pos]   # [R][nkv][128]
    if bound is None:
        assert np.array_equal(got, ref.view(np.uint16)), f"{what}: rows differ from fp16(v)"
        return 0.0
    assert not (got == 0xFFFF).all(-1).any(), f"{what}: a row was never written"
    return ku.check_values(got.reshape(len(seq), -1), ref, bound, fp16=True, what=what)


def vt_expected(case, v):
    """the whole V^T cache after the launch: v's elements at vt_index, the sentinel elsewhere"""
    nkv, n = case["n_kv_head"], 128 * vt_ctx(case["max_ctx"])
    want = np.full((case["slots"], nkv, n), 0xFFFF, np.uint16)
    d = np.arange(128)
    for r in range(case["rows"]):
        want[case["row_seq"][r], :, vt_index(int(case["row_pos"][r]), d)] = v[r].view(np.uint16).T
    return want.reshape(-1)


def check_vt(vt, want):
    if not np.array_equal(vt, want):
        i = int(np.argwhere(vt != want)[0, 0])
        raise AssertionError(f"vt: {int((vt != want).sum())} elements differ, first at {i}: got {int(vt[i]):#06x} want {int(want[i]):#06x}")


# ============================================================ softmax bound
def softmax_terms(s, eps, v, mask, *, tiles, adds, p_rel=0.0, p_abs=0.0, v_err=None):
    """float64 softmax(s) v over the visible keys and the first-order bound of a flash-style fp32 kernel whose
    scores err by at most eps (per query and key).
      * A score error delta_k multiplies p_k by e^delta_k =: 1 + eta_k; the output moves by
        sum_k w_k eta_k (v_k - O) / (1 + sum w eta), bounded by sum_k w_k |eta_k| (|v_k| + |O|) / (1 - max eta):
        "propagated through softmax to sum p |v| / sum p".
      * Into delta_k also go the kernel's own roundings of p_k: the fp32 subtraction s - m (U |s - m| in the
        exponent; over the running-maximum rescales the |m' - m| telescope to the same total), expf at <= 1 ulp (2 U),
        and per 64-key tile one more expf, subtraction and multiply for the rescale (3 U each, tiles + 1 with the final
        merge).
      * sum p and sum p v: each term passes at most `adds` fp32 additions: (adds + 2) U (sum w |v| + |O|).
      * 1 / l and the final multiply: 3 U |O|.
      * p_rel / p_abs: a kernel that feeds P to the MFMA as fp16 hi + lo parts represents p to p_rel relatively, or
        p_abs absolutely where lo is subnormal (p is relative to a running maximum, so sum p >= 1 and p_abs enters as
        p_abs sum |v| / sum p); v_err: likewise per element of V ([keys][dv]).
    s, eps, mask [nq][nk]; v [nk][dv].  Returns (O, bound) [nq][dv]."""
    s = np.where(mask, s, -np.inf)
    m = s.max(1, keepdims=True)
    p = np.exp(s - m)
    D = p.sum(1, keepdims=True)
    w = p / D
    av = np.abs(v)
    O, A = w @ v, w @ av
    e = np.where(mask, eps + U * np.where(mask, m - s, 0.0) + (2 + 3 * (tiles + 1)) * U, 0.0)
    eta = np.expm1(e)
    we = w * eta
    b = (we @ av + np.abs(O) * we.sum(1, keepdims=True)) / (1.0 - eta.max(1, keepdims=True))
    b += (adds + 2) * U * (A + np.abs(O)) + 3 * U * np.abs(O)
    b += p_rel * A + p_abs * (mask.astype(np.float64) @ av) / D
    if v_err is not None:
        b += w @ v_err
    return O, b


def _f16_split_err(x, floor=2.0 ** -25):
    """|x - (hi + lo)| for hi = fp16(x), lo = fp16(x - hi): lo <= 2^-11 |x| is itself rounded to 11 bits,
    2^-22 |x|, or to half the subnormal spacing 2^-25 where lo is below 2^-14"""
    return np.maximum(2.0 ** -22 * np.abs(x), floor)


# ======================================================== encoder attention
ENC_N = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193)


@functools.lru_cache(maxsize=None)
def enc_case(H, scale_log2=0, spike=False, lens=ENC_N):
    """one launch of ragged segments, a NaN row between neighbours (and after the last); spike: in every segment
    one key's score sits 40 above the rest for every query"""
    rng = np.random.default_rng([H, scale_log2 + 16, int(spike), len(lens)])
    D = 64 * H
    order = [lens[i] for i in rng.permutation(len(lens))]
    start, r = [], 0
    for n in order:
        start.append(r)
        r += n + 1
    qkv = np.full((r, 3 * D), np.nan, np.float32)
    for s0, n in zip(start, order):
        x = rng.standard_normal((n, 3 * D))
        if spike:   # q[:, 0] = 8 and one key with k[0] = 40: 0.125 * 8 * 40 = 40 on top of the N(0, 1) scores
            j = n // 2
            for h in range(H):
                x[:, 64 * h] = 8.0
                x[:, D + 64 * h] = 0.0
                x[j, D + 64 * h] = 40.0
        qkv[s0:s0 + n] = (x * 2.0 ** scale_log2).astype(np.float32)
    case = dict(H=H, D=D, rows=r, qkv=qkv, seg_start=np.array(start, np.int32), seg_len=np.array(order, np.int32),
                max_len=max(order))
    qkv.setflags(write=False)
    return case


def run_enc_attention(case, f32_mfma, f32_out, expect_rc=0, **over):
    a = dict(case, **over)
    c = EncAttnCall(rows=a["rows"], D=a["D"], H=a["H"], n_seg=len(a["seg_len"]), max_len=a["max_len"], f32_mfma=int(f32_mfma),
                    guard=GUARD)
    outs = dict(out32=_out(a["rows"], a["D"], np.float32)) if f32_out else dict(out=_out(a["rows"], a["D"], np.uint16))
    keep = ku._set(c, [], qkv=a["qkv"], seg_start=a["seg_start"], seg_len=a["seg_len"], **outs)
    if _call("qasr_kt_enc_attention", c, keep, expect_rc):
        return None
    return Out(c, outs)


def enc_reference(case, f32_mfma, keys_of=None):
    """float64 attention of every segment and head; returns (ref, bound, valid) over [rows][D] / [rows].
    Scores: 64 fp32 products and additions and the multiply by the scale: (d + 2) U scale sum |q k| (dense_bound's
    count).  The split-fp16 form (attention.hip, enc_attn_h_kernel) adds the rounding of q * qscale and of the
    constant qscale (2 U) and what its three MFMAs leave out of (qh + ql)(kh + kl): ql kl <= 2^-22 |q k| and the
    parts of q and k below hi + lo (_f16_split_err; for q the split is of q * qscale); P is split from p * 2^12
    (relative 3 * 2^-22 with the lo . lo term, absolute 2^-25 / 2^12 = 2^-37) and V by _f16_split_err.
    keys_of(i) -> the absolute rows segment i attends (default its own): the sharpness cases plant defects there"""
    H, D, qkv = case["H"], case["D"], case["qkv"].astype(np.float64)
    ref, bound = np.zeros((case["rows"], D)), np.zeros((case["rows"], D))
    valid = np.zeros(case["rows"], bool)
    scale, qscale = 0.125, 0.125 * 1.4426950408889634
    for i, (r0, n) in enumerate(zip(case["seg_start"], case["seg_len"])):
        kr = np.arange(r0, r0 + n) if keys_of is None else np.asarray(keys_of(i))
        valid[r0:r0 + n] = True
        tiles = (len(kr) + 63) // 64
        for h in range(H):
            q, k, v = qkv[r0:r0 + n, 64 * h:64 * h + 64], qkv[kr, D + 64 * h:D + 64 * h + 64], qkv[kr, 2 * D + 64 * h:2 * D + 64 * h + 64]
            s, mag = scale * (q @ k.T), scale * (np.abs(q) @ np.abs(k).T)
            eps = (64 + 2) * U * mag
            kw = {}
            if not f32_mfma:
                eps = eps + 2 * U * mag + scale * (np.abs(q) @ _f16_split_err(k).T + _f16_split_err(q, 2.0 ** -25 / qscale) @ np.abs(k).T) \
                    + 2.0 ** -22 * mag
                kw = dict(p_rel=3 * 2.0 ** -22, p_abs=2.0 ** -37, v_err=_f16_split_err(v))
            o, b = softmax_terms(s, eps, v, np.ones(s.shape, bool), tiles=tiles, adds=len(kr), **kw)
            ref[r0:r0 + n, 64 * h:64 * h + 64], bound[r0:r0 + n, 64 * h:64 * h + 64] = o, b
    return ref, bound, valid


def check_rows(buf, valid, ref, bound, fp16, what):
    """an output [rows + 2 GUARD][ld] whose rows outside `valid` keep the sentinel: guards and those rows untouched,
    every valid element written and no NaN, values within the bound.  Returns the worst error / bound"""
    raw = buf.view(ku._SENT[buf.dtype.itemsize])
    full = np.iinfo(raw.dtype).max
    assert raw.shape[0] == len(valid) + 2 * GUARD, (what, raw.shape)
    assert (raw[:GUARD] == full).all() and (raw[GUARD + len(valid):] == full).all(), f"{what}: guard rows overwritten"
    body = raw[GUARD:GUARD + len(valid)]
    assert (body[~valid] == full).all(), f"{what}: a row outside every segment was written"
    assert not (body[valid] == full).any(), f"{what}: elements of a segment's rows never written"
    vals = buf[GUARD:GUARD + len(valid)][valid]
    return ku.check_values(vals, ref[valid], bound[valid], fp16=fp16, what=what)


# ======================================================== prefill attention
PREFILL_L = (1, 15, 16, 17, 31, 32, 33, 64, 65, 129, 161)
PREFILL_CACHED = ((1, 1), (63, 5), (64, 33), (100, 33), (127, 17))
MAX_CTX = 176
EXACT_SEED, EXACT_SEED_CACHED = 3, 5   # picked on the CPU (near-tie share under 5 %), as GEMV_SEED was


@functools.lru_cache(maxsize=None)
def prefill_case(n_head, n_kv_head, seqs, seed, lattice, with32=False):
    """one launch of sequences (pos0, L): permuted cache slots (one slot unused), gaps of NaN rows between the
    sequences' q rows, every cache row at or past a sequence's key count NaN.  lattice: q and k are multiples of
    1 / 8 in [-2, 2], so every fp32 partial sum of a score's 128 products is exact in any order.  with32: fp32
    q32 / k32 rows (normal; key k of a sequence at row seq_row0 + k, pos0 = 0) from which the scores come instead"""
    rng = np.random.default_rng([n_head, n_kv_head, len(seqs), seed])
    QD, KD = n_head * 128, n_kv_head * 128
    slots = len(seqs) + 1
    slot = rng.permutation(slots)[:len(seqs)].astype(np.int32)
    row0, r = [], 0
    for i, (p0, L) in enumerate(seqs):
        r += i % 3   # gaps of 0, 1, 2 rows
        row0.append(r)
        r += L
    rows = r + 1
    q = np.full((rows, QD), np.nan, np.float16)
    kc = np.full((slots, n_kv_head, MAX_CTX, 128), np.nan, np.float16)
    vc = kc.copy()
    q32 = np.full((rows, QD), np.nan, np.float32) if with32 else None
    k32 = np.full((rows, KD), np.nan, np.float32) if with32 else None

    def draw(shape):
        return (rng.integers(-16, 17, shape) / 8.0 if lattice else rng.standard_normal(shape)).astype(np.float16)
    for (p0, L), s, r0 in zip(seqs, slot, row0):
        q[r0:r0 + L] = draw((L, QD))
        kc[s, :, :p0 + L] = draw((n_kv_head, p0 + L, 128))
        vc[s, :, :p0 + L] = rng.standard_normal((n_kv_head, p0 + L, 128)).astype(np.float16)
        if with32:
            assert p0 == 0
            q32[r0:r0 + L] = rng.standard_normal((L, QD)).astype(np.float32)
            k32[r0:r0 + L] = rng.standard_normal((L, KD)).astype(np.float32)
    case = dict(n_head=n_head, n_kv_head=n_kv_head, rows=rows, slots=slots, max_ctx=MAX_CTX, q=q, kc=kc, vc=vc, q32=q32, k32=k32,
                seq_row0=np.array(row0, np.int32), seq_len=np.array([L for _, L in seqs], np.int32), seq_slot=slot,
                seq_pos0=np.array([p for p, _ in seqs], np.int32) if any(p for p, _ in seqs) else None,
                max_len=max(L for _, L in seqs), scale=np.float32(128 ** -0.5))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def run_prefill(case, exact, f32_out, **over):
    a = dict(case, **over)
    c = PrefillCall(exact=int(exact), rows=a["rows"], n_head=a["n_head"], n_kv_head=a["n_kv_head"], max_ctx=a["max_ctx"],
                    slots=a["slots"], n_seq=len(a["seq_len"]), max_len=a["max_len"], guard=GUARD, scale=float(a["scale"]))
    QD = a["n_head"] * 128
    outs = dict(out32=_out(a["rows"], QD, np.float32)) if f32_out else dict(out=_out(a["rows"], QD, np.uint16))
    keep = ku._set(c, [], q=ku.bits(a["q"]), kc=ku.bits(a["kc"]), vc=ku.bits(a["vc"]), seq_row0=a["seq_row0"], seq_len=a["seq_len"],
                   seq_slot=a["seq_slot"], seq_pos0=a["seq_pos0"], q32=a["q32"] if exact else None, k32=a["k32"] if exact else None,
                   **outs)
    _call("qasr_kt_prefill_attention", c, keep)
    return Out(c, outs)


def _seqs(case):
    p0 = case["seq_pos0"] if case["seq_pos0"] is not None else np.zeros(len(case["seq_len"]), np.int32)
    return [(int(case["seq_row0"][i]), int(case["seq_len"][i]), int(case["seq_slot"][i]), int(p0[i])) for i in range(len(p0))]


def prefill_valid(case):
    valid = np.zeros(case["rows"], bool)
    for r0, L, _, _ in _seqs(case):
        valid[r0:r0 + L] = True
    return valid


def _causal(L, P0, limit_shift, drop_key):
    KL = P0 + L
    lim = np.minimum(P0 + np.arange(L) + limit_shift, KL - 1)
    mask = np.arange(KL)[None, :] <= lim[:, None]
    if drop_key is not None and drop_key < KL:
        mask[:, drop_key] = False
        mask[np.arange(L), 0] |= ~mask.any(1)   # (a query whose only key was dropped keeps key 0)
    return mask


def prefill_reference(case, fp32_scores=False, limit_shift=0, drop_key=None):
    """float64 causal attention (query t of a sequence sees keys 0 .. pos0 + t) with bounds, [rows][n_head * 128].
    fp16 q . k products are exact in fp32; 128 additions and the scale: (d + 2) U scale sum |q k|
    (prefill_attn_kernel).  P enters the f16 MFMA as fp16 hi + lo: relative 2^-22, absolute 2^-25 where lo is
    subnormal (p < 2^-3); V is fp16 (exact); hi and lo are two accumulations a key: adds = 2 keys.
    fp32_scores: the exact kernel with q32 / k32 -- fp32 products (same count) and, in place of the P split, the
    chain's term: every key rounds the fp16 accumulator once (half an ulp, <= 2^-11 of the largest prefix
    accumulator A, relative to the running maximum) and every new maximum once more: (keys + maxima) 2^-11 A / S,
    first order, with A inflated by that sum itself.
    limit_shift / drop_key: the planted defects (a causal limit off by one; one key position never attended)"""
    nh, g = case["n_head"], case["n_head"] // case["n_kv_head"]
    ref, bound = np.zeros((case["rows"], nh * 128)), np.zeros((case["rows"], nh * 128))
    scale = float(case["scale"])
    for r0, L, slot, P0 in _seqs(case):
        KL = P0 + L
        mask = _causal(L, P0, limit_shift, drop_key)
        for h in range(nh):
            if fp32_scores:
                q, k = case["q32"][r0:r0 + L, 128 * h:128 * h + 128], case["k32"][r0:r0 + KL, 128 * (h // g):128 * (h // g) + 128]
            else:
                q, k = case["q"][r0:r0 + L, 128 * h:128 * h + 128], case["kc"][slot, h // g, :KL]
            q, k, v = q.astype(np.float64), k.astype(np.float64), case["vc"][slot, h // g, :KL].astype(np.float64)
            s, mag = scale * (q @ k.T), scale * (np.abs(q) @ np.abs(k).T)
            eps = (128 + 2) * U * mag
            if fp32_scores:
                o, b = softmax_terms(s, eps, v, mask, tiles=(KL + 127) // 128, adds=128)
                sm = np.where(mask, s, -np.inf)
                pm = np.maximum.accumulate(sm, 1)   # prefix maxima
                nmax = (np.diff(pm, axis=1, prepend=-np.inf) > 0).sum(1)
                # prefix accumulators relative to the prefix maximum, and S relative to the final one
                A = np.zeros((L, 128))
                for j in range(KL):
                    wj = np.where(mask[:, :j + 1], np.exp(sm[:, :j + 1] - pm[:, j:j + 1]), 0.0)
                    A = np.maximum(A, np.abs(wj @ v[:j + 1]))
                S = np.where(mask, np.exp(sm - pm[:, -1:]), 0.0).sum(1)
                steps = (mask.sum(1) + nmax) * 2.0 ** -11
                b = b + (steps * (1 + steps) / S)[:, None] * A
            else:
                o, b = softmax_terms(s, eps, v, mask, tiles=(KL + 63) // 64, adds=2 * KL, p_rel=2.0 ** -22, p_abs=2.0 ** -25)
            ref[r0:r0 + L, 128 * h:128 * h + 128], bound[r0:r0 + L, 128 * h:128 * h + 128] = o, b
    return ref, bound


def _expf(x):
    """expf of fp32 arguments, correctly rounded (float64 exp, rounded once): numpy's own float32 exp errs by up to
    2.4 ulps, which with the device expf's 1 ulp would leave the two-ulp window of exact_chain"""
    return np.exp(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def _near16(un, win):
    """un within win of a boundary of the chain's rounding, fp16(fp32(un)): its two ends round apart.  (The boundary
    is not the fp16 midpoint itself: every value within half an fp32 ulp of the midpoint rounds onto it first and
    then to the even neighbour.)"""
    return (un + win).astype(np.float32).astype(np.float16) != (un - win).astype(np.float32).astype(np.float16)


def exact_chain(case, limit_shift=0, drop_key=None):
    """numpy restatement of ggml's CPU flash-attention chain as fa_exact.hip runs it, per query row and head, keys in
    order: s = fp32(q . k) * scale (the fp32 sum is exact for lattice inputs -- asserted against float64); a new
    maximum rescales the accumulator, acc = fp16(fp32(acc) * ms), ms = expf(M - s) (0 at the first key), and takes
    vs = 1; any other key vs = expf(s - M); every key then acc = fp16(fma(v, vs, acc)) (fma rounded to fp32, then to
    fp16); out = fp32(acc) / S.  expf is correctly rounded here (_expf) and within 1 ulp on the device, so the two
    differ by at most 1.5 ulps of any weight, and by the order of S:
    an element is marked near-tie if at any key its unrounded value lay within two fp32 ulps of that key's v * vs (at
    a rescale: of acc * ms) of an fp16 rounding boundary -- ulps at their largest relative size, 2 * 2^-23 |v vs|: a
    weight 1.5 ulps off moves v * vs by up to 1.5 * 2^-23 |v vs|, which is up to three of the product's own ulps when
    the product sits low in its binade, so a window counted in the product's own ulps would miss flips.  Returns (acc / S in float64 [rows][QD], near-tie mask,
    one fp16 ulp of the largest prefix |acc| over S, relative bound of S and the divide):
      S: expf 2 U, the subtraction s - M at most U (M - min s), a 128-key tree of 7 additions plus the chunk's add
      and rescale (3 U a chunk); the divide and multiply 3 U."""
    nh, g = case["n_head"], case["n_head"] // case["n_kv_head"]
    QD = nh * 128
    out, tie, amax, rel = np.zeros((case["rows"], QD)), np.zeros((case["rows"], QD), bool), np.zeros((case["rows"], QD)), np.zeros(
        (case["rows"], 1))
    scale = np.float32(case["scale"])
    for r0, L, slot, P0 in _seqs(case):
        KL = P0 + L
        mask = _causal(L, P0, limit_shift, drop_key)
        q = case["q"][r0:r0 + L].astype(np.float32).reshape(L, nh, 128)
        k = np.repeat(case["kc"][slot, :, :KL].astype(np.float32), g, 0)       # [nh][KL][128]
        v = np.repeat(case["vc"][slot, :, :KL].astype(np.float64), g, 0)       # [nh][KL][128]
        dots = np.einsum("lhd,hkd->lhk", q, k)
        assert np.array_equal(dots.astype(np.float64), np.einsum("lhd,hkd->lhk", q.astype(np.float64), k.astype(np.float64))), \
            "the fp32 score sums are not exact: the chain's inputs would depend on the summation order"
        s = (dots * scale).astype(np.float32)                                   # [L][nh][KL]
        M = np.full((L, nh), -np.inf, np.float32)
        acc = np.zeros((L, nh, 128))             # fp16 values held in float64
        peak = np.zeros((L, nh, 128))
        tied = np.zeros((L, nh, 128), bool)
        for j in range(KL):
            on = mask[:, j]                      # the rows that see key j: a suffix (causal)
            if not on.any():
                continue
            f = int(np.argmax(on))
            assert on[f:].all()
            sj, Mo, a, tv = s[f:, :, j], M[f:], acc[f:], tied[f:]
            new = sj > Mo
            with np.errstate(invalid="ignore", over="ignore"):
                vs = np.where(new, np.float32(1), _expf(np.where(new, np.float32(0), sj - Mo))).astype(np.float64)
                if new.any():                    # ggml's order: the rescale, then the mad with vs = 1 (exact: never marked)
                    li, hi = np.nonzero(new)
                    ms = np.where(np.isneginf(Mo[li, hi]), np.float32(0), _expf(Mo[li, hi] - sj[li, hi])).astype(np.float64)
                    un = a[li, hi] * ms[:, None]
                    tv[li, hi] |= _near16(un, 2.0 ** -22 * np.abs(un))
                    a[li, hi] = un.astype(np.float32).astype(np.float16)
            t = v[None, :, j, :] * vs[..., None]
            un = t + a
            tv |= _near16(un, 2.0 ** -22 * np.abs(t)) & ~new[..., None]
            a[...] = un.astype(np.float32).astype(np.float16)
            np.maximum(peak[f:], np.abs(a), out=peak[f:])
            M[f:] = np.maximum(Mo, sj)
        s64 = np.where(mask[:, None, :], s.astype(np.float64), -np.inf)
        S = np.exp(s64 - M.astype(np.float64)[..., None]).sum(-1)               # [L][nh]
        out[r0:r0 + L] = (acc / S[..., None]).reshape(L, QD)
        tie[r0:r0 + L] = tied.reshape(L, QD)
        amax[r0:r0 + L] = (ulp16(peak) / S[..., None]).reshape(L, QD)
        spread = (M.astype(np.float64)[..., None] - np.where(mask[:, None, :], s64, np.inf)).max((1, 2))
        rel[r0:r0 + L, 0] = (2 + spread + 8 + 3 * ((KL + 127) // 128) + 3) * U
    return out, tie, amax, rel


def check_exact(buf, case, chain, fp16, what):
    """the exact kernel's output against exact_chain: unmarked elements within the relative bound of S and the
    divide (their accumulators are equal to the last bit), marked ones additionally within 2 fp16 ulps of the largest
    prefix accumulator over S.  Returns (worst error / bound, near-tie share); the share is capped at 5 %"""
    ref, tie, amax, rel = chain
    valid = prefill_valid(case)
    share = float(tie[valid].mean())
    assert share <= 0.05, f"{what}: {share:.3f} of the elements are near-ties -- the case no longer holds the chain to its bits"
    bound = np.abs(ref) * rel + np.where(tie, 2 * amax, 0.0)
    return check_rows(buf, valid, ref, bound, fp16, what), share


def fake_output(vals, valid, fp16):
    """the allocation a kernel computing `vals` [rows][ld] would leave: sentinel guard rows and rows outside `valid`"""
    dt = np.uint16 if fp16 else np.float32
    raw = np.full((len(valid) + 2 * GUARD, vals.shape[1]), 0xFFFF if fp16 else 0xFFFFFFFF, np.uint16 if fp16 else np.uint32)
    v = vals.astype(np.float32)
    body = (v.astype(np.float16).view(np.uint16) if fp16 else v.view(np.uint32))
    raw[GUARD:GUARD + len(valid)][valid] = body[valid]
    return raw.view(dt)
