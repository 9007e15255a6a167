"""Shared by the kernel tests (tests/test_gpu_kernels.py, tests/test_kernel_util_host.py):
ctypes bindings of the test-only launcher entries (include/qasr_capi.h,
csrc/kernel_harness.hip), float64 references of the GEMM / GEMV / Q8_0 kernels
over the same rounded operands, the bounds derived from their arithmetic, and
the comparators.  Nothing here is measured on the code under test.

Layouts (csrc/kernels.h):
  dense       A fp16 [M][lda], W fp16 [N][ldw] (PyTorch [out][in]), out [M][ldo]
  Q8_0        int8 quants [rows][ld] + one scale per 32 values: activations fp32
              Ad [M][ldad], weights fp16 Wd [N][K / 32]
  SwiGLU      weight rows come in groups of 32: 16 gate rows, then 16 up rows.
              Output column o reads gate row 32 * (o >> 4) + (o & 15) and the up
              row 16 below it (swiglu_rows); 2 F weight rows give F columns.
  argmax key  (order-preserving bits of the fp32 value) << 32 | 0xffffffff - column

Every output comes back as its whole allocation: GUARD sentinel rows, the rows,
GUARD sentinel rows, each ld wide; every byte the kernel did not write is 0xFF.
"""
import ctypes as C

import numpy as np

EPI_F32, EPI_GELU_F16, EPI_SWIGLU_F16, EPI_ARGMAX, EPI_F16, EPI_SWIGLU_F32, EPI_SWIGLU_Q8 = range(7)
GEMM, GEMM_Q8, SKINNY, SKINNY_Q8 = range(4)
GUARD = 3
U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
F16_MIN_ULP = 2.0 ** -24


# ------------------------------------------------------------------ bindings
_P = C.c_void_p


class GemmCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "launcher", "epi", "M", "N", "K", "lda", "ldw", "ldad", "ldr", "ldo", "ldo16", "ldoq",
        "regs_staged", "n_valid", "skinny_inflight", "wdef", "guard", "pe_rows")] + [(n, _P) for n in (
            "A", "W", "Aq", "Ad", "Wq", "Wd", "bias", "res", "pe", "pe_pos",
            "out_f32", "out_f16", "out_q", "out_d", "amax", "gelu_out")] + [
        ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


class GemvCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "epi", "M", "N", "K", "wrows", "ldx", "ldxh", "ldr", "ldo", "ldo16", "embd_rows", "hist_stride",
        "guard", "launches")] + [("eps", C.c_float)] + [(n, _P) for n in (
            "x", "xh", "norm_w", "W", "Wq", "Wd", "bias", "res", "embd_ids", "embd",
            "x_store", "out_f32", "out_f16", "amax", "done", "tok_out", "hist", "step", "pos")] + [
        ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


class QuantCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("M", "K", "ldx", "gather_C", "guard")] + [(n, _P) for n in ("x32", "x16", "q", "d")]


def _lib():
    import qasr
    L = qasr.lib()
    for name, typ in (("qasr_kt_gemm", GemmCall), ("qasr_kt_gemv", GemvCall), ("qasr_kt_quantize_q8", QuantCall)):
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


class Result:
    """what one harness call gave: tag, declined / msg, and the whole output allocations"""

    def __init__(self, call, outs):
        self.tag = call.tag.decode()
        self.declined = bool(call.declined)
        self.msg = call.msg.decode()
        self.__dict__.update(outs)


def _set(call, keep, **arrays):
    for name, a in arrays.items():
        if a is not None:
            a = np.ascontiguousarray(a)
            keep.append(a)
            setattr(call, name, a.ctypes.data_as(_P))
    return keep


def pad_cols(a, ld, fill=None):
    """[rows][cols] -> [rows][ld] with the padding columns NaN (int8: 0x7F): a kernel
    that reads past a row's width shows up in its outputs"""
    a = np.asarray(a)
    out = np.empty((a.shape[0], ld), a.dtype)
    out[:] = (0x7F if a.dtype == np.int8 else np.nan) if fill is None else fill
    out[:, :a.shape[1]] = a
    return out


def _alloc(rows, ld, dtype):
    return np.zeros((rows + 2 * GUARD, ld), dtype)


def run_gemm(launcher, epi, M, N, K, *, A=None, W=None, Aq=None, Ad=None, Wq=None, Wd=None, bias=None, res=None,
             pe=None, pe_pos=None, ldo=0, ldo16=0, ldoq=0, amax=False, regs_staged=0, n_valid=0, inflight=1, wdef=1):
    """operands as [rows][ld] arrays (pad_cols); an output is allocated where its ld is non-zero"""
    c = GemmCall(launcher=launcher, epi=epi, M=M, N=N, K=K, regs_staged=regs_staged, n_valid=n_valid,
                 skinny_inflight=inflight, wdef=wdef, guard=GUARD, ldo=ldo, ldo16=ldo16, ldoq=ldoq)
    first = A if A is not None else Aq
    wfirst = W if W is not None else Wq
    c.lda, c.ldw = first.shape[1], wfirst.shape[1]
    if Ad is not None:
        c.ldad = Ad.shape[1]
    if res is not None:
        c.ldr = res.shape[1]
    if pe is not None:
        c.pe_rows = pe.shape[0]
    outs = dict(out_f32=_alloc(M, ldo, np.float32) if ldo else None, out_f16=_alloc(M, ldo16, np.uint16) if ldo16 else None,
                out_q=_alloc(M, ldoq, np.int8) if ldoq else None, out_d=_alloc(M, ldoq // 32, np.float32) if ldoq else None,
                amax=_alloc(M, 1, np.uint64) if amax else None, gelu_out=np.zeros(65536, np.uint16))
    keep = _set(c, [], A=A, W=W, Aq=Aq, Ad=Ad, Wq=Wq, Wd=Wd, bias=bias, res=res, pe=pe,
                pe_pos=None if pe_pos is None else np.asarray(pe_pos, np.int32), **outs)
    L = _lib()
    rc = L.qasr_kt_gemm(0, C.byref(c))
    _ok(L, rc)
    del keep
    return Result(c, outs)


def run_gemv(epi, M, N, K, *, wrows=None, x=None, xh=None, norm_w=None, eps=1e-6, W=None, Wq=None, Wd=None, bias=None,
             res=None, embd_ids=None, embd=None, x_store_ld=0, ldo=0, ldo16=0, amax=False, book=None, launches=1):
    """book: dict(step=, pos=[M], hist_stride=) switches the EPI_ARGMAX bookkeeping group on"""
    c = GemvCall(epi=epi, M=M, N=N, K=K, wrows=wrows or N, guard=GUARD, launches=launches, eps=eps, ldo=ldo, ldo16=ldo16)
    if x is not None:
        c.ldx = x.shape[1]
    if x_store_ld:
        c.ldx = x_store_ld
    if xh is not None:
        c.ldxh = xh.shape[1]
    if res is not None:
        c.ldr = res.shape[1]
    if embd is not None:
        c.embd_rows = embd.shape[0]
    outs = dict(x_store=_alloc(M, x_store_ld, np.float32) if x_store_ld else None,
                out_f32=_alloc(M, ldo, np.float32) if ldo else None, out_f16=_alloc(M, ldo16, np.uint16) if ldo16 else None,
                amax=np.zeros(8, np.uint64) if amax or book else None)
    if book:
        c.hist_stride = book["hist_stride"]
        pos = np.zeros(8, np.int32)
        pos[:M] = book["pos"]
        outs.update(done=np.zeros(1, np.uint32), tok_out=np.full(8, -7, np.int32),
                    hist=np.full((M, book["hist_stride"]), -7, np.int32), step=np.array([book["step"]], np.int32), pos=pos)
    keep = _set(c, [], x=x, xh=xh, norm_w=norm_w, W=W, Wq=Wq, Wd=Wd, bias=bias, res=res, embd=embd,
                embd_ids=None if embd_ids is None else np.asarray(embd_ids, np.int32), **outs)
    L = _lib()
    rc = L.qasr_kt_gemv(0, C.byref(c))
    _ok(L, rc)
    del keep
    return Result(c, outs)


def run_quantize(M, K, *, x32=None, x16=None, gather_C=0):
    src = x32 if x32 is not None else x16
    c = QuantCall(M=M, K=K, ldx=src.shape[1], gather_C=gather_C, guard=GUARD)
    outs = dict(q=_alloc(M, K, np.int8), d=_alloc(M, K // 32, np.float32))
    keep = _set(c, [], x32=x32, x16=x16, **outs)
    L = _lib()
    rc = L.qasr_kt_quantize_q8(0, C.byref(c))
    _ok(L, rc)
    del keep
    return outs["q"], outs["d"]


# -------------------------------------------------------------------- inputs
def f16_normal(rng, shape, scale=1.0):
    """seeded normal values already rounded to fp16 (as float16)"""
    return (rng.standard_normal(shape) * scale).astype(np.float16)


def bits(a16):
    return np.ascontiguousarray(a16, np.float16).view(np.uint16)


def q8_operand(rng, rows, K, scale_dtype, scale=1.0):
    """int8 quants [rows][K] in -127 .. 127 and positive block scales [rows][K / 32]"""
    q = rng.integers(-127, 128, (rows, K)).astype(np.int8)
    d = (np.abs(rng.standard_normal((rows, K // 32))) * scale + scale * 0.1).astype(np.float16)
    return q, d.astype(scale_dtype)


def swiglu_rows(F):
    """(gate row, up row) of every output column 0 .. F - 1 (module docstring)"""
    o = np.arange(F)
    gate = 32 * (o >> 4) + (o & 15)
    return gate, gate + 16


# ---------------------------------------------------------------- references
def dense_terms(A, W):
    """float64 A W^T and |A| |W|^T of fp16 operands [M][K], [N][K]"""
    a, w = np.asarray(A, np.float64), np.asarray(W, np.float64)
    return a @ w.T, np.abs(a) @ np.abs(w).T


def dense_bound(K, mag):
    """fp16 x fp16 products are exact in fp32; K fp32 additions in any order (plus the
    partial sums of a split K) err by at most (K + 2) 2^-24 sum |a w| to first order"""
    return (K + 2) * U * mag


def q8_terms(Aq, Ad, Wq, Wd):
    """sum_b d_w d_x idot_b and sum_b |d_w d_x idot_b| in float64 (the integer block dots are exact)"""
    M, K = Aq.shape
    N = Wq.shape[0]
    ref, mag = np.zeros((M, N)), np.zeros((M, N))
    ad, wd = np.asarray(Ad, np.float64), np.asarray(Wd, np.float64)
    for b in range(K // 32):
        idot = Aq[:, 32 * b:32 * b + 32].astype(np.float64) @ Wq[:, 32 * b:32 * b + 32].astype(np.float64).T
        t = ad[:, b, None] * wd[None, :, b] * idot
        ref += t
        mag += np.abs(t)
    return ref, mag


def q8_bound(K, mag):
    """one rounding of d_w d_x and one of the fma per block"""
    return (K // 32 + 1) * U * mag


def add_terms(ref, bound, *adds):
    """+ bias / PE / residual: one fp32 rounding each, 2^-24 |partial|"""
    for a in adds:
        if a is not None:
            ref = ref + a
            bound = bound + U * np.abs(ref)
    return ref, bound


def silu(g):
    return g / (1.0 + np.exp(-g))


def swiglu_terms(g, bg, u, bu):
    """silu(g) * u with the two dot-product bounds propagated (|silu'| <= 1.1) and
    8 roundings of <= 1 ulp for expf, add, divide and multiply"""
    v = silu(g) * u
    return v, np.abs(silu(g)) * bu + 1.1 * bg * (np.abs(u) + bu) + 8 * U * np.abs(v)


def ulp16(v):
    """spacing of fp16 at |v| (subnormals: 2^-24)"""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return np.maximum(2.0 ** (np.floor(np.log2(a)) - 10), F16_MIN_ULP)


def q8_quantize(v):
    """float32 restatement of q8_scale / q8_quant (csrc/dev_common.h) over rows [R][K]:
    d = fp16(amax / 127), q = rint(v * (127 / amax)); returns (q int8 [R][K], d fp32 [R][K / 32])"""
    v = np.asarray(v, np.float32)
    b = v.reshape(v.shape[0], -1, 32)
    amax = np.abs(b).max(-1)
    d = (amax / np.float32(127)).astype(np.float16).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(amax != 0, np.float32(127) / amax, np.float32(0)).astype(np.float32)
    q = np.rint(b * inv[..., None]).astype(np.int8)
    return q.reshape(v.shape), d


def rms_prologue(x, norm_w, eps):
    """the GEMV prologue (gemm.hip gemv_kernel): float32 squares summed in float64, scale =
    1 / sqrtf((float)(tot / K) + eps), two float32 multiplies, round to fp16.  Returns the fp16
    rows, the float32 values before that rounding, and the mask of elements within 2^-20
    relative of an fp16 rounding tie (a scale one fp32 ulp off may flip only those)"""
    x = np.asarray(x, np.float32)
    K = x.shape[1]
    tot = (x * x).astype(np.float64).sum(1)
    scale = np.float32(1) / np.sqrt((tot / K).astype(np.float32) + np.float32(eps), dtype=np.float32)
    v = (x * scale[:, None]).astype(np.float32) * np.asarray(norm_w, np.float32)[None, :]
    h = v.astype(np.float16)
    v64 = v.astype(np.float64)
    frac = np.mod(np.abs(v64) / ulp16(v64), 1.0)
    tie = np.abs(frac - 0.5) * ulp16(v64) <= 2.0 ** -20 * np.abs(v64)
    return h, v, tie


def tie_slack(h, tie, W):
    """one fp16 ulp of each near-tie element times |w|"""
    return (np.where(tie, ulp16(h.astype(np.float64)), 0.0)) @ np.abs(np.asarray(W, np.float64)).T


# --------------------------------------------------------------- comparators
_SENT = {4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}


def in_range(buf, M, ncols, what="out"):
    """the buffer state every case asserts: guard rows and padding columns still hold the
    sentinel, every in-range element was written and none is NaN; returns the [M][ncols] view"""
    raw = buf.view(_SENT[buf.dtype.itemsize])
    full = np.iinfo(raw.dtype).max
    assert raw.shape[0] == M + 2 * GUARD and raw.shape[1] >= ncols, (what, raw.shape, M, ncols)
    assert (raw[:GUARD] == full).all(), f"{what}: guard rows before the output overwritten"
    assert (raw[GUARD + M:] == full).all(), f"{what}: guard rows after the output overwritten"
    assert (raw[GUARD:GUARD + M, ncols:] == full).all(), f"{what}: padding columns overwritten"
    body = buf[GUARD:GUARD + M, :ncols]
    if buf.dtype == np.float32:
        unwritten = raw[GUARD:GUARD + M, :ncols] == full
        assert not unwritten.any(), f"{what}: {int(unwritten.sum())} elements never written, first {np.argwhere(unwritten)[0]}"
        assert not np.isnan(body).any(), f"{what}: NaN in range at {np.argwhere(np.isnan(body))[0]}"
    elif buf.dtype == np.uint16:   # fp16 bits
        unwritten = body == 0xFFFF
        assert not unwritten.any(), f"{what}: {int(unwritten.sum())} elements never written, first {np.argwhere(unwritten)[0]}"
        nan = np.isnan(body.view(np.float16))
        assert not nan.any(), f"{what}: NaN in range at {np.argwhere(nan)[0]}"
    return body


def untouched(*bufs):
    """a declined call: every output byte still holds the sentinel"""
    for b in bufs:
        if b is not None:
            assert (b.view(np.uint8) == 0xFF).all(), "a declined launcher wrote to its output"


def check_values(out, ref, bound, fp16=False, what="out"):
    """|out - ref| <= bound (+ half an fp16 ulp of the reference for fp16 outputs);
    out: fp32 values, or fp16 bits when fp16.  Returns the worst error / bound"""
    o = (out.view(np.float16) if fp16 else out).astype(np.float64)
    tol = bound + (0.5 * ulp16(ref) if fp16 else 0.0)
    err = np.abs(o - ref)
    bad = ~(err <= tol)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound, first {i}: "
                             f"got {o[i]!r} want {ref[i]!r} err {err[i]:.3e} tol {tol[i]:.3e}")
    return float((err / np.maximum(tol, 1e-300)).max())


def _f16_index(h):
    """fp16 values -> integers in value order (adjacent values differ by 1; -0 and +0 by 1)"""
    b = h.view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF) - 1, b)


def _f16_from_index(i):
    b = np.where(i < 0, (-(i + 1)) | 0x8000, i).astype(np.uint16)
    return b.view(np.float16)


def check_gelu(out_bits, table, ref, bound, what="gelu"):
    """set membership: out == table[h] for an fp16 h that some pre-activation within
    `bound` of the reference rounds to; past the clamps 0 (x <= -10) or fp16(x) (x >= 10).
    Returns the widest candidate set met (in fp16 values)"""
    lo = _f16_index((ref - bound).astype(np.float16))
    hi = _f16_index((ref + bound).astype(np.float16))
    # every (table value, index in value order) pair, sorted: is there an h in [lo, hi] with table[h] == out?
    allh = np.arange(65536, dtype=np.uint16)
    keys = np.sort(table.astype(np.int64) * (1 << 17) + (_f16_index(allh.view(np.float16)) + 32768))
    want = out_bits.astype(np.int64) * (1 << 17)
    first = np.searchsorted(keys, want + lo + 32768)
    ok = (first < len(keys)) & (keys[np.minimum(first, len(keys) - 1)] <= want + hi + 32768)
    oi = _f16_index(np.ascontiguousarray(out_bits).view(np.float16))
    ov = np.ascontiguousarray(out_bits).view(np.float16).astype(np.float64)
    ok |= (ov >= 10.0) & (lo <= oi) & (oi <= hi)                      # x >= 10: the fp16 of x itself
    ok |= (out_bits == 0) & ((ref - bound).astype(np.float16) <= -10.0)   # x <= -10: zero
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} outputs outside the table set, first {i}: got {int(out_bits[i]):#06x} "
                             f"for pre-activation {ref[i]!r} +- {bound[i]:.3e}")
    return int((hi - lo).max()) + 1


def key_index(keys):
    return (0xFFFFFFFF - (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int64)


def key_value(keys):
    u = (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32)
    return np.where(u >> 31, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


def check_argmax(idx, logits, n_valid=0, what="argmax"):
    """exact: the first index of the maximum of the kernel's own fp32 logits over the valid columns"""
    lg = logits[:, :n_valid] if n_valid else logits
    want = np.argmax(lg, axis=1)   # numpy returns the first maximum
    assert np.array_equal(np.asarray(idx), want), f"{what}: got {np.asarray(idx)[:8]} want {want[:8]}"


def check_q8(q, d, q_ref, d_ref, what="q8"):
    """bit for bit against the restatement"""
    assert np.array_equal(d.view(np.uint32), d_ref.view(np.uint32)), f"{what}: block scales differ"
    if not np.array_equal(q, q_ref):
        i = tuple(np.argwhere(q != q_ref)[0])
        raise AssertionError(f"{what}: {int((q != q_ref).sum())} quants differ, first {i}: got {int(q[i])} want {int(q_ref[i])}")
