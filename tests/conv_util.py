"""Shared by the conv front-end tests (tests/test_gpu_conv_kernels.py, tests/test_kernel_util_host.py): the ctypes
binding of qasr_kt_conv (include/qasr_capi.h, csrc/kernel_harness.hip), chunk tables, references of conv1 / conv2 /
conv3 that state the geometry on their own, the two input families and the comparators.  Nothing here is measured
on the code under test; the buffer-state checks, the GELU set comparator and the dense bound are kernel_util's.

Geometry.  Every chunk is an image convolved on its own: 3x3, stride 2, zero padding 1, NCHW float64, weights
[oc][ic][kh][kw], computed from the nine strided slices of the zero-padded input (`taps`) -- no (tap, channel) K
index and no row table appears in it.  conv1 reads the chunk's mel [1][128 bins][L frames] (frames from Lv on are
zeros), conv2 its act1 [C][64][W1], conv3 its act2 [C][32][W2]; an output size is (n - 1) // 2 + 1.
The device side (csrc/kernels.h):
  weights  conv1 [oc][kh * 3 + kw]; conv2 / conv3 [oc][(kh * 3 + kw) * C + ic], rows conv_kpad(C) long (`pack_weights`)
  act1     row row1 + oh * W1 + ow, 64 image rows      act2  row row2 + oh * W2 + ow, 32 image rows
  act3     row row3 + ow * 16 + oh: a chunk's 16 image rows of one output frame are consecutive, the order conv_out's
           dense A needs (`to_rows` / `from_rows` are the only statements of these three maps)
"""
import ctypes as C

import numpy as np

import kernel_util as ku
from kernel_util import GUARD, Result, _ok, _P, _set

HEIGHT = {0: 128, 1: 64, 2: 32, 3: 16}           # image rows of the mel (0) and of each layer's output
WIDTH = {0: "L", 1: "W1", 2: "W2", 3: "W3"}
ROW = {1: "row1", 2: "row2", 3: "row3"}


def conv_kpad(channels):
    return (9 * channels + 127) // 128 * 128


def out_size(n):
    return (n - 1) // 2 + 1


# ------------------------------------------------------------------ bindings
class Chunk(C.Structure):
    _fields_ = [("mel_off", C.c_int64)] + [(n, C.c_int32) for n in ("T", "L", "Lv", "W1", "W2", "W3", "row1", "row2", "row3", "enc_row")]


class ConvCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("layer", "C", "regs_staged", "n_chunks", "in_len", "out_rows", "guard", "guard_in", "max_w1")] + [
        (n, _P) for n in ("chunks", "mel", "act", "W", "bias", "out", "gelu_out")] + [
        ("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


def _lib():
    import qasr
    L = qasr.lib()
    L.qasr_kt_conv.argtypes = [C.c_int, C.POINTER(ConvCall)]
    L.qasr_kt_conv.restype = C.c_int
    return L


def make_chunks(clips):
    """the chunk table of clips given as frames T (ASR: 100-frame chunks, the last one short), ("al", T) (the
    aligner: every chunk 100 frames wide, Lv of them read) or ("whole", T) (one unchunked chunk); a clip's mel is
    [128][T] floats, the clips back to back"""
    out, r1, r2, r3, off = [], 0, 0, 0, 0
    for b, spec in enumerate(clips):
        kind, T = spec if isinstance(spec, tuple) else ("asr", spec)
        step = T if kind == "whole" else 100
        for s in range(0, T, step):
            Lv = min(step, T - s)
            L = 100 if kind == "al" else Lv
            W1 = out_size(L)
            W2 = out_size(W1)
            W3 = out_size(W2)
            out.append(dict(clip=b, start=s, mel_off=off + s, T=T, L=L, Lv=Lv, W1=W1, W2=W2, W3=W3, row1=r1, row2=r2, row3=r3,
                            enc_row=r3 // 16))
            r1 += 64 * W1
            r2 += 32 * W2
            r3 += 16 * W3
        off += 128 * T
    return out


def mel_len(chunks):
    return max(c["mel_off"] - c["start"] + 128 * c["T"] for c in chunks)


def rows_of(layer, ch):
    return HEIGHT[layer] * ch[WIDTH[layer]]


def total_rows(layer, chunks):
    return sum(rows_of(layer, c) for c in chunks)


def run_conv(layer, Cc, chunks, W, bias, *, mel=None, act=None, regs_staged=0, max_w1=None):
    """W / bias as the device holds them; mel flat float32, act [rows][C] fp16 bits; the whole output allocation back"""
    table = (Chunk * len(chunks))(*[Chunk(**{n: c[n] for n, _ in Chunk._fields_}) for c in chunks])
    M = total_rows(layer, chunks)
    src = mel if layer == 1 else act
    # guards wider than anything one mis-bounded tap can reach: a frame-row of the widest clip, an image row of the widest chunk
    gin = max(max(c["T"], c["L"]) for c in chunks) + 1 if layer == 1 else max(c[WIDTH[layer - 1]] for c in chunks) + 1
    call = ConvCall(layer=layer, C=Cc, regs_staged=regs_staged, n_chunks=len(chunks), in_len=src.shape[0], out_rows=M, guard=GUARD,
                    guard_in=gin, max_w1=max_w1 or max(c["W1"] for c in chunks), chunks=C.cast(table, _P))
    outs = dict(out=np.zeros((M + 2 * GUARD, Cc), np.uint16), gelu_out=np.zeros(65536, np.uint16))
    keep = _set(call, [table], W=W, bias=np.asarray(bias, np.float32), **{"mel" if layer == 1 else "act": src}, **outs)
    L = _lib()
    rc = L.qasr_kt_conv(0, C.byref(call))
    _ok(L, rc)
    del keep
    return Result(call, outs)


# ------------------------------------------------------------------ geometry
def taps(x, Ho, Wo):
    """the nine stride-2 views [..][Ho][Wo] of x [..][H][W] zero-padded by one on every side, in (kh, kw) order"""
    H, Wd = x.shape[-2:]
    xp = np.zeros(x.shape[:-2] + (H + 2, Wd + 2), x.dtype)
    xp[..., 1:H + 1, 1:Wd + 1] = x
    for kh in range(3):
        for kw in range(3):
            yield kh, kw, xp[..., kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]


def conv_ref(x, w, want_mag=False):
    """x [ic][H][W], w [oc][ic][3][3], float64 -> the convolution [oc][Ho][Wo] and, when asked, sum |x| |w|"""
    Ho, Wo = out_size(x.shape[1]), out_size(x.shape[2])
    out = np.zeros((w.shape[0], Ho * Wo))
    mag = np.zeros_like(out) if want_mag else None
    for kh, kw, sl in taps(x, Ho, Wo):
        flat, wk = sl.reshape(x.shape[0], -1), np.ascontiguousarray(w[:, :, kh, kw])   # (contiguous: the BLAS path)
        out += wk @ flat
        if want_mag:
            mag += np.abs(wk) @ np.abs(flat)
    shape = (w.shape[0], Ho, Wo)
    return out.reshape(shape), (mag.reshape(shape) if want_mag else None)


def pack_weights(w, pad):
    """[oc][ic][3][3] fp16 -> the device rows [oc][conv_kpad(ic)], column (kh * 3 + kw) * ic_count + ic; padding columns = pad"""
    oc, ic = w.shape[:2]
    out = np.full((oc, conv_kpad(ic)), pad, np.float16)
    out[:, :9 * ic] = np.asarray(w, np.float16).transpose(0, 2, 3, 1).reshape(oc, 9 * ic)
    return out


def to_rows(layer, y):
    """a chunk's output [C][Ho][Wo] -> its device rows [Ho * Wo][C] in the layer's row order"""
    return np.ascontiguousarray((y.transpose(2, 1, 0) if layer == 3 else y.transpose(1, 2, 0)).reshape(-1, y.shape[0]))


def from_rows(layer, rows, ch):
    """a chunk's device rows of act1 / act2 (layer 1 / 2) -> [C][H][W]"""
    assert layer in (1, 2)
    return rows.reshape(HEIGHT[layer], ch[WIDTH[layer]], -1).transpose(2, 0, 1)


def chunk_rows(layer, ch, table):
    """the rows of chunk ch in a layer's whole row table"""
    return table[ch[ROW[layer]]:ch[ROW[layer]] + rows_of(layer, ch)]


def per_chunk(layer, chunks, fn):
    """fn(chunk) -> [C][Ho][Wo] arrays (or a tuple of them) scattered into whole row tables"""
    outs = None
    for ch in chunks:
        ys = fn(ch)
        ys = ys if isinstance(ys, tuple) else (ys,)
        if outs is None:
            outs = [np.zeros((total_rows(layer, chunks), y.shape[0]), y.dtype) for y in ys]
        for o, y in zip(outs, ys):
            assert y.shape[1:] == (HEIGHT[layer], ch[WIDTH[layer]]), (y.shape, ch)
            chunk_rows(layer, ch, o)[:] = to_rows(layer, y)
    return outs if len(outs) > 1 else outs[0]


# ---------------------------------------------------------------- references
def gelu_bits(x32, table):
    """the epilogue on fp32 pre-activations: table[fp16(x)], past the clamps 0 (x <= -10) or fp16(x) (x >= 10)"""
    x32 = np.asarray(x32, np.float32)
    b = x32.astype(np.float16).view(np.uint16)
    return np.where(x32 <= -10, np.uint16(0), np.where(x32 >= 10, b, table[b])).astype(np.uint16)


def chunk_mel(ch, mel):
    """the image conv1 reads of a chunk: [1][128][L], frames from Lv on zeros"""
    clip = np.asarray(mel)[ch["mel_off"] - ch["start"]:][:128 * ch["T"]].reshape(128, ch["T"])
    img = np.zeros((1, 128, ch["L"]), clip.dtype)
    img[0, :, :ch["Lv"]] = clip[:, ch["start"]:ch["start"] + ch["Lv"]]
    return img


def conv1_reference(chunks, mel, w, bias, table):
    """the stated arithmetic of conv1 (csrc/elementwise.hip), bit for bit: the mel rounded to fp16, the nine exact
    products summed in float64 in tap order, rounded to float32, + bias in float32, the GELU table.  -> act1 bits"""
    h = np.asarray(mel, np.float32).astype(np.float16).astype(np.float64)
    w64, b32 = np.asarray(w, np.float64), np.asarray(bias, np.float32)

    def one(ch):
        sd = np.zeros((w64.shape[0], 64, ch["W1"]))
        for kh, kw, sl in taps(chunk_mel(ch, h), 64, ch["W1"]):
            sd = sd + w64[:, 0, kh, kw][:, None, None] * sl      # fp16 x fp16: exact in fp32 and in float64
        return gelu_bits(sd.astype(np.float32) + b32[:, None, None], table)
    return per_chunk(1, chunks, one)


def conv_reference(layer, chunks, act, w, want_mag=False):
    """float64 conv2 / conv3 (no bias) of the device rows `act` of the layer before, as whole row tables (ref, mag)"""
    a64, w64 = np.asarray(act.view(np.float16), np.float64), np.asarray(w, np.float64)
    return per_chunk(layer, chunks, lambda ch: conv_ref(from_rows(layer - 1, chunk_rows(layer - 1, ch, a64), ch), w64, want_mag)
                     if want_mag else conv_ref(from_rows(layer - 1, chunk_rows(layer - 1, ch, a64), ch), w64)[0])


# -------------------------------------------------------------------- inputs
def lattice_inputs(rng, layer, Cc, chunks):
    """activations k / 4 (|a| <= 1), weights k / 256 (|w| <= 1 / 64), biases k / 1024 (|b| < 1) with a few columns at
    +-14 (both GELU clamps): every product and every partial sum is a multiple of 2^-10 far below 2^14, so fp32
    accumulation in any order, the bias add and this float64 reference are all exact"""
    act = (rng.integers(-4, 5, (total_rows(layer - 1, chunks), Cc)) / 4).astype(np.float16)
    w = (rng.integers(-4, 5, (Cc, Cc, 3, 3)) / 256).astype(np.float16)
    bias = (rng.integers(-1023, 1024, Cc) / 1024).astype(np.float32)
    bias[[1, Cc // 2, Cc - 2]] = 14.0
    bias[[2, Cc // 2 + 1, Cc - 1]] = -14.0
    return act, w, bias


def lattice_exact(act, w, bias):
    """the exactness condition: operands on their lattices and every partial sum below 2^24 / 1024 in magnitude
    (sum |a| |w| over any subset of a row's terms <= max |a| * the largest weight row's sum |w|)"""
    a, w64, b = np.asarray(act, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    assert (a * 4 == np.rint(a * 4)).all() and (w64 * 256 == np.rint(w64 * 256)).all() and (b * 1024 == np.rint(b * 1024)).all()
    assert np.abs(a).max() <= 1 and np.abs(w64).max() <= 1 / 64
    top = np.abs(a).max() * np.abs(w64).reshape(w64.shape[0], -1).sum(1).max() + np.abs(b).max()
    assert top < 2 ** 24 / 1024, top
    return top


def lattice_expect(layer, chunks, act, w, bias, table):
    """the exact output bits of a lattice case"""
    ref = conv_reference(layer, chunks, act.view(np.uint16), w) + np.asarray(bias, np.float64)[None, :]
    assert (ref == ref.astype(np.float32)).all()
    return gelu_bits(ref.astype(np.float32), table)


def normal_inputs(rng, layer, Cc, chunks):
    """unit-normal activations and weights scaled for outputs of order 1"""
    act = ku.f16_normal(rng, (total_rows(layer - 1, chunks), Cc))
    w = ku.f16_normal(rng, (Cc, Cc, 3, 3), (9 * Cc) ** -0.5)
    return act, w, rng.standard_normal(Cc).astype(np.float32)


def normal_expect(layer, chunks, act, w, bias):
    """(float64 pre-activation, bound): K fp32 additions over the padded row length, one more for the bias"""
    ref, mag = conv_reference(layer, chunks, act, w, True)
    return ku.add_terms(ref, ku.dense_bound(conv_kpad(w.shape[1]), mag), np.asarray(bias, np.float64)[None, :])


# --------------------------------------------------------------- comparators
def check_exact(out_bits, want_bits, what="conv"):
    if not np.array_equal(out_bits, want_bits):
        bad = out_bits != want_bits
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} outputs differ from the exact reference, first (row, channel) {i}: "
                             f"got {int(out_bits[i]):#06x} want {int(want_bits[i]):#06x}")


def gelu_error_over_bound(out_bits, table, ref, bound):
    """a figure for the record (ku.check_gelu is the assertion and has passed): per output, the distance from the
    reference to the nearest pre-activation that rounds to an fp16 h with table[h] == out (past the clamps: h
    itself, or any h <= -10 for 0), over the bound; the largest of them.  The nearest such h on either side of the
    reference is found by one search in the (table value, h in value order) pairs, as check_gelu finds its own"""
    allh = np.arange(65536, dtype=np.uint16)
    finite = (allh & 0x7C00) != 0x7C00
    keys = np.sort(table[finite].astype(np.int64) * (1 << 17) + (ku._f16_index(allh[finite].view(np.float16)) + 32768))
    out_bits = np.ascontiguousarray(out_bits)
    want = out_bits.astype(np.int64) * (1 << 17)
    pos = np.searchsorted(keys, want + ku._f16_index(ref.astype(np.float16)) + 32768)

    def gap(h):
        return np.maximum(np.abs(h - ref) - 0.5 * ku.ulp16(h), 0.0)
    best = np.full(ref.shape, np.inf)
    for p in (pos - 1, pos):
        k = keys[np.clip(p, 0, len(keys) - 1)]
        h = ku._f16_from_index((k & 0x1FFFF) - 32768).astype(np.float64)
        best = np.where((k >> 17) == out_bits, np.minimum(best, gap(h)), best)
    ov = out_bits.view(np.float16).astype(np.float64)
    best = np.where(ov >= 10.0, np.minimum(best, gap(ov)), best)
    best = np.where((out_bits == 0) & (ref - bound <= -10.0), 0.0, best)
    return float((best / np.maximum(bound, 1e-300)).max())


# ---------------------------------------------------------------- GPU cases
# (layer, C, chunk lengths, tag, regs_staged twin's tag or None, normal family too)
HUNDREDS = (100,) * 8 + (97, 57, 100)
CASES = [
    (2, 64, (1, 2, 7, 57), "gemm<64,64,1>", None, True),
    (2, 96, (100, 97, 57, 1), "gemm<64,96,3>", None, True),                 # W1 = 49 and 29: odd
    (2, 96, (100,) * 5 + (97,), "gemm<128,96,3>", None, True),              # 4800 rows
    (2, 480, (97, 57), "glds<64,480,1,2,2>", "gemm<64,480,1>", True),
    (2, 480, (100, 97, 57, 100), "gemm8p", "gemm<64,480,1>", True),         # 2880 rows: shifted last row and column tiles
    (2, 256, (100, 97, 57, 100), "gemm8p", None, False),                    # no column shift, no K padding
    (3, 64, (1, 2, 7, 57), "gemm<64,64,1>", None, True),                    # W3 = 1, W2 = 15
    (3, 96, (100, 97, 57, 1), "gemm<64,96,3>", None, True),                 # W2 = 25 and 15: odd
    (3, 96, (100,) * 19 + (97,), "gemm<128,96,3>", None, True),             # 4160 rows
    (3, 480, (97, 57), "glds<64,480,1,2,2>", "gemm<64,480,1>", True),
    (3, 480, HUNDREDS, "gemm8p", "gemm<64,480,1>", True),                   # 2208 rows
    (3, 256, HUNDREDS, "gemm8p", None, False),
]
CONV1_CLIPS = (257, 1, 2, ("al", 37), ("whole", 257))


def case_id(case):
    return f"conv{case[0]}-C{case[1]}-{len(case[2])}x-{case[3]}"


def case_rng(case):
    return np.random.default_rng([case[0], case[1], len(case[2]), sum(case[2])])
