"""The comparators of tests/kernel_util.py are sharp (CPU only): fed the float64
reference itself, rounded as a correct kernel would, they accept; fed the same
output with one defect a subtly wrong kernel would produce, they reject.  This is
the evidence that tests/test_gpu_kernels.py fails on such a kernel."""
import numpy as np
import pytest

import kernel_util as ku

G = ku.GUARD
M, N, K = 40, 64, 128


def _alloc(body, ld, dtype):
    """a harness output allocation around `body`: sentinel guard rows and padding columns"""
    raw = np.full((body.shape[0] + 2 * G, ld), np.iinfo(ku._SENT[np.dtype(dtype).itemsize]).max,
                  ku._SENT[np.dtype(dtype).itemsize])
    raw[G:G + body.shape[0], :body.shape[1]] = np.ascontiguousarray(body).view(raw.dtype)
    return raw.view(dtype)


@pytest.fixture(scope="module")
def dense():
    rng = np.random.default_rng(7)
    A = ku.f16_normal(rng, (M, K))
    W = ku.f16_normal(rng, (N, K), K ** -0.5)
    ref, mag = ku.dense_terms(A, W)
    return A, W, ref, ku.dense_bound(K, mag)


def _check_f32(buf, ref, bound):
    return ku.check_values(ku.in_range(buf, M, N), ref, bound)


def test_clean_reference_is_accepted(dense):
    A, W, ref, bound = dense
    assert _check_f32(_alloc(ref.astype(np.float32), N + 4, np.float32), ref, bound) <= 1.0
    h = ref.astype(np.float32).astype(np.float16)
    assert ku.check_values(ku.in_range(_alloc(h, N + 4, np.uint16), M, N), ref, bound, fp16=True) <= 1.0


def test_missing_k_slab_in_one_tile_is_rejected(dense):
    A, W, ref, bound = dense
    a, w = A.astype(np.float64), W.astype(np.float64)
    out = ref.copy()
    out[16:32, 32:48] -= a[16:32, 64:96] @ w[32:48, 64:96].T   # one 32-wide slab of one 16 x 16 tile
    with pytest.raises(AssertionError, match="outside the bound"):
        _check_f32(_alloc(out.astype(np.float32), N + 4, np.float32), ref, bound)


def test_swapped_rows_in_one_tile_are_rejected(dense):
    A, W, ref, bound = dense
    out = ref.copy()
    out[[17, 18], 16:32] = out[[18, 17], 16:32]
    with pytest.raises(AssertionError, match="outside the bound"):
        _check_f32(_alloc(out.astype(np.float32), N + 4, np.float32), ref, bound)


def test_unwritten_element_is_rejected(dense):
    A, W, ref, bound = dense
    buf = _alloc(ref.astype(np.float32), N + 4, np.float32)
    buf.view(np.uint32)[G + 5, 9] = 0xFFFFFFFF
    with pytest.raises(AssertionError, match="never written"):
        _check_f32(buf, ref, bound)
    b16 = _alloc(ref.astype(np.float32).astype(np.float16), N + 4, np.uint16)
    b16[G + M - 1, N - 1] = 0xFFFF
    with pytest.raises(AssertionError, match="never written"):
        ku.in_range(b16, M, N)


def test_overwritten_padding_or_guard_is_rejected(dense):
    A, W, ref, bound = dense
    buf = _alloc(ref.astype(np.float32), N + 4, np.float32)
    buf[G + 3, N] = 0.0
    with pytest.raises(AssertionError, match="padding columns"):
        _check_f32(buf, ref, bound)
    for row, what in ((G - 1, "before"), (G + M, "after")):
        buf = _alloc(ref.astype(np.float32), N + 4, np.float32)
        buf[row, 0] = 1.0
        with pytest.raises(AssertionError, match=what):
            _check_f32(buf, ref, bound)
    with pytest.raises(AssertionError, match="declined"):
        ku.untouched(buf)


def test_argmax_off_by_one_on_a_tie_is_rejected():
    rng = np.random.default_rng(8)
    logits = rng.standard_normal((4, 64)).astype(np.float32)
    logits[2, [10, 11, 26, 42]] = 9.0   # a tie: the lowest column wins
    want = np.argmax(logits, 1)
    assert want[2] == 10
    ku.check_argmax(want, logits)
    wrong = want.copy()
    wrong[2] = 11
    with pytest.raises(AssertionError):
        ku.check_argmax(wrong, logits)
    # padded columns holding the largest values never win
    logits[1, 60:] = 50.0
    ku.check_argmax(np.argmax(logits[:, :60], 1), logits, n_valid=60)
    with pytest.raises(AssertionError):
        ku.check_argmax(np.argmax(logits, 1), logits, n_valid=60)
    # the key packing of csrc/dev_common.h argmax_key
    v = np.array([-1.5, 0.0, 3.25], np.float32)
    u = v.view(np.uint32)
    enc = np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    keys = (enc << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.array([5, 0, 151935], np.uint64))
    assert list(ku.key_index(keys)) == [5, 0, 151935] and np.array_equal(ku.key_value(keys), v)
    assert keys[2] > keys[1] > keys[0]


def test_gelu_two_table_indices_away_is_rejected(dense):
    A, W, ref, bound = dense
    rng = np.random.default_rng(9)
    table = rng.integers(0, 0x7BFF, 65536).astype(np.uint16)   # any injective-enough table serves the comparator
    pre, bound = ku.add_terms(ref, bound, np.linspace(-14, 14, N)[None, :])   # both clamps and the table
    h = pre.astype(np.float32).astype(np.float16)
    out = table[h.view(np.uint16)]
    x = pre.astype(np.float32)
    out = np.where(x >= 10, h.view(np.uint16), np.where(x <= -10, 0, out)).astype(np.uint16)
    assert (x >= 10).any() and (x <= -10).any() and (np.abs(x) < 10).any()
    ku.check_gelu(out, table, pre, bound)
    # where an fp16 ulp is far above the bound (|x| >= 1) the set is one value, or two at a rounding boundary
    big = np.abs(x) >= 1
    assert ku.check_gelu(out[big], table, pre[big], bound[big]) <= 2
    i = tuple(np.argwhere(big & (np.abs(x) < 5))[3])
    bad = out.copy()
    two_away = ku._f16_from_index(ku._f16_index(np.array([h[i]])) + 2)
    bad[i] = table[two_away.view(np.uint16)[0]]
    assert bad[i] != out[i]
    with pytest.raises(AssertionError, match="outside the table set"):
        ku.check_gelu(bad, table, pre, bound)
    # past the clamp, the table value is no longer acceptable where it differs from fp16(x)
    j = tuple(np.argwhere(x >= 11)[0])
    bad = out.copy()
    bad[j] = 0
    with pytest.raises(AssertionError, match="outside the table set"):
        ku.check_gelu(bad, table, pre, bound)


def test_q8_quant_off_by_one_is_rejected():
    rng = np.random.default_rng(10)
    v = rng.standard_normal((5, 96)).astype(np.float32)
    v[3, 32:64] = 0.0   # an all-zero block: scale 0, quants 0
    q, d = ku.q8_quantize(v)
    assert d[3, 1] == 0 and not q[3, 32:64].any() and np.abs(q).max() == 127
    # d = fp16(amax / 127): the documented definition, restated independently per block
    for r, b in ((0, 0), (4, 2)):
        blk = v[r, 32 * b:32 * b + 32]
        am = np.abs(blk).max()
        assert d[r, b] == np.float32(np.float16(am / np.float32(127)))
        assert np.array_equal(q[r, 32 * b:32 * b + 32], np.rint(blk * (np.float32(127) / am)).astype(np.int8))
    ku.check_q8(q, d, q.copy(), d.copy())
    bad = q.copy()
    bad[2, 17] += 1 if bad[2, 17] < 127 else -1
    with pytest.raises(AssertionError, match="quants differ"):
        ku.check_q8(bad, d, q, d)
    dbad = d.copy()
    dbad.view(np.uint32)[1, 1] += 1 << 13   # one fp16 ulp
    with pytest.raises(AssertionError, match="scales differ"):
        ku.check_q8(q, dbad, q, d)


def test_q8_product_reference_and_missing_block():
    rng = np.random.default_rng(11)
    Aq, Ad = ku.q8_operand(rng, 9, 96, np.float32)
    Wq, Wd = ku.q8_operand(rng, 64, 96, np.float16, 0.02)
    ref, mag = ku.q8_terms(Aq, Ad, Wq, Wd)
    deq = (Aq.reshape(9, 3, 32) * Ad[:, :, None].astype(np.float64)).reshape(9, 96) @ \
          (Wq.reshape(64, 3, 32) * Wd[:, :, None].astype(np.float64)).reshape(64, 96).T
    assert np.abs(ref - deq).max() <= 1e-12 * mag.max()
    bound = ku.q8_bound(96, mag)
    buf = _alloc(ref.astype(np.float32), 68, np.float32)
    assert ku.check_values(ku.in_range(buf, 9, 64), ref, bound) <= 1.0
    out = ref.copy()
    blk = Aq[:, 32:64].astype(np.float64) @ Wq[:, 32:64].astype(np.float64).T
    out[4, 7] -= Ad[4, 1] * float(Wd[7, 1]) * blk[4, 7]
    if blk[4, 7] != 0:
        with pytest.raises(AssertionError, match="outside the bound"):
            ku.check_values(ku.in_range(_alloc(out.astype(np.float32), 68, np.float32), 9, 64), ref, bound)


def test_gemv_last_column_group_shifted_is_rejected():
    rng = np.random.default_rng(12)
    Mv, Nv, Kv, CPW = 2, 2050, 256, 2
    x = ku.f16_normal(rng, (Mv, Kv))
    W = ku.f16_normal(rng, (Nv, Kv), Kv ** -0.5)
    ref, mag = ku.dense_terms(x, W)
    bound = ku.dense_bound(Kv, mag)
    buf = _alloc(ref.astype(np.float32), Nv + 4, np.float32)
    assert ku.check_values(ku.in_range(buf, Mv, Nv), ref, bound) <= 1.0
    out = ref.copy()
    out[:, Nv - CPW:] = ref[:, Nv - 2 * CPW:Nv - CPW]   # the last group computed from the group before it
    with pytest.raises(AssertionError, match="outside the bound"):
        ku.check_values(ku.in_range(_alloc(out.astype(np.float32), Nv + 4, np.float32), Mv, Nv), ref, bound)


def test_swiglu_layout_and_bound():
    gate, up = ku.swiglu_rows(48)
    assert list(gate[:3]) == [0, 1, 2] and gate[15] == 15 and gate[16] == 32 and up[0] == 16 and up[47] == 95
    assert sorted(np.concatenate([gate, up])) == list(range(96))
    g, u = np.array([[-3.0, 0.5, 8.0]]), np.array([[2.0, -1.0, 0.25]])
    v, bv = ku.swiglu_terms(g, np.full_like(g, 1e-6), u, np.full_like(u, 1e-6))
    # the propagated bound covers moving both dot products to the ends of their intervals
    for dg in (-1e-6, 1e-6):
        for du in (-1e-6, 1e-6):
            assert (np.abs(ku.silu(g + dg) * (u + du) - v) <= bv).all()
    assert (bv < 1e-5).all()


def test_rms_prologue_tie_mask():
    rng = np.random.default_rng(13)
    x = ku.f16_normal(rng, (3, 256)).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(256)).astype(np.float32)
    h, v, tie = ku.rms_prologue(x, w, 1e-6)
    assert h.dtype == np.float16 and v.dtype == np.float32
    assert np.allclose((v.astype(np.float64) / w) ** 2 @ np.ones(256) / 256, 1.0, rtol=1e-4)   # unit mean square
    assert tie.mean() <= 0.01
    # an exact midpoint between two fp16 values is a tie; one 2^-18 relative off it is not
    s = ku.ulp16(np.array([1.0]))[0]
    mid = np.array([1.0 + s / 2, (1.0 + s / 2) * (1 + 2.0 ** -18)])
    frac = np.mod(mid / ku.ulp16(mid), 1.0)
    assert list(np.abs(frac - 0.5) * ku.ulp16(mid) <= 2.0 ** -20 * mid) == [True, False]
