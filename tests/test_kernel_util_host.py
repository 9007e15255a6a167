"""The comparators of tests/kernel_util.py are sharp (CPU only): fed the float64
reference itself, rounded as a correct kernel would, they accept; fed the same
output with one defect a subtly wrong kernel would produce, they reject.  This is
the evidence that tests/test_gpu_kernels.py fails on such a kernel."""
import numpy as np
import pytest

import conv_util as cu
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


# ------------------------------------------------- tests/attn_util.py: norms, RoPE, attention
# On the inputs of the smallest GPU case of each family (tests/test_gpu_attn_kernels.py): the reference itself is
# accepted, the reference with one planted defect is rejected.
import attn_util as au   # noqa: E402
import decode_attn_util as du   # noqa: E402


def _enc_small(f32_mfma):
    case = au.enc_case(1)
    return (case,) + au.enc_reference(case, f32_mfma)


@pytest.mark.parametrize("f32_mfma", [False, True])
@pytest.mark.parametrize("fp16", [False, True])
def test_enc_attention_defects_are_rejected(f32_mfma, fp16):
    case, ref, bound, valid = _enc_small(f32_mfma)
    assert au.check_rows(au.fake_output(ref, valid, fp16), valid, ref, bound, fp16, "clean") <= 1.0
    starts, lens = case["seg_start"], case["seg_len"]

    def drop_tile_last(i):   # the last key of the first 64-key tile
        own = np.arange(starts[i], starts[i] + lens[i])
        return np.delete(own, 63) if lens[i] >= 64 else own

    def neighbour(i):        # the segment before's last row (the first segment: the next one's first row)
        own = np.arange(starts[i], starts[i] + lens[i])
        other = starts[i] - 2 if starts[i] >= 2 else starts[i] + lens[i] + 1
        return np.append(own, other)
    for keys_of in (drop_tile_last, neighbour):
        bad = au.enc_reference(case, f32_mfma, keys_of)[0]
        with pytest.raises(AssertionError, match="outside the bound"):
            au.check_rows(au.fake_output(bad, valid, fp16), valid, ref, bound, fp16, keys_of.__name__)
    # a row between two segments written, a segment's element left unwritten
    buf = au.fake_output(ref, valid, fp16)
    buf.view(np.uint16 if fp16 else np.uint32)[au.GUARD + int(np.argwhere(~valid)[0, 0]), 3] = 0
    with pytest.raises(AssertionError, match="outside every segment"):
        au.check_rows(buf, valid, ref, bound, fp16, "gap")
    buf = au.fake_output(ref, valid, fp16)
    buf.view(np.uint16 if fp16 else np.uint32)[au.GUARD + int(np.argwhere(valid)[-1, 0]), 63] = 0xFFFF if fp16 else 0xFFFFFFFF
    with pytest.raises(AssertionError, match="never written"):
        au.check_rows(buf, valid, ref, bound, fp16, "hole")


@pytest.mark.parametrize("fp16", [False, True])
def test_prefill_causal_limit_off_by_one_after_a_cached_prefix_is_rejected(fp16):
    case = au.prefill_case(2, 1, au.PREFILL_CACHED, 11, False)
    valid = au.prefill_valid(case)
    ref, bound = au.prefill_reference(case)
    assert au.check_rows(au.fake_output(ref, valid, fp16), valid, ref, bound, fp16, "clean") <= 1.0
    for kw in (dict(limit_shift=1), dict(limit_shift=-1), dict(drop_key=63)):
        bad = au.prefill_reference(case, **kw)[0]
        with pytest.raises(AssertionError, match="outside the bound"):
            au.check_rows(au.fake_output(bad, valid, fp16), valid, ref, bound, fp16, str(kw))


@pytest.mark.parametrize("fp16", [False, True])
def test_exact_chain_defects_are_rejected(fp16):
    case = au.prefill_case(2, 1, au.PREFILL_CACHED, au.EXACT_SEED_CACHED, True)
    chain = au.exact_chain(case)
    valid = au.prefill_valid(case)
    ratio, share = au.check_exact(au.fake_output(chain[0], valid, fp16), case, chain, fp16, "clean")
    assert ratio <= 1.0 and 0 < share <= 0.05
    for kw in (dict(limit_shift=1), dict(limit_shift=-1), dict(drop_key=63)):
        bad = au.exact_chain(case, **kw)[0]
        with pytest.raises(AssertionError, match="outside the bound"):
            au.check_exact(au.fake_output(bad, valid, fp16), case, chain, fp16, str(kw))
    # one fp16 ulp of the accumulator on an element that is no near-tie (fp32 output: the chain's own bits)
    if not fp16:
        ref, tie, step, rel = chain
        r, c = np.argwhere(valid[:, None] & ~tie & (np.abs(ref) > 0.05))[7]
        bad = ref.copy()
        bad[r, c] += step[r, c]
        with pytest.raises(AssertionError, match="outside the bound"):
            au.check_exact(au.fake_output(bad, valid, False), case, chain, False, "one ulp")
    # a case whose elements are mostly near-ties no longer tests the chain's bits
    with pytest.raises(AssertionError, match="near-ties"):
        au.check_exact(au.fake_output(chain[0], valid, fp16), case, (chain[0], np.ones_like(chain[1]), chain[2], chain[3]), fp16, "cap")


def test_qkv_post_defects_are_rejected():
    case = au.qkv_case(2, 1, 3)
    q, bq, k, bk, v = au.qkv_post_ref(case)
    q_bad, _, k_bad, _, _ = au.qkv_post_ref(case, pair_adjacent=True)   # the rotation's pair (i, i + 64) taken as (i, i + 1)
    assert ku.check_values(q.astype(np.float32), q, bq) <= 1.0
    assert ku.check_values(q.astype(np.float32).astype(np.float16).view(np.uint16), q, bq, fp16=True) <= 1.0
    for fp16 in (False, True):
        for good, bad, bound in ((q, q_bad, bq), (k, k_bad, bk)):
            out = bad.astype(np.float32)
            with pytest.raises(AssertionError, match="outside the bound"):
                ku.check_values(out.astype(np.float16).view(np.uint16) if fp16 else out, good, bound, fp16=fp16)
    # the caches: a row at a neighbouring position, two keys swapped inside a V^T 8-key block
    want = au.vt_expected(case, v)
    au.check_vt(want.copy(), want)
    n = 128 * au.vt_ctx(case["max_ctx"])
    d = np.arange(128)
    assert (case["row_seq"][0], case["row_pos"][0]) == (2, 7)
    base = (2 * case["n_kv_head"] + 0) * n
    bad = want.copy()
    bad[base + au.vt_index(7, d)], bad[base + au.vt_index(6, d)] = want[base + au.vt_index(6, d)], want[base + au.vt_index(7, d)]
    with pytest.raises(AssertionError, match="vt:"):
        au.check_vt(bad, want)
    cache = np.full((case["slots"], case["n_kv_head"], case["max_ctx"], 128), 0xFFFF, np.uint16)
    cache[case["row_seq"], :, case["row_pos"]] = k.astype(np.float32).astype(np.float16).view(np.uint16).reshape(3, 1, 128)
    assert au.check_cache_rows(cache.reshape(-1), case, k, bk, "kc") <= 1.0
    moved = cache.copy()
    moved[2, :, 6], moved[2, :, 7] = cache[2, :, 7], cache[2, :, 6]
    with pytest.raises(AssertionError, match="outside"):
        au.check_cache_rows(moved.reshape(-1), case, k, bk, "kc")


def test_layernorm_one_pass_variance_is_rejected():
    rng = np.random.default_rng([256, 1])
    D = 256
    w = (1 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    x = au.norm_rows(rng, 5, D)   # row 1: mean 50 x its spread
    ref, bound = au.layernorm_ref(x, w, b, 1e-5)
    assert ku.check_values(ref.astype(np.float32), ref, bound) <= 1.0
    bad = au.layernorm_one_pass(x, w, b, 1e-5)
    assert np.abs(bad[0] - ref[0]).max() < 1e-5   # an ordinary row hides it
    with pytest.raises(AssertionError, match="outside the bound"):
        ku.check_values(bad[1:2], ref[1:2], bound[1:2])
    # RMSNorm: the restatement's bits, and one fp16 ulp off outside the near-tie mask
    xr = au.norm_rows(rng, 5, D)
    h, v, tie = ku.rms_prologue(xr, w, 1e-6)
    assert au.check_rms_bits(h.view(np.uint16), xr, w, 1e-6) <= 0.01
    r, c = np.argwhere(~tie & (np.abs(v) > 0.1))[0]
    off = h.copy()
    off[r, c] = ku._f16_from_index(ku._f16_index(h[r:r + 1, c:c + 1]) + 1)[0, 0]
    with pytest.raises(AssertionError, match="restatement"):
        au.check_rms_bits(off.view(np.uint16), xr, w, 1e-6)


def test_exact_chain_mask_covers_an_expf_one_ulp_off(monkeypatch):
    """what the near-tie mask is for: a device expf within 1 ulp of the restatement's may change marked elements
    only, and those by no more than their slack"""
    case = au.prefill_case(2, 1, au.PREFILL_CACHED, au.EXACT_SEED_CACHED, True)
    chain = au.exact_chain(case)
    valid = au.prefill_valid(case)
    exact = au._expf
    for step in (np.inf, -np.inf):
        def off_by_one(x, step=step):
            y = exact(x)
            return np.where(np.asarray(x) == 0, y, np.nextafter(y, np.float32(step))).astype(np.float32)   # (expf(0) is 1 anywhere)
        monkeypatch.setattr(au, "_expf", off_by_one)
        dev = au.exact_chain(case)[0]
        monkeypatch.setattr(au, "_expf", exact)
        moved = np.abs(dev - chain[0]) > 1e-12 * np.abs(chain[0])
        assert moved[valid].any() and not (moved & ~chain[1])[valid].any()
        assert au.check_exact(au.fake_output(dev, valid, False), case, chain, False, "expf off by one")[0] <= 1.0


# ======================================================= decode attention
DEC_POS = (0, 1, 15, 16, 31, 32, 33, 62, 64, 129)   # the smallest GPU cases' lengths: one split, a seam, three chunks


def test_decode_lattice_family_is_exact_and_under_the_mask_cap():
    """the float32 restatement of the norm and rotation gives the float64 reference's q and k, the fp32 score sums
    are exact (asserted inside lattice_scores), and the restatement alone keeps its near-tie share under the cap for
    every lattice case and seed the GPU file uses"""
    for pos, ctx, wmax in (((0, 30, 31, 32, 62, 63, 64, 129), 320, 12), ((0, 30, 31, 32, 62, 63, 64, 129, 257), 320, 12),
                           ((2046, 2047), 2112, 32), ((2048, 32), 2112, 32), ((2048, 2047, 2046, 64, 63, 0, 1, 500, 1000), 2112, 32)):
        case = du.decode_case(pos, 1, ctx, du.LATTICE_SEED, True, wmax=wmax)
        s = du.lattice_scores(case)
        assert np.array_equal(s[~np.isnan(s)].astype(np.float32).astype(np.float64), s[~np.isnan(s)])
        chain = du.lattice_chain(case)
        assert 0 < chain[1].mean() <= 0.05, (pos, chain[1].mean())
    for rise in ("late", "early"):
        case = du.chain_case((2048, 2047), 2, 1, 2112, du.CHAIN_SEED, rise, 4.0)
        assert du.chain_case_reference(case)[1].mean() <= 0.05
        s = case["scores_in"][0, :, :2049]
        first = np.argmax(s, 1)
        assert (first == (2048 if rise == "late" else 5)).all()   # the maximum rises in the second weights chunk / never there
    for ratio, nkv in ((2, 1), (3, 1), (4, 2), (1, 1)):
        case = du.chain_case((0, 30, 31, 32, 62, 63, 64), ratio, nkv, 96, du.CHAIN_SEED)
        assert du.chain_case_reference(case)[1].mean() <= 0.05


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("spl", [64, 0])
def test_decode_reference_defects_are_rejected(fp16, spl):
    case = du.decode_case(DEC_POS, 1, 320, 11)
    gs = 3
    ref, bound = du.decode_reference(case, spl, gs)
    B, QD = ref.shape
    clean = ku.in_range(du.fake(ref, fp16), B, QD)
    assert ku.check_values(clean, ref, bound, fp16=fp16) <= 1.0
    assert np.abs(ref).max() < 100   # the junk of row pos is nowhere in it
    for defect in ("stale", "drop_last_split", "empty_split", "seam_twice", "next_key"):
        bad = du.decode_reference(case, spl, gs, defect)[0]
        with pytest.raises(AssertionError, match="outside the bound|NaN in range"):
            ku.check_values(ku.in_range(du.fake(bad, fp16), B, QD), ref, bound, fp16=fp16, what=defect)


@pytest.mark.parametrize("fp16", [False, True])
def test_decode_chain_defects_are_rejected(fp16):
    case = du.decode_case(DEC_POS[:8] + (64, 129), 1, 320, du.LATTICE_SEED, True)
    chain = du.lattice_chain(case)
    ratio, share = du.check_chain(du.fake(chain[0], fp16), chain, fp16, "clean")
    assert ratio <= 1.0 and 0 < share <= 0.05
    bad = du.lattice_chain(case, vshift=8)[0]   # the V^T block taken as (k >> 3) + 1
    with pytest.raises(AssertionError, match="outside the bound"):
        du.check_chain(du.fake(bad, fp16), chain, fp16, "vt block")
    # one fp16 ulp of the accumulator on an element that is no near-tie (fp32 output: the chain's own bits)
    if not fp16:
        ref, tie, step, rel = chain
        r, c = np.argwhere(~tie & (np.abs(ref) > 0.05))[7]
        off = ref.copy()
        off[r, c] += step[r, c]
        with pytest.raises(AssertionError, match="outside the bound"):
            du.check_chain(du.fake(off, False), chain, False, "one ulp")
    with pytest.raises(AssertionError, match="near-ties"):
        du.check_chain(du.fake(chain[0], fp16), (chain[0], np.ones_like(chain[1]), chain[2], chain[3]), fp16, "cap")


def test_decode_chain_missed_rescale_in_the_second_weights_chunk_is_rejected():
    case = du.chain_case((2048, 2047), 2, 1, 2112, du.CHAIN_SEED, "late", 4.0)
    chain = du.chain_case_reference(case)
    assert du.check_chain(du.fake(chain[0]), chain, False, "clean")[0] <= 1.0
    bad = du.chain_case_reference(case, skip_rescale_from=2048)[0]
    assert np.array_equal(bad[1], chain[0][1])   # 2048 keys: one chunk, untouched
    with pytest.raises(AssertionError, match="outside the bound"):
        du.check_chain(du.fake(bad), chain, False, "no rescale")


def test_decode_chain_mask_covers_an_expf_one_ulp_off():
    case = du.decode_case(DEC_POS[:8] + (64, 129), 1, 320, du.LATTICE_SEED, True)
    chain = du.lattice_chain(case)
    exact = au._expf
    for step in (np.inf, -np.inf):
        def off_by_one(x, step=step):
            y = exact(x)
            return np.where(np.asarray(x) == 0, y, np.nextafter(y, np.float32(step))).astype(np.float32)   # (expf(0) is 1 anywhere)
        dev = du.lattice_chain(case, expf=off_by_one)[0]
        moved = np.abs(dev - chain[0]) > 1e-12 * np.abs(chain[0])
        assert moved.any() and not (moved & ~chain[1]).any()
        assert du.check_chain(du.fake(dev), chain, False, "expf off by one")[0] <= 1.0


# ================================================================ conv front end


def _conv_table(seed):
    """a stand-in GELU table: any injective-enough table serves an exact comparator; NaN inputs give NaN as the real one"""
    t = np.random.default_rng(seed).integers(0, 0x7BFF, 65536).astype(np.uint16)
    idx = np.arange(65536)
    t[((idx & 0x7C00) == 0x7C00) & ((idx & 0x3FF) != 0)] = 0x7E00
    return t


def _guarded(a, g):
    out = np.full((a.shape[0] + 2 * g,) + a.shape[1:], np.nan)
    out[g:g + a.shape[0]] = a
    return out


def gather_conv(layer, chunks, act, wdev, bias, table, defect=None):
    """conv2 / conv3 as the device computes them -- an im2col row per output row, gathered from the NHWC row table by
    the address base + ih * Win + iw, times the packed weights -- with one planted defect.  The input sits between
    guard rows of NaN as in the harness"""
    Cc, Hin = act.shape[1], 64 if layer == 2 else 32
    gin = max(c[cu.WIDTH[layer - 1]] for c in chunks) + 1
    a = _guarded(act.astype(np.float64), gin)
    w = wdev[:, :9 * Cc].astype(np.float64)
    # the output-row table the chunk search reads, and each output row's chunk: the largest c with row_start[c] <= row
    row_start = np.array([ch[cu.ROW[layer]] for ch in chunks])
    if defect == "row_start":
        row_start[1] += 1
    row = np.arange(cu.total_rows(layer, chunks))
    c = np.searchsorted(row_start, row, side="right") - 1
    local = row - row_start[c]
    Wout, Win = (np.array([ch[cu.WIDTH[l]] for ch in chunks])[c] for l in (layer, layer - 1))
    base = np.array([ch[cu.ROW[layer - 1]] for ch in chunks])[c] + (1 if defect == "in_base" else 0) * (c == 1)
    if layer == 2 or defect == "row_order":
        oh, ow = local // Wout, local % Wout
    else:
        oh, ow = local % 16, local // 16
    oy, ox = (2 * oh, 2 * ow) if defect == "origin" else (2 * oh - 1, 2 * ow - 1)
    A = np.zeros((len(row), 9, Cc))
    for kh in range(3):
        for kw in range(3):
            ih, iw = oy + kh, ox + kw
            ok = ((ih >= 0) | (defect == "top")) & (ih < Hin) & (iw >= 0) & ((iw < Win) | (defect == "right"))
            A[:, kh * 3 + kw] = np.where(ok[:, None], a[np.clip(base + ih * Win + iw + gin, 0, len(a) - 1)], 0.0)
    if defect == "k_order":
        A = A.transpose(0, 2, 1)
    out = A.reshape(len(row), 9 * Cc) @ w.T
    return cu.gelu_bits((out + bias[None, :].astype(np.float64)).astype(np.float32), table)


def gather_conv1(chunks, mel, w9, bias, table, defect=None):
    """conv1 as the device computes it (one tap per (row, t), mel[mel_off + ih * T + iw]) with one planted defect"""
    g = max(max(c["T"], c["L"]) for c in chunks) + 1
    h = _guarded(mel.astype(np.float16).astype(np.float64), g)
    w64 = w9.astype(np.float64)
    out = np.zeros((cu.total_rows(1, chunks), w9.shape[0]), np.uint16)
    for ch in chunks:
        local = np.arange(64 * ch["W1"])
        oh, ow = local // ch["W1"], local % ch["W1"]
        sd = np.zeros((len(local), w9.shape[0]))
        for t in range(9):
            ih, iw = 2 * oh - 1 + t // 3, 2 * ow - 1 + t % 3
            ok = (ih >= 0) & (ih < 128) & ((iw >= 0) | (defect == "left" and ch["start"] > 0)) & (iw < (ch["L"] if defect == "lv" else ch["Lv"]))
            tap = np.where(ok, h[np.clip(ch["mel_off"] + ih * ch["T"] + iw + g, 0, len(h) - 1)], 0.0)
            sd = sd + tap[:, None] * w64[None, :, t]
        cu.chunk_rows(1, ch, out)[:] = cu.gelu_bits(sd.astype(np.float32) + bias[None, :], table)
    return out


def _conv_compare(bits, want, what):
    rows, Cc = want.shape
    cu.check_exact(ku.in_range(_alloc(bits, Cc, np.uint16), rows, Cc, what), want, what)


def test_conv1_reference_defects_are_rejected():
    """the smallest conv1 GPU case's inputs: the device-style gather gives the reference's bits; chunk 2's left tap
    reading the chunk before, or frames past Lv read from the mel, do not"""
    Cc = 96
    rng = np.random.default_rng(Cc)
    chunks = cu.make_chunks(cu.CONV1_CLIPS)
    mel = (rng.standard_normal(cu.mel_len(chunks)) * 0.7 + 0.3).astype(np.float32)
    w = ku.f16_normal(rng, (Cc, 1, 3, 3), 0.5)
    bias = rng.standard_normal(Cc).astype(np.float32)
    table = _conv_table(1)
    want = cu.conv1_reference(chunks, mel, w, bias, table)
    _conv_compare(gather_conv1(chunks, mel, w.reshape(Cc, 9), bias, table), want, "clean")
    for defect in ("left", "lv"):
        bad = gather_conv1(chunks, mel, w.reshape(Cc, 9), bias, table, defect)
        with pytest.raises(AssertionError, match="differ from the exact reference"):
            _conv_compare(bad, want, defect)


@pytest.mark.parametrize("layer", [2, 3])
def test_conv_gemm_reference_defects_are_rejected(layer):
    """the smallest conv2 / conv3 GPU case's lattice inputs: the device-style gather gives the reference's bits; a
    right pad tap of an odd width read from the next image row, ih = -1 read from the rows before, a stride origin
    of 2 o, K ordered (ic, tap), one chunk's row_start (the output-row table of the chunk search) off by one row, one
    chunk's first input row off by one and (conv3) rows ordered (oh, ow) do not"""
    case = next(c for c in cu.CASES if c[0] == layer)
    Cc, chunks = case[1], cu.make_chunks(case[2])
    assert any(c[cu.WIDTH[layer - 1]] % 2 == 1 and c[cu.WIDTH[layer - 1]] > 1 for c in chunks)
    act, w, bias = cu.lattice_inputs(cu.case_rng(case), layer, Cc, chunks)
    table = _conv_table(layer)
    want = cu.lattice_expect(layer, chunks, act, w, bias, table)
    wdev = cu.pack_weights(w, np.nan)
    _conv_compare(gather_conv(layer, chunks, act, wdev, bias, table), want, "clean")
    for defect in ("right", "top", "origin", "k_order", "row_start", "in_base") + (("row_order",) if layer == 3 else ()):
        bad = gather_conv(layer, chunks, act, wdev, bias, table, defect)
        with pytest.raises(AssertionError, match="differ from the exact reference|NaN in range"):
            _conv_compare(bad, want, defect)
    # the normal family's comparator on the same geometry: the clean gather is inside the bound, a right pad tap is not
    act, w, bias = cu.normal_inputs(cu.case_rng(case), layer, Cc, chunks)
    ref, bound = cu.normal_expect(layer, chunks, act, w, bias)
    wdev = cu.pack_weights(w, np.nan)
    ku.check_gelu(gather_conv(layer, chunks, act, wdev, bias, table), table, ref, bound, "clean normal")
    with pytest.raises(AssertionError, match="outside the table set"):
        ku.check_gelu(gather_conv(layer, chunks, act, wdev, bias, table, "right"), table, ref, bound, "right normal")


def test_conv_lattice_is_exact_for_every_gpu_case():
    for case in cu.CASES:
        layer, Cc, lengths = case[:3]
        act, w, bias = cu.lattice_inputs(cu.case_rng(case), layer, Cc, cu.make_chunks(lengths))
        assert cu.lattice_exact(act, w, bias) < 2 ** 14
    # the weight packing against its statement, element by element
    w = ku.f16_normal(np.random.default_rng(3), (8, 16, 3, 3))
    p = cu.pack_weights(w, np.nan)
    assert p.shape == (8, 256) and np.isnan(p[:, 144:]).all()
    for oc, ic, kh, kw in ((0, 0, 0, 0), (7, 15, 2, 2), (3, 5, 1, 2), (4, 9, 2, 0)):
        assert p[oc, (kh * 3 + kw) * 16 + ic] == w[oc, ic, kh, kw]
