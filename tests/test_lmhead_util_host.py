"""No GPU: the references and input constructions of tests/lmhead_util.py against plain float64, and the premises
the adversarial rows of tests/test_gpu_lmhead_kernels.py rest on."""
import numpy as np
import pytest

import kernel_util as ku
import lmhead_util as lu


def plain_lp(row, n_valid, col):
    v = np.asarray(row[:n_valid], np.float64)
    fin = v[np.isfinite(v)]
    return float(v[col] - (fin.max() + np.log(np.exp(fin - fin.max()).sum())))


def test_key_order_is_value_then_lower_column():
    rng = np.random.default_rng(1)
    row = (rng.integers(-3, 4, 500) / 2).astype(np.float32)        # many ties, both signs, +0
    row[[17, 300]] = -np.inf
    row[[5, 400]] = 7.0
    want = np.argsort(-row.astype(np.float64), kind="stable")
    assert np.array_equal(np.argsort(lu.argmax_keys(row))[::-1], want)
    assert lu.topk_order(row, 3).tolist() == [5, 400] + [int(want[2])]
    assert lu.topk_order(row, 8, n_valid=5).tolist() == want[np.isin(want, np.arange(5))].tolist() + [-1] * 3
    keys = lu.argmax_keys(row)
    assert np.array_equal(ku.key_index(keys), np.arange(500)) and np.array_equal(ku.key_value(keys).view(np.uint32), row.view(np.uint32))
    assert (keys > 0).all()                                         # -inf too: 0 is "no key"


def test_expect_rows_and_the_bar():
    rng = np.random.default_rng(2)
    lg = (rng.standard_normal((3, 200)) * 4).astype(np.float32)
    lg[1, :50] = -np.inf
    ids, lps = lu.expect_rows(lg, 4, n_valid=197)
    for b in range(3):
        assert ids[b].tolist() == np.argsort(-lg[b, :197].astype(np.float64), kind="stable")[:4].tolist()
        assert np.allclose(lps[b], [plain_lp(lg[b], 197, i) for i in ids[b]], rtol=0, atol=1e-12)
    ids, lps = lu.expect_rows(lg[1:2, :60], 12)                     # ten finite columns, then -inf ones in column order
    assert ids[0, 10:].tolist() == [0, 1] and np.isneginf(lps[0, 10:]).all() and np.isfinite(lps[0, :10]).all()
    lu.check_lp(np.float32([-1.0, -np.inf]), [-1.0 + 1.9e-5, -np.inf])
    lu.check_lp(np.float32([-220.0]), [-220.0 - 3.2e-5])            # 2e-5 + 2^-24 * 220 = 3.3e-5
    for got, want in (([-1.0], [-1.0 + 2.2e-5]), ([np.nan], [-1.0]), ([-np.inf], [-1.0]), ([-50.0], [-np.inf]), ([-220.0], [-220.0 - 3.5e-5])):
        with pytest.raises(AssertionError):
            lu.check_lp(np.float32(got), want)


@pytest.mark.parametrize("ld,n_valid", [(5000, 4999), (5001, 4998), (700, 700)])
def test_inf_rows_through_the_restated_row_kernel(ld, n_valid):
    """the -inf rows: the restated kernel with the fixed lse_add agrees with plain float64; with lse_add as it was,
    each of them is NaN (the case the GPU module pins), while rows without -inf keep their bits"""
    lg = lu.inf_rows(np.random.default_rng(ld), ld, n_valid)
    th = lu.thread_of(np.arange(ld), ld, n_valid)
    assert set(np.unique(th[:n_valid])) <= set(range(1024)) and (th[n_valid:] == -1).all()
    assert np.isneginf(lg[3, th == 7]).all() and np.isneginf(lg[4, :n_valid]).sum() == n_valid - 1
    for b in range(6):
        col = int(np.argmax(lg[b, :n_valid])) if b % 2 else n_valid - 1 - b
        if np.isneginf(lg[b, col]):
            col = int(np.argmax(lg[b, :n_valid]))
        new, old = lu.row_logprob_np(lg[b], ld, n_valid, col), lu.row_logprob_np(lg[b], ld, n_valid, col, fixed=False)
        assert abs(float(new) - plain_lp(lg[b], n_valid, col)) <= 2e-5, (b, new)
        if 1 <= b <= 4:
            assert np.isnan(old), (b, old)
        else:
            assert old.view(np.uint32) == new.view(np.uint32)
    # a -inf column's own log-probability is -inf, not NaN
    assert np.isneginf(lu.row_logprob_np(lg[1], ld, n_valid, 0))


def test_lse_pairs_with_inf():
    ninf, f = np.float32(-np.inf), np.float32
    assert lu.lse_add_np(ninf, f(0), ninf) == (ninf, 0) and lu.lse_add_np(ninf, f(0), f(2)) == (2, 1)
    assert lu.lse_add_np(f(2), f(1.5), ninf) == (2, 1.5)
    assert np.isnan(lu.lse_add_np(ninf, f(0), ninf, fixed=False)[1])
    assert lu.lse_merge_np(ninf, f(0), ninf, f(0)) == (ninf, 0) and lu.lse_merge_np(ninf, f(0), f(1), f(3)) == (1, 3)
    assert lu.lse_merge_np(f(1), f(3), ninf, f(0)) == (1, 3)


def test_pressure_row_fills_the_candidate_list_without_overflowing_it():
    row = lu.pressure_row()
    n = lu.PRESSURE_N
    assert n % 4096 == 0 and 8 * (n // 1024 + 8) == lu.TOPK_CAND and 8 * (lu.PRESSURE_DECLINED_N // 1024 + 8) > lu.TOPK_CAND
    cnt = lu.topk_candidates(row, n, n, 8)
    assert cnt == 7 * 248 + 1 and cnt <= lu.TOPK_CAND
    ids = lu.topk_order(row, 8)
    assert (row[ids] == 13).all() and (np.diff(ids) > 0).all()       # equal values: ascending columns
    assert len(set(lu.thread_of(ids, n, n).tolist()) & set(lu.PRESSURE_THREADS[1:])) >= 1
    assert lu.topk_candidates(np.arange(5, dtype=np.float32), 8, 5, 8) == 5      # fewer than K threads: every key


def test_adversarial_rows_satisfy_their_premises():
    G = 256
    sizes = lu.vocab_sizes(G)
    assert sizes == dict(half=2048, g1=4112, g3=12368, g5=20592, g8=32784) and all(n % 16 == 0 for n in sizes.values())
    for N in sizes.values():
        U = N // 16
        t, t1, t16, far = lu.tie_columns(N)
        (w0, g0, h0), (w1, g1, h1), (w2, _, _), (w3, g3, h3) = (lu.unit_owner(c // 16, U, G) for c in (t, t1, t16, far))
        assert w0 == w1 and (g0, h0) == (g1, h1) and t16 // 16 == t // 16 + 1
        assert w3 != w0 and g3 != g0 and h3 != h0 and far < N - 5
        if U >= 8 * G:
            assert w2 != w0                                             # every wave a unit: the next unit is another wave's
        nv = lu.first_range_valid(N, G)
        assert 0 < nv <= max(16, 16 * (U // G)) and nv % 16 != 0
    # half the workgroups idle; every batch-kernel wave busy and exactly one with two units
    assert len({lu.unit_owner(u, 128, G)[2] for u in range(128)}) == 128
    per_wave = np.bincount([lu.unit_owner(u, 8 * G + 1, G)[0] for u in range(8 * G + 1)], minlength=8 * G)
    assert per_wave.min() == 1 and (per_wave == 2).sum() == 1
    N = sizes["half"]
    X, nw, W, ref, bound = lu.reference(N, "abs")
    assert (W > 0).all() and (X < 0).all() and (nw > 0).all() and (ref + bound < 0).all()       # all negative, for certain
    X, nw, W, ref, bound = lu.reference(N, "normal")
    assert not X[lu.ZERO_ROW].any() and (ref[lu.ZERO_ROW] == 0).all() and (bound[lu.ZERO_ROW] == 0).all()
    tie = ref[lu.TIE_ROW]
    cols = lu.tie_columns(N)
    assert len(set(tie[cols])) == 1 and (np.delete(tie, cols) + np.delete(bound[lu.TIE_ROW], cols) < tie[3] - bound[lu.TIE_ROW, 3]).all()
    assert (np.abs(ref[0] - ref[1]) > bound[0] + bound[1]).any()                                 # distinct rows
    X, nw, W, ref, bound = lu.reference(N, "wide")
    top2 = np.sort(ref[:16], axis=1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 150).all() and (ref[:16].max(1) - ref[:16].min(1) > 200).all()
