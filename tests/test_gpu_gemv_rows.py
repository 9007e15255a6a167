"""launch_gemv_rows (csrc/gemv_rows.hip: 2 .. 8 rows on v_mfma_f32_16x16x32_f16, the workgroup's four waves split K)
against the float64 dot product of the fp16-rounded operands under kernel_util.dense_bound (derived from the
arithmetic, whatever the summation order), its declines, and the decode step that option gemv_rows = 2 routes
through it, end to end against the CPU oracle.

Teacher-forced errors (rel, abs of the largest logit) measured at the time of writing: DESIGN.md 5.12."""
import functools
import os

import numpy as np
import pytest

import kernel_util as ku
import oracle_py as op
import qasr
from gemv_rows_util import run_gemv_rows

pytestmark = pytest.mark.gpu
F32, F16, SWIGLU = ku.EPI_F32, ku.EPI_F16, ku.EPI_SWIGLU_F16


@functools.lru_cache(maxsize=None)
def operands(K, N):
    """8 rows of fp16 x, fp32 rows for the norm with their prologue values, W (2 N rows: SwiGLU reads gate and up),
    bias, residual, embedding rows: seeded, made once"""
    rng = np.random.default_rng(K + N)
    xr = ku.f16_normal(rng, (8, K))
    x32 = (ku.f16_normal(rng, (8, K)).astype(np.float32) * 3).astype(np.float32)
    nw = (1 + 0.25 * rng.standard_normal(K)).astype(np.float32)
    W = ku.f16_normal(rng, (2 * N, K), K ** -0.5)
    bias = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((8, N)).astype(np.float32)
    return xr, x32, nw, W, bias, res


def reference(h, W, K, tie=None):
    ref, mag = ku.dense_terms(h, W)
    return ref, ku.dense_bound(K, mag) + (ku.tie_slack(h, tie, W) if tie is not None else 0.0)


CASES = {"xh_f32": F32, "norm_f32": F32, "f16": F16, "swiglu": SWIGLU}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("N", [5, 2050])
@pytest.mark.parametrize("K", [256, 2048, 6144])
@pytest.mark.parametrize("M", [2, 5, 8])
def test_values(gpu, M, K, N, case):
    epi = CASES[case]
    if epi == SWIGLU:
        N = {5: 48, 2050: 2064}[N]
    xr, x32, nw, W, bias, res = operands(K, N)
    W = W if epi == SWIGLU else W[:N]
    kw, tie = dict(xh=ku.bits(ku.pad_cols(xr[:M], K + 8))), None
    h = xr[:M]
    if case in ("norm_f32", "swiglu"):
        h, _, tie = ku.rms_prologue(x32[:M], nw, 1e-6)
        assert tie.mean(1).max() <= 0.01, tie.mean(1)   # near-tie elements: at most 1 % of a row
        kw = dict(x=ku.pad_cols(x32[:M], K + 4), norm_w=nw)
    if case == "xh_f32":
        kw.update(bias=bias, res_inplace=res[:M])
    if case == "f16":
        kw.update(bias=bias)
    kw.update(dict(ldo=N + 5) if epi == F32 else dict(ldo16=N + 3))
    r = [run_gemv_rows(epi, M, N, K, W=ku.bits(W), **kw) for _ in range(2)]
    assert not r[0].declined and r[0].tag.startswith("gemv_rows"), (r[0].tag, r[0].msg)
    ref, bound = reference(h, W, K, tie)
    if epi == SWIGLU:
        gate, up = ku.swiglu_rows(N)
        want, bound = ku.swiglu_terms(ref[:, gate], bound[:, gate], ref[:, up], bound[:, up])
    else:
        want, bound = ku.add_terms(ref, bound, bias[None, :] if "bias" in kw else None, res[:M] if case == "xh_f32" else None)
    out = [a.out_f32 if epi == F32 else a.out_f16 for a in r]
    err = ku.check_values(ku.in_range(out[0], M, N), want, bound, fp16=epi != F32)
    print(f"gemv_rows {case} M={M} K={K} N={N}: worst error / bound {err:.3f}")
    assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8)), "two launches on the same state differ"


@pytest.mark.parametrize("where", ["0", "K/4-8", "K/4", "32", "K-8"])
@pytest.mark.parametrize("K", [2048, 6144])
def test_one_hot_slice(gpu, K, where):
    """x is zero but for 8 consecutive elements at a wave-quarter or MFMA-step boundary; rows 0 and 2 differ and row 1
    is zero, so its outputs are exactly bias + residual: a fragment lane mapped to the wrong row or k shows"""
    M, N = 3, 70
    k0 = {"0": 0, "K/4-8": K // 4 - 8, "K/4": K // 4, "32": 32, "K-8": K - 8}[where]
    rng = np.random.default_rng(K + k0)
    W = ku.f16_normal(rng, (N, K))
    bias = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((M, N)).astype(np.float32)
    xr = np.zeros((M, K), np.float16)
    xr[0, k0:k0 + 8], xr[2, k0:k0 + 8] = ku.f16_normal(rng, (2, 8))
    r = run_gemv_rows(F32, M, N, K, xh=ku.bits(ku.pad_cols(xr, K + 8)), W=ku.bits(W), bias=bias, res_inplace=res, ldo=N + 5)
    assert not r.declined, r.msg
    ref, bound = reference(xr, W, K)
    want, bound = ku.add_terms(ref, bound, bias[None, :], res)
    out = ku.in_range(r.out_f32, M, N)
    ku.check_values(out, want, bound)
    assert np.array_equal(out[1], bias + res[1])


def test_embedding_gather(gpu):
    """layer 0: rows gathered from embd by id give the outputs of the x + norm_w launch fed those rows, and x_store them"""
    M, N, K = 3, 70, 2048
    _, _, nw, W, _, _ = operands(K, N)
    rng = np.random.default_rng(11)
    embd = ku.f16_normal(rng, (9, K))
    ids = [7, 0, 7]
    rows = embd[ids].astype(np.float32)
    a = run_gemv_rows(F32, M, N, K, embd=ku.bits(embd), embd_ids=ids, x_store_ld=K + 4, norm_w=nw, W=ku.bits(W[:N]), ldo=N + 5)
    b = run_gemv_rows(F32, M, N, K, x=ku.pad_cols(rows, K + 4), norm_w=nw, W=ku.bits(W[:N]), ldo=N + 5)
    assert not a.declined and not b.declined, (a.msg, b.msg)
    assert np.array_equal(ku.in_range(a.out_f32, M, N), ku.in_range(b.out_f32, M, N))
    assert np.array_equal(ku.in_range(a.x_store, M, K), rows)


@pytest.mark.parametrize("case", ["M=1", "M=9", "Wd", "K=384", "K=8448", "argmax", "swiglu N=40"])
def test_declines(gpu, case):
    K = {"K=384": 384, "K=8448": 8448}.get(case, 2048)
    M = {"M=1": 1, "M=9": 9}.get(case, 2)
    N = 40 if case == "swiglu N=40" else 16
    kw = dict(xh=np.zeros((M, K), np.uint16), W=np.zeros((2 * N, K), np.uint16), ldo=N, ldo16=N)
    if case == "Wd":
        kw["Wd"] = np.zeros((2 * N, K // 32), np.uint16)
    epi = {"argmax": ku.EPI_ARGMAX, "swiglu N=40": SWIGLU}.get(case, F32)
    r = run_gemv_rows(epi, M, N, K, **kw)
    assert r.declined and r.tag == "", (r.tag, r.msg)
    ku.untouched(r.out_f32, r.out_f16)


# ------------------------------------------------------------------ the decode step through the kernel
@pytest.fixture(scope="module", params=["tiny", "tiny-ffn6144"])
def model(request, gpu, built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("models") / f"{request.param}-f16.gguf")
    qasr.write_synthetic_gguf(path, request.param, 42, 1)
    m = qasr.Model(path)
    c = qasr.Context(m, max_batch=9, max_ctx=640)
    yield path, m, c
    c.close()
    m.close()


def test_decode_steps_teacher_forced(model, parity):
    """12 teacher-forced steps of one clip at 2 and 8 rows (option gemv_rows = 2: the four layer projections on the
    MFMA kernel) and at 9 rows (the untouched skinny GEMMs), each against the CPU oracle: all are fp32 sums of the
    same fp16 products in another order, so the <= 8-row path may err at most twice as much as the 9-row path."""
    path, m, c = model
    name = os.path.basename(path)[:-9].replace("-", "_")
    op.set_threads(min(8, os.cpu_count() or 1))
    om = op.OracleModel(path)
    feats = om.encode(op.log_mel(qasr.synth_pcm(6100, 16000)))
    ids, pos = m.build_prompt(feats.shape[0])
    toks = [int(t) for t in np.random.default_rng(7).integers(0, 151643, 12)]
    d = op.OracleDecoder(om, 512)
    d.forward(ids, 0, feats, pos)
    want = [d.forward([t], len(ids) + i).copy() for i, t in enumerate(toks)]
    c.prefill([ids] * 2, [feats] * 2, [pos] * 2, want_logits=False)
    c.decode_step([toks[0]] * 2, [len(ids)] * 2)
    assert c.get_option("gemv_rows") == 1 and c.get_option("gemv_rows_path") == 0, "a hidden < 2048 decoder changed its kernels"
    c.set_option("gemv_rows", 2)
    err = {}
    for B in (2, 8, 9):
        c.prefill([ids] * B, [feats] * B, [pos] * B, want_logits=False)
        rel = ab = 0.0
        for i, (t, lo) in enumerate(zip(toks, want)):
            lg, am = c.decode_step([t] * B, [len(ids) + i] * B)
            scale, e = float(np.abs(lo).max()), float(np.abs(lg - lo[None, :]).max())
            rel, ab = max(rel, e / scale), max(ab, e)
            s = np.sort(lo)
            if s[-1] - s[-2] > 0.05 * scale:
                assert (am == int(np.argmax(lo))).all(), (B, i)
        assert c.get_option("gemv_rows_path") == (15 if B <= 8 else 0), B   # QKV, o, gate/up, down
        err[B] = (rel, ab)
        parity(f"{name}_gemv_rows_decode_12_steps_B{B}", rel_max=rel, abs_max=ab)
    print(f"{name} teacher-forced (rel, abs) by rows, gemv_rows = 2:", err)
    for B in (2, 8):
        assert err[B][0] <= 2 * err[9][0] and err[B][1] <= 2 * err[9][1], err
    r = c.transcribe([qasr.synth_pcm(1000, 16000)], max_tokens=16, ignore_eos=True)
    assert len(r.tokens[0]) == 16
    c.set_option("gemv_rows", 1)
