"""launch_gemv_wide (csrc/gemv_wide.hip: f16 rows of 6144 / 8192, the workgroup's four waves split K) against the
float64 dot product of the fp16-rounded operands, under the bound of the other GEMV tests (kernel_util.dense_bound:
derived from the arithmetic, whatever the summation order), and the "tiny-ffn6144" model, whose batch <= 8 decode
step needs that kernel, end to end."""
import functools
import os

import numpy as np
import pytest

import kernel_util as ku
import oracle_py as op
import qasr
from gemv_wide_util import run_gemv_wide

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def operands(K, N):
    """8 rows of fp32 x, their fp16 rounding (what the kernel multiplies), W, bias, residual: seeded, made once"""
    rng = np.random.default_rng(K + N)
    x32 = rng.standard_normal((8, K)).astype(np.float32)
    W = ku.f16_normal(rng, (N, K), K ** -0.5)
    bias = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((8, N)).astype(np.float32)
    xr = x32.astype(np.float16)
    return x32, xr, W, bias, res, ku.dense_terms(xr, W)


def launch(epi, M, N, K, xr, W, x32=None, bias=None, res=None):
    """x32 given: the fp32 input (ldx = K + 4), else xh (ldxh = K + 8); outputs with padded leading dimensions"""
    kw = dict(x=ku.pad_cols(x32[:M], K + 4)) if x32 is not None else dict(xh=ku.bits(ku.pad_cols(xr[:M], K + 8)))
    if epi == ku.EPI_F32:
        kw.update(ldo=N + 5, res=None if res is None else ku.pad_cols(res[:M], N + 3))
    else:
        kw.update(ldo16=N + 3)
    return run_gemv_wide(epi, M, N, K, W=ku.bits(W), bias=bias, **kw)


@pytest.mark.parametrize("fp32_x", [True, False], ids=["x", "xh"])
@pytest.mark.parametrize("epi", [ku.EPI_F32, ku.EPI_F16], ids=["f32", "f16"])
@pytest.mark.parametrize("N", [5, 2050])
@pytest.mark.parametrize("K", [6144, 8192])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_values(gpu, M, K, N, epi, fp32_x):
    x32, xr, W, bias, res, (ref, mag) = operands(K, N)
    f32 = epi == ku.EPI_F32
    r = [launch(epi, M, N, K, xr, W, x32 if fp32_x else None, bias, res if f32 else None) for _ in range(2)]
    assert not r[0].declined and r[0].tag.startswith("gemv_wide"), (r[0].tag, r[0].msg)
    want, bound = ku.add_terms(ref[:M], ku.dense_bound(K, mag[:M]), bias[None, :], res[:M] if f32 else None)
    out = [a.out_f32 if f32 else a.out_f16 for a in r]
    ku.check_values(ku.in_range(out[0], M, N), want, bound, fp16=not f32)
    assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8)), "two launches on the same state differ"


@pytest.mark.parametrize("where", ["0", "K/4-8", "K/4", "K-8"])
@pytest.mark.parametrize("K", [6144, 8192])
def test_one_hot_slice(gpu, K, where):
    """x is zero but for 8 consecutive elements: a wave reading a neighbour's quarter, or a clamped last sweep,
    multiplies them with the wrong weights"""
    M, N = 2, 70
    k0 = {"0": 0, "K/4-8": K // 4 - 8, "K/4": K // 4, "K-8": K - 8}[where]
    rng = np.random.default_rng(K + k0)
    W = ku.f16_normal(rng, (N, K))
    xr = np.zeros((M, K), np.float16)
    xr[:, k0:k0 + 8] = ku.f16_normal(rng, (M, 8))
    r = launch(ku.EPI_F32, M, N, K, xr, W)
    ref, mag = ku.dense_terms(xr, W)
    ku.check_values(ku.in_range(r.out_f32, M, N), ref, ku.dense_bound(K, mag))


@pytest.mark.parametrize("case", ["K=4608", "K=10240", "M=9", "Wd", "norm_w", "swiglu"])
def test_declines(gpu, case):
    K = {"K=4608": 4608, "K=10240": 10240}.get(case, 6144)
    M, N = (9 if case == "M=9" else 2), 16
    kw = dict(xh=np.zeros((M, K), np.uint16), W=np.zeros((2 * N, K), np.uint16), ldo=N, ldo16=N)
    if case == "Wd":
        kw["Wd"] = np.zeros((2 * N, K // 32), np.uint16)
    if case == "norm_w":
        kw.update(norm_w=np.ones(K, np.float32), x=np.zeros((M, K), np.float32), xh=None)
    r = run_gemv_wide(ku.EPI_SWIGLU_F16 if case == "swiglu" else ku.EPI_F32, M, N, K, **kw)
    assert r.declined and r.tag == "", (r.tag, r.msg)
    ku.untouched(r.out_f32, r.out_f16)


# ------------------------------------------------------------------ the model whose batch <= 8 step needs the kernel
@pytest.fixture(scope="module")
def wide(gpu, built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("models") / "tiny-ffn6144-f16.gguf")
    qasr.write_synthetic_gguf(path, "tiny-ffn6144", 42, 1)
    m = qasr.Model(path)
    c = qasr.Context(m, max_batch=9, max_ctx=640)
    yield path, m, c
    c.close()
    m.close()


def test_transcribe(wide):
    _, m, c = wide
    assert m.hp.dec_ffn == 6144
    r = c.transcribe([qasr.synth_pcm(1000, 16000)], max_tokens=16, ignore_eos=True)
    assert len(r.tokens[0]) == 16


def test_decode_steps_teacher_forced(wide, parity):
    """12 teacher-forced steps of one clip at 1 and 8 rows (the K-split GEMV in the down projection) and at 9 rows
    (the skinny GEMMs), each against the CPU oracle: both are fp32 sums of the same fp16 products in another order,
    so the batch <= 8 path may err at most twice as much as the 9-row path does."""
    path, m, c = wide
    op.set_threads(min(8, os.cpu_count() or 1))
    om = op.OracleModel(path)
    feats = om.encode(op.log_mel(qasr.synth_pcm(6100, 16000)))
    ids, pos = m.build_prompt(feats.shape[0])
    toks = [int(t) for t in np.random.default_rng(7).integers(0, 151643, 12)]
    d = op.OracleDecoder(om, 512)
    d.forward(ids, 0, feats, pos)
    want = [d.forward([t], len(ids) + i).copy() for i, t in enumerate(toks)]
    err = {}
    for B in (1, 8, 9):
        c.prefill([ids] * B, [feats] * B, [pos] * B, want_logits=False)
        rel = ab = 0.0
        for i, (t, lo) in enumerate(zip(toks, want)):
            lg, am = c.decode_step([t] * B, [len(ids) + i] * B)
            scale, e = float(np.abs(lo).max()), float(np.abs(lg - lo[None, :]).max())
            rel, ab = max(rel, e / scale), max(ab, e)
            s = np.sort(lo)
            if s[-1] - s[-2] > 0.05 * scale:
                assert (am == int(np.argmax(lo))).all(), (B, i)
        err[B] = (rel, ab)
        parity(f"tiny_ffn6144_decode_12_steps_B{B}", rel_max=rel, abs_max=ab)
    print("tiny-ffn6144 teacher-forced (rel, abs) by rows:", err)
    for B in (1, 8):
        assert err[B][0] <= 2 * err[9][0] and err[B][1] <= 2 * err[9][1], err
