"""launch_gemv_rows_q8 (csrc/gemv_rows_q8.hip: 2 .. 8 rows of a Q8_0 model on the int8 MFMA, the workgroup's four waves
split K) against the float64 sum of the exact block products under kernel_util.q8_bound (which holds for any
summation order), its norm / gather prologues against launch_gemv's on the same arrays, single live blocks exactly, its
declines, and the decode step that option gemv_rows = 2 routes through it, against the CPU oracle.

Teacher-forced logit errors measured at the time of writing: DESIGN.md 5.13."""
import functools
import os

import numpy as np
import pytest

import kernel_util as ku
import oracle_py as op
import qasr
from gemv_rows_q8_util import run_gemv_rows_q8

pytestmark = pytest.mark.gpu
F32, SWIGLU = ku.EPI_F32, ku.EPI_SWIGLU_F32


@functools.lru_cache(maxsize=None)
def operands(K, N):
    """8 fp32 rows, norm weights, Q8_0 W (2 N rows: SwiGLU reads gate and up), bias, residual: seeded, made once"""
    rng = np.random.default_rng(K + N)
    x = (rng.standard_normal((8, K)) * 3).astype(np.float32)
    nw = (1 + 0.25 * rng.standard_normal(K)).astype(np.float32)
    Wq, Wd = ku.q8_operand(rng, 2 * N, K, np.float16, 0.02 * K ** -0.5)
    return x, nw, Wq, Wd, rng.standard_normal(N).astype(np.float32), rng.standard_normal((8, N)).astype(np.float32)


def finish(epi, N, ref, bound, bias=None, res=None):
    if epi == SWIGLU:
        gate, up = ku.swiglu_rows(N)
        return ku.swiglu_terms(ref[:, gate], bound[:, gate], ref[:, up], bound[:, up])
    return ku.add_terms(ref, bound, bias, res)


@pytest.mark.parametrize("epi,N", [(F32, 5), (F32, 2050), (SWIGLU, 48), (SWIGLU, 2064)])
@pytest.mark.parametrize("K", [256, 2048, 6144])
@pytest.mark.parametrize("M", [2, 5, 8])
def test_values(gpu, M, K, N, epi):
    x, _, Wq, Wd, bias, res = operands(K, N)
    wr = 2 * N if epi == SWIGLU else N
    kw = dict(bias=bias, res_inplace=res[:M]) if epi == F32 else {}
    r = [run_gemv_rows_q8(epi, M, N, K, x=ku.pad_cols(x[:M], K + 4), Wq=Wq[:wr], Wd=Wd[:wr], ldo=N + 5, **kw) for _ in range(2)]
    assert not r[0].declined and r[0].tag.startswith("gemv_rows_q8"), (r[0].tag, r[0].msg)
    Aq, Ad = ku.q8_quantize(x[:M])
    ref, mag = ku.q8_terms(Aq, Ad, Wq[:wr], Wd[:wr])
    want, bound = finish(epi, N, ref, ku.q8_bound(K, mag), bias[None, :], res[:M])
    err = ku.check_values(ku.in_range(r[0].out_f32, M, N), want, bound)
    print(f"gemv_rows_q8 epi={epi} M={M} K={K} N={N}: worst error / bound {err:.3f}")
    assert np.array_equal(r[0].out_f32.view(np.uint8), r[1].out_f32.view(np.uint8)), "two launches on the same state differ"


@pytest.mark.parametrize("M,epi,gather", [(3, F32, False), (8, F32, False), (3, SWIGLU, False), (8, SWIGLU, False), (3, F32, True)])
def test_prologues_against_launch_gemv(gpu, M, epi, gather):
    """norm_w (and once the layer-0 gather) through launch_gemv and through the new launcher on the same arrays: both
    multiply the same quants, each within one q8_bound (SwiGLU: propagated by swiglu_terms) of their exact product"""
    K, N = 2048, 70 if epi == F32 else 48
    x, nw, Wq, Wd, _, _ = operands(K, N)
    wr = 2 * N if epi == SWIGLU else N
    if gather:
        embd, ids = ku.f16_normal(np.random.default_rng(11), (9, K)), [7, 0, 7]
        rows = embd[ids].astype(np.float32)
        kw = dict(embd=ku.bits(embd), embd_ids=ids, x_store_ld=K + 4)
    else:
        rows = x[:M]
        kw = dict(x=ku.pad_cols(rows, K + 4))
    old = ku.run_gemv(epi, M, N, K, wrows=wr, norm_w=nw, Wq=Wq[:wr], Wd=Wd[:wr], ldo=N + 5, **kw)
    new = run_gemv_rows_q8(epi, M, N, K, norm_w=nw, Wq=Wq[:wr], Wd=Wd[:wr], ldo=N + 5, **kw)
    assert not old.declined and not new.declined and new.tag.startswith("gemv_rows_q8"), (old.msg, new.msg, new.tag)
    Aq, Ad = ku.q8_quantize(ku.rms_prologue(rows, nw, 1e-6)[1])
    ref, mag = ku.q8_terms(Aq, Ad, Wq[:wr], Wd[:wr])
    _, bound = finish(epi, N, ref, ku.q8_bound(K, mag))
    a, b = ku.in_range(new.out_f32, M, N).astype(np.float64), ku.in_range(old.out_f32, M, N).astype(np.float64)
    print(f"gemv_rows_q8 vs gemv_q8 M={M} epi={epi}: worst |difference| / (2 bound) {(np.abs(a - b) / (2 * bound)).max():.3f}")
    assert (np.abs(a - b) <= 2 * bound).all()
    if gather:
        assert np.array_equal(ku.in_range(new.x_store, M, K), rows)


@pytest.mark.parametrize("where", ["first", "last of wave 0", "first of wave 1", "last"])
@pytest.mark.parametrize("K", [256, 6144])
def test_one_live_block_exact(gpu, K, where):
    """x is zero but for one 32-block of rows 0 and 2: every live output is one term, float32(float32(d_w d_x) idot),
    + bias, + residual, exactly; row 1 is exactly bias + residual"""
    M, N = 3, 70
    blk = {"first": 0, "last of wave 0": K // 128 - 1, "first of wave 1": K // 128, "last": K // 32 - 1}[where]
    _, _, Wq, Wd, bias, res = operands(K, N)
    x = np.zeros((M, K), np.float32)
    x[0::2, 32 * blk:32 * blk + 32] = np.random.default_rng(blk).standard_normal((2, 32))
    r = run_gemv_rows_q8(F32, M, N, K, x=ku.pad_cols(x, K + 4), Wq=Wq[:N], Wd=Wd[:N], bias=bias, res_inplace=res[:M], ldo=N + 5)
    assert not r.declined, r.msg
    Aq, Ad = ku.q8_quantize(x)
    sl = slice(32 * blk, 32 * blk + 32)
    idot = (Aq[:, sl].astype(np.int32) @ Wq[:N, sl].astype(np.int32).T).astype(np.float32)
    want = (Ad[:, blk, None] * Wd[None, :N, blk].astype(np.float32)) * idot + bias[None, :] + res[:M]
    assert want.dtype == np.float32
    out = ku.in_range(r.out_f32, M, N)
    assert np.array_equal(out, want), np.argwhere(out != want)[:4]
    assert np.array_equal(out[1], bias + res[1])


@pytest.mark.parametrize("case", ["M=1", "M=9", "K=384", "K=8448", "xh", "no Wd", "argmax", "swiglu N=40"])
def test_declines(gpu, case):
    K = {"K=384": 384, "K=8448": 8448}.get(case, 2048)
    M = {"M=1": 1, "M=9": 9}.get(case, 2)
    N = 40 if case == "swiglu N=40" else 16
    kw = dict(x=np.zeros((M, K), np.float32), Wq=np.zeros((2 * N, K), np.int8), Wd=np.zeros((2 * N, K // 32), np.uint16))
    if case == "xh":
        kw.update(x=None, xh=np.zeros((M, K), np.uint16))
    if case == "no Wd":
        kw.update(Wq=None, Wd=None, W=np.zeros((2 * N, K), np.uint16))
    epi = {"argmax": ku.EPI_ARGMAX, "swiglu N=40": SWIGLU}.get(case, F32)
    r = run_gemv_rows_q8(epi, M, N, K, ldo=N, ldo16=N, **kw)
    assert r.declined and r.tag == "", (r.tag, r.msg)
    ku.untouched(r.out_f32, r.out_f16)


# ------------------------------------------------------------------ the decode step through the kernel
@pytest.fixture(scope="module", params=["tiny", "tiny-ffn6144"])
def model(request, gpu, built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("models") / f"{request.param}-q8.gguf")
    qasr.write_synthetic_gguf(path, request.param, 42, 8)
    m = qasr.Model(path)
    c = qasr.Context(m, max_batch=8, max_ctx=640)
    yield path, m, c
    c.close()
    m.close()


def test_decode_steps_teacher_forced(model, parity):
    """12 teacher-forced steps of one clip at 2 and 8 rows against the CPU oracle, with gemv_rows = 0 (gemv_q8_kernel)
    and gemv_rows = 2 (the four layer projections on the int8 MFMA kernel).  Q8_0 logit errors are single int8 rounding
    flips, so the bar is the other path on the same model and rows: worst and median at most twice its values."""
    path, m, c = model
    name = os.path.basename(path)[:-8].replace("-", "_")
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
    err = {}
    for B in (2, 8):
        for mode in (0, 2):
            c.set_option("gemv_rows", mode)
            c.prefill([ids] * B, [feats] * B, [pos] * B, want_logits=False)
            e = [float(np.abs(c.decode_step([t] * B, [len(ids) + i] * B)[0] - lo[None, :]).max())
                 for i, (t, lo) in enumerate(zip(toks, want))]
            assert c.get_option("gemv_rows_path") == (15 if mode else 0), (B, mode)   # QKV, o, gate/up, down
            err[B, mode] = (max(e), float(np.median(e)))
            parity(f"{name}_q8_gemv_rows{mode}_decode_12_steps_B{B}", abs_max=err[B, mode][0], abs_median=err[B, mode][1])
    print(f"{name} Q8_0 teacher-forced (worst, median) absolute logit error by (rows, gemv_rows):", err)
    for B in (2, 8):
        assert err[B, 2][0] <= 2 * err[B, 0][0] and err[B, 2][1] <= 2 * err[B, 0][1], err
    r = c.transcribe([qasr.synth_pcm(1000, 16000)], max_tokens=16, ignore_eos=True)
    assert len(r.tokens[0]) == 16
    c.set_option("gemv_rows", 1)
