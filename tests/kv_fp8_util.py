"""Shared by the FP8 shadow KV cache tests: the rule of csrc/kv_fp8_host.h as torch states it on the CPU, the ctypes
bindings of qasr_kt_kv_fp8_convert and qasr_kt_decode_attn_fp8, and the cache reads of qasr_debug_read."""
import ctypes as C

import numpy as np
import torch

import attn_util as au
import kernel_util as ku
from kernel_util import GUARD

QASR_ERR_ARG, QASR_ERR_STATE = 1, 5


def rule(x16, s):
    """q = RNE_E4M3FN(clamp(x 2^s, -448, 448)) of an fp16 array, as uint8"""
    x = torch.from_numpy(np.ascontiguousarray(x16, np.float16).astype(np.float32)) * 2.0 ** s
    return x.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def dequant(q8, s):
    """the value the attention uses, float(q) 2^-s, as fp16 (exact)"""
    v = torch.from_numpy(np.ascontiguousarray(q8, np.uint8)).view(torch.float8_e4m3fn).to(torch.float32).numpy() * 2.0 ** -s
    h = v.astype(np.float16)
    assert np.array_equal(h.astype(np.float32), v, equal_nan=True), "a dequantised value is no fp16 value"
    return h


class ConvertCall(C.Structure):
    _fields_ = au._i32("layers", "n_kv_head", "max_ctx", "slots", "guard", "B", "span", "exp") + au._ptr(
        "slot", "from_", "to", "kc", "vc", "k8", "v8") + [("declined", C.c_int32)]


def run_convert(kc, vc, k8, v8, slot, frm, to, s, guard, span=0):
    """kc / vc uint16 (fp16 bits), k8 / v8 uint8, all [layers][slots + guard][n_kv_head][max_ctx][128] -> (k8, v8) after"""
    L, S, H, ctx, _ = kc.shape
    k8, v8 = k8.copy(), v8.copy()
    c = ConvertCall(layers=L, n_kv_head=H, max_ctx=ctx, slots=S - guard, guard=guard, B=len(slot), span=span, exp=s)
    keep = ku._set(c, [], slot=np.asarray(slot, np.int32), from_=np.asarray(frm, np.int32), to=np.asarray(to, np.int32),
                   kc=kc, vc=vc, k8=k8, v8=v8)
    au._call("qasr_kt_kv_fp8_convert", c, keep)
    assert not c.declined
    return k8, v8


class AttnCall(C.Structure):
    _fields_ = au._i32("B", "n_head", "n_kv_head", "max_ctx", "max_pos", "kv_nt", "exp", "repeat", "guard") + [
        ("scale", C.c_float), ("eps", C.c_float)] + au._ptr(
        "pos", "qkv", "q_norm", "k_norm", "rope", "kc", "vc", "vt", "k8", "v8", "out", "out_b", "out32", "out32_b", "outq", "outq_b",
        "outd", "outd_b") + [("declined", C.c_int32), ("tag", C.c_char * 64), ("msg", C.c_char * 256)]


def run_attn(case, k8, v8, s, kind="f32", repeat=1):
    """launch_decode_attention_fp8 on a decode_attn_util case and the shadows k8 / v8 [B + GUARD][n_kv_head][max_ctx][128]
    (the last GUARD slots 0xFF).  Returns an Out with tag and the whole allocations: the output(s) of `kind`
    ('f32' | 'f16' | 'q8', *_b with repeat 2), kc, vc, vt, k8, v8"""
    B, QD = case["B"], case["n_head"] * 128
    c = AttnCall(B=B, n_head=case["n_head"], n_kv_head=case["n_kv_head"], max_ctx=case["max_ctx"], max_pos=case["max_pos"], kv_nt=1,
                 exp=s, repeat=repeat, guard=GUARD, scale=float(case["scale"]), eps=case["eps"])
    outs = {}
    for sfx in ("", "_b")[:repeat]:
        if kind == "q8":
            outs.update({"outq" + sfx: au._out(B, QD, np.int8), "outd" + sfx: au._out(B, QD // 32, np.float32)})
        else:
            outs.update({("out32" if kind == "f32" else "out") + sfx: au._out(B, QD, np.float32 if kind == "f32" else np.uint16)})
    outs.update(kc=ku.bits(case["kc"]).copy(), vc=ku.bits(case["vc"]).copy(), vt=ku.bits(case["vt"]).copy(), k8=k8.copy(), v8=v8.copy())
    keep = ku._set(c, [], pos=case["pos"], **{k: case[k] for k in ("qkv", "q_norm", "k_norm", "rope")}, **outs)
    au._call("qasr_kt_decode_attn_fp8", c, keep)
    r = au.Out(c, outs)
    r.tag = c.tag.decode()
    return r


def read_cache(ctx, name, expect_rc=0):
    """qasr_debug_read of "kc" / "vc" (fp16) or "k8" / "v8" (uint8): [dec_layers][max_batch][n_kv_head][max_ctx][128]"""
    import qasr
    hp = ctx.model.hp
    out = np.zeros((hp.dec_layers, ctx.max_batch, hp.n_kv_heads, ctx.max_ctx, 128), np.uint8 if name.endswith("8") else np.float16)
    rc = qasr.lib().qasr_debug_read(ctx.h, name.encode(), out.ctypes.data_as(C.c_void_p), C.c_int64(out.nbytes))
    assert rc == expect_rc, (rc, qasr.lib().qasr_last_error())
    return out
