"""Binding of qasr_kt_gemv_wide (csrc/kernel_harness.hip): launch_gemv_wide on caller-supplied arrays,
with the struct, guards and reporting of kernel_util.run_gemv."""
import ctypes as C

import numpy as np

import kernel_util as ku


def run_gemv_wide(epi, M, N, K, *, x=None, xh=None, norm_w=None, W=None, Wd=None, bias=None, res=None, ldo=0, ldo16=0):
    c = ku.GemvCall(epi=epi, M=M, N=N, K=K, wrows=W.shape[0], guard=ku.GUARD, launches=1, eps=1e-6, ldo=ldo, ldo16=ldo16)
    if x is not None:
        c.ldx = x.shape[1]
    if xh is not None:
        c.ldxh = xh.shape[1]
    if res is not None:
        c.ldr = res.shape[1]
    outs = dict(out_f32=ku._alloc(M, ldo, np.float32) if ldo else None, out_f16=ku._alloc(M, ldo16, np.uint16) if ldo16 else None)
    keep = ku._set(c, [], x=x, xh=xh, norm_w=norm_w, W=W, Wd=Wd, bias=bias, res=res, **outs)
    L = ku._lib()
    L.qasr_kt_gemv_wide.argtypes = [C.c_int, C.POINTER(ku.GemvCall)]
    L.qasr_kt_gemv_wide.restype = C.c_int
    ku._ok(L, L.qasr_kt_gemv_wide(0, C.byref(c)))
    del keep
    return ku.Result(c, outs)
