"""Binding of qasr_kt_gemv_rows_q8 (csrc/kernel_harness.hip): launch_gemv_rows_q8 on caller-supplied arrays, with the
struct, guards and reporting of kernel_util.run_gemv.  res_inplace: the residual rows [M][N], placed into the fp32
output allocation itself, which is passed as res and out_f32 at once -- the launch runs in place."""
import ctypes as C

import numpy as np

import kernel_util as ku


def run_gemv_rows_q8(epi, M, N, K, *, x=None, xh=None, norm_w=None, W=None, Wq=None, Wd=None, bias=None, res_inplace=None,
                     embd_ids=None, embd=None, x_store_ld=0, ldo=0, ldo16=0):
    wrows = (Wq if Wq is not None else W).shape[0]
    c = ku.GemvCall(epi=epi, M=M, N=N, K=K, wrows=wrows, guard=ku.GUARD, launches=1, eps=1e-6, ldo=ldo, ldo16=ldo16)
    c.ldx = x_store_ld or (x.shape[1] if x is not None else 0)
    if xh is not None:
        c.ldxh = xh.shape[1]
    if embd is not None:
        c.embd_rows = embd.shape[0]
    outs = dict(x_store=ku._alloc(M, x_store_ld, np.float32) if x_store_ld else None,
                out_f32=ku._alloc(M, ldo, np.float32) if ldo else None, out_f16=ku._alloc(M, ldo16, np.uint16) if ldo16 else None)
    keep = ku._set(c, [], x=x, xh=xh, norm_w=norm_w, W=W, Wq=Wq, Wd=Wd, bias=bias, embd=embd,
                   embd_ids=None if embd_ids is None else np.asarray(embd_ids, np.int32), **outs)
    if res_inplace is not None:
        outs["out_f32"].view(np.uint32)[:] = 0xFFFFFFFF   # what the harness makes of every output byte
        outs["out_f32"][ku.GUARD:ku.GUARD + M, :N] = res_inplace
        c.res, c.ldr = c.out_f32, ldo
    L = ku._lib()
    L.qasr_kt_gemv_rows_q8.argtypes = [C.c_int, C.POINTER(ku.GemvCall)]
    L.qasr_kt_gemv_rows_q8.restype = C.c_int
    ku._ok(L, L.qasr_kt_gemv_rows_q8(0, C.byref(c)))
    del keep
    return ku.Result(c, outs)
