"""CPU: the top-K additions at the boundary -- the three C-ABI symbols, their
argument checks without a context, and the unchanged shape of the Python results.
No device calls."""
import ctypes as C
import os
import re

import qasr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QASR_ERR_ARG = 1
NAMES = ("qasr_get_step_topk", "qasr_get_topk", "qasr_stream_topk")


def test_topk_symbols_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "qasr_capi.h")).read()
    decl = set(re.findall(r"\b(qasr_[a-z0-9_]+)\s*\(", hdr))
    lib = qasr.lib()
    for n in NAMES:
        assert n in decl and n in qasr.EXPORTS and hasattr(lib, n), n
    assert "no reference counterpart" in hdr[hdr.index("top-K token alternatives"):][:200]
    assert re.search(r"#define\s+QASR_TOPK_MAX\s+8\b", hdr)


def test_topk_calls_reject_a_null_context(built):
    """QASR_ERR_ARG for a null context; qasr_stream_topk returns a count on
    success, so its errors are minus the code (as qasr_stream_logprobs)"""
    lib = qasr.lib()
    ids, lps = (C.c_int32 * 16)(), (C.c_float * 16)()
    assert lib.qasr_get_step_topk(None, ids, lps, 2, 8) == QASR_ERR_ARG
    assert b"argument" in lib.qasr_last_error()
    assert lib.qasr_get_topk(None, ids, lps, 1, 2, 8) == QASR_ERR_ARG
    assert lib.qasr_stream_topk(None, ids, lps, 2, 8) == -QASR_ERR_ARG


def test_run_result_keeps_its_forms():
    t = qasr.Timings()
    r = qasr.RunResult([[1, 2]], t)
    assert r.tokens == [[1, 2]] and r.timings is t and r.logprobs is None and r.topk is None
    r = qasr.RunResult([[1]], t, [[-0.5]])
    assert r.logprobs == [[-0.5]] and r.topk is None
