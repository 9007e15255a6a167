"""CPU: the token log-probability additions at the boundary -- the three C-ABI
symbols, their argument checks without a context, and the unchanged shape of
the Python results.  No device calls."""
import ctypes as C
import os
import re

import qasr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QASR_ERR_ARG, QASR_ERR_STATE = 1, 5
NAMES = ("qasr_get_step_logprobs", "qasr_get_logprobs", "qasr_stream_logprobs")


def test_logprob_symbols_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "qasr_capi.h")).read()
    decl = set(re.findall(r"\b(qasr_[a-z0-9_]+)\s*\(", hdr))
    lib = qasr.lib()
    for n in NAMES:
        assert n in decl and n in qasr.EXPORTS and hasattr(lib, n), n
    assert "no reference counterpart" in hdr[hdr.index("token log-probabilities"):][:200]


def test_logprob_calls_reject_a_null_context(built):
    """QASR_ERR_ARG for a null context (and the message set).  qasr_stream_logprobs
    returns a count on success, so its errors are minus the code -- the
    convention of qasr_align_json -- or a count of 1 could not be told from
    QASR_ERR_ARG."""
    lib = qasr.lib()
    buf = (C.c_float * 8)()
    assert lib.qasr_get_step_logprobs(None, buf, 8) == QASR_ERR_ARG
    assert b"argument" in lib.qasr_last_error()
    assert lib.qasr_get_logprobs(None, buf, 2, 4) == QASR_ERR_ARG
    assert lib.qasr_stream_logprobs(None, buf, 8) == -QASR_ERR_ARG


def test_run_result_keeps_its_two_field_form():
    t = qasr.Timings()
    r = qasr.RunResult([[1, 2]], t)
    assert r.tokens == [[1, 2]] and r.timings is t and r.logprobs is None
    assert qasr.RunResult([[1]], t, [[-0.5]]).logprobs == [[-0.5]]
