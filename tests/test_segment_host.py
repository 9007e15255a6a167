"""CPU: the pause segmentation of long recordings without a device -- the new names, every range of
qasr_segment_validate, qasr_segment_host against the rule's NumPy restatement (tests/segment_util.py) in cuts, peak bits
and silent flags, the two worked cases of the rule (digital silence, a planted pause), and csrc/segment_host.h alone
under the host sanitizers (tools/segment_host_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import qasr
import segment_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
QASR_ERR_ARG = 1
NAMES = ("qasr_segment_validate", "qasr_segment_host", "qasr_segment", "qasr_segment_last_us", "qasr_stage_long",
         "qasr_get_segments")
SMALL = dict(max_frames=8, min_frames=3, smooth_half=2)


@pytest.fixture(scope="module")
def lib(built):
    return qasr.lib()


def test_names_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "qasr_capi.h")).read()
    for n in NAMES + ("qasr_kt_segment",):
        assert re.search(r"\b%s\(" % n, header), n
        assert hasattr(lib, n), n
    for n in NAMES:
        assert n in qasr.EXPORTS, n
    assert "qasr_kt_segment" not in qasr.EXPORTS   # test only
    assert "qasr_segment_params" in header and C.sizeof(qasr.SegmentParams) == 24


def _validate(lib, **kw):
    p = qasr.segment_params(**kw)
    rc = lib.qasr_segment_validate(C.byref(p))
    return rc, lib.qasr_last_error().decode()


def test_every_range_of_validate(lib):
    assert lib.qasr_segment_validate(None) == 0   # the defaults
    assert _validate(lib)[0] == 0
    for ok in (dict(min_frames=1, max_frames=2), dict(max_frames=2 ** 20, min_frames=2 ** 19), dict(smooth_half=0),
               dict(smooth_half=64), dict(skip_ratio=0.0), dict(skip_ratio=float("inf")), dict(skip_ratio=-5.0), SMALL):
        assert _validate(lib, **ok)[0] == 0, ok
    for bad, word in ((dict(min_frames=0), "min_frames"), (dict(min_frames=-3), "min_frames"),
                      (dict(max_frames=1999, min_frames=1000), "max_frames"), (dict(max_frames=1, min_frames=1), "max_frames"),
                      (dict(max_frames=2 ** 20 + 1), "max_frames"), (dict(smooth_half=-1), "smooth_half"),
                      (dict(smooth_half=65), "smooth_half"), (dict(skip_ratio=float("nan")), "skip_ratio")):
        rc, msg = _validate(lib, **bad)
        assert rc == QASR_ERR_ARG and word in msg, (bad, msg)
        with pytest.raises(qasr.QasrError, match=word):
            qasr.segment_validate(**bad)
    # the message names the range
    assert "2 * min_frames <= max_frames <= 1048576" in _validate(lib, max_frames=5, min_frames=3)[1]
    assert "0 <= smooth_half <= 64" in _validate(lib, smooth_half=65)[1]
    # the host rule and the entry points refuse the same parameters
    x = np.zeros(400, f32)
    p = qasr.segment_params(max_frames=5, min_frames=3)
    assert lib.qasr_segment_host(qasr._f(x), 400, C.byref(p), None, None, None, 0) == -QASR_ERR_ARG
    assert lib.qasr_segment_host(None, 400, None, None, None, None, 0) == -QASR_ERR_ARG
    assert lib.qasr_segment_host(qasr._f(x), -1, None, None, None, None, 0) == -QASR_ERR_ARG


def _rec(rng, n):
    # amplitudes over several decades, so that frames differ by far more than rounding
    return (rng.standard_normal(n) * np.exp(rng.uniform(-6, 0, n))).astype(f32)


def _same(segs, want):
    assert [s.start for s in segs] == want["start"] and [s.n for s in segs] == want["n"]
    assert (su.bits([s.peak for s in segs]) == su.bits(want["peak"])).all()
    assert [s.silent for s in segs] == want["silent"]


@pytest.mark.parametrize("tail", [0, 37])
def test_host_equals_the_numpy_rule(lib, tail):
    rng = np.random.default_rng(11 + tail)
    for F in (0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 100):
        x = _rec(rng, 160 * F + tail)
        for skip in (-1.0, 0.3):
            want = su.rule(x, skip_ratio=skip, **SMALL)
            got = qasr.segment_host(x, skip_ratio=skip, **SMALL)
            _same(got, want)
            # lengths within [min, max] once there is more than one segment; starts and lengths tile [0, n)
            assert got[0].start == 0 and sum(s.n for s in got) == len(x)
            assert all(a.start + a.n == b.start for a, b in zip(got, got[1:]))
            if len(got) > 1:
                assert all(3 <= s.n // 160 <= 8 for s in got[:-1]) and 3 <= (got[-1].n - tail) // 160 <= 8, (F, [s.n for s in got])
            assert len(got) >= 1 and (F <= 8) == (len(got) == 1)


def test_digital_silence_cuts_every_max_frames(lib):
    """equal values go to the larger frame: the longest segments, not the shortest"""
    x = np.zeros(160 * 100 + 5, f32)
    got = qasr.segment_host(x, **SMALL)
    cuts = [s.start // 160 for s in got]
    assert cuts[:11] == list(range(0, 88, 8)) and cuts == su.rule(x, **SMALL)["cuts"]
    assert all(s.n == 8 * 160 for s in got[:-2])
    assert cuts[:3] != [0, 3, 6]   # (the other tie)
    assert all(s.peak == 0.0 for s in got) and not any(s.silent for s in got)   # skip_ratio -1: never silent


def test_planted_pause_is_the_cut(lib):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(160 * 300) * 0.1).astype(f32)
    x[160 * 140:160 * 160] = 0.0
    want = su.rule(x, max_frames=200, min_frames=80, smooth_half=5)
    assert (want["s"][145:155] == 0.0).all() and want["s"][144] > 0 and want["s"][155] > 0
    got = qasr.segment_host(x, max_frames=200, min_frames=80, smooth_half=5)
    assert [s.start for s in got] == [0, 154 * 160] == want["start"]


def test_skip_ratio_on_a_recording_with_one_silent_segment(lib):
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(160 * 24) * 0.1).astype(f32)
    x[160 * 8:160 * 17] = 0.0   # frames 8 .. 16: the second cut's tie among 12 .. 16 goes to 16
    prm = dict(max_frames=8, min_frames=4, smooth_half=0)
    base = qasr.segment_host(x, skip_ratio=-1.0, **prm)
    assert [s.start // 160 for s in base] == [0, 8, 16] and base[1].peak == 0.0 and base[0].peak > 0 and base[2].peak > 0
    assert [s.silent for s in base] == [False, False, False]
    assert [s.silent for s in qasr.segment_host(x, skip_ratio=0.0, **prm)] == [False, True, False]
    assert [s.silent for s in qasr.segment_host(x, skip_ratio=1e-6, **prm)] == [False, True, False]
    assert [s.silent for s in qasr.segment_host(x, skip_ratio=1.0, **prm)] == [True, True, True]   # peak <= 1 * peak_rec
    for skip in (-1.0, 0.0, 1e-6, 1.0):
        _same(qasr.segment_host(x, skip_ratio=skip, **prm), su.rule(x, skip_ratio=skip, **prm))


def test_short_buffer_and_empty_recording(lib):
    x = np.zeros(160 * 100, f32)
    p = qasr.segment_params(**SMALL)
    cuts = np.full(4, -7, np.int32)
    K = lib.qasr_segment_host(qasr._f(x), len(x), C.byref(p), qasr._i(cuts), None, None, 3)
    assert K == 13 and cuts.tolist() == [0, 8, 16, -7]   # the count may exceed cap: nothing past cap is written
    one = qasr.segment_host(np.zeros(0, f32), **SMALL)
    assert len(one) == 1 and (one[0].start, one[0].n, one[0].peak, one[0].silent) == (0, 0, 0.0, False)
    one = qasr.segment_host(np.ones(159, f32), skip_ratio=0.0, **SMALL)
    assert len(one) == 1 and (one[0].n, one[0].peak, one[0].silent) == (159, 0.0, True)   # no frame: peak 0 <= 0 * 0


def _build_check(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "qwen3-asr.cpp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "segment_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("san", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")])
def test_host_header_alone_and_under_the_sanitizers(tmp_path, san):
    exe = _build_check(tmp_path, "segment_host_check", san)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "segment_host_check OK" in r.stdout, r.stdout + r.stderr


def test_null_arguments(lib):
    lib.qasr_kt_segment.argtypes = [C.c_int, C.c_void_p]
    lib.qasr_kt_segment.restype = C.c_int
    assert lib.qasr_kt_segment(0, None) == QASR_ERR_ARG
    assert lib.qasr_segment(None, None, None, 1, None, None, None, None, None, None, None, None, 0) == QASR_ERR_ARG
    assert lib.qasr_stage_long(None, None, None, None, 1, None) == -QASR_ERR_ARG
    assert lib.qasr_get_segments(None, 0, None, None, None, None, 0) == -QASR_ERR_ARG
    assert lib.qasr_segment_last_us(None, None) == -QASR_ERR_ARG
