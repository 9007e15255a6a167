"""CPU: the resampler to 16 kHz without a device -- the plan, the output length and the tap
table of libqasr.so's host-only entry points against the rule's NumPy restatement (tests/resample_util.py), the C++
reference filter bit for bit against it, the quality of the rule itself on sines, csrc/resample_host.h alone under the
host sanitizers (tools/resample_host_check.cpp), and the CLI's present answer to a 48 kHz file without --resample."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qasr
import resample_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
QASR_ERR_ARG = 1
NAMES = ("qasr_resample_plan", "qasr_resample_len", "qasr_resample_taps", "qasr_resample_host", "qasr_resample",
         "qasr_stage_audio_rate", "qasr_transcribe_batch_rate", "qasr_run_stream_rate", "qasr_kt_resample")
PLANS = {8000: (2, 1, 34), 11025: (640, 441, 34), 12000: (4, 3, 34), 22050: (320, 441, 46), 24000: (2, 3, 51),
         32000: (1, 2, 67), 44100: (160, 441, 92), 48000: (1, 3, 101), 88200: (80, 441, 184), 96000: (1, 6, 201),
         176400: (40, 441, 368), 192000: (1, 12, 401), 16000: (1, 1, 0)}


@pytest.fixture(scope="module")
def lib(built):
    L = qasr.lib()
    for n in NAMES:
        assert hasattr(L, n), n
    return L


def test_plan_of_every_supported_rate(lib):
    assert set(ru.RATES) | {16000} == set(PLANS)
    for sr, want in PLANS.items():
        assert ru.plan(sr) == want, sr                 # the rule's integers (taps a phase: 69 at 8 k, 185 at 44.1 k, 203 at 48 k)
        assert qasr.resample_plan(sr) == want, sr
    assert 2 * PLANS[48000][2] + 1 == 203 and 2 * PLANS[44100][2] + 1 == 185 and 2 * PLANS[8000][2] + 1 == 69


@pytest.mark.parametrize("sr", [44101, 0, -1, 3999, 200000])
def test_unsupported_rates_are_refused_by_name(lib, sr):
    assert not ru.supported(sr)
    assert lib.qasr_resample_plan(sr, None, None, None) == QASR_ERR_ARG
    assert str(sr) in lib.qasr_last_error().decode()
    assert lib.qasr_resample_len(10, sr) == -QASR_ERR_ARG and str(sr) in lib.qasr_last_error().decode()
    assert lib.qasr_resample_taps(sr, None, 0) == -QASR_ERR_ARG
    x = np.zeros(4, f32)
    assert lib.qasr_resample_host(qasr._f(x), 4, sr, qasr._f(x)) == -QASR_ERR_ARG
    with pytest.raises(qasr.QasrError, match=str(sr)):
        qasr.resample_len(10, sr)


def test_output_length_at_the_edges(lib):
    for sr, (L, M, _H) in PLANS.items():
        for n in (0, 1, M - 1, M, M + 1):
            want = (n * L + M - 1) // M
            assert qasr.resample_len(n, sr) == want == ru.out_len(n, sr), (sr, n)
        assert qasr.resample_len(0, sr) == 0 and qasr.resample_len(M, sr) == L
    assert lib.qasr_resample_len(-1, 48000) == -QASR_ERR_ARG
    # 64-bit arithmetic: 2^31 - 1 samples at 48 kHz fit; at 8 kHz the output would not fit int
    assert qasr.resample_len(2 ** 31 - 1, 48000) == (2 ** 31 - 1 + 2) // 3
    assert lib.qasr_resample_len(2 ** 31 - 1, 8000) == -QASR_ERR_ARG and "fit" in lib.qasr_last_error().decode()


@pytest.fixture(scope="module")
def tables(lib):
    """per rate (library table, NumPy table), computed once"""
    return {sr: (qasr.resample_taps(sr), ru.taps(sr)) for sr in PLANS}


def test_taps_within_one_ulp_of_numpy(tables):
    """both sides compute in fp64 with an error far below half an fp32 ulp: only a rounding boundary can differ"""
    for sr, (a, b) in tables.items():
        assert a.shape == b.shape == (PLANS[sr][0], 2 * PLANS[sr][2] + 1), sr
        ulp = np.spacing(np.abs(b).astype(f32)).astype(np.float64)
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        assert (d <= ulp).all(), (sr, float((d / ulp).max()))
        assert (ru.bits(a) == ru.bits(b)).mean() > 0.99, sr
    assert tables[16000][0].tolist() == [[1.0]]
    # the buffer protocol of qasr_resample_taps: the size alone, a short buffer
    L = qasr.lib()
    assert L.qasr_resample_taps(48000, None, 0) == 203
    buf = np.zeros(10, f32)
    assert L.qasr_resample_taps(48000, qasr._f(buf), 10) == -QASR_ERR_ARG


@pytest.mark.parametrize("sr", sorted(PLANS))
def test_host_filter_equals_the_rule_bit_for_bit(tables, sr):
    rng = np.random.default_rng(sr)
    _L, M, H = PLANS[sr]
    h = tables[sr][0]
    for n in (0, 1, 2, H, H + 1, 2 * H + 1, 3 * M + 5, 2500):
        x = rng.standard_normal(n).astype(f32)
        if n:
            x[0] = x[-1] = 1.0
        got, want = qasr.resample_host(x, sr), ru.resample(x, sr, h)
        assert len(got) == len(want) == ru.out_len(n, sr)
        assert (ru.bits(got) == ru.bits(want)).all(), (sr, n)
    if sr == 16000:
        x = np.array([0.0, -0.0, 1e-45, -1.5, 3.0e38], f32)   # a copy: signed zero and denormals as they are
        assert (ru.bits(qasr.resample_host(x, sr)) == ru.bits(x)).all()


def _sine(freq, sr, n):
    return np.sin(2 * np.pi * freq * np.arange(n) / sr + 0.3)


@pytest.mark.parametrize("sr", [8000, 44100, 48000])
def test_quality_of_the_rule(sr):
    """0.5 s sines of amplitude 1 and phase 0.3, the first and last 600 outputs ignored: error against the analytic
    16 kHz sine <= 1e-4 for tones <= 7 kHz, leakage <= 1e-4 for tones >= 8.8 kHz (4 x the worst value measured for
    the rule in NumPy, 2.5e-5).  A condition on the rule, not on the device."""
    h = ru.taps(sr)
    n = sr // 2
    passband = [1000, 3000] if sr == 8000 else [1000, 3000, 6000, 7000]
    stopband = [] if sr == 8000 else [8800, 9000, 10000, 16000]
    for f in passband:
        y = ru.resample(_sine(f, sr, n).astype(f32), sr, h).astype(np.float64)
        err = np.abs(y - _sine(f, 16000, len(y)))[600:-600].max()
        print(f"rate {sr} tone {f}: error {err:.3g}")
        assert err <= 1e-4, (sr, f, err)
    for f in stopband:
        y = ru.resample(_sine(f, sr, n).astype(f32), sr, h)
        leak = np.abs(y)[600:-600].max()
        print(f"rate {sr} tone {f}: leakage {leak:.3g}")
        assert leak <= 1e-4, (sr, f, leak)


def _build_check(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "qwen3-asr.cpp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "resample_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("san", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")])
def test_host_header_alone_and_under_the_sanitizers(tmp_path, san):
    exe = _build_check(tmp_path, "resample_host_check", san)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "resample_host_check OK" in r.stdout, r.stdout + r.stderr


def test_null_arguments(lib):
    lib.qasr_kt_resample.argtypes = [C.c_int, C.c_void_p]
    lib.qasr_kt_resample.restype = C.c_int
    assert lib.qasr_kt_resample(0, None) == QASR_ERR_ARG
    assert lib.qasr_resample(None, None, None, None, 1, None) == QASR_ERR_ARG
    assert lib.qasr_stage_audio_rate(None, None, None, None, 1) == QASR_ERR_ARG
    assert lib.qasr_resample_host(None, 3, 48000, None) == -QASR_ERR_ARG
