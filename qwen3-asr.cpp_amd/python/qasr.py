"""qasr -- ctypes binding of libqasr.so (include/qasr_capi.h).

Host-side mirror of the reference's Qwen3ASR / AudioEncoder / TextDecoder
surface (src/qwen3_asr.h:55-116, src/audio_encoder.h:27-33,
src/text_decoder.h:116-137) for tests, bench and scripting.  Every call goes
through the C-ABI into hand-written HIP kernels; there is no CPU fallback:
loading fails loudly if the in-tree libqasr.so is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("QASR_LIB_OVERRIDE") or os.path.join(PKG_DIR, "libqasr.so")   # (override: diagnostic builds only)

EXPORTS = [
    "qasr_last_error", "qasr_version", "qasr_device_count", "qasr_check_expf_nonpos",
    "qasr_model_load", "qasr_model_free", "qasr_model_hparams", "qasr_model_device_bytes",
    "qasr_ctx_create", "qasr_ctx_free",
    "qasr_mel_frames", "qasr_encoder_frames", "qasr_prompt_len", "qasr_build_prompt",
    "qasr_mel", "qasr_encode", "qasr_encode_conv", "qasr_encode_no_chunk", "qasr_encoder_frames_no_chunk",
    "qasr_prefill", "qasr_prefill_chunk", "qasr_prefill_chunk_audio", "qasr_decode_step",
    "qasr_stage_audio", "qasr_run", "qasr_run_staged", "qasr_run_stream", "qasr_run_stream_staged", "qasr_set_system_prompt", "qasr_transcribe_batch",
    "qasr_set_probe", "qasr_get_probe", "qasr_get_probe_device",
    "qasr_ctx_set_option", "qasr_ctx_get_option", "qasr_debug_read",
    "qasr_set_token_callback", "qasr_set_profile", "qasr_profile_report",
    "qasr_detokenize", "qasr_tokenize",
    "qasr_load_wav", "qasr_write_wav", "qasr_synth_pcm", "qasr_write_synthetic_gguf", "qasr_synthetic_gguf_version",
    "qasr_align", "qasr_align_tokenize", "qasr_model_load_korean_dict", "qasr_fix_timestamps",
    "qasr_align_prompt_len", "qasr_align_json", "qasr_align_json_batch", "qasr_align_words",
    "qasr_ctx_grow_shape",
    "qasr_get_step_logprobs", "qasr_get_logprobs", "qasr_stream_logprobs",
    "qasr_get_step_topk", "qasr_get_topk", "qasr_stream_topk",
    "qasr_kv_fork", "qasr_get_beams", "qasr_prefill_slots",
    "qasr_prefill_score", "qasr_score",
    "qasr_set_sampling", "qasr_get_sampling", "qasr_set_sample_streams", "qasr_get_samples",
    "qasr_constraints_validate", "qasr_set_constraints", "qasr_get_constraints",
    "qasr_phrases_validate", "qasr_set_phrases", "qasr_get_phrases", "qasr_phrase_tokenize",
    "qasr_resample_plan", "qasr_resample_len", "qasr_resample_taps", "qasr_resample_host",
    "qasr_resample", "qasr_resample_last_us", "qasr_stage_audio_rate", "qasr_transcribe_batch_rate", "qasr_run_stream_rate",
    "qasr_segment_validate", "qasr_segment_host", "qasr_segment", "qasr_segment_last_us", "qasr_stage_long", "qasr_get_segments",
]


class Hparams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("enc_layers", "d_model", "enc_heads", "enc_ffn", "conv_channels", "n_mel")] + [
        ("enc_eps", C.c_float)] + [(n, C.c_int32) for n in (
            "vocab_size", "hidden_size", "dec_layers", "n_heads", "n_kv_heads", "head_dim", "dec_ffn")] + [
        ("rms_eps", C.c_float), ("rope_theta", C.c_float)] + [(n, C.c_int32) for n in (
            "eos_id", "pad_id", "audio_start_id", "audio_end_id", "audio_pad_id", "weight_type",
            "classify_num", "timestamp_token_id")]


class Timings(C.Structure):
    _fields_ = [("t_mel_ms", C.c_double), ("t_encode_ms", C.c_double), ("t_prefill_ms", C.c_double),
                ("t_decode_ms", C.c_double), ("t_total_ms", C.c_double), ("n_decode_steps", C.c_int32)]


class StreamStats(C.Structure):
    _fields_ = [("n_clips", C.c_int32), ("n_errors", C.c_int32), ("n_prefills", C.c_int32), ("n_steps", C.c_int64),
                ("slot_steps", C.c_int64), ("live_steps", C.c_int64), ("t_prefill_ms", C.c_double),
                ("t_decode_ms", C.c_double), ("t_total_ms", C.c_double), ("t_mel_ms", C.c_double),
                ("t_encode_ms", C.c_double), ("kv_keys", C.c_int64)]


class Sampling(C.Structure):
    """qasr_sampling"""
    _fields_ = [("temperature", C.c_float), ("min_p", C.c_float), ("seed", C.c_uint64), ("n_best", C.c_int32)]


class Constraints(C.Structure):
    """qasr_constraints"""
    _fields_ = [("no_repeat_ngram", C.c_int32), ("repetition_penalty", C.c_float), ("penalty_last_n", C.c_int32),
                ("n_bias", C.c_int32), ("bias_ids", C.POINTER(C.c_int32)), ("bias", C.POINTER(C.c_float))]


class Phrases(C.Structure):
    """qasr_phrases"""
    _fields_ = [("n_phrases", C.c_int32), ("ids", C.POINTER(C.c_int32)), ("len", C.POINTER(C.c_int32)),
                ("boost", C.POINTER(C.c_float))]


class SegmentParams(C.Structure):
    """qasr_segment_params"""
    _fields_ = [("max_frames", C.c_int32), ("min_frames", C.c_int32), ("smooth_half", C.c_int32), ("skip_ratio", C.c_double)]


QASR_BEAM_MAX = 8
QASR_SAMPLE_MAX = 8
QASR_NGRAM_MAX = 8
QASR_BIAS_MAX = 1024
QASR_PHRASE_MAX = 4096
QASR_PHRASE_LEN_MAX = 16
_lib = None
# void (*)(void *user, int seq, int n_generated, int32_t token)
TOKEN_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int32)
# int (*)(void *user, const float **pcm, int *n_samples, int *max_tokens)
FETCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int), C.POINTER(C.c_int))
# int (*)(void *user, const float **pcm, int *n_samples, int *rate, int *max_tokens)
FETCH_RATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int), C.POINTER(C.c_int),
                            C.POINTER(C.c_int))
# int (*)(void *user, int *max_tokens)
FETCH_STAGED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int))
# void (*)(void *user, int id, int status, const int32_t *tokens, int n_tokens)
SINK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int)


def lib() -> C.CDLL:
    """Load the in-tree libqasr.so (raises if it was not built).  A process
    that also uses torch's HIP (torch.distributed over RCCL) initialises that
    first: torch bundles its own libamdhip64 / libhsa-runtime, which
    libqasr.so then binds to by soname; loaded before them, two HSA runtimes
    end up in one process and torch's, initialised second, sees no device
    (or the other way round)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libqasr.so not built at {LIB_PATH} (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        P, I, F = C.c_void_p, C.c_int, C.POINTER(C.c_float)
        I32P, IP, DP = C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_double)
        sig = {
            "qasr_last_error": ([], C.c_char_p), "qasr_version": ([], C.c_char_p),
            "qasr_device_count": ([IP], I),
            "qasr_check_expf_nonpos": ([I, C.POINTER(C.c_uint64)], I),
            "qasr_model_load": ([C.c_char_p, I, C.POINTER(P)], I), "qasr_model_free": ([P], None),
            "qasr_model_hparams": ([P, C.POINTER(Hparams)], I), "qasr_model_device_bytes": ([P], C.c_int64),
            "qasr_ctx_create": ([P, I, I, C.POINTER(P)], I), "qasr_ctx_free": ([P], None),
            "qasr_mel_frames": ([I], I), "qasr_encoder_frames": ([I], I), "qasr_prompt_len": ([I], I),
            "qasr_build_prompt": ([P, I, I32P, IP], I),
            "qasr_mel": ([P, C.POINTER(F), IP, I, F], I),
            "qasr_encode": ([P, F, IP, I, F], I), "qasr_encode_conv": ([P, F, IP, I, F], I),
            "qasr_encode_no_chunk": ([P, F, IP, I, F], I), "qasr_encoder_frames_no_chunk": ([I], I),
            "qasr_prefill": ([P, I32P, IP, F, IP, IP, I, F, I32P], I),
            "qasr_decode_step": ([P, I32P, IP, I, F, I32P], I),
            "qasr_prefill_chunk": ([P, I32P, IP, IP, I, F, I32P], I),
            "qasr_prefill_chunk_audio": ([P, I32P, IP, IP, F, IP, IP, I, F, I32P], I),
            "qasr_stage_audio": ([P, C.POINTER(F), IP, I], I),
            "qasr_run": ([P, I, I, I32P, IP, C.POINTER(Timings)], I),
            "qasr_run_staged": ([P, IP, I, I, I, I32P, IP, C.POINTER(Timings)], I),
            "qasr_run_stream": ([P, I, FETCH_FN, SINK_FN, P, I, I, C.POINTER(StreamStats)], I),
            "qasr_run_stream_staged": ([P, I, FETCH_STAGED_FN, SINK_FN, P, I, I, C.POINTER(StreamStats)], I),
            "qasr_set_system_prompt": ([P, I32P, I], I),
            "qasr_transcribe_batch": ([P, C.POINTER(F), IP, I, I, I, I32P, IP, C.POINTER(Timings)], I),
            "qasr_set_probe": ([P, I], I),
            "qasr_get_probe": ([P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)], I),
            "qasr_get_probe_device": ([P, C.POINTER(C.c_double), C.POINTER(C.c_int64)], I),
            "qasr_ctx_set_option": ([P, C.c_char_p, I], I), "qasr_ctx_get_option": ([P, C.c_char_p, IP], I),
            "qasr_debug_read": ([P, C.c_char_p, P, C.c_int64], I),
            "qasr_get_step_logprobs": ([P, F, I], I), "qasr_get_logprobs": ([P, F, I, I], I),
            "qasr_stream_logprobs": ([P, F, I], I),
            "qasr_get_step_topk": ([P, I32P, F, I, I], I), "qasr_get_topk": ([P, I32P, F, I, I, I], I),
            "qasr_stream_topk": ([P, I32P, F, I, I], I),
            "qasr_kv_fork": ([P, IP, IP, IP, I, I], I),
            "qasr_get_beams": ([P, I, I32P, F, IP, F, IP, I, I], I),
            "qasr_prefill_slots": ([P, I32P, IP, F, IP, IP, IP, I, F, I32P], I),
            "qasr_prefill_score": ([P, I32P, IP, IP, F, IP, IP, IP, I, I32P, F, I32P, F, I], I),
            "qasr_score": ([P, IP, I32P, IP, I, I, F, I32P, F, F, C.POINTER(Timings)], I),
            "qasr_set_sampling": ([P, C.POINTER(Sampling)], I), "qasr_get_sampling": ([P, C.POINTER(Sampling)], I),
            "qasr_set_sample_streams": ([P, I32P, I32P, I32P, I], I),
            "qasr_get_samples": ([P, I, I32P, F, IP, F, I, I], I),
            "qasr_constraints_validate": ([C.POINTER(Constraints), I], I),
            "qasr_set_constraints": ([P, C.POINTER(Constraints)], I),
            "qasr_get_constraints": ([P, C.POINTER(Constraints), I32P, F, I], I),
            "qasr_phrases_validate": ([C.POINTER(Phrases), I], I),
            "qasr_set_phrases": ([P, C.POINTER(Phrases)], I),
            "qasr_get_phrases": ([P, C.POINTER(Phrases), I32P, I32P, F, I, I], I),
            "qasr_phrase_tokenize": ([P, C.c_char_p, I32P, I32P, I], I),
            "qasr_resample_plan": ([I, IP, IP, IP], I), "qasr_resample_len": ([I, I], I),
            "qasr_resample_taps": ([I, F, I], I), "qasr_resample_host": ([F, I, I, F], I),
            "qasr_resample": ([P, C.POINTER(F), IP, IP, I, F], I),
            "qasr_resample_last_us": ([P], I),
            "qasr_stage_audio_rate": ([P, C.POINTER(F), IP, IP, I], I),
            "qasr_transcribe_batch_rate": ([P, C.POINTER(F), IP, IP, I, I, I, I32P, IP, C.POINTER(Timings)], I),
            "qasr_run_stream_rate": ([P, I, FETCH_RATE_FN, SINK_FN, P, I, I, C.POINTER(StreamStats)], I),
            "qasr_segment_validate": ([C.POINTER(SegmentParams)], I),
            "qasr_segment_host": ([F, I, C.POINTER(SegmentParams), IP, DP, IP, I], I),
            "qasr_segment": ([P, C.POINTER(F), IP, I, C.POINTER(SegmentParams), DP, DP, IP, DP, IP, IP, DP, I], I),
            "qasr_segment_last_us": ([P, IP], I),
            "qasr_stage_long": ([P, C.POINTER(F), IP, IP, I, C.POINTER(SegmentParams)], I),
            "qasr_get_segments": ([P, I, C.POINTER(C.c_longlong), IP, DP, IP, I], I),
            "qasr_set_token_callback": ([P, TOKEN_CB, P], I),
            "qasr_set_profile": ([P, I], I), "qasr_profile_report": ([P, C.c_char_p, I], I),
            "qasr_detokenize": ([P, I32P, I, C.c_char_p, I], I), "qasr_tokenize": ([P, C.c_char_p, I32P, I], I),
            "qasr_load_wav": ([C.c_char_p, F, I, IP], I), "qasr_write_wav": ([C.c_char_p, F, I, I], I),
            "qasr_synth_pcm": ([C.c_uint64, I, F], I),
            "qasr_write_synthetic_gguf": ([C.c_char_p, C.c_char_p, C.c_uint64, I], I),
            "qasr_synthetic_gguf_version": ([], I),
            "qasr_align": ([P, F, I, I32P, I, I32P, I, IP, C.POINTER(Timings)], I),
            "qasr_align_tokenize": ([P, C.c_char_p, C.c_char_p, I32P, I, IP], I),
            "qasr_model_load_korean_dict": ([P, C.c_char_p], I),
            "qasr_fix_timestamps": ([I32P, I, I32P], I),
            "qasr_ctx_grow_shape": ([I, I, I, I, IP, IP], None),
            "qasr_align_prompt_len": ([I, I], I),
            "qasr_align_words": ([P, C.c_char_p, C.c_char_p, C.c_char_p, I], I),
            "qasr_align_json": ([P, F, I, C.c_char_p, C.c_char_p, C.c_char_p, I, C.POINTER(Timings)], I),
            "qasr_align_json_batch": ([P, C.POINTER(F), IP, C.POINTER(C.c_char_p), I, C.c_char_p, C.c_char_p, I,
                                       C.POINTER(Timings)], I),
        }
        for name, (args, res) in sig.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _lib = L
    return _lib


class QasrError(RuntimeError):
    pass


def make_constraints(no_repeat_ngram: int = 0, repetition_penalty: float = 1.0, penalty_last_n: int = 0, bias=None,
                     suppress=None):
    """a qasr_constraints from Python values, with the arrays it points into (keep them alive as long as it is
    used); a token both biased and suppressed is suppressed"""
    table = {int(i): float(b) for i, b in (bias or {}).items()}
    for i in (suppress or ()):
        table[int(i)] = float("-inf")
    ids = np.array(list(table.keys()), np.int32)
    val = np.array(list(table.values()), np.float32)
    k = Constraints(int(no_repeat_ngram), float(repetition_penalty), int(penalty_last_n), len(ids),
                    _i32(ids) if len(ids) else None, _f(val) if len(ids) else None)
    return k, (ids, val)


def constraints_validate(vocab: int = 0, **kw) -> None:
    """qasr_constraints_validate (host only): raises QasrError naming the violated range"""
    k, _keep = make_constraints(**kw)
    _check(lib().qasr_constraints_validate(C.byref(k), int(vocab)), "qasr_constraints_validate")


def make_phrases(phrases, boost: float = 5.0, tokenize=None):
    """a qasr_phrases from Python values, with the arrays it points into (keep them alive as long as it is used).
    Each phrase is a list of ids, an (ids, boost) pair or a string; a string goes through `tokenize` (text ->
    list of id lists: Model.phrase_tokenize) and yields every variant; `boost` is the boost of a phrase without
    its own"""
    ids, lens, val = [], [], []
    for ph in phrases or ():
        b = float(boost)
        if isinstance(ph, tuple) and len(ph) == 2 and not isinstance(ph[0], (int, np.integer)):
            ph, b = ph[0], float(ph[1])
        if isinstance(ph, str):
            if tokenize is None:
                raise QasrError("a phrase given as text needs the model's tokenizer")
            variants = tokenize(ph)
        else:
            variants = [[int(x) for x in ph]]
        for v in variants:
            ids += v
            lens.append(len(v))
            val.append(b)
    a_ids, a_len, a_val = np.array(ids or [0], np.int32), np.array(lens or [0], np.int32), np.array(val or [0], np.float32)
    p = Phrases(len(lens), _i32(a_ids), _i32(a_len), _f(a_val))
    return p, (a_ids, a_len, a_val)


def phrases_validate(phrases, boost: float = 5.0, vocab: int = 0) -> None:
    """qasr_phrases_validate (host only): raises QasrError naming the violated range"""
    p, _keep = make_phrases(phrases, boost)
    _check(lib().qasr_phrases_validate(C.byref(p), int(vocab)), "qasr_phrases_validate")


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise QasrError(f"{what}: {lib().qasr_last_error().decode(errors='replace')}")


def _f(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i32(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _i(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int))


# ------------------------------------------------------------------ host utils
def mel_frames(n: int) -> int:
    return lib().qasr_mel_frames(n)


def encoder_frames(T: int) -> int:
    return lib().qasr_encoder_frames(T)


def synth_pcm(seed: int, n: int) -> np.ndarray:
    out = np.zeros(n, np.float32)
    _check(lib().qasr_synth_pcm(seed, n, _f(out)), "synth_pcm")
    return out


def write_synthetic_gguf(path: str, config: str = "tiny", seed: int = 42, wtype: int = 1) -> None:
    _check(lib().qasr_write_synthetic_gguf(path.encode(), config.encode(), seed, wtype), "write_synthetic_gguf")


def load_wav(path: str):
    sr = C.c_int(0)
    n = lib().qasr_load_wav(path.encode(), None, 0, C.byref(sr))
    if n < 0:
        raise QasrError(f"load_wav: {lib().qasr_last_error().decode()}")
    out = np.zeros(n, np.float32)
    lib().qasr_load_wav(path.encode(), _f(out), n, C.byref(sr))
    return out, sr.value


def write_wav(path: str, pcm: np.ndarray, sr: int = 16000) -> None:
    pcm = np.ascontiguousarray(pcm, np.float32)
    _check(lib().qasr_write_wav(path.encode(), _f(pcm), len(pcm), sr), "write_wav")


# ---- the resampler to 16 kHz (host only) ----
def _neg(rc: int, what: str) -> int:
    if rc < 0:
        raise QasrError(f"{what}: {lib().qasr_last_error().decode(errors='replace')}")
    return rc


def resample_plan(rate: int) -> Tuple[int, int, int]:
    """(L, M, H) of a rate: 16000 / gcd, rate / gcd, taps a side; raises QasrError for an unsupported rate"""
    L, M, H = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().qasr_resample_plan(int(rate), C.byref(L), C.byref(M), C.byref(H)), "qasr_resample_plan")
    return L.value, M.value, H.value


def resample_len(n_in: int, rate: int) -> int:
    """samples at 16 kHz of n_in samples at `rate`"""
    return _neg(lib().qasr_resample_len(int(n_in), int(rate)), "qasr_resample_len")


def resample_taps(rate: int) -> np.ndarray:
    """the tap table h[L][2H + 1] of a rate (fp32)"""
    L, _M, H = resample_plan(rate)
    out = np.zeros((L, 2 * H + 1), np.float32)
    _neg(lib().qasr_resample_taps(int(rate), _f(out), out.size), "qasr_resample_taps")
    return out


def resample_host(pcm: np.ndarray, rate: int) -> np.ndarray:
    """the rule on the CPU (qasr_resample_host): the reference of the device resampler"""
    pcm = np.ascontiguousarray(pcm, np.float32)
    out = np.zeros(max(resample_len(len(pcm), rate), 1), np.float32)
    n = _neg(lib().qasr_resample_host(_f(pcm), len(pcm), int(rate), _f(out)), "qasr_resample_host")
    return out[:n]


# ---- pause segmentation of long recordings (host only) ----
def _d(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def segment_params(max_frames: int = 3000, min_frames: int = 1000, smooth_half: int = 5, skip_ratio: float = -1.0) -> SegmentParams:
    return SegmentParams(int(max_frames), int(min_frames), int(smooth_half), float(skip_ratio))


def segment_validate(**kw) -> None:
    """raises QasrError naming the violated range (qasr_segment_validate)"""
    p = segment_params(**kw)
    _check(lib().qasr_segment_validate(C.byref(p)), "qasr_segment_validate")


@dataclass
class Segment:
    rec: int          # the recording it belongs to
    start: int        # 16 kHz samples from the recording's own start
    n: int            # samples
    peak: float       # the maximum smoothed energy of its frames
    silent: bool


def segment_host(pcm: np.ndarray, **kw) -> List["Segment"]:
    """the rule on the CPU (qasr_segment_host): the reference of the device segmentation"""
    pcm = np.ascontiguousarray(pcm, np.float32)
    p = segment_params(**kw)
    K = _neg(lib().qasr_segment_host(_f(pcm), len(pcm), C.byref(p), None, None, None, 0), "qasr_segment_host")
    cuts, peak, silent = np.zeros(K, np.int32), np.zeros(K, np.float64), np.zeros(K, np.int32)
    _neg(lib().qasr_segment_host(_f(pcm), len(pcm), C.byref(p), _i(cuts), _d(peak), _i(silent), K), "qasr_segment_host")
    ends = [int(c) * 160 for c in cuts[1:]] + [len(pcm)]
    return [Segment(0, int(cuts[k]) * 160, ends[k] - int(cuts[k]) * 160, float(peak[k]), bool(silent[k])) for k in range(K)]


def fix_timestamps(classes: Sequence[int]) -> List[int]:
    """LIS repair of raw timestamp classes (src/forced_aligner.cpp:1183-1265)."""
    a = np.ascontiguousarray(classes, np.int32)
    out = np.zeros(max(len(a), 1), np.int32)
    _check(lib().qasr_fix_timestamps(_i32(a) if len(a) else None, len(a), _i32(out) if len(a) else None), "fix_timestamps")
    return out[:len(a)].tolist()


def align_prompt_len(n_samples: int, n_text: int) -> int:
    return lib().qasr_align_prompt_len(n_samples, n_text)


def device_count() -> int:
    n = C.c_int(0)
    lib().qasr_device_count(C.byref(n))
    return n.value


# ---------------------------------------------------------------------- model
class Model:
    """qasr_model: weights in one device arena (src/qwen3_asr.cpp:21-42)."""

    def __init__(self, path: str, device: int = 0):
        self.h = C.c_void_p()
        _check(lib().qasr_model_load(path.encode(), device, C.byref(self.h)), "qasr_model_load")
        hp = Hparams()
        _check(lib().qasr_model_hparams(self.h, C.byref(hp)), "qasr_model_hparams")
        self.hp = hp
        self.path = path

    def close(self):
        if self.h:
            lib().qasr_model_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self) -> int:
        return lib().qasr_model_device_bytes(self.h)

    def build_prompt(self, n_audio: int):
        P = lib().qasr_prompt_len(n_audio)
        ids = np.zeros(P, np.int32)
        pos = C.c_int(0)
        lib().qasr_build_prompt(self.h, n_audio, _i32(ids), C.byref(pos))
        return ids, pos.value

    def detokenize(self, ids: Sequence[int]) -> str:
        a = np.ascontiguousarray(ids, np.int32)
        n = lib().qasr_detokenize(self.h, _i32(a), len(a), None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().qasr_detokenize(self.h, _i32(a), len(a), buf, n + 1)
        return buf.raw[:n].decode("utf-8", errors="replace")

    def tokenize(self, text: str) -> List[int]:
        n = lib().qasr_tokenize(self.h, text.encode(), None, 0)
        a = np.zeros(max(n, 1), np.int32)
        lib().qasr_tokenize(self.h, text.encode(), _i32(a), n)
        return a[:n].tolist()


    def phrase_tokenize(self, text: str) -> List[List[int]]:
        """qasr_phrase_tokenize: the tokenisations a hotword needs, of the trimmed text and of " " + text (one
        where they are equal)"""
        ids, ln = np.zeros(2 * QASR_PHRASE_LEN_MAX, np.int32), np.zeros(2, np.int32)
        n = lib().qasr_phrase_tokenize(self.h, text.encode(), _i32(ids), _i32(ln), len(ids))
        if n < 0:
            raise QasrError(f"qasr_phrase_tokenize: {lib().qasr_last_error().decode(errors='replace')}")
        out, at = [], 0
        for i in range(n):
            out.append(ids[at:at + ln[i]].tolist())
            at += int(ln[i])
        return out

    # ---- forced aligner (Qwen3-ForcedAligner files) -------------------------
    @property
    def is_aligner(self) -> bool:
        return self.hp.classify_num > 0

    def align_tokenize(self, text: str, language: str = ""):
        """ForcedAligner::tokenize_with_timestamps -> (ids, n_words)."""
        nw = C.c_int(0)
        n = lib().qasr_align_tokenize(self.h, text.encode(), language.encode(), None, 0, C.byref(nw))
        a = np.zeros(max(n, 1), np.int32)
        lib().qasr_align_tokenize(self.h, text.encode(), language.encode(), _i32(a), n, C.byref(nw))
        return a[:n].tolist(), nw.value

    def align_words(self, text: str, language: str = "") -> List[str]:
        n = lib().qasr_align_words(self.h, text.encode(), language.encode(), None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().qasr_align_words(self.h, text.encode(), language.encode(), buf, n + 1)
        s = buf.raw[:n].decode("utf-8")
        return s.split("\n") if s else []

    def load_korean_dict(self, path: str) -> None:
        _check(lib().qasr_model_load_korean_dict(self.h, path.encode()), "qasr_model_load_korean_dict")


@dataclass
class RunResult:
    tokens: List[List[int]]
    timings: Timings
    # log-probability of every token (context option "token_logprobs"), the shape of tokens; None with the option off
    logprobs: Optional[List[List[float]]] = None
    # the K most likely tokens of every step (context option "top_k"): per row (ids [n][K] int32, logprobs [n][K]
    # float32), n the row's tokens and entry 0 of a step the token itself; None with the option off
    topk: Optional[List[Tuple[np.ndarray, np.ndarray]]] = None
    # every hypothesis of every clip of a beam run (context option "beam_width" >= 2), best first; tokens[b] is
    # beams[b][0].tokens; None after a greedy run
    beams: Optional[List[List["Beam"]]] = None
    # every hypothesis of every clip of a sampling run (Context.set_sampling), in sample order; tokens[b] is
    # samples[b][0].tokens; None with sampling off
    samples: Optional[List[List["Sample"]]] = None


@dataclass
class Sample:
    tokens: List[int]
    logprobs: List[float]      # log softmax(logits)[token] at T = 1, one per token (a popped EOS takes its value with it)
    sum_logprob: float         # ... but the sum counts the EOS step


@dataclass
class Beam:
    tokens: List[int]
    logprobs: List[float]      # one per token (a popped EOS takes its value with it)
    sum_logprob: float         # ... but the sum counts the EOS step
    finished: bool


@dataclass
class Score:
    """one scored sequence (Context.score / Context.prefill_score): per scored position the log-probability
    of the given token, the model's own greedy token there and that token's log-probability"""
    logprobs: np.ndarray         # float32 [n]
    greedy_ids: np.ndarray       # int32 [n]
    greedy_logprobs: np.ndarray  # float32 [n]
    sum: float                   # float32 sum of logprobs, in order


def _sink_into(out: dict, failed: list, ctx=None, tk_ctx=None):
    """ctx: the running context when the caller asked for log-probabilities --
    the sink then stores (tokens, logprobs) per clip (qasr_stream_logprobs);
    tk_ctx: likewise for the top-K alternatives -- (ids [n][K], logprobs
    [n][K]) is appended to the clip's tuple (qasr_stream_topk)"""
    def sink(_u, cid, status, toks, n):
        try:
            if status:
                out[cid] = QasrError(lib().qasr_last_error().decode(errors="replace"))
                return
            item = [[int(toks[i]) for i in range(n)]]
            if ctx is not None:
                lp = np.zeros(max(n, 1), np.float32)
                k = lib().qasr_stream_logprobs(ctx.h, _f(lp), n)
                if k != n:
                    raise QasrError(f"qasr_stream_logprobs: {lib().qasr_last_error().decode(errors='replace')}")
                item.append(lp[:n].tolist())
            if tk_ctx is not None:
                K = max(tk_ctx.get_option("top_k"), 1)
                ids, lps = np.zeros((max(n, 1), K), np.int32), np.zeros((max(n, 1), K), np.float32)
                k = lib().qasr_stream_topk(tk_ctx.h, _i32(ids), _f(lps), n, K)
                if k != n:
                    raise QasrError(f"qasr_stream_topk: {lib().qasr_last_error().decode(errors='replace')}")
                item.append((ids[:n], lps[:n]))
            out[cid] = item[0] if len(item) == 1 else tuple(item)
        except BaseException as e:   # (ctypes would swallow it)
            failed.append(e)
    return sink


def _guarded_fetch(fetch, failed: list):
    """A ctypes callback cannot raise: an exception in next_clip() (e.g. a
    TCPStore failure of the shared queue) is stored, the queue reported empty
    (-1, so the engine drains its slots and returns), and the caller re-raises
    it after the run instead of the engine taking 0 as a clip id."""
    def f(*a):
        if failed:
            return -1
        try:
            return fetch(*a)
        except BaseException as e:
            failed.append(e)
            return -1
    return f


class Context:
    """qasr_ctx: stream, KV cache, scratch (TextDecoder::init_kv_cache analogue)."""

    def __init__(self, model: Model, max_batch: int = 1, max_ctx: int = 2048):
        self.model = model
        self.h = C.c_void_p()
        _check(lib().qasr_ctx_create(model.h, max_batch, max_ctx, C.byref(self.h)), "qasr_ctx_create")
        self.max_batch, self.max_ctx = max_batch, max_ctx

    def close(self):
        if self.h:
            lib().qasr_ctx_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stages ------------------------------------------------------------
    def mel(self, clips: Sequence[np.ndarray]) -> List[np.ndarray]:
        clips = [np.ascontiguousarray(c, np.float32) for c in clips]
        n = np.array([len(c) for c in clips], np.int32)
        T = [mel_frames(int(k)) for k in n]
        out = np.zeros(max(1, 128 * sum(T)), np.float32)
        ptrs = (C.POINTER(C.c_float) * len(clips))(*[_f(c) for c in clips])
        _check(lib().qasr_mel(self.h, ptrs, _i(n), len(clips), _f(out)), "qasr_mel")
        res, o = [], 0
        for t in T:
            res.append(out[o:o + 128 * t].reshape(128, t))
            o += 128 * t
        return res

    def resample(self, clips: Sequence[np.ndarray], rates: Sequence[int]) -> List[np.ndarray]:
        """qasr_resample: clips at `rates` -> the clips at 16 kHz, resampled on the device"""
        clips = [np.ascontiguousarray(c, np.float32) for c in clips]
        n = np.array([len(c) for c in clips], np.int32)
        r = np.ascontiguousarray(rates, np.int32)
        if len(r) != len(clips):
            raise QasrError("resample: one rate per clip")
        no = [resample_len(int(k), int(q)) for k, q in zip(n, r)]
        out = np.zeros(max(1, sum(no)), np.float32)
        ptrs = (C.POINTER(C.c_float) * len(clips))(*[_f(c) for c in clips])
        _check(lib().qasr_resample(self.h, ptrs, _i(n), _i(r), len(clips), _f(out)), "qasr_resample")
        res, o = [], 0
        for k in no:
            res.append(out[o:o + k].copy())
            o += k
        return res

    def segment(self, recs: Sequence[np.ndarray], want_energy: bool = False, **kw):
        """qasr_segment: recordings at 16 kHz -> per recording its List[Segment], cut on the device (the pool stays as it
        is).  want_energy: -> (segments, e per recording, s per recording), the frame and smoothed energies (float64)"""
        recs = [np.ascontiguousarray(c, np.float32) for c in recs]
        B = len(recs)
        n = np.array([len(c) for c in recs], np.int32)
        p = segment_params(**kw)
        _check(lib().qasr_segment_validate(C.byref(p)), "qasr_segment_validate")
        F = [int(k) // 160 for k in n]
        cap = max(f // p.min_frames + 1 for f in F)
        e, s = np.zeros(max(1, sum(F)), np.float64), np.zeros(max(1, sum(F)), np.float64)
        cuts, peak, silent = np.zeros((B, cap), np.int32), np.zeros((B, cap), np.float64), np.zeros((B, cap), np.int32)
        nseg = np.zeros(B, np.int32)
        ptrs = (C.POINTER(C.c_float) * B)(*[_f(c) for c in recs])
        _check(lib().qasr_segment(self.h, ptrs, _i(n), B, C.byref(p), _d(e) if want_energy else None, _d(s) if want_energy else None,
                                  _i(cuts), _d(peak), _i(silent), _i(nseg), None, cap), "qasr_segment")
        out = []
        for b in range(B):
            K = int(nseg[b])
            ends = [int(c) * 160 for c in cuts[b, 1:K]] + [int(n[b])]
            out.append([Segment(b, int(cuts[b, k]) * 160, ends[k] - int(cuts[b, k]) * 160, float(peak[b, k]), bool(silent[b, k]))
                        for k in range(K)])
        if not want_energy:
            return out
        o = np.concatenate([[0], np.cumsum(F)])
        return out, [e[o[b]:o[b + 1]].copy() for b in range(B)], [s[o[b]:o[b + 1]].copy() for b in range(B)]

    def segment_last_us(self) -> Tuple[int, int]:
        """device time of the last segment() call's launches and the cut kernel's share of it, microseconds"""
        cut = C.c_int(0)
        return _neg(lib().qasr_segment_last_us(self.h, C.byref(cut)), "qasr_segment_last_us"), cut.value

    def resample_last_us(self) -> int:
        """device time of the last resample() call's kernel launch, microseconds"""
        return _neg(lib().qasr_resample_last_us(self.h), "qasr_resample_last_us")

    def _encode(self, mels: Sequence[np.ndarray], conv_only: bool, no_chunk: bool = False) -> List[np.ndarray]:
        T = np.array([m.shape[1] for m in mels], np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(m, np.float32).ravel() for m in mels]))
        N = [lib().qasr_encoder_frames_no_chunk(int(t)) if no_chunk else encoder_frames(int(t)) for t in T]
        width = self.model.hp.d_model if conv_only else self.model.hp.hidden_size
        out = np.zeros(max(1, sum(N) * width), np.float32)
        fn = lib().qasr_encode_no_chunk if no_chunk else lib().qasr_encode_conv if conv_only else lib().qasr_encode
        _check(fn(self.h, _f(flat), _i(T), len(mels), _f(out)), "qasr_encode")
        res, o = [], 0
        for k in N:
            res.append(out[o * width:(o + k) * width].reshape(k, width))
            o += k
        return res

    def encode(self, mels):
        return self._encode(mels, False)

    def encode_no_chunk(self, mels):
        """AudioEncoder::encode_no_chunk: the conv stack over all frames at once, PE 0..N-1"""
        return self._encode(mels, False, True)

    def encode_conv(self, mels):
        return self._encode(mels, True)

    def prefill(self, ids_list, feats_list=None, audio_pos=None, want_logits=True, slots=None):
        """slots: sequence b's KV-cache slot (qasr_prefill_slots); None: slot b"""
        B = len(ids_list)
        P = np.array([len(x) for x in ids_list], np.int32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in ids_list]))
        feats = None
        N = np.zeros(B, np.int32)
        ap = np.full(B, -1, np.int32) if audio_pos is None else np.asarray(audio_pos, np.int32)
        if feats_list is not None:
            N = np.array([f.shape[0] for f in feats_list], np.int32)
            feats = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float32) for f in feats_list]))
        V = self.model.hp.vocab_size
        logits = np.zeros((B, V), np.float32) if want_logits else None
        am = np.zeros(B, np.int32)
        if slots is not None:
            sl = np.ascontiguousarray(slots, np.int32)
            _check(lib().qasr_prefill_slots(self.h, _i32(ids), _i(P), _f(feats) if feats is not None else None, _i(ap), _i(N),
                                            _i(sl), B, _f(logits) if want_logits else None, _i32(am)), "qasr_prefill_slots")
            return logits, am
        _check(lib().qasr_prefill(self.h, _i32(ids), _i(P), _f(feats) if feats is not None else None, _i(ap), _i(N), B,
                                  _f(logits) if want_logits else None, _i32(am)), "qasr_prefill")
        return logits, am

    def prefill_score(self, ids_list, targets_list, n_past=None, feats_list=None, audio_pos=None, slots=None) -> List["Score"]:
        """qasr_prefill_score: the prefill of ids_list (n_past / feats_list + audio_pos / slots as in prefill,
        prefill_chunk and prefill(slots=...); None as there) with the row of ids_list[b][t] scored against
        targets_list[b][t] (< 0: not scored).  One Score per sequence over its scored rows, in order."""
        B = len(ids_list)
        P = np.array([len(x) for x in ids_list], np.int32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in ids_list]), np.int32)
        tg = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in targets_list]), np.int32)
        if len(tg) != len(ids) or any(len(t) != len(x) for t, x in zip(targets_list, ids_list)):
            raise ValueError("targets_list must have the shape of ids_list")
        npast = None if n_past is None else np.ascontiguousarray(n_past, np.int32)
        sl = None if slots is None else np.ascontiguousarray(slots, np.int32)
        feats, N, ap = None, None, None
        if feats_list is not None:
            N = np.array([f.shape[0] for f in feats_list], np.int32)
            feats = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float32) for f in feats_list]))
            ap = np.ascontiguousarray(audio_pos, np.int32)
        cap = max(int((tg >= 0).sum()), 1)
        lp, gid, glp = np.zeros(cap, np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        n = lib().qasr_prefill_score(self.h, _i32(ids), _i(P), _i(npast) if npast is not None else None,
                                     _f(feats) if feats is not None else None, _i(ap) if ap is not None else None,
                                     _i(N) if N is not None else None, _i(sl) if sl is not None else None, B, _i32(tg),
                                     _f(lp), _i32(gid), _f(glp), cap)
        if n < 0:
            raise QasrError(f"qasr_prefill_score: {lib().qasr_last_error().decode(errors='replace')}")
        res, o = [], 0
        for t in targets_list:
            k = int((np.asarray(t) >= 0).sum())
            res.append(Score(lp[o:o + k].copy(), gid[o:o + k].copy(), glp[o:o + k].copy(),
                             float(np.cumsum(lp[o:o + k], dtype=np.float32)[-1]) if k else 0.0))   # (in order, as qasr_score)
            o += k
        return res

    def score(self, clips: Sequence[int], hyps, include_eos: bool = True, timings: Optional["Timings"] = None) -> List["Score"]:
        """qasr_score: hyps[s] (token ids) scored as a transcript of staged clip clips[s] (stage_audio); one
        Score per sequence with len(hyps[s]) + include_eos entries.  Hypotheses of one clip (at most 8 a call,
        anywhere in the list) share the clip's mel, encoder and prompt prefill."""
        idx = np.ascontiguousarray(clips, np.int32)
        S = len(idx)
        if len(hyps) != S:
            raise ValueError("one hypothesis per clip index")
        nt = np.array([len(h) for h in hyps], np.int32)
        toks = np.ascontiguousarray(np.concatenate([np.asarray(h, np.int32).reshape(-1) for h in hyps] + [np.zeros(0, np.int32)]), np.int32)
        e = 1 if include_eos else 0
        total = int(nt.sum()) + e * S
        lp, gid, glp = (np.zeros(max(total, 1), np.float32), np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.float32))
        sums = np.zeros(max(S, 1), np.float32)
        t = timings if timings is not None else Timings()
        n = lib().qasr_score(self.h, _i(idx), _i32(toks) if len(toks) else None, _i(nt), S, e, _f(lp), _i32(gid), _f(glp), _f(sums),
                             C.byref(t))
        if n < 0:
            raise QasrError(f"qasr_score: {lib().qasr_last_error().decode(errors='replace')}")
        res, o = [], 0
        for s in range(S):
            k = int(nt[s]) + e
            res.append(Score(lp[o:o + k].copy(), gid[o:o + k].copy(), glp[o:o + k].copy(), float(sums[s])))
            o += k
        return res

    def kv_fork(self, parent, frm, to, group: int) -> None:
        """qasr_kv_fork: positions [frm[b], to[b]) of cache slot b take what slot parent[b] held (rows forked
        inside groups of `group` consecutive rows)"""
        par, f, t = (np.ascontiguousarray(x, np.int32) for x in (parent, frm, to))
        _check(lib().qasr_kv_fork(self.h, _i(par), _i(f), _i(t), len(par), int(group)), "qasr_kv_fork")

    def beams(self, clip: int) -> List[Beam]:
        """qasr_get_beams: every hypothesis of clip `clip` of the last beam run, best first"""
        W, T = QASR_BEAM_MAX, self.max_ctx
        toks, lps = np.zeros((W, T), np.int32), np.zeros((W, T), np.float32)
        nt, fin, sums = np.zeros(W, np.int32), np.zeros(W, np.int32), np.zeros(W, np.float32)
        n = lib().qasr_get_beams(self.h, int(clip), _i32(toks), _f(lps), _i(nt), _f(sums), _i(fin), W, T)
        if n < 0:
            raise QasrError(f"qasr_get_beams: {lib().qasr_last_error().decode(errors='replace')}")
        return [Beam(toks[i, :nt[i]].tolist(), lps[i, :nt[i]].tolist(), float(sums[i]), bool(fin[i])) for i in range(n)]

    def set_sampling(self, temperature: float = 0.0, min_p: float = 0.0, seed: int = 0, n_best: int = 1) -> None:
        """qasr_set_sampling: temperature <= 0 turns sampling off"""
        sp = Sampling(float(temperature), float(min_p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_best))
        _check(lib().qasr_set_sampling(self.h, C.byref(sp)), "qasr_set_sampling")

    def get_sampling(self) -> Sampling:
        sp = Sampling()
        _check(lib().qasr_get_sampling(self.h, C.byref(sp)), "qasr_get_sampling")
        return sp

    def set_sample_streams(self, clip, sample, t) -> None:
        """qasr_set_sample_streams: the (clip, sample, t) identities rows 0 .. B - 1 of prefill / decode_step draw with"""
        cl, sm, tt = (np.ascontiguousarray(x, np.int32) for x in (clip, sample, t))
        _check(lib().qasr_set_sample_streams(self.h, _i32(cl), _i32(sm), _i32(tt), len(cl)), "qasr_set_sample_streams")

    def samples(self, clip: int) -> List[Sample]:
        """qasr_get_samples: the hypotheses of clip `clip` of the last sampling run, in sample order"""
        W, T = QASR_SAMPLE_MAX, self.max_ctx
        toks, lps = np.zeros((W, T), np.int32), np.zeros((W, T), np.float32)
        nt, sums = np.zeros(W, np.int32), np.zeros(W, np.float32)
        n = lib().qasr_get_samples(self.h, int(clip), _i32(toks), _f(lps), _i(nt), _f(sums), W, T)
        if n < 0:
            raise QasrError(f"qasr_get_samples: {lib().qasr_last_error().decode(errors='replace')}")
        return [Sample(toks[i, :nt[i]].tolist(), lps[i, :nt[i]].tolist(), float(sums[i])) for i in range(n)]

    def set_constraints(self, no_repeat_ngram: int = 0, repetition_penalty: float = 1.0, penalty_last_n: int = 0,
                        bias=None, suppress=None) -> None:
        """qasr_set_constraints: bias {token id: additive bias}, suppress ids (a bias of -inf); the neutral values
        with neither turn constraints off"""
        k, _keep = make_constraints(no_repeat_ngram, repetition_penalty, penalty_last_n, bias, suppress)
        _check(lib().qasr_set_constraints(self.h, C.byref(k)), "qasr_set_constraints")

    def get_constraints(self) -> dict:
        """qasr_get_constraints: the setting in force, the bias list as {token id: bias}"""
        ids, bias = np.zeros(QASR_BIAS_MAX, np.int32), np.zeros(QASR_BIAS_MAX, np.float32)
        k = Constraints()
        _check(lib().qasr_get_constraints(self.h, C.byref(k), _i32(ids), _f(bias), QASR_BIAS_MAX), "qasr_get_constraints")
        return {"no_repeat_ngram": int(k.no_repeat_ngram), "repetition_penalty": float(k.repetition_penalty),
                "penalty_last_n": int(k.penalty_last_n),
                "bias": {int(i): float(b) for i, b in zip(ids[:k.n_bias], bias[:k.n_bias])}}

    def set_phrases(self, phrases=None, boost: float = 5.0) -> None:
        """qasr_set_phrases: hotwords the decoder prefers.  Each phrase is a list of token ids,
        an (ids, boost) pair or a string (tokenised by the model, with and without a leading space); None or an
        empty list turns phrases off"""
        p, _keep = make_phrases(phrases, boost, self.model.phrase_tokenize)
        _check(lib().qasr_set_phrases(self.h, C.byref(p)), "qasr_set_phrases")

    def get_phrases(self) -> list:
        """qasr_get_phrases: the list in force as [(ids, boost)]"""
        ids, ln = np.zeros(QASR_PHRASE_MAX * QASR_PHRASE_LEN_MAX, np.int32), np.zeros(QASR_PHRASE_MAX, np.int32)
        val = np.zeros(QASR_PHRASE_MAX, np.float32)
        p = Phrases()
        _check(lib().qasr_get_phrases(self.h, C.byref(p), _i32(ids), _i32(ln), _f(val), len(ids), len(ln)), "qasr_get_phrases")
        at = np.concatenate([[0], np.cumsum(ln[:p.n_phrases])])
        return [(ids[at[k]:at[k + 1]].tolist(), float(val[k])) for k in range(p.n_phrases)]

    def _sampling_on(self) -> bool:
        return self.get_sampling().temperature > 0 and not self.model.is_aligner

    def _run_result(self, toks, nt, t, max_tokens: int) -> RunResult:
        B = len(nt)
        tokens = [toks[b, :nt[b]].tolist() for b in range(B)]
        if self._sampling_on():
            many = self.get_sampling().n_best >= 2   # (the per-row readers are the n_best = 1 run's)
            return RunResult(tokens, t, None if many else self._run_logprobs(nt, max_tokens),
                             None if many else self._run_topk(nt, max_tokens), samples=[self.samples(b) for b in range(B)])
        if self._beam_on():
            return RunResult(tokens, t, beams=[self.beams(b) for b in range(B)])
        return RunResult(tokens, t, self._run_logprobs(nt, max_tokens), self._run_topk(nt, max_tokens))

    def _beam_on(self) -> bool:
        return self.get_option("beam_width") >= 2 and not self.model.is_aligner

    def decode_step(self, tok, n_past, want_logits=True):
        tok = np.ascontiguousarray(tok, np.int32)
        npast = np.ascontiguousarray(n_past, np.int32)
        B = len(tok)
        logits = np.zeros((B, self.model.hp.vocab_size), np.float32) if want_logits else None
        am = np.zeros(B, np.int32)
        _check(lib().qasr_decode_step(self.h, _i32(tok), _i(npast), B, _f(logits) if want_logits else None, _i32(am)),
               "qasr_decode_step")
        return logits, am

    def prefill_chunk(self, ids_list, n_past, want_logits=True, feats_list=None, audio_pos=None):
        """qasr_prefill_chunk: sequence b's tokens ids_list[b] after n_past[b]
        cached ones, one causal chunk (TextDecoder::forward, n_tokens > 1);
        with feats_list / audio_pos: qasr_prefill_chunk_audio, the audio rows
        spliced at audio_pos[b] of the chunk (forward_with_audio at n_past > 0);
        returns (logits of each chunk's last row, argmax)"""
        P = np.array([len(x) for x in ids_list], np.int32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in ids_list]), np.int32)
        npast = np.ascontiguousarray(n_past, np.int32)
        B = len(P)
        logits = np.zeros((B, self.model.hp.vocab_size), np.float32) if want_logits else None
        am = np.zeros(B, np.int32)
        if feats_list is None:
            _check(lib().qasr_prefill_chunk(self.h, _i32(ids), _i(P), _i(npast), B, _f(logits) if want_logits else None,
                                            _i32(am)), "qasr_prefill_chunk")
            return logits, am
        N = np.array([f.shape[0] for f in feats_list], np.int32)
        feats = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float32) for f in feats_list]))
        ap = np.ascontiguousarray(audio_pos, np.int32)
        _check(lib().qasr_prefill_chunk_audio(self.h, _i32(ids), _i(P), _i(npast), _f(feats), _i(ap), _i(N), B,
                                              _f(logits) if want_logits else None, _i32(am)), "qasr_prefill_chunk_audio")
        return logits, am

    # ---- whole path --------------------------------------------------------
    def stage_audio(self, clips: Sequence[np.ndarray], rates: Optional[Sequence[int]] = None) -> None:
        """rates: the clips' sample rates (qasr_stage_audio_rate resamples them to 16 kHz on the device);
        None: every clip is 16 kHz PCM"""
        self._staged = [np.ascontiguousarray(c, np.float32) for c in clips]
        n = np.array([len(c) for c in self._staged], np.int32)
        ptrs = (C.POINTER(C.c_float) * len(self._staged))(*[_f(c) for c in self._staged])
        if rates is not None:
            r = np.ascontiguousarray(rates, np.int32)
            if len(r) != len(self._staged):
                raise QasrError("stage_audio: one rate per clip")
            _check(lib().qasr_stage_audio_rate(self.h, ptrs, _i(n), _i(r), len(self._staged)), "qasr_stage_audio_rate")
            return
        _check(lib().qasr_stage_audio(self.h, ptrs, _i(n), len(self._staged)), "qasr_stage_audio")

    def run(self, max_tokens: int, ignore_eos: bool = False) -> RunResult:
        B = len(self._staged)
        if B > self.max_batch:
            raise QasrError(f"{B} staged clips exceed max_batch {self.max_batch}: use run_staged")
        toks = np.zeros((B, max_tokens), np.int32)
        nt = np.zeros(B, np.int32)
        t = Timings()
        _check(lib().qasr_run(self.h, max_tokens, int(ignore_eos), _i32(toks), _i(nt), C.byref(t)), "qasr_run")
        return self._run_result(toks, nt, t, max_tokens)

    def _run_logprobs(self, nt, max_tokens: int):
        """the last run's log-probabilities per row (None with option token_logprobs off)"""
        if not self.get_option("token_logprobs"):
            return None
        B = len(nt)
        lp = np.zeros((B, max_tokens), np.float32)
        _check(lib().qasr_get_logprobs(self.h, _f(lp), B, max_tokens), "qasr_get_logprobs")
        return [lp[b, :nt[b]].tolist() for b in range(B)]

    def _run_topk(self, nt, max_tokens: int):
        """the last run's top-K alternatives per row (None with option top_k off)"""
        K = self.get_option("top_k")
        if not K:
            return None
        B = len(nt)
        ids, lps = np.zeros((B, max_tokens, K), np.int32), np.zeros((B, max_tokens, K), np.float32)
        _check(lib().qasr_get_topk(self.h, _i32(ids), _f(lps), B, max_tokens, K), "qasr_get_topk")
        return [(ids[b, :nt[b]].copy(), lps[b, :nt[b]].copy()) for b in range(B)]

    def step_topk(self, B: int) -> Tuple[np.ndarray, np.ndarray]:
        """(ids [B][K], logprobs [B][K]) of the last prefill / decode_step (option top_k = K)"""
        K = max(self.get_option("top_k"), 1)
        ids, lps = np.zeros((B, K), np.int32), np.zeros((B, K), np.float32)
        _check(lib().qasr_get_step_topk(self.h, _i32(ids), _f(lps), B, K), "qasr_get_step_topk")
        return ids, lps

    def step_logprobs(self, B: int) -> np.ndarray:
        """log-probability of each row's argmax of the last prefill / decode_step (option token_logprobs)"""
        out = np.zeros(B, np.float32)
        _check(lib().qasr_get_step_logprobs(self.h, _f(out), B), "qasr_get_step_logprobs")
        return out

    def run_staged(self, clips: Sequence[int], max_tokens: int, ignore_eos: bool = False) -> RunResult:
        """transcribe staged clips (indices into the last stage_audio call) as one batch"""
        idx = np.ascontiguousarray(clips, np.int32)
        B = len(idx)
        toks = np.zeros((B, max_tokens), np.int32)
        nt = np.zeros(B, np.int32)
        t = Timings()
        _check(lib().qasr_run_staged(self.h, _i(idx), B, max_tokens, int(ignore_eos), _i32(toks), _i(nt), C.byref(t)),
               "qasr_run_staged")
        return self._run_result(toks, nt, t, max_tokens)

    def run_stream(self, next_clip, max_tokens: int, ignore_eos: bool = False, slots: int = 0, logprobs: bool = False,
                   topk: bool = False, with_rates: bool = False):
        """Continuous batching (qasr_run_stream): next_clip() -> (id, pcm[, budget])
        or None when the queue is empty; returns ({id: tokens | QasrError},
        StreamStats).  Slots (0: max_batch) freed by a finished clip are
        refilled at the next chunk boundary; a clip that fails alone maps to
        its QasrError.  logprobs=True (option token_logprobs on): a clip maps
        to (tokens, logprobs) instead.  topk=True (option top_k on) appends
        (ids [n][K], logprobs [n][K]) to that tuple.  with_rates=True
        (qasr_run_stream_rate): next_clip() -> (id, pcm, rate[, budget]), the
        clip resampled to 16 kHz on the device when its slot is refilled."""
        out, keep = {}, []

        def fetch_rate(_u, pcm_pp, n_p, rate_p, budget_p):
            item = next_clip()
            if item is None:
                return -1
            cid, pcm = int(item[0]), np.ascontiguousarray(item[1], np.float32)
            keep[:] = [pcm]
            pcm_pp[0] = _f(pcm)
            n_p[0] = len(pcm)
            rate_p[0] = int(item[2])
            if len(item) > 3:
                budget_p[0] = int(item[3])
            return cid

        def fetch(_u, pcm_pp, n_p, budget_p):
            item = next_clip()
            if item is None:
                return -1
            cid, pcm = int(item[0]), np.ascontiguousarray(item[1], np.float32)
            keep[:] = [pcm]   # alive until the next fetch (the engine copies it first)
            pcm_pp[0] = _f(pcm)
            n_p[0] = len(pcm)
            if len(item) > 2:
                budget_p[0] = int(item[2])
            return cid

        failed = []
        f = FETCH_RATE_FN(_guarded_fetch(fetch_rate, failed)) if with_rates else FETCH_FN(_guarded_fetch(fetch, failed))
        k = SINK_FN(_sink_into(out, failed, self if logprobs else None, self if topk else None))
        st = StreamStats()
        rc = (lib().qasr_run_stream_rate if with_rates else lib().qasr_run_stream)(self.h, int(slots), f, k, None, int(max_tokens), int(ignore_eos), C.byref(st))
        if failed:
            raise failed[0]
        _check(rc, "qasr_run_stream")
        return out, st

    def run_stream_staged(self, next_clip, max_tokens: int, ignore_eos: bool = False, slots: int = 0,
                          logprobs: bool = False, topk: bool = False):
        """run_stream over the staged pool (stage_audio): next_clip() -> staged
        index (its id) or (index, budget), None when the queue is empty"""
        out = {}

        def fetch(_u, budget_p):
            item = next_clip()
            if item is None:
                return -1
            if isinstance(item, tuple):
                budget_p[0] = int(item[1])
                return int(item[0])
            return int(item)

        failed = []
        f, k = FETCH_STAGED_FN(_guarded_fetch(fetch, failed)), SINK_FN(_sink_into(out, failed, self if logprobs else None,
                                                                                     self if topk else None))
        st = StreamStats()
        rc = lib().qasr_run_stream_staged(self.h, int(slots), f, k, None, int(max_tokens), int(ignore_eos), C.byref(st))
        if failed:
            raise failed[0]
        _check(rc, "qasr_run_stream_staged")
        return out, st

    def set_system_prompt(self, ids: Sequence[int]) -> None:
        a = np.ascontiguousarray(ids, np.int32)
        _check(lib().qasr_set_system_prompt(self.h, _i32(a) if len(a) else None, len(a)), "qasr_set_system_prompt")

    def set_option(self, name: str, value: int) -> None:
        _check(lib().qasr_ctx_set_option(self.h, name.encode(), int(value)), "qasr_ctx_set_option")

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        _check(lib().qasr_ctx_get_option(self.h, name.encode(), C.byref(v)), "qasr_ctx_get_option")
        return v.value

    def debug_read(self, buffer: str) -> np.ndarray:
        """Decode-step state after decode_step: x (fp32), act (fp16), qkv (fp32), att (fp16)."""
        hp = self.model.hp
        qd, kd = hp.n_heads * 128, hp.n_kv_heads * 128
        n, dt = {"x": (hp.hidden_size, np.float32), "act": (hp.dec_ffn, np.float16),
                 "qkv": (qd + 2 * kd, np.float32), "att": (qd, np.float16)}[buffer]
        out = np.zeros((self.max_batch, n), dt)
        _check(lib().qasr_debug_read(self.h, buffer.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes), "qasr_debug_read")
        return out

    def set_token_callback(self, fn) -> None:
        """fn(seq, n_generated, token) after every greedy token of run() (None removes)"""
        self._tok_cb = TOKEN_CB(lambda _u, seq, n, tok: fn(seq, n, tok)) if fn else None
        _check(lib().qasr_set_token_callback(self.h, self._tok_cb if fn else TOKEN_CB(), None), "qasr_set_token_callback")

    def set_profile(self, on: bool) -> None:
        _check(lib().qasr_set_profile(self.h, int(on)), "qasr_set_profile")

    def profile_report(self) -> str:
        n = lib().qasr_profile_report(self.h, None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().qasr_profile_report(self.h, buf, n + 1)
        return buf.raw[:n].decode()

    def set_probe(self, kernel: int) -> None:
        _check(lib().qasr_set_probe(self.h, kernel), "qasr_set_probe")

    def get_probe(self):
        ms, n, b = C.c_double(0), C.c_int64(0), C.c_double(0)
        _check(lib().qasr_get_probe(self.h, C.byref(ms), C.byref(n), C.byref(b)), "qasr_get_probe")
        return ms.value, n.value, b.value

    def get_probe_device(self):
        """(total ms, launches) of the probed launches by the device clock"""
        ms, n = C.c_double(0), C.c_int64(0)
        _check(lib().qasr_get_probe_device(self.h, C.byref(ms), C.byref(n)), "qasr_get_probe_device")
        return ms.value, n.value

    # ---- forced aligner ------------------------------------------------------
    def align(self, pcm: np.ndarray, text_ids: Sequence[int]):
        """Raw timestamp classes of one clip (qasr_align) -> (classes, timings)."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        ids = np.ascontiguousarray(text_ids, np.int32)
        cap = max(int(np.sum(ids == self.model.hp.timestamp_token_id)), 1)
        out = np.zeros(cap, np.int32)
        nts = C.c_int(0)
        t = Timings()
        _check(lib().qasr_align(self.h, _f(pcm), len(pcm), _i32(ids) if len(ids) else None, len(ids), _i32(out), cap,
                                C.byref(nts), C.byref(t)), "qasr_align")
        return out[:nts.value].tolist(), t

    def align_json(self, pcm: np.ndarray, text: str, language: str = ""):
        """ForcedAligner::align -> the CLI JSON document (parsed) and timings.
        qasr_align_json returns the document length, or minus an error code."""
        import json
        pcm = np.ascontiguousarray(pcm, np.float32)
        t = Timings()
        cap = 8192 + 40 * len(text.encode())   # (one call in practice: the escaped words + ~50 B a word)
        buf = C.create_string_buffer(cap)
        n = lib().qasr_align_json(self.h, _f(pcm), len(pcm), text.encode(), language.encode(), buf, cap, C.byref(t))
        if n < 0:
            raise QasrError(f"qasr_align_json: {lib().qasr_last_error().decode(errors='replace')}")
        if n >= cap:   # larger than the bound: run again into a buffer of the reported size
            buf = C.create_string_buffer(n + 1)
            lib().qasr_align_json(self.h, _f(pcm), len(pcm), text.encode(), language.encode(), buf, n + 1, C.byref(t))
        return json.loads(buf.raw[:n].decode("utf-8")), t

    def align_json_batch(self, pcms, texts, language: str = ""):
        """qasr_align_json_batch: B clips in one aligner pass -> (list of the
        CLI documents, parsed, in input order; timings)"""
        import json
        arrs = [np.ascontiguousarray(p, np.float32) for p in pcms]
        B = len(arrs)
        ptrs = (C.POINTER(C.c_float) * B)(*[_f(a) for a in arrs])
        n = np.array([len(a) for a in arrs], np.int32)
        tx = (C.c_char_p * B)(*[t.encode() for t in texts])
        t = Timings()
        cap = 8192 * B + 40 * sum(len(x.encode()) for x in texts)
        buf = C.create_string_buffer(cap)
        k = lib().qasr_align_json_batch(self.h, ptrs, _i(n), tx, B, language.encode(), buf, cap, C.byref(t))
        if k < 0:
            raise QasrError(f"qasr_align_json_batch: {lib().qasr_last_error().decode(errors='replace')}")
        if k >= cap:
            buf = C.create_string_buffer(k + 1)
            lib().qasr_align_json_batch(self.h, ptrs, _i(n), tx, B, language.encode(), buf, k + 1, C.byref(t))
        return json.loads(buf.raw[:k].decode("utf-8")), t

    def transcribe(self, clips, max_tokens=1024, ignore_eos=False, rates=None) -> RunResult:
        self.stage_audio(clips, rates)
        return self.run(max_tokens, ignore_eos)

    # ---- long recordings ------------------------------------
    def stage_long(self, recs: Sequence[np.ndarray], rates: Optional[Sequence[int]] = None, **kw) -> List[Segment]:
        """qasr_stage_long: the recordings are uploaded once (resampled on the device where rates says so) and cut at
        their pauses on the device; the pool becomes the segments, in recording order, each pointing into its
        recording.  Returns the table (entry k is pool clip k for run_staged / run_stream_staged / score)"""
        recs = [np.ascontiguousarray(c, np.float32) for c in recs]
        n = np.array([len(c) for c in recs], np.int32)
        ptrs = (C.POINTER(C.c_float) * len(recs))(*[_f(c) for c in recs])
        r = None
        if rates is not None:
            r = np.ascontiguousarray(rates, np.int32)
            if len(r) != len(recs):
                raise QasrError("stage_long: one rate per recording")
        p = segment_params(**kw)
        K = _neg(lib().qasr_stage_long(self.h, ptrs, _i(n), _i(r) if r is not None else None, len(recs), C.byref(p)), "qasr_stage_long")
        self._staged = [None] * K   # (the pool size run() checks)
        self._long_recs = len(recs)
        return self.get_segments()

    def get_segments(self, rec: Optional[int] = None) -> List[Segment]:
        """qasr_get_segments: the table of the last stage_long, of one recording or of all in pool order"""
        if rec is None:
            return [s for b in range(getattr(self, "_long_recs", 1)) for s in self.get_segments(b)]
        K = _neg(lib().qasr_get_segments(self.h, int(rec), None, None, None, None, 0), "qasr_get_segments")
        start, n = np.zeros(K, np.int64), np.zeros(K, np.int32)
        peak, silent = np.zeros(K, np.float64), np.zeros(K, np.int32)
        _neg(lib().qasr_get_segments(self.h, int(rec), start.ctypes.data_as(C.POINTER(C.c_longlong)), _i(n), _d(peak), _i(silent), K),
             "qasr_get_segments")
        return [Segment(int(rec), int(start[k]), int(n[k]), float(peak[k]), bool(silent[k])) for k in range(K)]

    def transcribe_long(self, pcm: np.ndarray, max_tokens: int = 1024, ignore_eos: bool = False, rate: int = 16000, **kw):
        """one recording of any length: stage_long, then every segment that is not silent through the staged stream
        (beam search, sampling, constraints or hotwords on, which the stream refuses: run_staged in groups of
        max_batch).  -> (text, [(Segment, tokens)]): silent segments have no tokens, text joins the others' by a space"""
        segs = self.stage_long([pcm], None if rate == 16000 else [rate], **kw)
        todo = [k for k, s in enumerate(segs) if not s.silent]
        toks = {k: [] for k in range(len(segs))}
        cons = self.get_constraints()
        grouped = self._beam_on() or self._sampling_on() or bool(self.get_phrases()) or bool(
            cons["no_repeat_ngram"] or cons["repetition_penalty"] != 1.0 or len(cons["bias"]))
        if grouped:
            per = max(1, self.max_batch // max(self.get_option("beam_width"), self.get_sampling().n_best, 1))
            for i in range(0, len(todo), per):
                r = self.run_staged(todo[i:i + per], max_tokens, ignore_eos)
                for k, t in zip(todo[i:i + per], r.tokens):
                    toks[k] = list(t)
        elif todo:
            it = iter(todo)
            res, _ = self.run_stream_staged(lambda: next(it, None), max_tokens, ignore_eos)
            for k in todo:
                if isinstance(res.get(k), Exception):
                    raise res[k]
                toks[k] = list(res[k])
        texts = [self.model.detokenize(toks[k]) for k in todo]
        return " ".join(t for t in texts if t), [(s, toks[k]) for k, s in enumerate(segs)]
