"""Option kv_fp8 measured on the full-size synthetic f16 model (results: profiles/kv_fp8/).

  attention   64 and 128 rows of 30 s clips, 48 tokens, EOS ignored.  Probe 4 (the attention launch of layer
              probe_layer alone, device clock) and the decode step time of the same runs, for
                fp8          kv_fp8 = 1
                f16_fx0      kv_fp8 = 0, fa_exact_decode = 0   (the same arithmetic on fp16 keys)
                f16_default  kv_fp8 = 0, options at their defaults
              alternating on one context, round 0 discarded (graph capture).  The prefill time of the same runs stands
              beside it: with kv_fp8 = 1 it includes the conversion of the rows the prefill wrote.
  step4       4 rows: the decode step with and without the one conversion launch a step.
  parity      12 clips, 12 teacher-forced 12-row steps: the worst |logit difference| of kv_fp8 = 1 against
              kv_fp8 = 0, fa_exact_decode = 0 on the same tokens, for the tiny and the full-size model (random weights:
              recorded, not a bar).
KV_FP8_COST_ONLY=attention|step4|parity runs one part.
"""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import qasr
from beam_util import prompts

SR, TOK, ROUNDS = 16000, 48, 4
CONFIGS = [("fp8", dict(kv_fp8=1, fa_exact_decode=0)), ("f16_fx0", dict(kv_fp8=0, fa_exact_decode=0)),
           ("f16_default", dict(kv_fp8=0, fa_exact_decode=1))]
only = os.environ.get("KV_FP8_COST_ONLY")


def med(v):
    return float(np.median(v))


def timed_runs(c, pcms, configs, probe):
    res = {name: dict(step=[], prefill=[], attn=[]) for name, _ in configs}
    for rnd in range(ROUNDS):
        for name, opts in configs:
            for k, v in opts.items():
                c.set_option(k, v)
            c.set_probe(probe)
            r = c.transcribe(pcms, max_tokens=TOK, ignore_eos=True)
            assert r.timings.n_decode_steps == TOK - 1
            if probe:
                assert c.get_option("kv_fp8_path") == opts["kv_fp8"], name
            ms, n = c.get_probe_device() if probe else (0.0, 1)
            if rnd:
                res[name]["step"].append(r.timings.t_decode_ms / r.timings.n_decode_steps)
                res[name]["prefill"].append(r.timings.t_prefill_ms)
                res[name]["attn"].append(1e3 * ms / max(n, 1))
    c.set_probe(0)
    return res


def attention(m):
    for rows in (64, 128):
        c = qasr.Context(m, max_batch=rows, max_ctx=512)
        pcms = [qasr.synth_pcm(7000 + i, 30 * SR) for i in range(rows)]
        res = timed_runs(c, pcms, CONFIGS, 4)
        for name, _ in CONFIGS:
            r = res[name]
            print(f"rows {rows:3d} {name:12s} attention us/launch {np.round(r['attn'], 2).tolist()} median {med(r['attn']):.2f}   "
                  f"decode ms/step {np.round(r['step'], 3).tolist()} median {med(r['step']):.3f}   "
                  f"prefill ms {np.round(r['prefill'], 2).tolist()} median {med(r['prefill']):.2f}", flush=True)
        a = {n: med(res[n]["attn"]) for n, _ in CONFIGS}
        s = {n: med(res[n]["step"]) for n, _ in CONFIGS}
        p = {n: med(res[n]["prefill"]) for n, _ in CONFIGS}
        print(f"rows {rows:3d} attention fp8 / f16_fx0 = {a['fp8'] / a['f16_fx0']:.3f}, fp8 / f16_default = {a['fp8'] / a['f16_default']:.3f}; "
              f"step fp8 / f16_fx0 = {s['fp8'] / s['f16_fx0']:.3f}, fp8 / f16_default = {s['fp8'] / s['f16_default']:.3f}; "
              f"prefill fp8 - f16_fx0 = {p['fp8'] - p['f16_fx0']:.2f} ms (the conversion of the prompt rows)", flush=True)
        c.close()


def step4(m):
    c = qasr.Context(m, max_batch=4, max_ctx=512)
    pcms = [qasr.synth_pcm(7100 + i, 30 * SR) for i in range(4)]
    res = timed_runs(c, pcms, [("fp8", dict(kv_fp8=1)), ("off", dict(kv_fp8=0))], 0)
    on, off = med(res["fp8"]["step"]), med(res["off"]["step"])
    print(f"rows   4 decode ms/step kv_fp8 = 1 {np.round(res['fp8']['step'], 4).tolist()} median {on:.4f}; kv_fp8 = 0 "
          f"{np.round(res['off']['step'], 4).tolist()} median {off:.4f}; the conversion launch: {1e3 * (on - off):.1f} us a step", flush=True)
    c.close()


def parity(m, label):
    ref, fp8 = qasr.Context(m, max_batch=12, max_ctx=256), qasr.Context(m, max_batch=12, max_ctx=256, kv_fp8=1)
    ref.set_option("fa_exact_decode", 0)
    pcms = [qasr.synth_pcm(7200 + i, SR + 3200 * (i % 4)) for i in range(12)]
    feats, ids, apos = prompts(ref, pcms)
    n = np.array([len(x) for x in ids], np.int32)
    _, tok = ref.prefill(ids, feats, apos)
    fp8.prefill(ids, feats, apos)
    worst, peak, flips = 0.0, 0.0, 0
    for k in range(12):
        a, nxt = ref.decode_step(tok, n + k)
        b, nb = fp8.decode_step(tok, n + k)
        assert fp8.get_option("kv_fp8_path") == 1
        worst, peak, flips = max(worst, float(np.abs(a - b).max())), max(peak, float(np.abs(a).max())), flips + int((nxt != nb).sum())
        tok = nxt
    print(f"parity {label}: worst |logit difference| {worst:.5f} over 12 teacher-forced 12-row steps (largest |logit| {peak:.3f}); "
          f"argmax differs on {flips} of 144 rows", flush=True)
    ref.close()
    fp8.close()


with tempfile.TemporaryDirectory() as d:
    full, tiny = os.path.join(d, "full.gguf"), os.path.join(d, "tiny.gguf")
    qasr.write_synthetic_gguf(full, "full", 42, 1)
    qasr.write_synthetic_gguf(tiny, "tiny", 42, 1)
    m = qasr.Model(full)
    if only in (None, "attention"):
        attention(m)
    if only in (None, "step4"):
        step4(m)
    if only in (None, "parity"):
        mt = qasr.Model(tiny)
        parity(mt, "tiny")
        mt.close()
        parity(m, "full")
    m.close()
