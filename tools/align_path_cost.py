"""Cost of the forced aligner's monotone path next to the stages around it, on the synthetic
Qwen3-ForcedAligner-0.6B-shaped model ("aligner", f16): 64 clips of 30 s with 100 words each in one pass, and one
clip of 300 s with 1000 words.
  mel / encode / prefill   qasr_timings of the pass (HIP events on the context stream); prefill ends after the head
  gemm / path / rows       qasr_align_path_last_us: the fp32 classify GEMM, align_path_kernel, align_lse_kernel
  default                  the same clips with option align_monotone at 0: the arg-max head inside the prefill figure,
                           and the host's fix_timestamp_classes over every clip's classes (wall clock)
Each figure is the median (min .. max) of ROUNDS rounds; a round measures every case once, default and monotone one
after the other, so they alternate; one untimed round comes first.  Writes profiles/align_path/align_path_cost.txt (or
the path given as the first argument)."""
import os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
import numpy as np
import qasr

ROUNDS = 3
CASES = ((64, 30, 100, 1024), (1, 300, 1000, 10240))   # (clips, seconds, words, max_ctx)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "align_path", "align_path_cost.txt")


def stat(v):
    return f"{float(np.median(v)):.3f} ({min(v):.3f} .. {max(v):.3f})"


lines = [f"synthetic aligner (0.6B shapes, f16), one MI355X; ms, median (min .. max) of {ROUNDS} alternating rounds after a warm-up round"]
with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "aligner.gguf")
    qasr.write_synthetic_gguf(p, "aligner", 42, 1)
    m = qasr.Model(p)
    for B, secs, words, ctx in CASES:
        c = qasr.Context(m, max_batch=B, max_ctx=ctx)
        clips = [qasr.synth_pcm(9900 + b, secs * 16000) for b in range(B)]
        text = " ".join(chr(97 + i % 26) + chr(97 + (i // 26) % 26) for i in range(words))
        ids = [m.align_tokenize(text)[0]] * B
        r = {k: [] for k in ("mel", "enc", "pre0", "pre1", "gemm", "path", "rows", "fix")}
        for rnd in range(ROUNDS + 1):
            c.set_option("align_monotone", 0)
            _, t0 = c.align_json_batch(clips, [text] * B)
            cls = [c.align(clips[b], ids[b])[0] for b in range(min(B, 4))]
            w = time.perf_counter()
            for k in cls:
                qasr.fix_timestamps(k)
            fix = (time.perf_counter() - w) * 1000.0 * B / len(cls)
            res = c.align_path(clips, ids)
            t1 = c.last_align_timings
            us = c.align_path_last_us()
            if rnd:
                r["mel"].append(t1.t_mel_ms); r["enc"].append(t1.t_encode_ms); r["pre0"].append(t0.t_prefill_ms)
                r["pre1"].append(t1.t_prefill_ms); r["gemm"].append(us[0] / 1000); r["path"].append(us[1] / 1000)
                r["rows"].append(us[2] / 1000); r["fix"].append(fix)
        rows = sum(len(x[0]) for x in res)
        stage = float(np.median(r["gemm"]) + np.median(r["path"]) + np.median(r["rows"]))
        head0 = float(np.median(r["pre0"])) - (float(np.median(r["pre1"])) - stage)
        lines += [f"{B} x {secs} s, {words} words a clip: {rows} timestamp rows, C = {min(m.hp.classify_num, secs * 16000 // 1280 + 2)}, prompt {qasr.align_prompt_len(secs * 16000, len(ids[0]))} tokens",
                  f"  mel {stat(r['mel'])}   encode {stat(r['enc'])}   prefill + head: default {stat(r['pre0'])}, monotone {stat(r['pre1'])}",
                  f"  monotone stage: fp32 classify GEMM {stat(r['gemm'])}   path kernel {stat(r['path'])}   row kernel {stat(r['rows'])}   sum {stage:.3f}",
                  f"  default: arg-max head {head0:.3f} (prefill + head, default, minus monotone less its stage)   host fix_timestamp_classes {stat(r['fix'])}",
                  f"  ratios: stage / prefill {stage / float(np.median(r['pre1'])):.4f}   path kernel / prefill {float(np.median(r['path'])) / float(np.median(r['pre1'])):.4f}   stage / (arg-max head + host fix) {stage / max(head0 + float(np.median(r['fix'])), 1e-9):.2f}"]
        print("\n".join(lines[-5:]), flush=True)
        c.close()
    m.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
