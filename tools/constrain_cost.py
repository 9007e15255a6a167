"""Cost of decoding constraints on the full-size synthetic f16 model: decode time per step and the LM-head
launch group by HIP events (probe 1: with constraints on it includes the stage's three launches), at 1, 64 and
128 rows, alternating rounds (tools/sample_cost.py's scheme).  Cases:
  off      constraints off: the yardstick, the parent's step
  sample   temperature sampling, constraints off: the other yardstick, it pays the same logits store
  guard    a guard that never fires: a bias of -0.0 on 16 tokens the model never emits, so the raw argmax is outside
           the edited set on every row and no row is scanned (its tokens must equal the greedy run's)
  scan     a penalty one ulp above 1 over the whole history: the synthetic model repeats itself, so the raw argmax
           is in the history, every row takes the scan (the share of such steps is printed) and no token changes
  ngram    no_repeat_ngram = 2: what a caller would set; the share of scanned steps is whatever the transcript gives
"""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
import numpy as np
import qasr

SR = 16000
TOK = 64
# (name, temperature, constraints)
CASES = [("off", 0.0, {}), ("sample", 0.8, {}),
         ("guard", 0.0, dict(bias={i: -0.0 for i in range(16)})),
         ("scan", 0.0, dict(repetition_penalty=float(np.nextafter(np.float32(1), np.float32(2))))),
         ("ngram", 0.0, dict(no_repeat_ngram=2))]


def seen_share(tokens):
    """share of the steps whose token had occurred before in its row"""
    hit = sum(t[k] in t[:k] for t in tokens for k in range(1, len(t)))
    return hit / max(1, sum(len(t) - 1 for t in tokens))


with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "full.gguf")
    qasr.write_synthetic_gguf(p, "full", 42, 1)
    m = qasr.Model(p)
    pcm = qasr.synth_pcm(9300, int(1.1 * SR))
    for B in [int(x) for x in os.environ.get("CC_B", "1,64,128").split(",")]:
        c = qasr.Context(m, max_batch=B, max_ctx=256)
        res = {k[0]: {"probe_us": [], "step_us": []} for k in CASES}
        toks = {}
        for rnd in range(4):   # round 0 warms up (graph capture)
            for name, T, con in CASES:
                c.set_sampling(T, 0.0, 1234, 1)
                c.set_constraints(**con)
                c.set_probe(0)
                r = c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                r = c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                toks.setdefault(name, r.tokens)
                assert toks[name] == r.tokens
                step = r.timings.t_decode_ms / r.timings.n_decode_steps * 1e3
                c.set_probe(1)
                c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                ms, n, _ = c.get_probe()
                c.set_probe(0)
                if rnd:
                    res[name]["step_us"].append(step)
                    res[name]["probe_us"].append(ms / n * 1e3)
        assert toks["guard"] == toks["off"], "the guard fired"
        assert 0 not in {t for row in toks["off"] for t in row[:1]} and not any(t < 16 for row in toks["off"] for t in row)
        for k in CASES:
            v = res[k[0]]
            print(f"B={B:3d} {k[0]:7s} lm-head group (events) us {np.round(v['probe_us'], 2).tolist()}  "
                  f"decode step us {np.round(v['step_us'], 2).tolist()}  seen-before share {seen_share(toks[k[0]]):.2f}"
                  f"{'  tokens = off' if toks[k[0]] == toks['off'] else ''}", flush=True)
        c.set_sampling(0)
        c.set_constraints()
        c.close()
    m.close()
