"""Cost of temperature sampling on the full-size synthetic f16 model: decode time per step and the LM-head
launch group by HIP events (probe 1: with sampling on it includes the sampler's two launches and the token
log-probability kernel), at 1, 64 and 128 rows.  The yardstick is the greedy step with token_logprobs = 1
(sampling off: the parent's code, which also stores its logits below 9 rows and runs a row kernel);
alternating rounds (tools/topk_cost.py's scheme).  SC_SLICES sweeps option sample_slices (0 = the
launcher's choice)."""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
import numpy as np
import qasr

SR = 16000
TOK = 64
SLICES = [int(x) for x in os.environ.get("SC_SLICES", "0").split(",")]
# (name, token_logprobs, lmh, temperature, min_p, sample_slices)
CASES = [("greedy", 0, 1, 0.0, 0.0, 0), ("greedy_lp", 1, 1, 0.0, 0.0, 0), ("greedy_lp_rowk", 1, 0, 0.0, 0.0, 0)]
CASES += [(f"sample_s{s}", 0, 1, 0.8, 0.0, s) for s in SLICES]
CASES += [("sample_minp0.1", 0, 1, 0.8, 0.1, 0)]
with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "full.gguf")
    qasr.write_synthetic_gguf(p, "full", 42, 1)
    m = qasr.Model(p)
    pcm = qasr.synth_pcm(9300, int(1.1 * SR))
    for B in [int(x) for x in os.environ.get("SC_B", "1,64,128").split(",")]:
        c = qasr.Context(m, max_batch=B, max_ctx=256)
        res = {k[0]: {"probe_us": [], "step_us": []} for k in CASES}
        toks = {}
        for rnd in range(4):   # round 0 warms up (graph capture)
            for name, lp, lmh, T, mp, sl in CASES:
                c.set_option("token_logprobs", lp)
                c.set_option("lmh", lmh)
                c.set_option("sample_slices", sl)
                c.set_sampling(T, mp, 1234, 1)
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
        same = [toks[k[0]] for k in CASES if k[0].startswith("sample_s")]
        assert all(t == same[0] for t in same), "the draws depend on the slice count"
        for k in CASES:
            v = res[k[0]]
            print(f"B={B:3d} {k[0]:15s} lm-head group (events) us {np.round(v['probe_us'], 2).tolist()}  "
                  f"decode step us {np.round(v['step_us'], 2).tolist()}", flush=True)
        c.close()
    m.close()
