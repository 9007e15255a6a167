"""Cost of option top_k on the full-size synthetic f16 model: LM-head launch
group by HIP events (probe 1: with the option on it includes the row kernel),
the LM-head kernel alone by the device clock, and decode time per step, at 1,
64 and 128 rows; option off, token_logprobs only, top_k 1 / 2 / 4 / 8, each with
lmh 1 and 0, and top_k with lmh_topk 0 (the one-launch head + the row kernel);
alternating rounds (tools/logprob_cost.py's scheme)."""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
import numpy as np
import qasr

SR = 16000
TOK = 64
OPTS = [("off", dict(token_logprobs=0, top_k=0)), ("logprobs", dict(token_logprobs=1, top_k=0)),
        ("top1", dict(token_logprobs=0, top_k=1)), ("top2", dict(token_logprobs=0, top_k=2)),
        ("top4", dict(token_logprobs=0, top_k=4)), ("top8", dict(token_logprobs=0, top_k=8))]
# lmh 1 with lmh_topk 2: the fused top-K variant at 9 .. 64 rows whatever K
CASES = [(f"{n}_lmh{l}", dict(o, lmh=l, lmh_topk=2)) for l in (1, 0) for n, o in OPTS]
# the one-launch LM head writing its logits for the row kernel instead of its fused top-K variant (9 .. 64 rows)
CASES += [(f"{n}_rowk", dict(o, lmh=1, lmh_topk=0)) for n, o in OPTS if o["top_k"]]
with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "full.gguf")
    qasr.write_synthetic_gguf(p, "full", 42, 1)
    m = qasr.Model(p)
    pcm = qasr.synth_pcm(9300, int(1.1 * SR))
    if os.environ.get("TK_CASES"):
        CASES = [c for c in CASES if c[0] in os.environ["TK_CASES"].split(",")]
    for B in [int(x) for x in os.environ.get("TK_B", "1,64,128").split(",")]:
        c = qasr.Context(m, max_batch=B, max_ctx=256)
        res = {k: {"probe_us": [], "dev_us": [], "step_us": []} for k, _ in CASES}
        toks = {}
        for rnd in range(4):   # round 0 warms up (graph capture)
            for name, opts in CASES:
                for k, v in opts.items():
                    c.set_option(k, v)
                c.set_probe(0)
                r = c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                r = c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                toks.setdefault(name, r.tokens)
                assert toks[name] == r.tokens
                step = r.timings.t_decode_ms / r.timings.n_decode_steps * 1e3
                c.set_probe(1)
                c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                ms, n, _ = c.get_probe()
                dms, dn = c.get_probe_device()
                c.set_probe(0)
                if rnd:
                    res[name]["step_us"].append(step)
                    res[name]["probe_us"].append(ms / n * 1e3)
                    res[name]["dev_us"].append(dms / dn * 1e3 if dn else float("nan"))
        assert all(t == toks[CASES[0][0]] for t in toks.values()), "tokens differ between cases"
        for name, _ in CASES:
            v = res[name]
            print(f"B={B:3d} {name:13s} lm-head group (events) us {np.round(v['probe_us'], 2).tolist()}  "
                  f"lm-head kernel (device clock) us {np.round(v['dev_us'], 2).tolist()}  "
                  f"decode step us {np.round(v['step_us'], 2).tolist()}", flush=True)
        c.close()
    m.close()
