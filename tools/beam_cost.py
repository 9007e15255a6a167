"""Cost of a beam step on the full-size synthetic f16 model: one 92 s synthetic
clip, EOS ignored, 322 tokens (bench.py's flagship shape).  ms per decode step
(device events around the decode loop / its steps) for
  greedy1     greedy, 1 row
  greedyW_tk  greedy at W identical rows with top_k = W -- what the parent commit
              can run at that width: the yardstick of a W-wide beam step
  beamW       beam search, W = 2, 4, 8
in alternating rounds (round 0 warms up: graph capture).  The last lines give
each beam step over its yardstick and the fork's algorithmic bytes: the rows
that took another row's history at each step come from the host beam search of
tests/beam_util.py over the stage calls, which the device loop equals bit for
bit (tests/test_gpu_beam_full.py); a row that keeps its own history copies
nothing.  Divide by the fork kernel's time of a kernel trace for bytes a second.

BEAM_COST_ONLY=beam4 runs that one case twice and nothing else (for a
rocprofv3 --kernel-trace --stats run of its own).
"""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import qasr

SR, TOK, SECONDS = 16000, 322, 92.0
WIDTHS = (2, 4, 8)
CASES = [("greedy1", 1, dict(beam_width=0, top_k=0))]
CASES += [(f"greedy{w}_tk", w, dict(beam_width=0, top_k=w)) for w in WIDTHS]
CASES += [(f"beam{w}", 1, dict(beam_width=w, top_k=0)) for w in WIDTHS]
only = os.environ.get("BEAM_COST_ONLY")
if only:
    CASES = [c for c in CASES if c[0] == only]
ROUNDS = 2 if only else 4

with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "full.gguf")
    qasr.write_synthetic_gguf(p, "full", 42, 1)
    m = qasr.Model(p)
    pcm = qasr.synth_pcm(4242, int(SECONDS * SR))
    c = qasr.Context(m, max_batch=max(WIDTHS), max_ctx=2048)
    res = {name: [] for name, _, _ in CASES}
    P = None
    for rnd in range(ROUNDS):
        for name, rows, opts in CASES:
            for k, v in opts.items():
                c.set_option(k, v)
            r = c.transcribe([pcm] * rows, max_tokens=TOK, ignore_eos=True)
            assert r.timings.n_decode_steps == TOK - 1 and all(len(t) == TOK for t in r.tokens)
            if rnd:
                res[name].append(r.timings.t_decode_ms / r.timings.n_decode_steps)
    P = len(m.build_prompt(c.encode(c.mel([pcm]))[0].shape[0])[0])
    for name, _, _ in CASES:
        print(f"{name:12s} ms/step {np.round(res[name], 4).tolist()}  median {np.median(res[name]):.4f}", flush=True)
    hp = m.hp
    if not only:
        for w in WIDTHS:
            print(f"beam{w} / greedy{w}_tk = {np.median(res[f'beam{w}']) / np.median(res[f'greedy{w}_tk']):.4f}   "
                  f"beam{w} / greedy1 = {np.median(res[f'beam{w}']) / np.median(res['greedy1']):.4f}")
    # the fork of step t copies positions [P, P + t) of K, V and V^T of every row whose parent is another row: read + written
    per_pos = hp.dec_layers * hp.n_kv_heads * 128 * 2 * 3
    if not only:
        from beam_util import host_beam
        for w in WIDTHS:
            (_, st), = host_beam(c, [pcm], w, TOK, True)
            forked = [int((st.hist[t][0] != np.arange(w)).sum()) for t in range(1, TOK)]
            total = sum(2 * f * t * per_pos for t, f in enumerate(forked, 1))
            print(f"fork, W = {w}: {sum(forked)} forked rows in {TOK - 1} steps ({sum(1 for f in forked if f)} steps with any), "
                  f"{per_pos} B a position and row read and as many written: {total / 1e6:.1f} MB a run, {total / (TOK - 1) / 1e6:.3f} MB a step "
                  f"(every row forked would be {sum(2 * w * t * per_pos for t in range(1, TOK)) / (TOK - 1) / 1e6:.1f} MB a step); "
                  f"step 0 copies the prompt's {P} positions to {w - 1} rows: {2 * (w - 1) * P * per_pos / 1e6:.1f} MB", flush=True)
    c.close()
    m.close()
