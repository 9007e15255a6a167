"""Cost of hotword boosting on the full-size synthetic f16 model: decode time per step and the LM-head launch group
by HIP events (probe 1: with the constraint stage on it includes the stage's three launches), at 1, 64 and 128 rows,
three alternating rounds after a warm-up round (tools/constrain_cost.py's scheme).  Legs:
  a  off      constraints off: the yardstick
  b  stage    a constraint stage that edits nothing: a bias of -0.0 on token 0
  c  ph100    b plus 100 phrases of 4 tokens the model never emits (only their first tokens are ever boosted)
  d  ph4096   b plus 4096 phrases of 8 tokens: every 7 consecutive tokens of the transcript are the stem of an equal share
              of them, each with a tail of its own, so every step's history matches to depth 7 (min(t, 7) while it is
              shorter; asserted) in a node whose children are that share.  Stems overlap as the transcript does, so a
              shallower match usually names the transcript's next token, the raw argmax: those rows take the scan as well
              (the share of such steps is printed).  The boost is 1e-30, which changes no logit's bits, so legs a to d
              decode the same tokens (asserted)
  e  forced   a bias of +1000 on a token X the model never emits: every row's transcript is X X X ... (asserted); the
              yardstick of leg f
  f  ph4096x  e plus 4096 phrases X^7 + a tail each: every step from the 8th on matches to depth 7 in ONE node with 4096
              children (asserted), X is biased and boosted, the raw argmax is not touched: the fast path
PC_LEGS=ab runs the first two only: with QASR_LIB_OVERRIDE and PC_PYTHON naming the library and the python directory of
a build of the parent commit, leg b of the parent for the comparison DESIGN.md §5.7 records.
"""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("PC_PYTHON") or os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
import numpy as np
import qasr

SR = 16000
TOK = 64
LEGS = os.environ.get("PC_LEGS", "abcdef")
NAMES = {"a": "off", "b": "stage", "c": "ph100", "d": "ph4096", "e": "forced", "f": "ph4096x"}
TINY = 1e-30
DEPTH = 7


def match_stats(phrases, rows):
    """over every step of every row (history = the tokens before it): whether the deepest phrase position the history
    spells is min(t, DEPTH), and whether the step's own token is one a matched position boosts"""
    nxt = {}
    for ids, _ in phrases:
        for j in range(len(ids)):
            nxt.setdefault(tuple(ids[:j]), set()).add(ids[j])
    full = hit = n = 0
    for row in rows:
        for k in range(len(row)):
            js = [j for j in range(min(k, 15) + 1) if tuple(row[k - j:k]) in nxt]
            full += max(js) == min(k, DEPTH)
            hit += any(row[k] in nxt[tuple(row[k - j:k])] for j in js)
            n += 1
    return full / n, hit / n


with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "full.gguf")
    qasr.write_synthetic_gguf(p, "full", 42, 1)
    m = qasr.Model(p)
    pcm = qasr.synth_pcm(9300, int(1.1 * SR))
    for B in [int(x) for x in os.environ.get("PC_B", "1,64,128").split(",")]:
        c = qasr.Context(m, max_batch=B, max_ctx=256)
        off = c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True).tokens
        emitted = {t for row in off for t in row}
        fresh = [x for x in range(2000, 2000 + 5000) if x not in emitted]
        stems = sorted({tuple(row[k - DEPTH:k]) for row in off for k in range(DEPTH, TOK)})
        X = fresh[4096]
        lists = {"c": [(fresh[4 * k:4 * k + 4], TINY) for k in range(100)],
                 "d": [(list(stems[k % len(stems)]) + [fresh[k]], TINY) for k in range(4096)],
                 "f": [([X] * DEPTH + [fresh[k]], TINY) for k in range(4096)]}
        forced = [[X] * TOK] * B
        note = {}
        if "d" in LEGS:
            full, hit = match_stats(lists["d"], off)
            assert full == 1.0, f"leg d: {full:.2f} of the steps match to depth {DEPTH}"
            note["d"] = f"  {len(stems)} stems of {4096 // len(stems)}+ tails, steps matching to depth {DEPTH}: {full:.2f}, raw argmax boosted: {hit:.2f}"
        if "f" in LEGS:
            full, _ = match_stats(lists["f"], forced)
            assert full == 1.0
            note["f"] = f"  one node of 4096 children, steps matching to depth {DEPTH}: {full:.2f}"
        res = {k: {"probe_us": [], "step_us": []} for k in LEGS}
        for rnd in range(4):   # round 0 warms up (graph capture)
            for leg in LEGS:
                c.set_constraints(**({} if leg == "a" else dict(bias={X: 1000.0}) if leg in "ef" else dict(bias={0: -0.0})))
                if LEGS != "ab":
                    c.set_phrases(lists.get(leg))
                c.set_probe(0)
                r = c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                r = c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                assert r.tokens == (forced if leg in "ef" else off), f"leg {leg}: other tokens than expected"
                step = r.timings.t_decode_ms / r.timings.n_decode_steps * 1e3
                c.set_probe(1)
                c.transcribe([pcm] * B, max_tokens=TOK, ignore_eos=True)
                ms, n, _ = c.get_probe()
                c.set_probe(0)
                if rnd:
                    res[leg]["step_us"].append(step)
                    res[leg]["probe_us"].append(ms / n * 1e3)
        for leg in LEGS:
            v = res[leg]
            print(f"B={B:3d} {leg} {NAMES[leg]:7s} lm-head group (events) us {np.round(v['probe_us'], 2).tolist()}  "
                  f"decode step us {np.round(v['step_us'], 2).tolist()}"
                  f"{note.get(leg, '')}", flush=True)
        c.set_constraints()
        if LEGS != "ab":
            c.set_phrases()
        c.close()
    m.close()
