"""What prompt sharing saves: qasr_score of 8 hypotheses x 64 tokens of one 30 s clip against eight
independent full prefills of prompt + hypothesis through qasr_prefill_score, and against a greedy
qasr_run of 64 tokens, on the full-size synthetic f16 model; alternating repetitions, host wall time
around each synchronous call (milliseconds, median).

    python tools/score_cost.py [--reps 5] [--model full-f16.gguf] > profiles/score/score_cost.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
import qasr   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model", default="")
    ap.add_argument("--hyps", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    a = ap.parse_args()
    tmp = None
    path = a.model
    if not path:
        tmp = tempfile.TemporaryDirectory()
        path = os.path.join(tmp.name, "full-f16.gguf")
        qasr.write_synthetic_gguf(path, "full", 42, 1)
    m = qasr.Model(path)
    pcm = qasr.synth_pcm(9000, int(a.seconds * 16000))
    P = qasr.lib().qasr_prompt_len(qasr.encoder_frames(qasr.mel_frames(len(pcm))))
    c = qasr.Context(m, max_batch=a.hyps, max_ctx=P + a.tokens + 8)
    rng = np.random.default_rng(1)
    hyps = [rng.integers(0, 151643, a.tokens).tolist() for _ in range(a.hyps)]
    c.stage_audio([pcm])
    feats = c.encode(c.mel([pcm]))[0]
    ids, pos = m.build_prompt(feats.shape[0])
    eos = m.hp.eos_id

    def shared():
        t = qasr.Timings()
        r = c.score([0] * a.hyps, hyps, include_eos=True, timings=t)
        return r, t

    def independent():
        out = []
        for h in hyps:   # the front end is not repeated: features from the host, as a caller holding them would
            seq = list(ids) + h
            tg = [-1] * (len(ids) - 1) + h + [eos]
            out.append(c.prefill_score([seq], [tg], feats_list=[feats], audio_pos=[pos])[0])
        return out

    def greedy():
        return c.run(a.tokens, ignore_eos=True)

    times = {"score (shared prompt)": [], "8 x prefill_score (prompt + hypothesis)": [], "greedy run": []}
    stage = []
    for it in range(-1, a.reps):   # one warm-up round
        for name, fn in zip(times, (shared, independent, greedy)):
            t0 = time.perf_counter()
            r = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= 0:
                times[name].append(dt)
                if name.startswith("score"):
                    t = r[1]
                    stage.append((t.t_mel_ms, t.t_encode_ms, t.t_prefill_ms, t.t_decode_ms))
    s, _ = shared()
    ind = independent()
    worst = max(float(np.abs(x.logprobs - y.logprobs).max()) for x, y in zip(s, ind))
    print(f"full-size f16, one {a.seconds:.0f} s clip (prompt {P} tokens), {a.hyps} hypotheses x {a.tokens} tokens + EOS, "
          f"{a.reps} alternating repetitions; host wall ms of the synchronous call (median, min .. max)")
    for name, v in times.items():
        print(f"  {name:42s} {statistics.median(v):9.2f}   {min(v):9.2f} .. {max(v):9.2f}")
    st = np.median(np.array(stage), axis=0)
    print(f"  score, device time by stage (median): mel {st[0]:.2f}  encoder {st[1]:.2f}  prompt prefill {st[2]:.2f}  "
          f"fork + chunk prefill + score heads {st[3]:.2f}")
    print(f"  max |shared - independent| over all entries: {worst:.3g}")
    c.close()
    m.close()


if __name__ == "__main__":
    main()
