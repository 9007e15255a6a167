"""Cost of the pause segmentation of long recordings next to the stages around it, tiny synthetic
model (none of these stages reads the model's size): one recording of 1, 10 and 60 minutes and 16 recordings of 10
minutes, at the default parameters (max 3000, min 1000 frames, H = 5).
  segment   device time of the two launches of Context.segment (HIP events around the launches alone,
            qasr_segment_last_us) and the cut kernel's share of it
  resample  device time of the one resample launch of Context.resample over the same audio at 48 kHz
            (qasr_resample_last_us)
  mel       the mel stage's device time over the same audio as staged by stage_long: the sum of qasr_timings.t_mel_ms
            of run_staged over the pool in groups of 16 segments
Each figure is the median (min .. max) of ROUNDS rounds; a round measures every case once, one after another, so the
cases alternate; one untimed round comes first.  Writes profiles/segment/segment_cost.txt (or the path given as the
first argument)."""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
import numpy as np
import qasr

ROUNDS, GROUP = 3, 16
CASES = ((1, 1), (1, 10), (1, 60), (16, 10))   # (recordings, minutes each)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "segment", "segment_cost.txt")


def audio(minutes, rate, seed):
    """a seeded minute with a slow envelope, repeated"""
    n = 60 * rate
    x = qasr.synth_pcm(seed, n) * (0.05 + np.abs(np.sin(np.arange(n) * (2 * np.pi / (7.3 * rate)))))
    return np.tile(x.astype(np.float32), minutes)


def stat(v):
    return f"{float(np.median(v)):.0f} ({min(v):.0f} .. {max(v):.0f})"


lines = [f"default parameters, tiny synthetic f16 model, one MI355X; device time by HIP events, median (min .. max) of {ROUNDS} alternating rounds after a warm-up round",
         "recordings  minutes  segments  segment us            of which cut us       resample 48k us       mel us                 segment / mel  audio-s per segment-s"]
with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "tiny.gguf")
    qasr.write_synthetic_gguf(p, "tiny", 42, 1)
    m = qasr.Model(p)
    c = qasr.Context(m, max_batch=GROUP, max_ctx=512)
    data = {mins: (audio(mins, 16000, 9600 + mins), audio(mins, 48000, 9700 + mins)) for mins in sorted({k[1] for k in CASES})}
    res = {k: dict(seg=[], cut=[], rs=[], mel=[], n=0) for k in CASES}
    for rnd in range(ROUNDS + 1):
        for B, mins in CASES:
            x16, x48 = data[mins]
            c.segment([x16] * B)
            us, cut = c.segment_last_us()
            c.resample([x48] * B, [48000] * B)
            rs = c.resample_last_us()
            segs = c.stage_long([x16] * B)
            mel = 0.0
            for i in range(0, len(segs), GROUP):
                mel += c.run_staged(list(range(i, min(i + GROUP, len(segs)))), 2, ignore_eos=True).timings.t_mel_ms * 1000.0
            r = res[(B, mins)]
            r["n"] = len(segs)
            if rnd:
                r["seg"].append(us); r["cut"].append(cut); r["rs"].append(rs); r["mel"].append(mel)
    for (B, mins), r in res.items():
        a, b = float(np.median(r["seg"])), float(np.median(r["mel"]))
        lines.append(f"{B:10d}  {mins:7d}  {r['n']:8d}  {stat(r['seg']):<20s}  {stat(r['cut']):<20s}  {stat(r['rs']):<20s}  {stat(r['mel']):<21s}  {a / b:13.3f}  {B * mins * 60 / (a * 1e-6):21.0f}")
        print(lines[-1], flush=True)
    c.close()
    m.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
