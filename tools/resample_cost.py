"""Cost of the resampler to 16 kHz next to the mel stage it feeds, tiny synthetic model (neither
stage reads the model's size): 30 s clips at 8000, 44100, 48000 and 96000 Hz, 1 and 64 clips a launch.
  resample  device time of the one resample launch of Context.resample (HIP events around the launch alone,
            qasr_resample_last_us), median and range of RUNS calls after a warm-up call
  mel       the mel stage's device time (qasr_timings.t_mel_ms, HIP events around both mel kernels) of a run over the
            same clips staged with their rate, median and range of RUNS runs after a warm-up run
Writes profiles/resample/resample_cost.txt (or the path given as the first argument)."""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr.cpp_amd", "python"))
import numpy as np
import qasr

SECONDS, RUNS = 30, 7
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resample", "resample_cost.txt")
lines = [f"30 s clips, tiny synthetic f16 model, one MI355X; device time by HIP events, median (min .. max) of {RUNS} after a warm-up",
         "rate Hz  clips  taps  L    resample us           mel us                resample / mel  audio-s per resample-s"]
with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "tiny.gguf")
    qasr.write_synthetic_gguf(p, "tiny", 42, 1)
    m = qasr.Model(p)
    for B in (1, 64):
        c = qasr.Context(m, max_batch=B, max_ctx=512)
        for sr in (8000, 44100, 48000, 96000):
            L, _M, H = qasr.resample_plan(sr)
            clip = qasr.synth_pcm(9500 + sr % 97, SECONDS * sr)
            clips, rates = [clip] * B, [sr] * B
            rs, mel = [], []
            for k in range(RUNS + 1):
                c.resample(clips, rates)
                us = c.resample_last_us()
                c.stage_audio(clips, rates)
                t = c.run(2, ignore_eos=True).timings.t_mel_ms * 1000.0
                if k:
                    rs.append(us)
                    mel.append(t)
            a, b = float(np.median(rs)), float(np.median(mel))
            rs_s, mel_s = f"{a:.0f} ({min(rs):.0f} .. {max(rs):.0f})", f"{b:.0f} ({min(mel):.0f} .. {max(mel):.0f})"
            lines.append(f"{sr:7d}  {B:5d}  {2 * H + 1:4d}  {L:3d}  {rs_s:<20s}  {mel_s:<20s}  {a / b:14.2f}  {B * SECONDS / (a * 1e-6):22.0f}")
            print(lines[-1], flush=True)
        c.close()
    m.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
