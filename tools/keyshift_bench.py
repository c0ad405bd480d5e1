"""svc_mel_keyshift (the key-shifted start mel of shallow diffusion, a direct f64 DFT of rint(n_fft * factor) points per
frame) at the benchmark's batch, B = 32 clips of 240,000 samples (T = 937), with every clip at one factor: 0.5, 1,
2 ** (4 / 12) and 2 (n_new = 512, 1024, 1290, 2048), and svc_mel_energy (the radix FFT of n_fft points) timed in the
same run.

Each figure is the HIP-event time of one call, warm (3 calls of every side first); the sides alternate, and the median,
minimum and maximum of 20 calls are recorded. The audio is the seeded synthetic clip of the tests (timing does not
depend on its values). Nothing is gated. Prints one JSON line; --out FILE also writes it there.

Usage: python tools/keyshift_bench.py [--reps 20] [--out profiles/keyshift_bench.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402
from svc_inference_pipeline_amd.synth import synth_clip  # noqa: E402

B, N = 32, 240000
FACTORS = {"0.5": 0.5, "1": 1.0, "2^(4/12)": 2.0 ** (4 / 12), "2": 2.0}


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("keyshift_bench: needs a GPU (no CPU timing)")
    cfg = C.load_config()
    eng = SVCEngine(cfg, 0)
    wav = torch.from_numpy(synth_clip(0, N / cfg.fs, cfg.fs))[None].repeat(B, 1).cuda().contiguous()
    sides = {"mel_energy": lambda: eng.mel_energy(wav)[0]}
    for name, f in FACTORS.items():
        fac = torch.full((B,), f, dtype=torch.float64).cuda()
        sides["keyshift_" + name] = lambda fac=fac: eng.mel_keyshift(wav, fac)[0]
    finite = all(bool(torch.isfinite(fn()).all()) for fn in sides.values())
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(args.reps):
        for name, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[name].append(a.elapsed_time(b))
    T = mel_frames(N, cfg.n_fft, cfg.hop_length)
    res = {"tool": "keyshift_bench", "B": B, "n_samples": N, "T": T, "n_fft": cfg.n_fft, "reps": args.reps,
           "outputs_finite": finite, "mel_energy": {"ms": spread(t["mel_energy"])}}
    for name, f in FACTORS.items():
        n_new = int(min(max(round(cfg.n_fft * f), cfg.n_fft // 2), 2 * cfg.n_fft))
        bins = min(cfg.n_fft, n_new) // 2 + 1
        ms = t["keyshift_" + name]
        med = statistics.median(ms)
        # two f64 FMAs per (frame, bin > 0, sample)
        res["keyshift_" + name] = {"factor": f, "n_new": n_new, "ms": spread(ms),
                                   "f64_gfma_per_s": round(2.0 * B * T * (bins - 1) * n_new / med / 1e6, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
