"""The DiffSVC sampler stage under shallow diffusion (svc_diffsvc_sample_from, k_step) at the benchmark's batch,
B = 32, T = 937, PLMS at interval 10, against the existing full call (svc_diffsvc_sample from device noise) run from the
same build:

  - full:  SVCEngine.diffsvc_sample(cond, fast_inference=True, speedup=10, seed, utt_ids): 101 denoiser calls;
  - K = 1000, 500, 300, 100: the same with k_step=K, mel_src=mel: (K - 1) // 10 + 2 denoiser calls after one fused
    normalise + q_sample launch.

Each figure is HIP-event time around a group of back-to-back calls, per call, after a warm-up of every side; the sides'
groups alternate, and the median, minimum and maximum over the rounds are recorded (the spread). Weights are the seeded
random mapper of the reference architecture (timing does not depend on their values). Nothing is gated: the
expectation is only that time follows the denoiser-call count. Prints one JSON line; --out FILE also writes it there.

Usage: python tools/shallow_bench.py [--rounds 7] [--out profiles/shallow_bench.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

B, T, INTERVAL = 32, 937, 10
KS = (1000, 500, 300, 100)


def denoiser_calls(K, interval=INTERVAL):
    """PLMS iterations i = ((K - 1) // interval) * interval, ..., 0, and the first one calls the denoiser twice."""
    return (K - 1) // interval + 2


def alternate(sides, rounds, warm=2):
    """sides: {name: (fn, calls per group)} -> {name: per-call milliseconds, one per round}, the groups alternating"""
    for fn, _ in sides.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for name, (fn, calls) in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / calls)
    return out


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shallow_bench: needs a GPU (no CPU timing)")
    cfg = C.load_config()
    eng = SVCEngine(cfg, 0, mapper_state=W.make_mapper_state(cfg.mapper, 0))
    gen = torch.Generator().manual_seed(0)
    cond = (torch.randn(B, T, cfg.mapper.residual_channels, generator=gen) * 0.5).cuda()
    st = C.load_stats(cfg)
    mn, mx = torch.from_numpy(st["mel_min"]), torch.from_numpy(st["mel_max"])
    mel = (mn + (mx - mn) * torch.rand(B, T, cfg.mapper.n_mel, generator=gen)).cuda().contiguous()
    utt = torch.arange(B, dtype=torch.int32).cuda()
    kw = dict(fast_inference=True, speedup=INTERVAL, seed=0, utt_ids=utt)
    sides = {"full": (lambda: eng.diffsvc_sample(cond, **kw), 1)}
    for K in KS:
        sides["k%d" % K] = (lambda K=K: eng.diffsvc_sample(cond, k_step=K, mel_src=mel, **kw), 2 if K <= 100 else 1)
    finite = all(bool(torch.isfinite(fn()).all()) for fn, _ in sides.values())
    t = alternate(sides, args.rounds)
    full = statistics.median(t["full"])
    res = {"tool": "shallow_bench", "B": B, "T": T, "mode": "plms", "interval": INTERVAL, "rounds": args.rounds,
           "outputs_finite": finite,
           "full": {"denoiser_calls": denoiser_calls(1000), "ms": spread(t["full"])}}
    for K in KS:
        ms = t["k%d" % K]
        res["k_step_%d" % K] = {"denoiser_calls": denoiser_calls(K), "ms": spread(ms),
                                "ms_per_denoiser_call": round(statistics.median(ms) / denoiser_calls(K), 4),
                                "time_over_full": round(statistics.median(ms) / full, 4),
                                "calls_over_full": round(denoiser_calls(K) / denoiser_calls(1000), 4)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
