"""The DiffSVC sampler stage under the DPM-Solver++(2M) solver (svc_diffsvc_sample_steps) at the benchmark's batch,
B = 32, T = 937, against the existing full PLMS call (svc_diffsvc_sample, interval 10, from device noise) run from the
same build:

  - plms:            SVCEngine.diffsvc_sample(cond, fast_inference=True, speedup=10, seed, utt_ids): 101 denoiser calls;
  - dpmpp2m 50/20/10: the same with solver="dpmpp2m", solver_steps=N from device noise: one denoiser call per timestep of
                     config.solver_timesteps (logsnr spacing drops coinciding nodes, so the list may be shorter than N);
  - k300 20/10:      the same from k_step=300, mel_src=mel (one fused normalise + q_sample launch first).

Each figure is HIP-event time around a group of back-to-back calls, per call, after a warm-up of every side; the sides'
groups alternate, and the median, minimum and maximum over the rounds are recorded (the spread). Weights are the seeded
random mapper of the reference architecture (timing does not depend on their values; neither does this tool say
anything about output quality at N steps, which has been checked on an analytic denoiser and random weights only).
Nothing is gated: the expectation is only that time follows the denoiser-call count. Prints one JSON line; --out FILE
also writes it there.

Usage: python tools/dpm_bench.py [--rounds 7] [--out profiles/dpm_bench.json]"""
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
PLMS_CALLS = (1000 - 1) // INTERVAL + 2
SIDES = [("dpmpp2m_50", None, 50), ("dpmpp2m_20", None, 20), ("dpmpp2m_10", None, 10), ("k300_dpmpp2m_20", 300, 20),
         ("k300_dpmpp2m_10", 300, 10)]


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
        raise SystemExit("dpm_bench: needs a GPU (no CPU timing)")
    cfg = C.load_config()
    eng = SVCEngine(cfg, 0, mapper_state=W.make_mapper_state(cfg.mapper, 0))
    gen = torch.Generator().manual_seed(0)
    cond = (torch.randn(B, T, cfg.mapper.residual_channels, generator=gen) * 0.5).cuda()
    st = C.load_stats(cfg)
    mn, mx = torch.from_numpy(st["mel_min"]), torch.from_numpy(st["mel_max"])
    mel = (mn + (mx - mn) * torch.rand(B, T, cfg.mapper.n_mel, generator=gen)).cuda().contiguous()
    utt = torch.arange(B, dtype=torch.int32).cuda()
    kw = dict(seed=0, utt_ids=utt)
    sides = {"plms": (lambda: eng.diffsvc_sample(cond, fast_inference=True, speedup=INTERVAL, **kw), 1)}
    calls = {"plms": PLMS_CALLS}
    for name, K, n in SIDES:
        calls[name] = len(C.solver_timesteps(cfg, K, n))
        shallow = {} if K is None else dict(k_step=K, mel_src=mel)
        sides[name] = (lambda n=n, shallow=shallow: eng.diffsvc_sample(cond, solver="dpmpp2m", solver_steps=n, **shallow,
                                                                       **kw), 1 if n >= 50 else 2)
    finite = all(bool(torch.isfinite(fn()).all()) for fn, _ in sides.values())
    t = alternate(sides, args.rounds)
    full = statistics.median(t["plms"])
    res = {"tool": "dpm_bench", "B": B, "T": T, "rounds": args.rounds, "outputs_finite": finite}
    for name in sides:
        ms = t[name]
        res[name] = {"denoiser_calls": calls[name], "ms": spread(ms),
                     "ms_per_denoiser_call": round(statistics.median(ms) / calls[name], 4),
                     "time_over_plms": round(statistics.median(ms) / full, 4),
                     "calls_over_plms": round(calls[name] / PLMS_CALLS, 4)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
