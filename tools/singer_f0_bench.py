"""The pooled voiced median (svc_f0_voiced_median) at the size of the reference's recorded target contours, against
the one-workgroup select it complements:

  - new:      svc_f0_voiced_median on 223,087 frames as one pooled row (the fixture's contours tiled to that size;
              109 workgroups, 10 stream operations per call);
  - baseline: svc_pitch_shift with B = 1, T = 223,087 on the same data: pitch_shift_kernel's 64-pass select, twice for
              an even voiced count, all in one workgroup (its target is the data's own median, so the factor is exactly
              1 and the in-place call leaves the data as it was);
  - for information: svc_pitch_shift_ex against svc_pitch_shift at B = 32, T = 937 (the same kernel plus a staged table);
  - the histogram pass with one LDS atomic per cell (what the library runs) against the wave-aggregated forms, from
    tools/median_ab (built from tools/median_ab.hip with the command in its header when the program is not there).

Each figure is HIP-event time around a group of back-to-back calls, per call, after a warm-up; the groups of the two
sides alternate, and the median, minimum and maximum over the rounds are recorded (the spread). The new entry's result
is checked against np.median first. Prints one JSON line; --out FILE also writes it there.

Usage: python tools/singer_f0_bench.py [--rounds 15] [--out profiles/singer_f0_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

N_FRAMES = 223087  # frames of the reference's config/f0.pkl


def alternate(sides, rounds, warm=5):
    """sides: {name: (fn, calls per group)} -> {name: per-call microseconds, one per round}, the sides' groups alternating"""
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
            out[name].append(1e3 * a.elapsed_time(b) / calls)
    return out


def spread(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}


def median_ab(n):
    exe = os.path.join(REPO, "tools", "median_ab")
    if not os.path.exists(exe):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "-I" + os.path.join(REPO, "include"),
                        "-I" + os.path.join(REPO, "svc_inference_pipeline_amd", "csrc"),
                        os.path.join(REPO, "tools", "median_ab.hip"), "-o", exe], check=True)
    r = subprocess.run([exe, str(n)], check=True, capture_output=True, text=True, timeout=300)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = np.load(os.path.join(REPO, "tests", "golden", "target_f0_contours.npz"))
    host = np.resize(g["f0"], N_FRAMES)
    voiced = host[host != 0]
    want = float(np.median(voiced))
    eng = SVCEngine(C.load_config(), 0)
    x = torch.from_numpy(host).cuda()[None].contiguous()
    med, cnt = eng.f0_voiced_median(x)
    torch.cuda.synchronize()
    ok = float(med.item()) == want and int(cnt.item()) == voiced.size
    y = x.clone()
    t = alternate({"new": (lambda: eng.f0_voiced_median(x), 20), "baseline": (lambda: eng.pitch_shift(y, want), 3)},
                  args.rounds)
    unchanged = bool(torch.equal(x, y))  # factor exactly 1: every baseline call saw the same data
    # B = 32, T = 937: one contour-like row repeated, shifted onto its own median (factor 1 again)
    row = np.resize(g["f0"], 937)
    m = float(np.median(row[row != 0]))
    a = torch.from_numpy(np.tile(row, (32, 1))).cuda().contiguous()
    b = a.clone()
    t2 = alternate({"ex": (lambda: eng.pitch_shift(a, [m] * 32), 20), "scalar": (lambda: eng.pitch_shift(b, m), 20)},
                   args.rounds)
    ab = median_ab(N_FRAMES)
    res = {
        "tool": "singer_f0_bench", "frames": N_FRAMES, "voiced": int(voiced.size), "median_hz": want,
        "matches_np_median": bool(ok), "baseline_data_unchanged": unchanged, "rounds": args.rounds,
        "workgroups": -(-N_FRAMES // 2048), "stream_operations_per_call": 10,
        "svc_f0_voiced_median_us": spread(t["new"]),
        "baseline_svc_pitch_shift_B1_us": spread(t["baseline"]),
        "speedup_median": round(statistics.median(t["baseline"]) / statistics.median(t["new"]), 2),
        "speedup_worst_case": round(min(t["baseline"]) / max(t["new"]), 2),
        "B32_T937_svc_pitch_shift_ex_us": spread(t2["ex"]), "B32_T937_svc_pitch_shift_us": spread(t2["scalar"]),
        "histogram_forms": ab,
    }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    if not ok:
        raise SystemExit("svc_f0_voiced_median differs from np.median")


if __name__ == "__main__":
    main()
