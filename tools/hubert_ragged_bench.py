"""ContentVec content features of a ragged batch (SVCPipeline.ragged_content, real ContentVec dims, default precision
mode): the one-pass form (one padded svc_hubert_encode_ragged + one svc_map_content_ragged) against the per-bucket form
(hubert_ragged=False: one encoder pass, one mapping and one copy per exact length), the two alternating in one process.

  (a) 32 clips of seeded, pairwise distinct lengths between 5 and 10 s: the per-bucket form runs 32 passes at B = 1;
  (b) 32 clips of 10 s: both forms run one pass, so the difference is what the length handling itself costs.

Per batch and form: host-clock ms around a call that ends synchronised (the per-bucket form's cost is partly host work),
median / min / max of `reps` calls on one input (warm) and again rotating over distinct inputs; launches per call from
the library's own events; outputs_match (torch.equal of the two forms' results). default_stands: the one-pass form is
at least as fast as the per-bucket form on both batches, within the per-bucket form's own spread (its max - min).
Prints one JSON line and writes it to profiles/hubert_ragged_bench.json. Usage: python tools/hubert_ragged_bench.py [reps]"""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from load_bench import clocks  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402

B = 32
N_ROT = 4


def make_batch(lengths, seed):
    """device 16 kHz clips of the given lengths (noise plus a tone, peak about 0.5) and their mel frame counts at
    24 kHz (1.5 x the samples)"""
    g = torch.Generator().manual_seed(seed)
    clips = []
    for i, n in enumerate(lengths):
        t = torch.arange(n, dtype=torch.float32) / 16000.0
        clips.append((0.3 * torch.sin(2 * np.pi * (180.0 + 9 * i) * t) + 0.05 * torch.randn(n, generator=g)).cuda())
    return clips, [mel_frames(n * 3 // 2) for n in lengths]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def launches(fn):
    _lib.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    n = sum(v["launches"] for v in _lib.profile_read().values())
    _lib.profile_enable(False)
    return int(n)


def bench_batch(forms, lengths, reps):
    inputs = [make_batch(lengths, 100 + k) for k in range(N_ROT)]
    T = max(inputs[0][1])
    run = {name: (lambda k, p=p: p.ragged_content(inputs[k][0], inputs[k][1], T)) for name, p in forms.items()}
    res = {name: run[name](0) for name in forms}
    names = list(forms)
    match = torch.equal(res[names[0]], res[names[1]])
    del res
    for name in names:  # warm every input in every form
        for k in range(N_ROT):
            run[name](k)
    warm = {n: [] for n in names}
    rot = {n: [] for n in names}
    for r in range(reps):
        for n in names:
            warm[n].append(timed(lambda: run[n](0)))
    for r in range(reps):
        for n in names:
            rot[n].append(timed(lambda: run[n](r % N_ROT)))
    out = {"samples_min": min(lengths), "samples_max": max(lengths), "distinct_lengths": len(set(lengths)),
           "outputs_match": bool(match)}
    for n in names:
        out[n] = {"warm_ms": stats(warm[n]), "rotating_ms": stats(rot[n]), "launches_per_call": launches(lambda: run[n](0))}
    return out


def main():
    reps = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 15
    d = W.HUBERT_DIMS["contentvec"]
    cfg = C.load_config()
    cfg.mapper.content_feature = ["contentvec"]
    cfg.mapper.input_content_dim["contentvec"] = d["final_dim"]
    eng = SVCEngine(cfg, 0, hubert_state=W.make_hubert_state(d, 1), hubert_output_layer=d["output_layer"])
    try:
        forms = {"one_pass": SVCPipeline(eng, hubert_ragged=True), "per_bucket": SVCPipeline(eng, hubert_ragged=False)}
        assert forms["one_pass"].hubert_ragged and not forms["per_bucket"].hubert_ragged
        rng = np.random.default_rng(0)
        ragged = sorted(int(v) * 2 for v in rng.choice(np.arange(40000, 80001), size=B, replace=False))  # 5 .. 10 s
        res = {"tool": "hubert_ragged_bench", "B": B, "dims": "contentvec", "reps": reps, "rotating_inputs": N_ROT,
               "ragged_5_10s": bench_batch(forms, ragged, reps),
               "equal_10s": bench_batch(forms, [160000] * B, reps)}
        res["clocks"] = clocks()
        ok = True
        for key in ("ragged_5_10s", "equal_10s"):
            for kind in ("warm_ms", "rotating_ms"):
                old, new = res[key]["per_bucket"][kind], res[key]["one_pass"][kind]
                ok = ok and new["median"] <= old["median"] + (old["max"] - old["min"])
        res["default_stands"] = bool(ok)
        res["outputs_match"] = bool(res["ragged_5_10s"]["outputs_match"] and res["equal_10s"]["outputs_match"])
        line = json.dumps(res)
        print(line, flush=True)
        out_dir = os.path.join(REPO, os.environ.get("HUBERT_RAGGED_BENCH_DIR", "profiles"))
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "hubert_ragged_bench.json"), "w") as fh:
            fh.write(line + "\n")
    finally:
        eng.close()
    if not res["outputs_match"]:
        raise SystemExit("the one-pass and per-bucket forms differ")


if __name__ == "__main__":
    main()
