"""Whisper content features of a ragged batch (SVCPipeline.ragged_content, Whisper-medium dims, default precision mode):
the one-pass form (one svc_whisper_content_ragged: every window that exists encoded once, one mapping launch) against
the two-group form (whisper_ragged=False: the path as it was before the one-pass form existed, left unchanged in the
code, so the comparison is never against the code under test), the two alternating in one process.

  (a) equal_10s: 32 clips of 10 s: both forms encode 32 windows in one pass, so the difference is what the window
      table and the mapping cost;
  (b) ragged_5_10s: 32 clips of seeded, pairwise distinct lengths between 5 and 10 s: still one window each;
  (c) mixed_10_65_125s: 16 clips of 10 s, 8 of 65 s and 8 of 125 s: the two-group form runs the encoder twice and pads
      every long clip to the longest one's 5 windows.

Per batch and form: host-clock ms around a call that ends synchronised, median / min / max of `reps` calls on one input
(warm) and again rotating over distinct inputs, after every input has been run once in every form; windows encoded per
call (counted at the engine's encoder entry points); launches per call from the library's own events; outputs_match
(torch.equal of the two forms' results). default_stands: in every case the one-pass form's median is no slower than the
two-group form's median by more than the two-group form's own spread (its max - min) in this run.
Prints one JSON line and writes it to profiles/whisper_ragged_bench.json. Usage: python tools/whisper_ragged_bench.py [reps]"""
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
N_ROT = 3


class CountingEngine:
    """the engine, counting the windows that go into its encoder entry points"""

    def __init__(self, engine):
        self._e = engine
        self.windows = 0

    def __getattr__(self, name):
        return getattr(self._e, name)

    def whisper_encode(self, wav16):
        self.windows += int(wav16.shape[0])
        return self._e.whisper_encode(wav16)

    def whisper_content(self, wav16, n_samples, frames, T, **kw):
        self.windows += sum(self._e.whisper_windows(t) for t in frames)
        return self._e.whisper_content(wav16, n_samples, frames, T, **kw)


def make_batch(lengths, seed):
    """device 16 kHz clips of the given lengths on the int16 grid (noise plus a tone, peak about 0.5) and their mel
    frame counts at 24 kHz (1.5 x the samples)"""
    g = torch.Generator().manual_seed(seed)
    clips = []
    for i, n in enumerate(lengths):
        t = torch.arange(n, dtype=torch.float64) / 16000.0
        x = 0.3 * torch.sin(2 * np.pi * (180.0 + 9 * i) * t).float() + 0.05 * torch.randn(n, generator=g)
        clips.append((torch.round(x * 32768.0).clamp(-32768, 32767) / 32768.0).cuda())
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
    names = list(forms)
    res, windows = {}, {}
    for name in names:
        forms[name].engine.windows = 0
        res[name] = run[name](0)
        windows[name] = forms[name].engine.windows
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
           "frames_max": T, "outputs_match": bool(match)}
    for n in names:
        out[n] = {"warm_ms": stats(warm[n]), "rotating_ms": stats(rot[n]), "windows_encoded": windows[n],
                  "launches_per_call": launches(lambda: run[n](0))}
    return out


def main():
    reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 10
    d = W.WHISPER_DIMS["medium"]
    cfg = C.load_config()
    cfg.mapper.content_feature = ["whisper"]
    cfg.mapper.input_content_dim["whisper"] = d["n_audio_state"]
    eng = SVCEngine(cfg, 0, whisper_state=W.make_whisper_state(d, 0))
    cases = ("equal_10s", "ragged_5_10s", "mixed_10_65_125s")
    try:
        forms = {"one_pass": SVCPipeline(CountingEngine(eng), whisper_ragged=True),
                 "two_group": SVCPipeline(CountingEngine(eng), whisper_ragged=False)}
        assert forms["one_pass"].whisper_ragged and not forms["two_group"].whisper_ragged
        rng = np.random.default_rng(0)
        ragged = sorted(int(v) * 2 for v in rng.choice(np.arange(40000, 80001), size=B, replace=False))  # 5 .. 10 s
        mixed = [160000] * 16 + [65 * 16000] * 8 + [125 * 16000] * 8
        res = {"tool": "whisper_ragged_bench", "B": B, "dims": "medium", "reps": reps, "rotating_inputs": N_ROT}
        for key, lengths in zip(cases, ([160000] * B, ragged, mixed)):
            res[key] = bench_batch(forms, lengths, reps)
            print(f"{key}: done", file=sys.stderr, flush=True)
        res["clocks"] = clocks()
        ok = True
        for key in cases:
            for kind in ("warm_ms", "rotating_ms"):
                old, new = res[key]["two_group"][kind], res[key]["one_pass"][kind]
                ok = ok and new["median"] <= old["median"] + (old["max"] - old["min"])
        res["default_stands"] = bool(ok)
        res["outputs_match"] = bool(all(res[key]["outputs_match"] for key in cases))
        line = json.dumps(res)
        print(line, flush=True)
        out_dir = os.path.join(REPO, os.environ.get("WHISPER_RAGGED_BENCH_DIR", "profiles"))
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "whisper_ragged_bench.json"), "w") as fh:
            fh.write(line + "\n")
    finally:
        eng.close()
    if not res["outputs_match"]:
        raise SystemExit("the one-pass and two-group forms differ")


if __name__ == "__main__":
    main()
