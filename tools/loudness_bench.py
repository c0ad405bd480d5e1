"""Loudness envelope transfer (svc_loudness_match) alone, at so-vits-svc's default window / hop (fs // 2 * 2, fs // 2),
for the two shapes a batch takes: 32 clips of 240,000 samples and one clip of 4,320,000 (three minutes).

  - HIP-event time per call, warm, median of `reps` (>= 20) calls on one input (which then sits in the 256 MB
    Infinity Cache), and again rotating over enough distinct inputs that every call reads from HBM;
  - the two launches alone (the library's own events around each, same rotation);
  - svc_pcm16 on the same batch, in the same run, as the yardstick: the stage that follows it in the pipeline and
    streams the same waveform;
  - an empty event pair (what the event method itself reads) and the GPU's clocks right behind the timed calls;
  - clip 0 of each shape against audio.loudness_match on the host (every sample within 1 f32 ulp).

Prints one JSON line and writes it to profiles/loudness_bench.json (or the path given).
Usage: python tools/loudness_bench.py [reps] [out.json]"""
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from load_bench import clocks  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

SHAPES = ((32, 240000), (1, 4320000))
N_ROT = 12     # distinct inputs: 12 x (wav + src + out) of 30.7 / 17.3 MB each between two reads of the same buffer
WARM_UP = 16   # calls before any timing: the staging ring's 8 slots allocate on their first use


def event_ms(fn, n_inputs, reps):
    """median / min HIP-event ms of fn(i % n_inputs) over reps calls, after warm passes over every input"""
    for i in range(max(WARM_UP, n_inputs)):
        fn(i % n_inputs)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i % n_inputs)
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return round(statistics.median(ms), 5), round(min(ms), 5)


def kernel_ms(prefix, fn, n_inputs, reps):
    """mean ms per launch of the kernels whose profiler name starts with prefix, and launches per call"""
    _lib.profile_filter(prefix)
    _lib.profile_enable(True)
    try:
        for i in range(reps):
            fn(i % n_inputs)
        torch.cuda.synchronize()
        stats = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
        _lib.profile_filter("")
    ms = {k.split("@")[0]: round(v["ms"] / v["launches"], 5) for k, v in stats.items()}
    return ms, sum(v["launches"] for v in stats.values()) / reps


def ulps(got, want):
    o = lambda a: np.where(a.view(np.int32) < 0, -(a.view(np.int32).astype(np.int64) & 0x7FFFFFFF),
                           a.view(np.int32).astype(np.int64))
    return int(np.abs(o(np.ascontiguousarray(got)) - o(np.ascontiguousarray(want))).max())


def bench_shape(eng, fs, B, S, reps):
    g = torch.Generator().manual_seed(B)
    env = torch.linspace(0.2, 1.0, S)
    wav0 = (torch.randn(B, S, generator=g) * 0.2).cuda()
    src0 = (torch.randn(B, S, generator=g) * 0.2 * env).cuda()
    wavs = [wav0] + [(wav0 * (1.0 - 0.01 * k)).contiguous() for k in range(1, N_ROT)]
    srcs = [src0] + [(src0 * (1.0 + 0.01 * k)).contiguous() for k in range(1, N_ROT)]
    outs = [torch.empty_like(wav0) for _ in range(N_ROT)]
    window, hop = A.loudness_params(fs)

    def loud(i):
        eng.loudness_match(wavs[i], srcs[i], mix=0.0, out=outs[i])

    def pcm(i):
        eng.pcm16(wavs[i])

    res = {"B": B, "S": S, "window": window, "hop": hop, "frames": 1 + S // hop,
           "algorithmic_bytes": B * S * 4 * 4}  # wav read twice, src once, out written once
    res["svc_loudness_match_ms_warm_median"], res["svc_loudness_match_ms_warm_min"] = event_ms(loud, 1, reps)
    res["svc_pcm16_ms_warm_median"], res["svc_pcm16_ms_warm_min"] = event_ms(pcm, 1, reps)
    rot = max(reps, 4 * N_ROT)
    res["svc_loudness_match_ms_rotating_median"], res["svc_loudness_match_ms_rotating_min"] = event_ms(loud, N_ROT, rot)
    res["svc_pcm16_ms_rotating_median"], res["svc_pcm16_ms_rotating_min"] = event_ms(pcm, N_ROT, rot)
    res["clocks"] = clocks()  # right behind the timed calls
    res["kernel_ms_rotating_mean"], res["launches_per_call"] = kernel_ms("loudness", loud, N_ROT, rot)
    res["pcm16_kernel_ms_rotating_mean"], res["pcm16_launches_per_call"] = kernel_ms("pcm16", pcm, N_ROT, rot)
    k_ms = sum(res["kernel_ms_rotating_mean"].values())
    res["kernels_bytes_per_s_rotating"] = round(res["algorithmic_bytes"] / (k_ms * 1e-3), 0)
    res["ratio_to_svc_pcm16_rotating"] = round(res["svc_loudness_match_ms_rotating_median"]
                                               / res["svc_pcm16_ms_rotating_median"], 3)
    want = A.loudness_match(wav0[0].cpu().numpy(), src0[0].cpu().numpy(), fs=fs, mix=0.0)
    loud(0)
    res["clip0_max_ulp_vs_host"] = ulps(outs[0][0].cpu().numpy(), want)
    return res


def main():
    reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 50
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "loudness_bench.json")
    cfg = C.load_config()
    eng = SVCEngine(cfg, 0)
    fs = int(cfg.fs)
    empty = event_ms(lambda i: None, 1, reps)
    res = {"tool": "loudness_bench", "fs": fs, "reps": reps, "mix": 0.0, "event_pair_empty_ms_median": empty[0],
           "shapes": [bench_shape(eng, fs, B, S, reps) for B, S in SHAPES], "torch_threads": torch.get_num_threads()}
    res["outputs_match"] = all(s["clip0_max_ulp_vs_host"] <= 1 for s in res["shapes"])
    line = json.dumps(res)
    print(line, flush=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    eng.close()
    if not res["outputs_match"]:
        raise SystemExit("svc_loudness_match differs from audio.loudness_match")


if __name__ == "__main__":
    main()
