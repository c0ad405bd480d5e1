"""save_audio's sample conversion on the GPU (svc_pcm16) for the headline batch shape (32 clips of 239,872 samples):

  - HIP-event time per call, warm, median of `reps` (>= 20) calls on one input (which then sits in the 256 MB
    Infinity Cache), and again rotating over enough distinct inputs that every call reads from HBM;
  - the fraction of HBM bandwidth that is against the algorithmic bytes (read wav twice, write pcm once);
  - end to end on this box: "device PCM + D2H of int16" against "D2H of f32 + audio.to_pcm16 per utterance" (what a
    caller did before), host clock around work that ends synchronised, median of 5; the two results are compared.

Prints one JSON line. Usage: python tools/pcm16_bench.py [reps]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

HBM_PEAK = 8.0e12       # bytes/s, MI355X specification
HBM_MEASURED = 6.29e12  # bytes/s, a float4 copy kernel on this GPU


def event_ms(fn, inputs, reps):
    """median / min HIP-event ms of fn(inputs[i % len]) over reps calls, after one warm pass over every input"""
    for x in inputs:
        fn(x)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(inputs[i % len(inputs)])
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms)


def host_ms(fn, n=5):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 50
    cfg = C.load_config()
    eng = SVCEngine(cfg, 0)
    B, S = 32, 239872
    g = torch.Generator().manual_seed(0)
    host = torch.randn(B, S, generator=g) * 0.2
    wav = host.cuda()
    L = S + 2 * (cfg.fs // 20)
    algo_bytes = B * S * 4 * 2 + B * L * 2
    # warm, one input
    warm_med, warm_min = event_ms(eng.pcm16, [wav], reps)
    # rotating inputs: 12 x 30.7 MB, so ~340 MB of other traffic passes between two reads of the same buffer
    rot = [wav] + [(wav * (1.0 - 0.01 * k)).contiguous() for k in range(1, 12)]
    rot_med, rot_min = event_ms(eng.pcm16, rot, max(reps, 48))
    # the two kernels alone (the library's own events around each launch), same rotation: a whole call also holds the
    # length table's copy and, when the host enqueues slower than the GPU drains, the gaps between its three commands
    _lib.profile_filter("pcm16")
    _lib.profile_enable(True)
    for i in range(48):
        eng.pcm16(rot[i % len(rot)])
    kern = {k: v["ms"] / v["launches"] for k, v in _lib.profile_read().items()}
    _lib.profile_enable(False)
    _lib.profile_filter("")
    kern_ms = kern["pcm16_peak"] + kern["pcm16_quant"]
    del rot

    # both paths copy into a pinned host buffer allocated once, as a service would (no allocator or page-fault time)
    pin16 = torch.empty(B, L, dtype=torch.int16).pin_memory()
    pin32 = torch.empty(B, S, dtype=torch.float32).pin_memory()

    def device_path():
        pin16.copy_(eng.pcm16(wav))
        return pin16.numpy()

    def host_path():
        pin32.copy_(wav)
        w = pin32.numpy()
        return [A.to_pcm16(w[b], cfg.fs) for b in range(B)]

    dev_pcm, ref_pcm = device_path(), host_path()
    match = all(np.array_equal(dev_pcm[b], ref_pcm[b]) for b in range(B))
    w_host = wav.cpu().numpy()
    res = {
        "tool": "pcm16_bench", "B": B, "S": S, "pcm_len": L, "reps": reps, "algorithmic_bytes": algo_bytes,
        "svc_pcm16_ms_warm_median": round(warm_med, 5), "svc_pcm16_ms_warm_min": round(warm_min, 5),
        "svc_pcm16_ms_rotating_median": round(rot_med, 5), "svc_pcm16_ms_rotating_min": round(rot_min, 5),
        "kernel_ms_rotating_mean": {k: round(v, 5) for k, v in sorted(kern.items())},
        "call_bytes_per_s_rotating": round(algo_bytes / (rot_med * 1e-3), 0),
        "call_fraction_of_hbm_peak_8TBs": round(algo_bytes / (rot_med * 1e-3) / HBM_PEAK, 4),
        "kernels_bytes_per_s_rotating": round(algo_bytes / (kern_ms * 1e-3), 0),
        "kernels_fraction_of_hbm_peak_8TBs": round(algo_bytes / (kern_ms * 1e-3) / HBM_PEAK, 4),
        "kernels_fraction_of_measured_copy_6.29TBs": round(algo_bytes / (kern_ms * 1e-3) / HBM_MEASURED, 4),
        "e2e_device_pcm_plus_d2h_int16_ms": round(host_ms(device_path), 3),
        "e2e_d2h_f32_plus_to_pcm16_loop_ms": round(host_ms(host_path), 3),
        "host_to_pcm16_loop_only_ms": round(host_ms(lambda: [A.to_pcm16(w_host[b], cfg.fs) for b in range(B)]), 3),
        "outputs_match": bool(match), "torch_threads": torch.get_num_threads(),
    }
    print(json.dumps(res), flush=True)
    eng.close()
    if not match:
        raise SystemExit("svc_pcm16 differs from audio.to_pcm16")


if __name__ == "__main__":
    main()
