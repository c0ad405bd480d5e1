"""Long-form conversion end to end: the 180 s song of BASELINE configs[3] (Whisper-medium content, PLMS speedup 10, seeded
weights) converted in chunks (SVCPipeline.convert_long at its defaults) against the same song as one utterance
(convert_ragged), on the same box in the same run:

  - audio-s/s of each (wall clock around `steps` synchronised conversions after `warmup` ones);
  - peak device memory of each: the context's workspace arena (svc_ctx_memory: exactly what the largest stage call so
    far needed) plus torch's peak allocation (inputs, activations handed between stages, outputs). The chunked run goes
    FIRST, in a context of its own, so neither arena has grown for the other;
  - the chunked run's overhead in frames: the sum of the chunks' frames over T_song;
  - the per-launch times of stitch_seams and stitch_write inside the chunked conversion.

Prints one JSON line and writes it to profiles/long_chunks_bench.json (or the path given).
Usage: python tools/long_bench.py [steps] [warmup] [out.json]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from load_bench import clocks  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402
from svc_inference_pipeline_amd.synth import synth_clip, synth_clip_16k_quantised  # noqa: E402

SECONDS = 180.0
KW = dict(fast_inference=True, speedup=10, seed=1234)


def measure(states, run, steps, warmup):
    """A fresh context, warmup + steps synchronised calls of run(pipe) -> figures, and the last result."""
    cfg, ws, ms, vs = states
    eng = SVCEngine(cfg, 0, whisper_state=ws, mapper_state=ms, vocoder_state=vs)
    pipe = SVCPipeline(eng)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = None
    for _ in range(warmup):
        out = run(pipe)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = run(pipe)
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    weights, workspace = eng.memory()
    res = {"s_per_song": round(dt, 4), "audio_s_per_s": round(SECONDS / dt, 1), "workspace_bytes": int(workspace),
           "torch_peak_bytes": int(torch.cuda.max_memory_allocated() - base), "weight_bytes": int(weights)}
    res["peak_bytes"] = res["workspace_bytes"] + res["torch_peak_bytes"]
    return res, out, eng, pipe


def main():
    steps = max(1, int(sys.argv[1])) if len(sys.argv) > 1 else 3
    warmup = max(1, int(sys.argv[2])) if len(sys.argv) > 2 else 2
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "long_chunks_bench.json")
    cfg = C.load_config()
    states = (cfg, W.make_whisper_state(W.WHISPER_DIMS["medium"], seed=0), W.make_mapper_state(cfg.mapper, seed=0),
              W.make_vocoder_state(cfg.vocoder, seed=0))
    w24 = [torch.from_numpy(synth_clip(0, SECONDS, 24000)).cuda()]
    w16 = [torch.from_numpy(synth_clip_16k_quantised(0, SECONDS)).cuda()]

    chunked, (wavs, info), eng, pipe = measure(
        states, lambda p: p.convert_long(w24, w16, [1], utt_ids=[0], return_chunks=True, **KW), steps, warmup)
    plan = info.plans[0]
    chunked.update(chunks=plan.chunks, T_song=plan.T_song, chunk_frames=sum(plan.frames),
                   frame_overhead=round(sum(plan.frames) / plan.T_song, 4), shifts=info.shifts[0].cpu().tolist(),
                   finite=bool(torch.isfinite(wavs[0]).all()))
    _lib.profile_filter("stitch")
    _lib.profile_enable(True)
    try:
        pipe.convert_long(w24, w16, [1], utt_ids=[0], **KW)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
        _lib.profile_filter("")
    chunked["stitch_kernel_ms"] = {k.split("@")[0]: round(v["ms"] / v["launches"], 5) for k, v in prof.items()}
    chunked["clocks"] = clocks()
    del wavs, info, pipe
    eng.close()
    torch.cuda.empty_cache()

    whole, out, eng, _ = measure(states, lambda p: p.convert_ragged(w24, w16, [1], utt_ids=[0], **KW), steps, warmup)
    whole["finite"] = bool(torch.isfinite(out[0]).all())
    whole["clocks"] = clocks()
    eng.close()

    res = {"tool": "long_bench", "seconds": SECONDS, "steps": steps, "warmup": warmup, "sampler": "plms speedup 10",
           "content": "whisper-medium (seeded weights)", "convert_long": chunked, "convert_ragged": whole,
           "throughput_ratio_chunked_over_whole": round(chunked["audio_s_per_s"] / whole["audio_s_per_s"], 4),
           "peak_bytes_ratio_chunked_over_whole": round(chunked["peak_bytes"] / whole["peak_bytes"], 4),
           "torch_threads": torch.get_num_threads()}
    line = json.dumps(res)
    print(line, flush=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
