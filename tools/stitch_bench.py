"""The long-form join (svc_stitch) alone, at the default plan (10 s chunks, 0.64 s context, xfade 1024, search 192), for
one 180 s song and for 32 songs of 60 s:

  - HIP-event time per call, warm, median of `reps` (>= 20) calls, rotating over enough distinct inputs that every
    call reads its rows from HBM;
  - the two launches alone (the library's own events around each, same rotation), and the time per seam: stitch_seams
    over the seams of one song (a song's seams are serial, songs run side by side);
  - svc_pcm16 on the stitched songs' sample count, in the same run, as the yardstick for a streaming pass of this size;
  - an empty event pair and the GPU's clocks right behind the timed calls;
  - song 0 of each shape against audio.stitch on the host (displacements equal, every sample within 1 f32 ulp).

Prints one JSON line and writes it to profiles/stitch_bench.json (or the path given).
Usage: python tools/stitch_bench.py [reps] [out.json]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from load_bench import clocks  # noqa: E402
from loudness_bench import event_ms, kernel_ms, ulps  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

SHAPES = ((1, 180.0), (32, 60.0))
N_ROT = 8  # distinct inputs: 8 x (rows + out) of 36 / 400 MB between two reads of the same buffer


def bench_shape(eng, cfg, songs, seconds, reps):
    fs, hop = int(cfg.fs), int(cfg.hop_length)
    plan = A.chunk_plan(int(round(seconds * fs)), fs, hop, cfg.n_fft)
    st = A.merge_stitch_plans([plan.stitch] * songs, plan.stitch.out_len)
    B, S = songs * plan.chunks, max(plan.frames) * hop
    g = torch.Generator().manual_seed(songs)
    base = (torch.randn(B, S, generator=g) * 0.2).cuda()  # a vocoder output: one padded batch, a chunk per row
    bufs = [base] + [(base * (1.0 - 0.01 * k)).contiguous() for k in range(1, N_ROT)]
    rows = [[buf[b, :plan.frames[b % plan.chunks] * hop] for b in range(B)] for buf in bufs]
    outs = [torch.zeros(songs, plan.stitch.out_len, device="cuda") for _ in range(N_ROT)]

    def stitch(i):
        eng.stitch(rows[i], st, out=outs[i])

    def pcm(i):
        eng.pcm16(outs[i])

    seams = plan.chunks - 1
    res = {"songs": songs, "seconds": seconds, "chunks_per_song": plan.chunks, "seams_per_song": seams, "B": B,
           "xfade": st.xfade, "search": st.search, "out_samples": songs * plan.stitch.out_len,
           "algorithmic_bytes": songs * plan.stitch.out_len * 8}  # every body sample read once and written once
    rot = max(reps, 4 * N_ROT)
    res["svc_stitch_ms_rotating_median"], res["svc_stitch_ms_rotating_min"] = event_ms(stitch, N_ROT, rot)
    res["svc_pcm16_ms_rotating_median"], res["svc_pcm16_ms_rotating_min"] = event_ms(pcm, N_ROT, rot)
    res["clocks"] = clocks()  # right behind the timed calls
    res["kernel_ms_rotating_mean"], res["launches_per_call"] = kernel_ms("stitch", stitch, N_ROT, rot)
    res["pcm16_kernel_ms_rotating_mean"], _ = kernel_ms("pcm16", pcm, N_ROT, rot)
    res["us_per_seam"] = round(1e3 * res["kernel_ms_rotating_mean"]["stitch_seams"] / max(seams, 1), 3)
    res["stitch_write_bytes_per_s"] = round(res["algorithmic_bytes"]
                                            / (res["kernel_ms_rotating_mean"]["stitch_write"] * 1e-3), 0)
    res["ratio_to_svc_pcm16_rotating"] = round(res["svc_stitch_ms_rotating_median"]
                                               / res["svc_pcm16_ms_rotating_median"], 3)
    host_rows = [r.cpu().numpy() for r in rows[0][:plan.chunks]]
    want, shifts = A.stitch(host_rows, plan.stitch, return_shifts=True)
    _, got_shifts = eng.stitch(rows[0], st, out=outs[0], return_shifts=True)
    res["song0_shifts"] = got_shifts[:plan.chunks].cpu().tolist()
    res["song0_shifts_match_host"] = res["song0_shifts"] == shifts.tolist()
    res["song0_max_ulp_vs_host"] = ulps(outs[0][0].cpu().numpy(), want)
    return res


def main():
    reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 40
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "stitch_bench.json")
    cfg = C.load_config()
    eng = SVCEngine(cfg, 0)
    empty = event_ms(lambda i: None, 1, reps)
    res = {"tool": "stitch_bench", "fs": int(cfg.fs), "reps": reps, "event_pair_empty_ms_median": empty[0],
           "shapes": [bench_shape(eng, cfg, n, s, reps) for n, s in SHAPES], "torch_threads": torch.get_num_threads()}
    res["outputs_match"] = all(s["song0_shifts_match_host"] and s["song0_max_ulp_vs_host"] <= 1 for s in res["shapes"])
    line = json.dumps(res)
    print(line, flush=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    eng.close()
    if not res["outputs_match"]:
        raise SystemExit("svc_stitch differs from audio.stitch")


if __name__ == "__main__":
    main()
