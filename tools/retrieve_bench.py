"""Feature retrieval (svc_content_retrieve) alone against what library calls would do, at the headline batch's content
shape (32 x 937 rows of D = 1024, k = 8) against indexes of 16,384, 65,536 and 262,144 rows, and for one clip of 937
rows against 65,536 (the small-M case the index splits exist for).

Per shape, in one process and one run:
  - HIP-event time of the fused call, median and min of `reps` calls after a warm-up that covers the workspace's first
    growth and the staging ring's slots;
  - its two kernels alone (the library's own events around each launch, a separate pass: profiling adds events);
  - 2 M N D / (knn_topk's time) as a fraction of the fp16 dense peak (2516.6 TFLOP/s, MI355X_MICROARCH's spec figure);
  - (a) the f16 torch.matmul of the same product alone, over row chunks that keep the score block under 2 GiB;
  - (b) the full library composition per chunk: matmul, norms - 2 dot, torch.topk, gather, weights, blend;
  - the clocks right behind the timed calls, and how often (b)'s nearest neighbour is the fused call's (its f16 scores
    are coarser, so this is information, not a check: the GPU tests are the check).
The gate: the fused call is faster than (b) at every shape; the ratio to (a) is recorded and not gated.

Every shape runs in a child process of its own under a time limit; after a child that fails or runs out of time
nothing more is started. Prints one JSON line and writes it to profiles/retrieve_bench.json (or the path given).
Usage: python tools/retrieve_bench.py [reps] [out.json]"""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

SHAPES = ((32, 937, 16384), (32, 937, 65536), (32, 937, 262144), (1, 937, 65536))
D, K, RATE = 1024, 8, 0.5
PEAK_FP16 = 2516.6e12
CHUNK_BYTES = 2 << 30
STEP_LIMIT_S = 240
HEADLINE_STEP_MS = 334.0  # the headline step of the last recorded benchmark round (r06fin5)


def event_ms(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return round(statistics.median(ms), 4), round(min(ms), 4)


def bench_shape(B, T, N, reps):
    import torch

    from load_bench import clocks
    from svc_inference_pipeline_amd import _lib
    from svc_inference_pipeline_amd import config as C
    from svc_inference_pipeline_amd.runtime import SVCEngine
    eng = SVCEngine(C.load_config(), 0)
    g = torch.Generator().manual_seed(N + B)
    x = torch.randn(N, D, generator=g).half().cuda()
    pick = torch.randint(0, N, (B * T,), generator=g)
    q = (0.7 * x[pick.cuda()].float() + 0.5 * torch.randn(B * T, D, generator=g).cuda()).half().view(B, T, D)
    norms = eng.index_norms(x)
    out = torch.empty_like(q)
    M = B * T
    floor = 1e-4 * D
    res = {"B": B, "T": T, "M": M, "N": N, "D": D, "k": K, "flops": 2.0 * M * N * D}

    def fused():
        eng.content_retrieve(q, x, norms, k=K, rate=RATE, out=out)

    rows = max(1, min(M, CHUNK_BYTES // (N * 2)))
    q2 = q.view(M, D)
    xt = x.t()
    nf = norms.half()

    def matmul_only():
        for r0 in range(0, M, rows):
            torch.matmul(q2[r0:r0 + rows], xt)

    comp_out = torch.empty(M, D, dtype=torch.float16, device="cuda")
    comp_idx = torch.empty(M, K, dtype=torch.int64, device="cuda")

    def composed():
        for r0 in range(0, M, rows):
            qc = q2[r0:r0 + rows]
            s = torch.matmul(qc, xt).mul_(-2.0).add_(nf)
            sv, si = torch.topk(s, K, dim=1, largest=False)
            d2 = (qc.float().square().sum(1, keepdim=True) + sv.float()).clamp_min_(floor)
            w = 1.0 / d2
            w = w / w.sum(1, keepdim=True)
            y = torch.bmm(w.unsqueeze(1), x[si].float()).squeeze(1)
            comp_out[r0:r0 + rows] = (RATE * y + (1.0 - RATE) * qc.float()).half()
            comp_idx[r0:r0 + rows] = si

    n = max(5, reps if N <= 65536 else reps // 4)
    res["reps"] = n
    res["fused_ms_median"], res["fused_ms_min"] = event_ms(fused, n)
    res["matmul_ms_median"], res["matmul_ms_min"] = event_ms(matmul_only, n)
    res["composed_ms_median"], res["composed_ms_min"] = event_ms(composed, n)
    res["fused_ms_median_again"], _ = event_ms(fused, n)  # the spread of the same call in the same process
    res["clocks"] = clocks()
    _lib.profile_filter("")
    _lib.profile_enable(True)
    try:
        for _ in range(n):
            fused()
        torch.cuda.synchronize()
        stats = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    res["kernel_ms_mean"] = {k_.split("@")[0]: round(v["ms"] / v["launches"], 4) for k_, v in stats.items()
                             if k_.startswith(("knn_topk", "retrieve_blend"))}
    # the grid svc_content_retrieve chooses at tune.retrieve_splits = 0 (csrc/retrieve.hip retrieve_splits)
    qtiles, tiles = -(-M // 128), -(-N // 128)
    res["query_tiles"], res["index_splits"] = qtiles, max(1, min(-(-768 // qtiles), tiles, 64))
    knn = res["kernel_ms_mean"].get("knn_topk")
    if knn:
        res["knn_topk_tflops"] = round(res["flops"] / (knn * 1e-3) / 1e12, 1)
        res["knn_topk_fraction_of_fp16_peak"] = round(res["flops"] / (knn * 1e-3) / PEAK_FP16, 4)
    res["fused_over_matmul"] = round(res["fused_ms_median"] / res["matmul_ms_median"], 3)
    res["fused_over_composed"] = round(res["fused_ms_median"] / res["composed_ms_median"], 3)
    res["share_of_headline_step"] = round(res["fused_ms_median"] / HEADLINE_STEP_MS, 4) if (B, N) == (32, 65536) else None
    _, idx, _ = eng.content_retrieve(q, x, norms, k=K, rate=RATE, out=out, return_neighbours=True)
    composed()
    torch.cuda.synchronize()
    res["top1_agreement_with_composed"] = round(float((idx.view(M, K)[:, 0] == comp_idx[:, 0]).float().mean()), 4)
    res["workspace_bytes"] = eng.memory()[1]
    eng.close()
    return res


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--shape":
        B, T, N = SHAPES[int(sys.argv[2])]
        print("RESULT " + json.dumps(bench_shape(B, T, N, int(sys.argv[3]))), flush=True)
        return
    reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "retrieve_bench.json")
    shapes = []
    for i in range(len(SHAPES)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(i), str(reps)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"retrieve_bench: shape {SHAPES[i]} ran past {STEP_LIMIT_S} s; nothing more is started")
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"retrieve_bench: shape {SHAPES[i]} failed (exit {p.returncode}); nothing more is started")
        shapes.append(json.loads(line[7:]))
    res = {"tool": "retrieve_bench", "reps": reps, "peak_fp16_dense_tflops": PEAK_FP16 / 1e12,
           "headline_step_ms": HEADLINE_STEP_MS, "shapes": shapes,
           "fused_faster_than_composed": all(s["fused_ms_median"] < s["composed_ms_median"] for s in shapes)}
    line = json.dumps(res)
    print(line, flush=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not res["fused_faster_than_composed"]:
        raise SystemExit("retrieve_bench: the fused call is not faster than the library composition at every shape")


if __name__ == "__main__":
    main()
