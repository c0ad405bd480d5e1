"""Index compaction (svc_index_assign / svc_index_update / svc_index_kmeans) at D = 1024, K = 8,192 centroids, for
N = 65,536 and 262,144 content frames (about 12 and 47 minutes of recordings).

Per shape, in one process and one run:
  - HIP-event time of one assignment and of one update, median and min of `reps` calls after a warm-up that covers the
    workspace's first growth;
  - their kernels alone (the library's own events around each launch, a separate pass: profiling adds events), and
    2 N K D / (knn_topk's time) in TFLOP/s beside the 553 TFLOP/s recorded for retrieval against a 16,384-row index;
  - the ratio update / assign (the bar: under 0.10);
  - the torch composition of the same iteration: f16 matmul over row chunks + argmin, then index_add_ in f32 and a
    division (its sums are f32 in arrival order: not the exact mean);
  - svc_index_kmeans with 10 iterations: its time, and the final inertia against thinning's (inertia[0]: the same rows
    assigned to the strided sample, iters = 0) on the same rows;
  - at N = 65,536: svc_content_retrieve for the headline batch (32 x 937 rows) against the compacted 8,192-row index
    and against the 65,536-row original.
The rows are 4,096 Gaussian clusters (sigma 0.5 around unit-normal centres) visited in runs of 64 consecutive frames, as
held notes fill a recording: a strided sample then spends rows in proportion to duration.

Every shape runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing
more is started. Prints one JSON line and writes it to profiles/kmeans_bench.json (or the path given).
Usage: python tools/kmeans_bench.py [reps] [out.json]"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from retrieve_bench import event_ms  # noqa: E402

SHAPES = (65536, 262144)
D, K, ITERS = 1024, 8192, 10
KNN_TOPK_RECORDED_TFLOPS = 553.0  # profiles/retrieve_bench.json, 16,384-row index
CHUNK_BYTES = 1 << 30
STEP_LIMIT_S = 300


def make_rows(N, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(4096, D, generator=g)
    w = torch.ones(4096)
    w[::4] = 4.0  # the cluster sizes are uneven: a quarter of the clusters are drawn four times as often
    which = torch.multinomial(w, N // 64, replacement=True, generator=g).repeat_interleave(64)
    return (centres[which] + 0.5 * torch.randn(N, D, generator=g)).half().cuda()


def bench_shape(N, reps):
    import torch

    from load_bench import clocks
    from svc_inference_pipeline_amd import _lib
    from svc_inference_pipeline_amd import config as C
    from svc_inference_pipeline_amd.runtime import SVCEngine
    eng = SVCEngine(C.load_config(), 0)
    x = make_rows(N, N)
    res = {"N": N, "D": D, "K": K, "flops_assign": 2.0 * N * K * D, "reps": reps}
    cent, norms, counts, inertia, labels = eng.index_kmeans(x, K, 2, return_labels=True)  # a state mid-iteration
    out = torch.empty_like(cent)

    def assign():
        eng.index_assign(x, cent, norms, return_inertia=True)

    def update():
        eng.index_update(x, labels, cent, out=out)

    res["assign_ms_median"], res["assign_ms_min"] = event_ms(assign, reps)
    res["update_ms_median"], res["update_ms_min"] = event_ms(update, reps)
    res["update_over_assign"] = round(res["update_ms_median"] / res["assign_ms_median"], 4)
    res["cluster_rows_max"], res["clusters_empty"] = int(counts.max()), int((counts == 0).sum())

    rows = max(1, min(N, CHUNK_BYTES // (K * 2)))
    ct = cent.t().contiguous()
    nh = norms.half()
    tl = torch.empty(N, dtype=torch.int64, device="cuda")

    def torch_iteration():
        for r0 in range(0, N, rows):
            tl[r0:r0 + rows] = torch.argmin(torch.matmul(x[r0:r0 + rows], ct).mul_(-2.0).add_(nh), dim=1)
        sums = torch.zeros(K, D, dtype=torch.float32, device="cuda").index_add_(0, tl, x.float())
        cnt = torch.bincount(tl, minlength=K).clamp_min_(1)
        return (sums / cnt[:, None]).half()

    def torch_update():
        sums = torch.zeros(K, D, dtype=torch.float32, device="cuda").index_add_(0, tl, x.float())
        return (sums / torch.bincount(tl, minlength=K).clamp_min_(1)[:, None]).half()

    res["torch_iteration_ms_median"], res["torch_iteration_ms_min"] = event_ms(torch_iteration, reps)
    res["torch_update_ms_median"], res["torch_update_ms_min"] = event_ms(torch_update, reps)
    res["iteration_over_torch"] = round((res["assign_ms_median"] + res["update_ms_median"])
                                        / res["torch_iteration_ms_median"], 3)
    res["labels_equal_to_torch_f16_argmin"] = round(float((tl == labels.long()).float().mean()), 4)  # information only
    res["clocks"] = clocks()

    _lib.profile_filter("")
    _lib.profile_enable(True)
    try:
        for _ in range(reps):
            assign()
            update()
        torch.cuda.synchronize()
        stats = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    res["kernel_ms_mean"] = {k.split("@")[0]: round(v["ms"] / v["launches"], 4) for k, v in sorted(stats.items())}
    knn = res["kernel_ms_mean"].get("knn_topk")
    if knn:
        res["knn_topk_tflops"] = round(res["flops_assign"] / (knn * 1e-3) / 1e12, 1)
        res["knn_topk_over_recorded"] = round(res["knn_topk_tflops"] / KNN_TOPK_RECORDED_TFLOPS, 3)

    def kmeans():
        return eng.index_kmeans(x, K, ITERS)

    res["kmeans_iters"] = ITERS
    res["kmeans_ms_median"], res["kmeans_ms_min"] = event_ms(kmeans, max(3, reps // 4), warm=1)
    cent10, norms10, counts10, inertia10 = kmeans()
    ine = inertia10.tolist()
    res["inertia_thinning"], res["inertia_kmeans"] = ine[0], ine[-1]
    res["inertia_per_iteration"] = [round(v, 1) for v in ine]
    res["inertia_ratio"] = round(ine[-1] / ine[0], 4)
    res["centroids_empty"] = int((counts10 == 0).sum())

    if N == 65536:  # retrieval for the headline batch against the compacted index and against the original
        B, T = 32, 937
        g = torch.Generator().manual_seed(1)
        pick = torch.randint(0, N, (B * T,), generator=g).cuda()
        q = (0.7 * x[pick].float() + 0.5 * torch.randn(B * T, D, generator=g).cuda()).half().view(B, T, D)
        qo = torch.empty_like(q)
        live = counts10 > 0
        small, small_n = cent10[live].contiguous(), norms10[live].contiguous()
        full_n = eng.index_norms(x)
        res["retrieve_rows_compacted"] = int(small.shape[0])
        res["retrieve_ms_compacted"], _ = event_ms(lambda: eng.content_retrieve(q, small, small_n, rate=0.5, out=qo), reps)
        res["retrieve_ms_original"], _ = event_ms(lambda: eng.content_retrieve(q, x, full_n, rate=0.5, out=qo), reps)
    res["workspace_bytes"] = eng.memory()[1]
    eng.close()
    return res


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--shape":
        print("RESULT " + json.dumps(bench_shape(SHAPES[int(sys.argv[2])], int(sys.argv[3]))), flush=True)
        return
    reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 12
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "kmeans_bench.json")
    shapes = []
    for i in range(len(SHAPES)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(i), str(reps)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"kmeans_bench: N = {SHAPES[i]} ran past {STEP_LIMIT_S} s; nothing more is started")
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"kmeans_bench: N = {SHAPES[i]} failed (exit {p.returncode}); nothing more is started")
        shapes.append(json.loads(line[7:]))
    res = {"tool": "kmeans_bench", "reps": reps, "knn_topk_recorded_tflops": KNN_TOPK_RECORDED_TFLOPS, "shapes": shapes,
           "update_under_a_tenth_of_assign": all(s["update_over_assign"] < 0.10 for s in shapes)}
    line = json.dumps(res)
    print(line, flush=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
