"""bench.py's command line on the CPU: --dump-outputs (what it writes, its size cap, its fixed sample) and the result
line's ms_per_step / steps in --dry-run mode."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_arrays(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    arrays = {"wav": rng.standard_normal((3, 50)).astype(np.float16), "f0": rng.standard_normal((3, 7)),
              "ids": np.arange(5, dtype=np.int32)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["f0.npy", "ids.npy", "wav.npy"]
    wav, f0, ids = (np.load(tmp_path / "d" / f"{k}.npy") for k in ("wav", "f0", "ids"))
    assert wav.dtype == np.float32 and np.array_equal(wav, arrays["wav"].astype(np.float32))
    assert f0.dtype == np.float64 and np.array_equal(f0, arrays["f0"])
    assert ids.dtype == np.float32 and np.array_equal(ids, arrays["ids"])


def test_dump_outputs_over_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    a = np.arange(3000, dtype=np.float32).reshape(30, 100)  # 12 000 bytes
    b = np.arange(500, dtype=np.float64) * 0.5              # 4 000 bytes
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    got = {k: np.load(tmp_path / "one" / f"{k}.npy") for k in ("a", "b")}
    assert got["a"].nbytes + got["b"].nbytes <= 4000
    assert got["a"].shape == (750,) and got["b"].shape == (125,)  # each array's proportional share
    for k, src in (("a", a), ("b", b)):
        assert got[k].dtype == src.dtype and np.isin(got[k], src).all() and (np.diff(got[k]) >= 0).all()
        assert np.array_equal(got[k], np.load(tmp_path / "two" / f"{k}.npy"))  # the same elements in every run


def test_bench_default_dump_budget():
    import bench
    assert bench.DUMP_BUDGET_BYTES <= 64 * 10 ** 6


def test_bench_dry_run_dump_outputs_and_ms_per_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["CUDA_VISIBLE_DEVICES"] = ""
    dump, outdir = str(tmp_path / "w.npy"), str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--dry-run", "--batch", "2",
                        "--seconds", "0.25", "--steps", "2", "--warmup", "0", "--dump", dump, "--dump-outputs", outdir],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["ms_per_step"] >= 0
    assert abs(line["ms_per_step"] - 1000.0 * line["elapsed_s"] / 2) <= 0.1
    wav = np.load(os.path.join(outdir, "wav.npy"))
    assert os.listdir(outdir) == ["wav.npy"] and wav.dtype == np.float32
    assert np.array_equal(wav, np.load(dump))


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--dry-run", "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
