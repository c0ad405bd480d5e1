"""Ramp / steady / drain split of one res_proj launch from its in-kernel stamps (res_proj.hip, DBG instance).
Usage (GPU): python tools/res_proj_stamps.py [M]            (environment: SVC_BENCH_RP_LANES, default -2)
Runs svc_gemm_bench variant 30 cold (every launch after a 1 GiB memset) with SVC_RP_STAMPS, then prints per-workgroup
s_memtime differences in shader cycles (median / max over the workgroups that ran a tile) and the launch's cold time.
Only differences inside one workgroup are formed (the workgroups' counters are not comparable: r07a)."""
import ctypes
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SVC_BENCH_RP_LANES", "-2")
path = os.path.join(tempfile.mkdtemp(), "stamps.bin")
os.environ["SVC_RP_STAMPS"] = path
from svc_inference_pipeline_amd import _lib  # noqa: E402


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 29984
    import torch
    torch.cuda.init()
    ms = ctypes.c_double()
    _lib.call("svc_gemm_bench", M, 384, 384, 1, 6, 30, -30, ctypes.byref(ms))
    print(f"M {M}: cold launch {ms.value * 1000:.2f} us (HIP events, mean of 30)")
    s = np.fromfile(path, dtype=np.uint64).reshape(-1, 8).astype(np.int64)
    live = s[:, 0] != 0
    s = s[live]
    wg = np.nonzero(live)[0]
    print(f"{len(s)} workgroups stamped")
    d = lambda a, b: s[:, a] - s[:, b]
    rows = [("entry -> W landed", d(1, 0)), ("entry -> tile 0 landed (ramp)", d(2, 0)),
            ("tile 0 landed -> last stores issued (steady)", d(3, 2)), ("last stores issued -> exit (drain)", d(4, 3)),
            ("entry -> exit", d(4, 0))]
    if (s[:, 5] != 0).any():  # the loader form's extra stamps
        rows[1:1] = [("entry -> W landed, last compute wave", d(7, 0)), ("entry -> first loader's tile 0 pieces", d(5, 0)),
                     ("entry -> second loader's tile 0 pieces", d(6, 0))]
    for name, v in rows:
        print(f"  {name:46s} median {int(np.median(v)):7d}  min {int(v.min()):7d}  max {int(v.max()):7d} cycles")


if __name__ == "__main__":
    main()
