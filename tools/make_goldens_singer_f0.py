"""tests/golden/target_f0_contours.npz: the leading contours of the reference's config/f0.pkl, the recorded target
F0 its pitch shift takes the median of (utils/acoustic_feature_extraction.py:21-30), with numpy's medians of their
voiced frames, for svc_f0_voiced_median (tests/test_gpu_singer_f0.py).

The pickle is read with tools/extract_config_stats.payloads, which walks the opcode stream and never unpickles.

  f0         f64 [65437]  the leading 321 contours, concatenated
  lengths    int32 [321]  their frame counts
  median_321 / voiced_321  np.median of the voiced (nonzero) frames of all 321 and their count (44,844: even)
  median_320 / voiced_320  the same for the leading 320 (44,671: odd)

The four numbers, and the whole file's median (config/stats.json's target_f0_median over 173,401 voiced frames of
223,087 in 656 contours, which is not stored), are asserted here against the values first computed for the fixture.

Run once where the reference is:  python tools/make_goldens_singer_f0.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extract_config_stats import REF, payloads  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CONTOURS = 321
EXPECT = dict(frames=65437, median_321=174.73750413040062, voiced_321=44844, median_320=174.49461696631786,
              voiced_320=44671, median_all=223.25784012425046, voiced_all=173401, frames_all=223087, n_all=656)


def voiced_median(contours):
    x = np.concatenate(contours)
    v = x[x != 0]
    return float(np.median(v)), int(v.size)


def main():
    f0s = [np.asarray(a, np.float64) for a in payloads(os.path.join(REF, "config/f0.pkl"))]
    lead = f0s[:N_CONTOURS]
    flat = np.concatenate(lead)
    m321, v321 = voiced_median(lead)
    m320, v320 = voiced_median(lead[:N_CONTOURS - 1])
    mall, vall = voiced_median(f0s)
    got = dict(frames=int(flat.size), median_321=m321, voiced_321=v321, median_320=m320, voiced_320=v320,
               median_all=mall, voiced_all=vall, frames_all=int(sum(a.size for a in f0s)), n_all=len(f0s))
    assert got == EXPECT, (got, EXPECT)
    assert not np.isnan(flat).any()
    stats = json.load(open(os.path.join(REPO, "svc_inference_pipeline_amd", "config", "stats.json")))
    assert stats["target_f0_median"] == mall and stats["target_f0_voiced_count"] == vall
    dst = os.path.join(REPO, "tests", "golden", "target_f0_contours.npz")
    np.savez_compressed(dst, f0=flat, lengths=np.array([a.size for a in lead], np.int32),
                        median_321=np.float64(m321), voiced_321=np.int64(v321), median_320=np.float64(m320),
                        voiced_320=np.int64(v320))
    print(got, "->", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    sys.exit(main())
