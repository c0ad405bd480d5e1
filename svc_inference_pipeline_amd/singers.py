"""Per-singer F0 targets (A4, utils/acoustic_feature_extraction.py:21-52).

The reference shifts a source clip's voiced F0 median onto the target singer's voiced F0 median, which it takes from
that singer's recorded contours. SingerF0Table holds that median per singer id, as SVCPipeline.enroll measures it on
the GPU (svc_f0_voiced_median) from the singer's own recordings; a singer without an entry keeps the global
`target_f0_median` of config/stats.json.
"""
import json


class SingerF0Table:
    """singer id (int) -> {"median": float (Hz), "voiced": int, "frames": int, "n_utts": int}."""

    def __init__(self, entries=None):
        self._e = {}
        for k, v in (entries or {}).items():
            self.set(k, **v)

    def set(self, singer, median, voiced=0, frames=0, n_utts=0):
        median = float(median)
        if not (median > 0.0 and median != float("inf")):
            raise ValueError(f"singer {singer}: F0 median {median!r} (must be finite and positive)")
        self._e[int(singer)] = dict(median=median, voiced=int(voiced), frames=int(frames), n_utts=int(n_utts))
        return self._e[int(singer)]

    def get(self, singer, default=None):
        """The singer's median in Hz, or `default` for a singer that was never enrolled."""
        e = self._e.get(int(singer))
        return default if e is None else e["median"]

    def entry(self, singer):
        return self._e.get(int(singer))

    def __len__(self):
        return len(self._e)

    def __bool__(self):
        return bool(self._e)

    def __contains__(self, singer):
        return int(singer) in self._e

    def __iter__(self):
        return iter(sorted(self._e))

    def __eq__(self, other):
        return isinstance(other, SingerF0Table) and self._e == other._e

    def save(self, path):
        """JSON; a median is written as float.hex (with its repr beside it for the reader), so it round-trips exactly."""
        doc = {"singer_f0": {str(k): dict(median=float(v["median"]).hex(), median_hz=repr(v["median"]),
                                          voiced=v["voiced"], frames=v["frames"], n_utts=v["n_utts"])
                             for k, v in sorted(self._e.items())}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    @classmethod
    def load(cls, path):
        with open(path) as f:
            doc = json.load(f)
        t = cls()
        for k, v in doc["singer_f0"].items():
            m = v["median"]
            t.set(int(k), float.fromhex(m) if isinstance(m, str) else float(m), v.get("voiced", 0), v.get("frames", 0),
                  v.get("n_utts", 0))
        return t
