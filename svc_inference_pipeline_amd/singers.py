"""Per-singer F0 targets (A4, utils/acoustic_feature_extraction.py:21-52).

The reference shifts a source clip's voiced F0 median onto the target singer's voiced F0 median, which it takes from
that singer's recorded contours. SingerF0Table holds that median per singer id, as SVCPipeline.enroll measures it on
the GPU (svc_f0_voiced_median) from the singer's own recordings; a singer without an entry keeps the global
`target_f0_median` of config/stats.json.
"""
import json

import numpy as np
import torch


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


def check_index_rate(index_rate):
    """Feature retrieval's blend rate as a float in [0, 1], else ValueError before any device work; None (the stage is
    not run) stays None."""
    if index_rate is None:
        return None
    ok = isinstance(index_rate, (int, float, np.integer, np.floating)) and not isinstance(index_rate, (bool, np.bool_))
    if not ok or not (0.0 <= float(index_rate) <= 1.0):
        raise ValueError(f"index_rate {index_rate!r}: a number in [0, 1] (None: no feature retrieval)")
    return float(index_rate)


INDEX_COMPACT = ("stride", "kmeans")


def check_index_compact(index_compact, index_iters=10):
    """enroll's index compaction mode and k-means iteration count -> (mode, iters), else ValueError before any device
    work: the mode is "stride" (keep rows floor(i N / M)) or "kmeans" (svc_index_kmeans' centroids); iters an int in
    [0, 1000] (svc_index_kmeans' range), checked in both modes."""
    if index_compact not in INDEX_COMPACT:
        raise ValueError(f"index_compact {index_compact!r}: one of {list(INDEX_COMPACT)}")
    ok = isinstance(index_iters, (int, np.integer)) and not isinstance(index_iters, (bool, np.bool_))
    if not ok or not 0 <= int(index_iters) <= 1000:
        raise ValueError(f"index_iters {index_iters!r}: an integer in [0, 1000]")
    return index_compact, int(index_iters)


def content_signature(cfg):
    """(D, content types) of the content buffer the configuration's conditioner reads: the types of
    cfg.mapper.content_feature in ascending name order and the sum of their widths (SVCPipeline.content)."""
    m = cfg.mapper
    types = sorted(m.content_feature)
    return sum(int(m.input_content_dim[t]) for t in types), types


class SingerIndexTable:
    """singer id (int) -> a retrieval index: {"rows": f16 [N, D] tensor of the singer's enrolled content frames,
    "norms": f32 [N] (svc_index_norms of the rows), "n_utts": int, "frames": int (content frames seen, before any
    thinning), "content_types": list of str the rows were built from}, and, only where k-means compacted the index
    (enroll(index_compact="kmeans") with more frames than index_max_rows), "compact": {"method": "kmeans", "iters":
    int, "inertia_first": float, "inertia_last": float, "dropped": int (centroids left without a row)}.
    SVCPipeline.enroll(index=True) fills it; svc_content_retrieve searches it (`index_rate=` on the conversion entry
    points)."""

    def __init__(self):
        self._e = {}

    def set(self, singer, rows, norms, n_utts=0, frames=0, content_types=(), compact=None):
        if rows.dim() != 2 or rows.dtype != torch.float16 or rows.shape[0] < 1:
            raise ValueError(f"singer {singer}: index rows must be f16 [N >= 1, D]")
        if norms.dtype != torch.float32 or norms.shape != (rows.shape[0],):
            raise ValueError(f"singer {singer}: norms must be f32 [{rows.shape[0]}]")
        self._e[int(singer)] = dict(rows=rows.contiguous(), norms=norms.contiguous(), n_utts=int(n_utts),
                                    frames=int(frames), content_types=[str(t) for t in content_types])
        if compact is not None:
            self._e[int(singer)]["compact"] = dict(
                method=str(compact["method"]), iters=int(compact["iters"]),
                inertia_first=float(compact["inertia_first"]), inertia_last=float(compact["inertia_last"]),
                dropped=int(compact["dropped"]))
        return self._e[int(singer)]

    def get(self, singer, default=None):
        return self._e.get(int(singer), default)

    def __len__(self):
        return len(self._e)

    def __bool__(self):
        return bool(self._e)

    def __contains__(self, singer):
        return int(singer) in self._e

    def __iter__(self):
        return iter(sorted(self._e))

    def save(self, path):
        """.npz: per singer the rows as uint16 bit patterns and the f32 norms, and one JSON document of the metadata."""
        arrays, meta = {}, {}
        for k, v in sorted(self._e.items()):
            arrays[f"rows_{k}"] = v["rows"].detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
            arrays[f"norms_{k}"] = v["norms"].detach().cpu().numpy()
            meta[str(k)] = dict(n_utts=v["n_utts"], frames=v["frames"], content_types=v["content_types"],
                                rows=int(v["rows"].shape[0]), dim=int(v["rows"].shape[1]))
            if "compact" in v:  # the inertias as float.hex, so they round-trip exactly
                meta[str(k)]["compact"] = dict(v["compact"], inertia_first=float(v["compact"]["inertia_first"]).hex(),
                                               inertia_last=float(v["compact"]["inertia_last"]).hex())
        with open(path, "wb") as f:
            np.savez(f, meta=np.array(json.dumps({"singer_index": meta})), **arrays)

    @classmethod
    def load(cls, path, device="cpu", dim=None, content_types=None):
        """dim / content_types (content_signature of the engine's configuration): an index whose row width or
        content types differ is a ValueError: its frames come from another content space."""
        t = cls()
        with np.load(path, allow_pickle=False) as doc:
            meta = json.loads(str(doc["meta"]))["singer_index"]
            for k, m in meta.items():
                rows = np.ascontiguousarray(doc[f"rows_{k}"])
                if rows.dtype != np.uint16 or rows.ndim != 2 or rows.shape != (m["rows"], m["dim"]):
                    raise ValueError(f"{path}: singer {k}: rows {rows.dtype} {rows.shape}, metadata says uint16 "
                                     f"[{m['rows']}, {m['dim']}]")
                if dim is not None and rows.shape[1] != int(dim):
                    raise ValueError(f"{path}: singer {k}: index rows are {rows.shape[1]} wide, the configuration's "
                                     f"content is {int(dim)}")
                if content_types is not None and list(m["content_types"]) != [str(c) for c in content_types]:
                    raise ValueError(f"{path}: singer {k}: index built from content types {m['content_types']}, the "
                                     f"configuration uses {list(content_types)}")
                t.set(int(k), torch.from_numpy(rows.view(np.int16)).view(torch.float16).to(device),
                      torch.from_numpy(np.ascontiguousarray(doc[f"norms_{k}"], np.float32)).to(device), m["n_utts"],
                      m["frames"], m["content_types"],
                      compact=None if "compact" not in m else dict(
                          m["compact"], inertia_first=float.fromhex(m["compact"]["inertia_first"]),
                          inertia_last=float.fromhex(m["compact"]["inertia_last"])))
        return t
