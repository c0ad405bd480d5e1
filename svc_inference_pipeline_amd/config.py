"""Configuration: a JSON5-subset reader + attribute-style hyper-parameter object.

Mirrors the reference's `load_config` / `JsonHParams` (utils/util.py:57-122). json5 is not
installed here, so `loads_json5` accepts exactly what the reference's config.json uses: `//` line
comments, `/* */` block comments and trailing commas. The `basic_config` inheritance through
`$WORD_DIR` (utils/util.py:68-77) is kept.

The package ships a condensed copy of the reference's config (svc_inference_pipeline_amd/config/):
the 1000-entry explicit `mapper.noise_schedule` list is omitted because DiffSVC overwrites it from
`noise_schedule_factors` (modules/diffsvc.py:248-252); `noise_schedule()` below derives it the same
way. Normalisation/F0 statistics come from config/stats.json (extracted from the reference pickles
without unpickling, tools/extract_config_stats.py).
"""
import json
import os
import re

import numpy as np

CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config")


def _strip_json5(text: str) -> str:
    out = []
    i, n = 0, len(text)
    in_str = None
    while i < n:
        c = text[i]
        if in_str:
            out.append(c)
            if c == "\\" and i + 1 < n:
                out.append(text[i + 1])
                i += 2
                continue
            if c == in_str:
                in_str = None
            i += 1
            continue
        if c in "\"'":
            in_str = c
            out.append('"')  # single-quoted JSON5 strings are normalised to double quotes
            i += 1
            continue
        if text.startswith("//", i):
            j = text.find("\n", i)
            i = n if j < 0 else j
            continue
        if text.startswith("/*", i):
            j = text.find("*/", i + 2)
            if j < 0:
                raise ValueError("unterminated block comment")
            i = j + 2
            continue
        out.append(c)
        i += 1
    s = "".join(out)
    return re.sub(r",(\s*[}\]])", r"\1", s)


def loads_json5(text: str):
    return json.loads(_strip_json5(text))


def override_config(basic_config, new_config):
    """utils/util.py:57-65."""
    for k, v in new_config.items():
        if isinstance(v, dict):
            basic_config[k] = override_config(basic_config.get(k, {}), v)
        else:
            basic_config[k] = v
    return basic_config


def _load_config(config_fn):
    """utils/util.py:68-78 (basic_config inheritance via $WORD_DIR)."""
    with open(config_fn, "r") as f:
        cfg = loads_json5(f.read())
    if "basic_config" in cfg:
        parent = os.path.join(os.getenv("WORD_DIR", ""), cfg["basic_config"])
        cfg = override_config(_load_config(parent), cfg)
    return cfg


class JsonHParams:
    """Attribute-style nested config (utils/util.py:92-122)."""

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            if isinstance(v, dict):
                v = JsonHParams(**v)
            self[k] = v

    def keys(self):
        return self.__dict__.keys()

    def items(self):
        return self.__dict__.items()

    def values(self):
        return self.__dict__.values()

    def __len__(self):
        return len(self.__dict__)

    def __getitem__(self, key):
        return getattr(self, key)

    def __setitem__(self, key, value):
        return setattr(self, key, value)

    def __contains__(self, key):
        return key in self.__dict__

    def __repr__(self):
        return self.__dict__.__repr__()

    def to_dict(self):
        return {k: (v.to_dict() if isinstance(v, JsonHParams) else v) for k, v in self.items()}


def load_config(config_fn=None):
    """utils/util.py:81-89. Defaults to the packaged config."""
    if config_fn is None:
        config_fn = os.path.join(CONFIG_DIR, "config.json")
    hps = JsonHParams(**_load_config(config_fn))
    hps.config_dir = os.path.dirname(os.path.abspath(config_fn))
    return hps


def noise_schedule(mapper_cfg):
    """modules/diffsvc.py:248-252: np.linspace(*noise_schedule_factors) (f64)."""
    a, b, n = mapper_cfg.noise_schedule_factors
    return np.linspace(a, b, int(n))


SOLVERS = {"ddim": 1, "dpmpp2m": 2}  # solver name -> order of svc_diffsvc_sample_steps
SOLVER_SPACINGS = ("logsnr", "uniform")


def check_solver(solver, solver_steps=20, solver_spacing="logsnr"):
    """The solver keywords of the sampler calls: solver None (the DDPM / PLMS call as before) or a name of SOLVERS,
    solver_steps an int >= 1, solver_spacing a name of SOLVER_SPACINGS; else ValueError before any device work."""
    if solver is None:
        return None
    if solver not in SOLVERS:
        raise ValueError(f"solver {solver!r}: None, {', '.join(map(repr, SOLVERS))}")
    ok = isinstance(solver_steps, (int, np.integer)) and not isinstance(solver_steps, bool)
    if not ok or solver_steps < 1:
        raise ValueError(f"solver_steps {solver_steps!r}: an integer >= 1")
    if solver_spacing not in SOLVER_SPACINGS:
        raise ValueError(f"solver_spacing {solver_spacing!r}: 'logsnr' or 'uniform'")
    return solver


def solver_timesteps(cfg, k_step, n, spacing="logsnr"):
    """The timesteps of an n-step solver run (svc_diffsvc_sample_steps) from noise level K - 1 down, K = k_step or with
    None the schedule's length: a strictly decreasing list of ints in [0, K - 1] that starts at K - 1.
    "logsnr": evenly spaced in lambda_t = ln(ac_t / (1 - ac_t)) / 2 between lambda_{K-1} and lambda_0 and snapped to the
    grid (node j is the first t nearest the j-th target; a node not below its predecessor is dropped, so the list may be
    shorter than n). lambda is f64 over the engine's f32 alphas_cumprod table widened exactly. Evenly spaced t ends on a
    last step of h = 2.9 (n = 20) in lambda with the linear beta schedule, which costs both orders their accuracy
    (DESIGN.md).
    "uniform": t_j = ((K - 1)(n - 1 - j)) // (n - 1).
    The library sees only the list: this is the one place the policy lives."""
    betas = noise_schedule(cfg.mapper)
    steps = len(betas)
    K = steps if k_step is None else int(k_step)
    if not 1 <= K <= steps:
        raise ValueError(f"k_step {k_step!r}: an integer in [1, {steps}]")
    n_ok = isinstance(n, (int, np.integer)) and not isinstance(n, bool)
    if not n_ok or n < 1 or n > K:
        raise ValueError(f"solver_steps {n!r}: an integer in [1, {K}]")
    if spacing not in SOLVER_SPACINGS:
        raise ValueError(f"solver_spacing {spacing!r}: 'logsnr' or 'uniform'")
    n = int(n)
    if n == 1:
        return [K - 1]
    if spacing == "uniform":
        return [((K - 1) * (n - 1 - j)) // (n - 1) for j in range(n)]
    ac = np.cumprod(1.0 - betas).astype(np.float32).astype(np.float64)[:K]
    lam = 0.5 * np.log(ac / (1.0 - ac))
    out = []
    for j in range(n):
        t = int(np.argmin(np.abs(lam - (lam[K - 1] + (lam[0] - lam[K - 1]) * j / (n - 1)))))
        if not out or t < out[-1]:
            out.append(t)
    return out


def load_stats(cfg):
    path = os.path.join(getattr(cfg, "config_dir", CONFIG_DIR), cfg.stats_file)
    with open(path) as f:
        s = json.load(f)
    return {
        "mel_min": np.asarray(s["mel_min"], dtype=np.float32),
        "mel_max": np.asarray(s["mel_max"], dtype=np.float32),
        "target_f0_median": float(s["target_f0_median"]),
    }


def load_singers(cfg):
    path = os.path.join(getattr(cfg, "config_dir", CONFIG_DIR), cfg.singer_file)
    with open(path) as f:
        return json.load(f)
