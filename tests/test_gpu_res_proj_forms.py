"""res_proj.hip's loader-wave form (two loader waves, six compute waves of two column blocks each, 16-B row stores) and
the form without the dead lo store, at the smallest shapes where that structure can go wrong. As
test_gpu_stages.py::test_res_proj_bit_identical: the whole denoiser (engine.diffsvc_eps) with res_proj = 0 (the tiled
conv_gemm3 with its LDS-staged split epilogue) is the reference and the outputs must be bit for bit equal.

The dead-lo form (the last residual layer stores no low half) is checked through eps alone: every diffsvc_eps call runs
the last residual layer in that form, and there is no debug read-back of the denoiser's workspace, so lo16 itself is not
inspected."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import dev  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

TINY = W.WHISPER_DIMS["tiny-test"]
STEPS = (250, 7)


@pytest.fixture(scope="module")
def cfg():
    c = C.load_config()
    c.mapper.input_content_dim["whisper"] = TINY["n_audio_state"]
    return c


@pytest.fixture(scope="module")
def states(cfg):
    return dict(whisper=W.make_whisper_state(TINY, 0), mapper=W.make_mapper_state(cfg.mapper, 0),
                vocoder=W.make_vocoder_state(cfg.vocoder, 0))


@pytest.fixture(scope="module")
def engine(cfg, states):
    e = SVCEngine(cfg, 0, whisper_state=states["whisper"], mapper_state=states["mapper"], vocoder_state=states["vocoder"])
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine_bf16(cfg, states):
    e = SVCEngine(cfg, 0, whisper_state=states["whisper"], mapper_state=states["mapper"],
                  vocoder_state=states["vocoder"], content_split=0, head_split=False, operands="bf16")
    yield e
    e.close()


def _inputs(B, T):
    rng = np.random.default_rng(B * 17 + T)
    cond = dev(rng.standard_normal((B, T, 384)).astype(np.float32))
    x = dev(rng.standard_normal((B, T, 100)).astype(np.float32))
    return cond, x


def _check(eng, tune, B, T, switches):
    cond, x = _inputs(B, T)
    tune(eng, res_proj=0)
    ref = [eng.diffsvc_eps(cond, x, t).cpu().numpy() for t in STEPS]
    for kv in switches:
        tune(eng, **kv)
        out = [eng.diffsvc_eps(cond, x, t).cpu().numpy() for t in STEPS]
        for k in range(len(STEPS)):
            assert np.isfinite(out[k]).all(), (kv, k)
            assert np.array_equal(out[k], ref[k]), (kv, k, float(np.abs(out[k] - ref[k]).max()))


# (1, 16) / (1, 17): exactly one tile, and one row into a second (every other workgroup's tiles, and the loaders' tiles
# past the end, are zero tiles). (3, 37): 111 rows, fewer tiles than row lanes and a ragged last tile (rows past M are
# dropped by the 16-B stores' range check). (3, 700): 2 100 rows, just past 128 lanes x 16 rows: a partly filled second
# iteration.
@pytest.mark.parametrize("B,T", [(1, 16), (1, 17), (3, 37), (3, 700)])
def test_loader_form_bit_identical(engine, tune, B, T):
    _check(engine, tune, B, T, [dict(res_proj=1)])


def test_loader_form_capped_lanes(engine, tune):
    """2 100 rows on 8 and 24 row lanes: 17 and 6 iterations per workgroup, the steady-state waits of the loader waves
    (counted vmcnt) and the compute waves (barrier only)."""
    _check(engine, tune, 3, 700, [dict(res_proj=8), dict(res_proj=24)])


def test_loader_form_bf16(engine_bf16, tune):
    """Op16<true> takes the same accumulator swap and 16-B stores."""
    _check(engine_bf16, tune, 3, 37, [dict(res_proj=1), dict(res_proj=8)])


def test_first_form_beside_another_stream(engine, tune):
    """Two sampler streams keep the first form (12 waves that load and store, 3/8 of the CUs), now also without the last
    layer's lo store."""
    _check(engine, tune, 3, 37, [dict(res_proj=1, sampler_streams=2)])
    _check(engine, tune, 3, 700, [dict(res_proj=1, sampler_streams=2)])
