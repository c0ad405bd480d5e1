"""GPU parity, stage level: each libsvc_hip stage against the oracle (which tests/test_oracle_golden.py
pins to reference-generated goldens) on the same seeded weights and inputs.

Tolerances (stated per test): the MFMA path rounds operands to fp16 (fp32 accumulate), so
network outputs are compared by relative L2 error; integer work (frame counts, bucketize indices,
content index maps) is bit-exact.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import dev, rel_l2  # noqa: E402
from oracle import features as OF  # noqa: E402
from oracle import models as OM  # noqa: E402
from oracle import noise as ON  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

TINY = W.WHISPER_DIMS["tiny-test"]


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


def test_mel_energy(engine, cfg, golden):
    g = golden("mel24k")
    for wav in (g["wav"], ON.synth_clip(3, 10.0, 24000), ON.synth_clip(4, 0.3, 24000)):
        mel, en = engine.mel_energy(dev(wav[None]))
        ref = OF.mel_spectrogram(torch.from_numpy(wav)[None], cfg)[0]
        assert mel.shape[1] == ref.shape[-1] == OF.mel_frames(len(wav))
        mel = mel[0].cpu().numpy().T
        # f64 FFT vs torch's f32 FFT: log-mel agrees to 1e-4 where the magnitude is above the 1e-5 clamp
        assert np.max(np.abs(mel - ref.numpy())) < 2e-3
        assert np.mean(np.abs(mel - ref.numpy())) < 3e-5
        ref_en = OF.energy_from_mel(ref[None])[0].numpy()
        np.testing.assert_allclose(en[0].cpu().numpy(), ref_en, rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (2048, 512)])
def test_mel_energy_other_fft_sizes(n_fft, hop):
    """The FFT plans the headline config does not use (n/2 = 256: four radix-4 stages; n/2 = 1024: five), through a
    features-only engine configured with that n_fft / hop / win_length, against the oracle's torch.stft mel."""
    c = C.load_config()
    c.n_fft, c.hop_length, c.win_length = n_fft, hop, n_fft
    e = SVCEngine(c, 0)
    try:
        wav = ON.synth_clip(5, 2.0, 24000)
        mel, en = e.mel_energy(dev(wav[None]))
        ref = OF.mel_spectrogram(torch.from_numpy(wav)[None], c)[0]
        mel = mel[0].cpu().numpy().T
        assert mel.shape == ref.shape
        assert np.max(np.abs(mel - ref.numpy())) < 2e-3
        assert np.mean(np.abs(mel - ref.numpy())) < 3e-5
        np.testing.assert_allclose(en[0].cpu().numpy(), OF.energy_from_mel(ref[None])[0].numpy(), rtol=2e-5, atol=1e-7)
    finally:
        e.close()


@pytest.mark.parametrize("direct", ["15", "0"])
def test_whisper_encoder_tiny(engine, golden, direct, tune):
    """Whisper encoder against the reference-pinned golden, with conv_gemm3's register epilogues (qkv / fc1: f16
    outputs, out / fc2: f32 residual) and with the LDS-staged epilogue (gemm3_direct = 0)."""
    tune(engine, gemm3_direct=direct)
    g = golden("whisper_logmel")
    wav16 = g["wav16"]
    feats = engine.whisper_encode(dev(wav16[None]))
    ref = golden("whisper_encoder_tiny")["feats"]
    assert rel_l2(feats[0].cpu().numpy(), ref) < 5e-3


def test_whisper_stream_split(engine, golden, tune):
    """whisper_streams = 2 / 3 (utterance-aligned sub-batches on concurrent streams) against the default single
    full-batch stream, on a batch of 3 clips; the sub-batch launches may pick other GEMM tiles, so the bound is fp32
    rounding, not bit equality."""
    g = golden("whisper_logmel")
    w = dev(np.stack([g["wav16"], g["wav16"][::-1].copy(), 0.5 * g["wav16"]]))
    tune(engine, whisper_streams=1)
    one = engine.whisper_encode(w).cpu().numpy()
    for ns in ("2", "3"):
        tune(engine, whisper_streams=ns)
        split = engine.whisper_encode(w).cpu().numpy()
        for b in range(3):
            assert rel_l2(split[b], one[b]) < 1e-4, (ns, b)


def test_content_map_exact(engine, golden):
    g = golden("content_map")
    raw = torch.from_numpy(g["raw"]).float()
    for tl in (1, 93, 379, 937, 2812):
        out = engine.map_content(dev(raw[None]), tl)[0].cpu().numpy()
        exp = g[f"T{tl}"].astype(np.float32).astype(np.float16)
        assert np.array_equal(out, exp), tl


def test_conditioner(engine, states, golden):
    g = golden("conditioner_diffsvc")
    content16 = dev(g["content"][None], torch.float16)
    cond = engine.condition(content16, dev(g["f0_shift"][None], torch.float64), dev(g["energy"][None]),
                            dev(np.array([1]), torch.int32))
    ref = OM.conditioner(states["mapper"], torch.from_numpy(g["content"].astype(np.float16).astype(np.float32))[None],
                         torch.from_numpy(g["f0_shift"])[None], torch.from_numpy(g["energy"])[None],
                         torch.tensor([[1]]))
    assert rel_l2(cond.cpu().numpy(), ref.numpy()) < 2e-3


def test_eps_single_step(engine, cfg, states, golden):
    g = golden("conditioner_diffsvc")
    cond = dev(g["cond"])
    for t in (0, 500, 999):
        eps = engine.diffsvc_eps(cond, dev(g["x_in"]), t)
        assert rel_l2(eps.cpu().numpy(), g[f"eps_t{t}"]) < 5e-3, t


@pytest.mark.parametrize("B,T", [(1, 93), (3, 50), (2, 700)])
def test_denoiser_vs_oracle(engine, states, cfg, B, T):
    """The denoiser (tiled GEMMs with the paired gate epilogue, the split-fp16 residual stream, the skip-sum GEMM)
    against the oracle on ragged shapes (B*T not a multiple of the GEMM tiles, utterance boundaries inside a tile):
    relative L2 <= 5e-3 (fp16 operands)."""
    rng = np.random.default_rng(B * 1000 + T)
    cond = rng.standard_normal((B, T, 384)).astype(np.float32)
    x = rng.standard_normal((B, T, 100)).astype(np.float32)
    table = W.step_embedding_table(1000)
    for t in (3, 640):
        eps = engine.diffsvc_eps(dev(cond), dev(x), t).cpu().numpy()
        with torch.no_grad():
            ref = OM.diffsvc_forward(states["mapper"], cfg.mapper, torch.from_numpy(x), torch.from_numpy(cond),
                                     torch.full((B,), t, dtype=torch.long), table).numpy()
        assert rel_l2(eps, ref) < 5e-3, (t, rel_l2(eps, ref))


@pytest.mark.parametrize("variant", ["20", "24"])
@pytest.mark.parametrize("B,T", [(3, 50), (2, 700), (5, 937)])
def test_gate_gemm_ragged(engine, states, cfg, variant, B, T, tune):
    """The DiffSVC gate GEMM kernels (conv_gemm4 with the LDS-staged and the in-register gate epilogue) on ragged row
    counts (B*T not a multiple of the 128-row tile, utterance boundaries inside tiles) against the oracle's eps."""
    rng = np.random.default_rng(B * 7 + T)
    cond = rng.standard_normal((B, T, 384)).astype(np.float32)
    x = rng.standard_normal((B, T, 100)).astype(np.float32)
    table = W.step_embedding_table(1000)
    tune(engine, gemm_variant=variant)
    eps = engine.diffsvc_eps(dev(cond), dev(x), 250).cpu().numpy()
    with torch.no_grad():
        ref = OM.diffsvc_forward(states["mapper"], cfg.mapper, torch.from_numpy(x), torch.from_numpy(cond),
                                 torch.full((B,), 250, dtype=torch.long), table).numpy()
    assert rel_l2(eps, ref) < 5e-3


@pytest.mark.parametrize("B,T,frames", [(1, 5, None), (1, 93, None), (3, 50, None), (2, 700, None), (5, 937, None),
                                         (16, 937, None), (4, 301, [301, 17, 160, 299]), (3, 40, [9, 40, 1])])
def test_gate_ws_bit_identical(engine, B, T, frames, tune):
    """gate_ws.hip (the DiffSVC dilated conv + gate as a weight-stationary row stream: W in VGPRs, one LDS image per
    64-row super-block shared by the three taps, the K chain split over a wave pair through the MFMA C operand) against
    conv_gemm4<128,128,gate> (gate_ws = 0): the same 32-deep K order, MFMA operand order and epilogue arithmetic, so the
    eps of every layer's dilation (1, 2, 4, 8) is bit for bit equal. Ragged row counts (parts of 16-row blocks, partial
    super-blocks, empty row parts), utterance boundaries inside blocks, ragged frame counts (taps past an utterance's
    valid rows read the zero row), one of them a single frame. gate_ws needs T >= 16 frames per batch row; (1, 5) checks
    that a shorter batch falls back to conv_gemm4 (the profiler records which kernel ran: gate_ws launches exactly when
    T >= 16, so no case passes by running conv_gemm4 on both sides)."""
    rng = np.random.default_rng(B * 29 + T)
    cond = dev(rng.standard_normal((B, T, 384)).astype(np.float32))
    x = dev(rng.standard_normal((B, T, 100)).astype(np.float32))
    tune(engine, gate_ws=0)
    ref = [engine.diffsvc_eps(cond, x, t, frames=frames).cpu().numpy() for t in (250, 7)]
    tune(engine, gate_ws=1)
    _lib.profile_enable(True)
    try:
        out = [engine.diffsvc_eps(cond, x, t, frames=frames).cpu().numpy() for t in (250, 7)]
        ran = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    n_ws = sum(v["launches"] for k, v in ran.items() if k.startswith("gate_ws"))
    n_g4 = sum(v["launches"] for k, v in ran.items() if k.startswith("conv_gemm4") and k.endswith("@diffsvc.dilated"))
    if T >= 16:
        assert n_ws > 0 and n_g4 == 0, ran.keys()
    else:
        assert n_ws == 0 and n_g4 > 0, ran.keys()
    for k in range(2):
        assert np.isfinite(out[k]).all()
        assert np.array_equal(out[k], ref[k]), (k, rel_l2(out[k], ref[k]))


@pytest.mark.parametrize("B,T", [(1, 93), (3, 50), (2, 700), (5, 937)])
def test_fused_head(engine, states, cfg, B, T, tune):
    """diff_head.hip (relu(skip_projection) + output_projection in one launch, u kept on chip) against the
    two unfused GEMMs: the same products, output_projection's K segments summed in another order (hi.W_hi, hi.W_lo,
    lo.W_hi), so within 1e-6 (f32 rounding order only); the oracle within 5e-3; ragged row counts."""
    rng = np.random.default_rng(B * 13 + T)
    cond = dev(rng.standard_normal((B, T, 384)).astype(np.float32))
    x = dev(rng.standard_normal((B, T, 100)).astype(np.float32))
    out = {}
    for name, v in (("fused", 1), ("unfused", 0)):
        tune(engine, diff_head=v)
        out[name] = (engine.diffsvc_eps(cond, x, 250), engine.diffsvc_eps(cond, x, 7))
    for k in range(2):
        assert torch.isfinite(out["fused"][k]).all()
        assert rel_l2(out["fused"][k].cpu().numpy(), out["unfused"][k].cpu().numpy()) < 1e-6
    table = W.step_embedding_table(1000)
    with torch.no_grad():
        ref = OM.diffsvc_forward(states["mapper"], cfg.mapper, x.cpu(), cond.cpu(), torch.full((B,), 7, dtype=torch.long),
                                 table).numpy()
    assert rel_l2(out["fused"][1].cpu().numpy(), ref) < 5e-3


@pytest.mark.parametrize("B,T", [(1, 5), (1, 93), (3, 50), (2, 700), (5, 937)])
def test_res_proj_bit_identical(engine, B, T, tune):
    """res_proj.hip (the DiffSVC residual projection as a weight-stationary row stream: W_res in VGPRs, 16-row tiles of
    g / hi / lo LDS-DMA'd through a ring) against the tiled conv_gemm3 GEMM with its LDS-staged split epilogue
    (res_proj = 0): the same 32-deep K order and epilogue arithmetic, so bit for bit equal. One workgroup per CU and
    capped grids of 8 / 24 row lanes (many ring iterations per workgroup, the steady-state vmcnt waits); tiny and
    ragged row counts (M < 16, rows past M inside the last tile read as zero and are not stored)."""
    rng = np.random.default_rng(B * 17 + T)
    cond = dev(rng.standard_normal((B, T, 384)).astype(np.float32))
    x = dev(rng.standard_normal((B, T, 100)).astype(np.float32))
    tune(engine, res_proj=0)
    ref = [engine.diffsvc_eps(cond, x, t).cpu().numpy() for t in (250, 7)]
    for v in (1, 8, 24):
        tune(engine, res_proj=v)
        out = [engine.diffsvc_eps(cond, x, t).cpu().numpy() for t in (250, 7)]
        for k in range(2):
            assert np.isfinite(out[k]).all()
            assert np.array_equal(out[k], ref[k]), (v, k, rel_l2(out[k], ref[k]))


def test_fused_head_plms(engine, golden, tune):
    """The fused head through PLMS-4 against the reference-generated golden (same bound as test_plms_and_ddpm)."""
    g = golden("samplers")
    cond = dev(golden("conditioner_diffsvc")["cond"])
    tune(engine, diff_head=1)
    x4 = engine.diffsvc_sample(cond, fast_inference=True, speedup=250, x_T=dev(g["x_T"]))
    assert rel_l2(x4[0].cpu().numpy().T, g["plms4"]) < 1e-3


@pytest.mark.parametrize("variant", ["10", "11", "12", "13", "14", "15", "16", "15lds", "15reg", "20", "24"])
def test_eps_gemm_variants(engine, golden, variant, tune):
    """The paired gate epilogue and the residual / skip GEMMs under every GEMM tile variant (unfused path); 15lds:
    conv_gemm3 with the LDS-staged epilogue everywhere; 15reg: with every register form, in the sampler too."""
    if variant in ("15lds", "15reg"):
        tune(engine, gemm3_direct=0 if variant == "15lds" else 15)
        variant = "15"
    tune(engine, gemm_variant=variant)
    g = golden("conditioner_diffsvc")
    eps = engine.diffsvc_eps(dev(g["cond"]), dev(g["x_in"]), 500)
    assert rel_l2(eps.cpu().numpy(), g["eps_t500"]) < 5e-3


def test_plms_and_ddpm(engine, cfg, states, golden):
    g = golden("samplers")
    cond = dev(golden("conditioner_diffsvc")["cond"])
    x4 = engine.diffsvc_sample(cond, fast_inference=True, speedup=250, x_T=dev(g["x_T"]))
    # measured 1.6e-4 (PLMS-4) and 2.1e-4 (DDPM-1000) against the reference-generated goldens (round 2)
    assert rel_l2(x4[0].cpu().numpy().T, g["plms4"]) < 1e-3
    # DDPM-1000 with the reference's injected noise: clipping keeps it stable, compare the final mel
    T = cond.shape[1]
    seed = int(g["seed"])
    noise = np.stack([ON.step_noise(seed, i, 1, T) for i in reversed(range(1000))])
    x = engine.diffsvc_sample(cond, fast_inference=False, x_T=dev(g["x_T"]), noise=dev(noise))
    assert rel_l2(x[0].cpu().numpy().T, g["ddpm1000"]) < 1.5e-3


def test_sampler_sub_streams_bit_identical(engine, golden, tune):
    """Utterance-aligned sub-batches on 2-3 streams (the default sampler schedule) reproduce the single-stream
    result bit for bit, for PLMS and for DDPM with device noise, including an uneven split (B = 3)."""
    g = golden("conditioner_diffsvc")
    cond = dev(np.concatenate([g["cond"]] * 3, 0))
    utt = dev(np.array([5, 6, 7]), torch.int32)
    outs = {}
    for ns in ("1", "2", "3"):
        tune(engine, sampler_streams=ns)
        plms = engine.diffsvc_sample(cond, fast_inference=True, speedup=250, seed=9, utt_ids=utt).cpu().numpy()
        ddpm = engine.diffsvc_sample(cond, fast_inference=False, seed=9, utt_ids=utt).cpu().numpy()
        outs[ns] = (plms, ddpm)
    for ns in ("2", "3"):
        assert np.array_equal(outs[ns][0], outs["1"][0]) and np.array_equal(outs[ns][1], outs["1"][1]), ns


@pytest.mark.parametrize("direct", ["15", "0"])
def test_bigvgan(engine, cfg, states, golden, direct, tune):
    tune(engine, gemm3_direct=direct)  # conv_gemm3 register epilogues (default) or the LDS-staged one
    g = golden("bigvgan")
    stats = C.load_stats(cfg)
    mel = g["mel"]  # de-normalised mel [100, T]
    x_norm = (mel - stats["mel_min"][:, None]) / (stats["mel_max"] - stats["mel_min"] + 1e-12)[:, None] * 2 - 1
    wav, mel_d = engine.bigvgan(dev(x_norm.T[None].astype(np.float32)), return_mel=True)
    assert np.max(np.abs(mel_d[0].cpu().numpy().T - mel)) < 1e-4
    # Random weights drive this generator into a chaotic, 97 % tanh-saturated regime where rounding
    # the conv operands to fp16 alone moves the waveform by ~4 % (relative L2). Tolerance: the HIP
    # result must be as close to the f32 oracle as the fp16-operand-emulated oracle is (x1.5 + 1e-3).
    with OM.Fp16Operands():
        emu = OM.bigvgan_forward(states["vocoder"], cfg.vocoder, torch.from_numpy(mel)[None])
    emu = OF.synthesis_fade(emu[0, 0], mel.shape[-1]).numpy()
    budget = 1.5 * rel_l2(emu, g["synth"]) + 1e-3
    assert rel_l2(wav[0].cpu().numpy(), g["synth"]) < budget
    # The emulation above also rounds AMPBlock1's convs1 output to f16 (the HIP path's storage since round 3), so its
    # budget could grow by what that storage gives up. Anchor it to fp32: the operand-rounding-only
    # emulation (the pre-round-3 one) sets a budget of its own, the HIP result must meet it too, and the storage term
    # must not move the emulation further from the f32 oracle (measured: 4.10e-2 with it, 4.18e-2 without; in this
    # chaotic regime any rounding moves the waveform by ~3-4 %).
    with OM.Fp16Operands(store16=False):
        emu_ops = OM.bigvgan_forward(states["vocoder"], cfg.vocoder, torch.from_numpy(mel)[None])
    emu_ops = OF.synthesis_fade(emu_ops[0, 0], mel.shape[-1]).numpy()
    d_ops = rel_l2(emu_ops, g["synth"])
    assert rel_l2(emu, g["synth"]) <= 1.1 * d_ops, (rel_l2(emu, g["synth"]), d_ops)
    assert rel_l2(wav[0].cpu().numpy(), g["synth"]) < 1.5 * d_ops + 1e-3


@pytest.mark.parametrize("variant", list(W.VOCODER_VARIANTS))
def test_bigvgan_variants(cfg, states, golden, variant, tune):
    """F4: AMPBlock2 / Snake (log and linear scale) generators against the oracle, which
    tests/test_oracle_golden.py::test_bigvgan_variants pins to the reference's own Generator. The fused
    small-channel path (amp_conv, C <= 48 or C <= 96) and the unfused activation1d + GEMM path (amp_maxc = 0) are checked,
    with test_bigvgan's tolerance (1.5 x the fp16-operand emulation's distance + 1e-3)."""
    import copy
    g = golden("bigvgan_variants")
    c2 = copy.deepcopy(cfg)
    c2.vocoder = W.vocoder_variant_cfg(cfg.vocoder, variant)
    vsd = W.make_vocoder_state(c2.vocoder, 0)
    stats = C.load_stats(c2)
    mel = g["mel"]
    T = mel.shape[-1]
    x_norm = (mel - stats["mel_min"][:, None]) / (stats["mel_max"] - stats["mel_min"] + 1e-12)[:, None] * 2 - 1
    ref = OF.synthesis_fade(torch.from_numpy(g[variant][0, 0]), T).numpy()
    with OM.Fp16Operands():
        emu = OM.bigvgan_forward(vsd, c2.vocoder, torch.from_numpy(mel)[None])
    budget = 1.5 * rel_l2(OF.synthesis_fade(emu[0, 0], T).numpy(), ref) + 1e-3
    e = SVCEngine(c2, 0, mapper_state=states["mapper"], vocoder_state=vsd)
    try:
        for maxc in ("48", "96", "192", "0"):
            tune(e, amp_maxc=maxc)
            wav = e.bigvgan(dev(x_norm.T[None].astype(np.float32)))[0].cpu().numpy()
            assert rel_l2(wav, ref) < budget, (maxc, rel_l2(wav, ref), budget)
    finally:
        e.close()


def test_bigvgan_ups_combined(engine, tune):
    """The rate-2 up-sampling ConvTranspose1d stages with 48 / 96 / 192 input channels (modules/bigvgan.py ups, `rate`
    phase GEMMs with tune.amp_ups = 0) as ONE conv over the input rows on amp_conv's plain-conv form (amp_ups = 1: 3 taps
    walked downwards, each phase's two taps in its GEMM's order, a zero tap for the one it lacks), for equal and ragged
    lengths. At 96 / 192 input channels each phase sums exactly its GEMM's products in the same order; at 48 the
    32-deep MFMA steps straddle taps and one phase's fp32 summation grouping moves, so the waveforms agree to fp32
    rounding (rel-L2 < 1e-5), not bit for bit."""
    rng = np.random.default_rng(11)
    x = dev(rng.uniform(-1, 1, (3, 41, 100)).astype(np.float32))
    outs, ran = {}, {}
    for v in ("0", "1"):
        tune(engine, amp_ups=v)
        _lib.profile_enable(True)
        try:
            outs[v] = (engine.bigvgan(x).cpu().numpy(), engine.bigvgan(x, frames=[41, 23, 33]).cpu().numpy())
            ran[v] = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
    # the combined kernel ran for every rate-2 stage it covers, and only when switched on (no case passes by running
    # the phase GEMMs on both sides)
    comb = {v: {n.split("@")[0]: r["launches"] for n, r in ran[v].items() if n.startswith("amp_conv<") and ",conv>" in n}
            for v in ran}
    assert comb["0"] == {}, comb["0"]
    assert set(comb["1"]) == {"amp_conv<48,conv>", "amp_conv<96,conv>", "amp_conv<192,conv>"}, comb["1"]
    assert all(n > 0 for n in comb["1"].values())
    for i in range(2):
        a, b = outs["0"][i], outs["1"][i]
        assert rel_l2(b, a) < 1e-5, (i, rel_l2(b, a))
        if i == 1:
            for u, n in enumerate([41, 23, 33]):  # ragged: each utterance's samples past its end stay untouched
                assert np.array_equal(a[u, n * 256:], b[u, n * 256:])


def test_vocoder_sub_streams_bit_identical(engine, tune):
    """BigVGAN with utterance-aligned sub-batches on 1, 2 or 3 streams: identical waveforms."""
    rng = np.random.default_rng(1)
    x = dev(rng.uniform(-1, 1, (3, 40, 100)).astype(np.float32))
    outs = {}
    for ns in ("1", "2", "3"):
        tune(engine, vocoder_streams=ns)
        outs[ns] = engine.bigvgan(x).cpu().numpy()
    assert np.array_equal(outs["2"], outs["1"]) and np.array_equal(outs["3"], outs["1"])


def test_bigvgan_batch_independence(engine, cfg):
    """Utterances in a batch never leak into each other through conv/activation halos."""
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (3, 30, 100)).astype(np.float32)
    wb = engine.bigvgan(dev(x)).cpu().numpy()
    for b in range(3):
        w1 = engine.bigvgan(dev(x[b:b + 1])).cpu().numpy()[0]
        assert np.array_equal(w1, wb[b])


def _adversarial_bucket_inputs(mbins, ebins):
    """f0 (f64) and energy (f32) values aimed at torch.bucketize's edge cases: every bin edge exactly, one f64 /
    f32 ulp either side of it, f64 values that round onto an f32 edge, zero and unvoiced f0, energy at and below
    the 1e-30 first edge and at and above 1.5, subnormals, NaN and infinities, plus random in-range values."""
    mb = mbins.astype(np.float64)
    f0 = [mb, np.nextafter(mb, np.inf), np.nextafter(mb, -np.inf),
          mb + mb * 2.0 ** -30, mb - mb * 2.0 ** -30,  # round onto the f32 edge when narrowed; compare in f64
          np.array([0.0, -0.0, -1.0, 1e-300, 32.6, 32.603, 2093.005, 2093.0046, 5000.0, 1e300,
                    np.nan, np.inf, -np.inf])]
    rng = np.random.default_rng(11)
    f0.append(np.exp(rng.uniform(np.log(20.0), np.log(3000.0), 4096)))
    f0 = np.concatenate(f0)
    eb = ebins.astype(np.float32)
    en = [eb, np.nextafter(eb, np.float32(np.inf)), np.nextafter(eb, np.float32(-np.inf)),
          np.array([0.0, -0.0, 1e-30, 9.99e-31, 1e-31, 1e-38, 1e-45, 1.4999999, 1.5, 1.5000001, 2.0, 1e30,
                    np.nan, np.inf, -np.inf], np.float32)]
    en.append(np.exp(rng.uniform(np.log(1e-32), np.log(3.0), 4096)).astype(np.float32))
    en = np.concatenate(en).astype(np.float32)
    n = max(len(f0), len(en))
    f0 = np.resize(f0, n)
    en = np.resize(en, n)
    return f0, en


def test_condition_indices_bit_exact(engine, states):
    """A10's integer half: the conditioner's melody / loudness indices equal torch.bucketize's (right=False, f64 f0
    against f32 bins compared in f64, NaN past the last bin) bit for bit on adversarial values
    (modules/encoder.py:47-57,70 and :93-102,115)."""
    p = "0.registered_modules_dict."
    mbins = np.asarray(states["mapper"][p + "melody.melody_bins"], np.float32)
    ebins = np.asarray(states["mapper"][p + "loudness.energy_bins"], np.float32)
    f0, en = _adversarial_bucket_inputs(mbins, ebins)
    im, ie = engine.condition_indices(dev(f0, torch.float64), dev(en))
    ref_m = torch.bucketize(torch.from_numpy(f0), torch.from_numpy(mbins)).numpy()
    ref_e = torch.bucketize(torch.from_numpy(en), torch.from_numpy(ebins)).numpy()
    assert np.array_equal(im.cpu().numpy(), ref_m)
    assert np.array_equal(ie.cpu().numpy(), ref_e)
    # the values that sit exactly on an edge land on that edge's index (number of bins < x)
    assert np.array_equal(ref_m[:len(mbins)], np.arange(len(mbins)))
    # and the oracle's index rule agrees (it is what the golden-pinned conditioner uses)
    assert np.array_equal(OM.bucketize_indices(torch.from_numpy(f0), torch.from_numpy(mbins)).numpy(), ref_m)


def test_condition_indices_empty_and_shapes(engine):
    im, ie = engine.condition_indices(dev(np.zeros((0,)), torch.float64), dev(np.zeros((0,))))
    assert im.numel() == 0 and ie.numel() == 0
    f0 = np.array([[0.0, 100.0, 440.0], [np.nan, 60.0, 900.0]])
    en = np.array([[0.0, 0.1, 1.0], [1e-31, 2.0, 0.5]], np.float32)
    im, ie = engine.condition_indices(dev(f0, torch.float64), dev(en))
    assert im.shape == (2, 3) and im.dtype == torch.int32


def test_ddpm_without_noise_or_utt_ids_is_rejected(engine, golden):
    """svc_diffsvc_sample in DDPM mode with x_T given but neither step noise nor utterance ids has no key for the
    device noise: the ABI must return SVC_ERR_INVALID (not read a NULL id table on the device)."""
    import ctypes
    from gpu_util import ptr, stream
    from svc_inference_pipeline_amd import _lib
    g = golden("samplers")
    cond = dev(golden("conditioner_diffsvc")["cond"])
    B, T, _ = cond.shape
    xT = dev(g["x_T"])
    x0 = torch.empty(B, T, 100, device="cuda")
    with pytest.raises(_lib.SVCError, match="utt_ids"):
        _lib.call("svc_diffsvc_sample", engine._ctx, ptr(cond), B, T, None, 0, 1, ptr(xT), None, ctypes.c_uint64(0), None,
                  ptr(x0), stream())
    # the host wrapper defaults the ids instead, and the run is reproducible
    a = engine.diffsvc_sample(cond, fast_inference=False, x_T=xT, seed=3).cpu().numpy()
    b = engine.diffsvc_sample(cond, fast_inference=False, x_T=xT, seed=3,
                              utt_ids=torch.zeros(B, dtype=torch.int32, device="cuda")).cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b)


def test_bigvgan_tamed_weights_tight(cfg, states, golden):
    """BigVGAN outside the chaotic regime: with every weight-normed conv's gain g halved (the reference's own
    parametrisation, modules/bigvgan.py weight_norm), the random-weight generator no longer saturates tanh, so an
    indexing or halo bug anywhere in the 6 up-sampling stages would show at the fp16-rounding scale. Tolerance: rel-L2
    vs the f32 oracle <= 2e-3 and <= 1.2x (+2e-4) the distance of the fp16-operand-emulated oracle (measured 8.5e-4
    against 8.8e-4, none of the output saturated)."""
    vsd = {k: (v * 0.5 if k.endswith("weight_g") else v) for k, v in W.make_vocoder_state(cfg.vocoder, 0).items()}
    e = SVCEngine(cfg, 0, mapper_state=states["mapper"], vocoder_state=vsd)
    try:
        g = golden("bigvgan")
        stats = C.load_stats(cfg)
        mel = g["mel"]
        T = mel.shape[-1]
        x_norm = (mel - stats["mel_min"][:, None]) / (stats["mel_max"] - stats["mel_min"] + 1e-12)[:, None] * 2 - 1
        wav = e.bigvgan(dev(x_norm.T[None].astype(np.float32)))[0].cpu().numpy()
        with torch.no_grad():
            ref = OF.synthesis_fade(OM.bigvgan_forward(vsd, cfg.vocoder, torch.from_numpy(mel)[None])[0, 0], T).numpy()
            with OM.Fp16Operands():
                emu = OF.synthesis_fade(OM.bigvgan_forward(vsd, cfg.vocoder, torch.from_numpy(mel)[None])[0, 0],
                                        T).numpy()
        sat = float(np.mean(np.abs(ref) > 0.97))
        d_hip, d_emu = rel_l2(wav, ref), rel_l2(emu, ref)
        print(f"tamed BigVGAN: saturated {sat:.3f}, rel-L2 HIP {d_hip:.2e}, fp16 emulation {d_emu:.2e}")
        assert sat < 0.05, sat  # the regime this test is about
        assert d_hip < 2e-3 and d_hip < 1.2 * d_emu + 2e-4, (d_hip, d_emu)
    finally:
        e.close()


@pytest.fixture(scope="module")
def engine_bf16(cfg, states):
    """The bf16 operand variant (content encoder, conditioner and DiffSVC GEMMs on v_mfma_f32_16x16x32_bf16), plain
    operands (no split modes), so it compares with the oracle's all-bf16 operand rounding."""
    e = SVCEngine(cfg, 0, whisper_state=states["whisper"], mapper_state=states["mapper"],
                  vocoder_state=states["vocoder"], content_split=0, head_split=False, operands="bf16")
    yield e
    e.close()


@pytest.mark.parametrize("B,T", [(1, 93), (3, 211)])
def test_bf16_eps_vs_emulated_oracle(engine_bf16, engine, states, cfg, B, T):
    """One denoiser call (gate GEMM, residual / skip / head GEMMs, hoisted conditioner projection) with bfloat16
    operands: its distance from the fp32 oracle is that of the oracle with every operand rounded to bf16 (within 1.5x
    + 1e-3; bf16 keeps 8 significand bits, so ~8x fp16's distance), and it is not the fp16 engine's result."""
    rng = np.random.default_rng(B * 3 + T)
    cond = rng.standard_normal((B, T, 384)).astype(np.float32)
    x = rng.standard_normal((B, T, 100)).astype(np.float32)
    table = W.step_embedding_table(1000)
    t = torch.full((B,), 250, dtype=torch.long)
    with torch.no_grad():
        ref = OM.diffsvc_forward(states["mapper"], cfg.mapper, torch.from_numpy(x), torch.from_numpy(cond), t,
                                 table).numpy()
        with OM.OperandRounding(torch.bfloat16, linear=True):
            emu = OM.diffsvc_forward(states["mapper"], cfg.mapper, torch.from_numpy(x), torch.from_numpy(cond), t,
                                     table).numpy()
    eps_bf = engine_bf16.diffsvc_eps(dev(cond), dev(x), 250).cpu().numpy()
    engine_bf16.tune(res_proj=0)  # the bf16 residual projection stream equals the tiled GEMM bit for bit
    try:
        assert np.array_equal(engine_bf16.diffsvc_eps(dev(cond), dev(x), 250).cpu().numpy(), eps_bf)
    finally:
        engine_bf16.tune(reset=1)
    eps_h = engine.diffsvc_eps(dev(cond), dev(x), 250).cpu().numpy()
    d_bf, d_emu, d_h = rel_l2(eps_bf, ref), rel_l2(emu, ref), rel_l2(eps_h, ref)
    assert np.isfinite(eps_bf).all()
    assert d_bf <= 1.5 * d_emu + 1e-3, (d_bf, d_emu)
    assert d_bf > 2 * d_h, (d_bf, d_h)  # really bf16 (fp16 is ~8x closer)


def test_bf16_whisper_encoder_vs_emulated_oracle(engine_bf16, states, golden):
    """The Whisper encoder (conv stem, LayerNorm operands, qkv / out / MLP GEMMs, attention with bf16 P) in the bf16
    operand variant against the oracle with bf16 operand rounding: the same distance class from fp32."""
    wav16 = golden("whisper_logmel")["wav16"]
    feats = engine_bf16.whisper_encode(dev(wav16[None]))[0].cpu().numpy()
    with torch.no_grad():
        lm = OF.whisper_log_mel(torch.from_numpy(OF.pad_or_trim(wav16))[None])
        ref = OM.whisper_encoder(states["whisper"], lm, TINY["n_audio_head"])[0].numpy()
        with OM.OperandRounding(torch.bfloat16, linear=True):
            emu = OM.whisper_encoder(states["whisper"], lm, TINY["n_audio_head"])[0].numpy()
    d_bf, d_emu = rel_l2(feats, ref), rel_l2(emu, ref)
    assert np.isfinite(feats).all()
    assert d_bf <= 1.5 * d_emu + 1e-3, (d_bf, d_emu)
