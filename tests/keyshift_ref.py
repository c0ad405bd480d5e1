"""The key-shifted log-mel in numpy, from its definition (include/svc_hip.h, svc_mel_keyshift): the transform in
float64 (np.fft.rfft) on the float32-windowed frames, float32 magnitude and rescale, float64 filterbank and log."""
import numpy as np

from oracle import features as OF


def n_new_of(factor, n_fft):
    """(n_new, info) of one utterance: rint(n_fft * factor) in float64 (half to even, as np.round) clamped to
    [n_fft / 2, 2 n_fft], info bit 1 when the clamp acted; a factor that is not finite or <= 0 counts as 1, info bit 0."""
    f = np.float64(factor)
    if not np.isfinite(f) or f <= 0:
        return n_fft, 1
    r = np.round(np.float64(n_fft) * f)
    if r < n_fft // 2:
        return n_fft // 2, 2
    if r > 2 * n_fft:
        return 2 * n_fft, 2
    return int(r), 0


def filterbank(cfg):
    return OF.slaney_mel_filterbank(cfg.fs, cfg.n_fft, cfg.n_mels, cfg.fmin, cfg.fmax)


def frames(wav, n_new, n_fft, hop):
    """The float32-windowed frames [T, n_new] of a 1-D float32 clip: frame t holds samples t hop + j - (n_new - hop) // 2,
    reflected once at either end of the clip; T is the unshifted mel's frame count."""
    wav = np.asarray(wav, np.float32)
    L = wav.shape[0]
    T = OF.mel_frames(L, n_fft, hop)
    idx = np.arange(T)[:, None] * hop + np.arange(n_new)[None, :] - (n_new - hop) // 2
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= L, 2 * (L - 1) - idx, idx)
    assert idx.min() >= 0 and idx.max() < L, "the clip is too short for one reflection"
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_new, dtype=np.float64) / n_new)).astype(np.float32)
    return wav[idx] * w[None, :]


def mel_keyshift(wav, factor, cfg, fb=None):
    """wav f32 [N], factor -> (log-mel f64 [T, n_mels], info)."""
    n, hop = cfg.n_fft, cfg.hop_length
    fb = filterbank(cfg) if fb is None else fb
    n_new, info = n_new_of(factor, n)
    xw = frames(wav, n_new, n, hop)
    assert xw.dtype == np.float32
    X = np.fft.rfft(xw.astype(np.float64), axis=-1)  # [T, n_new // 2 + 1]
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    mag = np.sqrt(re * re + im * im + np.float32(1e-9))
    if n_new != n:
        mag = mag * np.float32(n) / np.float32(n_new)
    assert mag.dtype == np.float32
    spec = np.zeros((mag.shape[0], n // 2 + 1), np.float32)
    k = min(n // 2 + 1, mag.shape[1])
    spec[:, :k] = mag[:, :k]
    mel = spec.astype(np.float64) @ fb.astype(np.float64).T
    return np.log(np.maximum(mel, 1e-5)), info
