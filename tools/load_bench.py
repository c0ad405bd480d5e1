"""The input end on the GPU (svc_load_pcm) for a service-sized batch: 32 PCM16 mono 44.1 kHz clips of 10 s, synthetic,
built in memory as whole wav files.

  (a) HIP-event time of one svc_load_pcm call (payloads already on the device): warm median of `reps` (>= 20) calls on
      one input, and again rotating over distinct inputs; the launches alone from the library's own events, and once
      more through svc_load_pcm_ex with the float 16 kHz rows (the mono launch then stores two rows);
  (b) end to end on this box, host clock around work that ends synchronised: audio.load_batch on the 32 byte strings
      (header parse, one concatenation, one upload, one call) against what a caller did before, 32 x
      (audio.load_audio + audio.load_whisper_audio) on the same files on disk; median of 5 each, the two alternating;
  (c) the two results are compared row by row (np.array_equal) and the tool fails when they differ.

Prints one JSON line. Usage: python tools/load_bench.py [reps]"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

B, SR, SECONDS = 32, 44100, 10.0


def make_clip(seed):
    """A whole PCM16 mono wav file in memory: a few drifting partials plus noise, peak about 0.5"""
    rng = np.random.default_rng(seed)
    n = int(SR * SECONDS)
    t = np.arange(n) / SR
    x = sum(a * np.sin(2 * np.pi * f * t * (1 + 0.01 * np.sin(2 * np.pi * 0.7 * t)))
            for a, f in ((0.25, 220.0 + 7 * seed), (0.12, 440.0 + 11 * seed), (0.06, 1320.0)))
    x = x + 0.02 * rng.standard_normal(n)
    pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2")
    path = os.path.join(tempfile.gettempdir(), f"load_bench_{os.getpid()}_{seed}.wav")
    A.write_wav_pcm16(path, pcm, SR)
    with open(path, "rb") as fh:
        data = fh.read()
    return path, data


def event_ms(fn, n_inputs, reps):
    """median / min HIP-event ms of fn(i % n_inputs) over reps calls, after one warm pass over every input"""
    for i in range(n_inputs):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i % n_inputs)
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms)


def alternating_host_ms(fns, n=5):
    """median host-clock ms of each function, the functions taking turns, every run ending synchronised"""
    out = [[] for _ in fns]
    for _ in range(n):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(v) for v in out]


def clocks():
    """the GPU's shader / memory clocks right now, read as bench.py's ClockSampler reads them (null with the reason
    where the box does not expose them)"""
    try:
        from bench import ClockSampler
        cs = ClockSampler(0)
        sc, mc, hw = cs.read() if cs.src and not cs.err else (None, None, None)
        return {"source": cs.src, "sclk_mhz": sc, "mclk_mhz": mc, "sclk_hwmon_mhz": hw, "error": cs.err}
    except Exception as e:  # noqa: BLE001 (reported, never fatal)
        return {"source": None, "error": f"{type(e).__name__}: {e}"}


def main():
    reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 50
    cfg = C.load_config()
    eng = SVCEngine(cfg, 0)
    fs = int(cfg.fs)
    clips = [make_clip(s) for s in range(B)]
    paths, datas = [p for p, _ in clips], [d for _, d in clips]
    try:
        infos = [A.parse_wav(d) for d in datas]
        lib = _lib.load()
        n_src = [int(lib.svc_resample_len(i.n_frames, i.sr, fs)) for i in infos]
        n_mono = [int(lib.svc_resample_len(i.n_frames, i.sr, A.WHISPER_SR)) for i in infos]
        payload = sum(len(i.payload) for i in infos)
        algo_bytes = payload * 2 + 4 * (sum(n_src) + sum(n_mono))  # each payload read by both row kernels

        # (a) the call alone: payloads resident on the device, outputs allocated once
        import ctypes
        host = np.concatenate([np.frombuffer(i.payload, dtype=np.uint8) for i in infos])
        offs = np.concatenate([[0], np.cumsum([len(i.payload) for i in infos])[:-1]]).tolist()
        n_rot = 12  # 12 x 28 MB of payload: ~340 MB of other traffic between two reads of the same buffer
        raws = [torch.from_numpy(host).cuda()]
        raws += [torch.roll(raws[0], 2 * k) for k in range(1, n_rot)]
        y_src = torch.empty(B, max(n_src), device="cuda")
        y_mono = torch.empty(B, max(n_mono), device="cuda")
        info = torch.empty(B, dtype=torch.int32, device="cuda")
        i64, i32 = ctypes.c_int64 * B, ctypes.c_int32 * B
        tables = (i64(*offs), i64(*[i.n_frames for i in infos]), i32(*[i.format for i in infos]),
                  i32(*[i.channels for i in infos]), i32(*[i.sr for i in infos]))

        def call(k):
            _lib.call("svc_load_pcm", eng._ctx, ctypes.c_void_p(raws[k].data_ptr()), B, *tables, fs, y_src.shape[1],
                      ctypes.c_void_p(y_src.data_ptr()), A.WHISPER_SR, y_mono.shape[1],
                      ctypes.c_void_p(y_mono.data_ptr()), ctypes.c_void_p(info.data_ptr()),
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

        warm_med, warm_min = event_ms(lambda i: call(0), 1, reps)
        rot_med, rot_min = event_ms(call, n_rot, max(reps, 48))
        clk = clocks()  # right behind the timed calls
        _lib.profile_filter("load_pcm")
        _lib.profile_enable(True)
        for i in range(48):
            call(i % n_rot)
        stats = _lib.profile_read()
        _lib.profile_enable(False)
        _lib.profile_filter("")
        kern = {k: v["ms"] / v["launches"] for k, v in stats.items()}
        launches_per_call = sum(v["launches"] for v in stats.values()) / 48
        y_float = torch.empty_like(y_mono)

        def call_ex(k):
            _lib.call("svc_load_pcm_ex", eng._ctx, ctypes.c_void_p(raws[k].data_ptr()), B, *tables, fs,
                      y_src.shape[1], ctypes.c_void_p(y_src.data_ptr()), A.WHISPER_SR, y_mono.shape[1],
                      ctypes.c_void_p(y_mono.data_ptr()), ctypes.c_void_p(y_float.data_ptr()),
                      ctypes.c_void_p(info.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

        for i in range(n_rot):
            call_ex(i)
        torch.cuda.synchronize()
        _lib.profile_filter("load_pcm")
        _lib.profile_enable(True)
        for i in range(48):
            call_ex(i % n_rot)
        stats = _lib.profile_read()
        _lib.profile_enable(False)
        _lib.profile_filter("")
        kern_float = {k: round(v["ms"] / v["launches"], 5) for k, v in sorted(stats.items())}
        del raws

        # (b) end to end, against the per-file path; (c) equal results
        def batched():
            return A.load_batch(datas, fs, eng)

        def per_file():
            return [A.load_audio(p, fs) for p in paths], [A.load_whisper_audio(p) for p in paths]

        new24, new16 = batched()
        old24, old16 = per_file()
        match = all(np.array_equal(a.cpu().numpy(), b.cpu().numpy())
                    for new, old in ((new24, old24), (new16, old16)) for a, b in zip(new, old))
        def batched_paths():
            return A.load_batch(paths, fs, eng)  # reads the files too, as the per-file path does

        batched_ms, per_file_ms, batched_paths_ms = alternating_host_ms([batched, per_file, batched_paths])
        parse = []
        for _ in range(5):
            t0 = time.perf_counter()
            for d in datas:
                A.parse_wav(d)
            parse.append((time.perf_counter() - t0) * 1e3)
        parse_ms = statistics.median(parse)
        res = {
            "tool": "load_bench", "B": B, "sr_in": SR, "seconds": SECONDS, "format": "pcm16 mono", "fs": fs,
            "payload_bytes": payload, "src_samples": n_src[0], "mono_samples": n_mono[0], "reps": reps,
            "algorithmic_bytes": algo_bytes,
            "svc_load_pcm_ms_warm_median": round(warm_med, 5), "svc_load_pcm_ms_warm_min": round(warm_min, 5),
            "svc_load_pcm_ms_rotating_median": round(rot_med, 5), "svc_load_pcm_ms_rotating_min": round(rot_min, 5),
            "kernel_ms_rotating_mean": {k: round(v, 5) for k, v in sorted(kern.items())},
            "kernel_ms_rotating_mean_with_float_row": kern_float, "launches_per_call": launches_per_call,
            "e2e_load_batch_ms": round(batched_ms, 3), "e2e_load_batch_from_paths_ms": round(batched_paths_ms, 3),
            "e2e_per_file_load_audio_plus_load_whisper_audio_ms": round(per_file_ms, 3),
            "e2e_ratio_per_file_over_batched": round(per_file_ms / batched_ms, 3),
            "host_parse_wav_32_ms": round(parse_ms, 3),
            "outputs_match": bool(match), "torch_threads": torch.get_num_threads(), "clocks": clk,
        }
        print(json.dumps(res), flush=True)
    finally:
        for p in paths:
            if os.path.exists(p):
                os.remove(p)
        eng.close()
    if not match:
        raise SystemExit("load_batch differs from load_audio / load_whisper_audio")


if __name__ == "__main__":
    main()
