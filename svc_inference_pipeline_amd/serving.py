"""Streaming request front end over the ragged-batch pipeline.

The reference converts one clip per call (infer.py:44-90, B = 1 throughout). A service receives clips one at a time
and of any length; SVCServer turns that stream into ragged GPU batches:

    server = SVCServer(SVCPipeline(engine), max_batch=32, max_wait_s=0.02)
    fut = server.submit(wav24, wav16, singer_id)       # returns at once (concurrent.futures.Future)
    wav = fut.result()                                 # f32 [T * hop] on the GPU
    fut = server.submit_file(wav_bytes_or_path, singer_id)   # a wav file: only its header is parsed here
    server.close()

A worker thread takes the oldest pending request, adds the pending requests whose length is within `length_ratio` of
it (so padding stays bounded: the kernels skip the padded tail, but its rows still occupy the batch) up to
`max_batch`, waits at most `max_wait_s` for a batch to fill, and runs SVCPipeline.convert_ragged on it. Each request
carries an utterance id (given, or a running counter) that keys its device noise, so its waveform is bit-identical to
converting that clip alone with the same id, whatever it was batched with (tests/test_gpu_ragged.py). A request may ask
for shallow diffusion (`k_step`, and `k_step_mel` for its start mel); a batch is formed only from requests with the same
`k_step` and `k_step_mel`, and the same solver setting (`solver`, `solver_steps`, `solver_spacing`: the server's
defaults or a request's own). The same holds for `loudness_mix` (loudness envelope transfer against the request's own
24 kHz source).

Streams: submit() records an event on the caller's current stream, and the worker's stream waits for it before it
reads the request's tensors, so inputs produced by kernels still in flight on the caller's stream are safe to
submit. A result is a view into the batch's output, recorded for use on the submitting stream (record_stream), and
the future resolves once it is complete. File requests carry no tensors: the worker decodes all of a batch's files in
one audio.load_batch (svc_load_pcm; with a HuBERT / ContentVec configuration svc_load_pcm_ex, which also gives each its
float 16 kHz input `wav16_float`) on its own stream. The engine's lock (SVCEngine.lock) serialises the worker's conversions with
any direct use of the same engine.
"""
import collections
import itertools
import os
import threading
import time
from concurrent.futures import Future
from dataclasses import dataclass, field

import torch

from . import _lib
from . import audio as A
from .config import check_solver, solver_timesteps
from .pipeline import SVCPipeline, wants_float16k
from .runtime import check_k_step, check_k_step_mel, mel_frames
from .singers import check_index_rate


@dataclass
class _Request:
    wav24: torch.Tensor
    wav16: torch.Tensor
    singer: int
    utt_id: int
    wav16_float: torch.Tensor = None
    frames: int = 0
    t_submit: float = 0.0
    ready: object = None    # torch.cuda.Event recorded on the submitting stream (None on the CPU)
    stream: object = None   # the submitting stream
    future: Future = field(default_factory=Future)
    file: object = None     # audio.WavInfo of a submit_file request (wav24 / wav16 are decoded by the worker)
    float16k: bool = False  # a file request whose decoding also fills wav16_float (a HuBERT configuration)
    key_shift: float = 0.0  # semitones on top of the shift to the singer's F0 median
    k_step: object = None   # shallow diffusion: the sampler starts from the clip's own mel at this step (None: full)
    k_step_mel: str = "source"  # that start mel: the clip's own ("source") or its key-shifted one ("shifted")
    loudness_mix: object = None  # loudness envelope transfer against the source (None: not run)
    solver: object = None   # (solver, solver_steps, solver_spacing), or None: the server's DDPM / PLMS sampler
    index_rate: object = None  # feature retrieval against the singer's enrolled index (None: not run)


class SVCServer:
    def __init__(self, pipeline: SVCPipeline, max_batch=32, max_wait_s=0.02, length_ratio=2.0, fast_inference=True,
                 speedup=10, seed=0, pcm16=False, solver=None, solver_steps=20, solver_spacing="logsnr"):
        """solver, solver_steps, solver_spacing: the default sampler of the requests (SVCPipeline.convert(solver=)); a
        request may override each in submit() / submit_file(), and a batch holds requests of one setting only.
        pcm16=True: each future resolves to save_audio's samples of its waveform, int16 [T * hop + 2 * (fs // 20)]
        (convert_ragged(pcm16=True): half the bytes to copy back, no host normalisation), instead of the f32 waveform."""
        if max_batch < 1 or max_wait_s < 0 or length_ratio < 1.0:
            raise ValueError("SVCServer: max_batch >= 1, max_wait_s >= 0, length_ratio >= 1")
        self.pipeline = pipeline
        self.max_batch = int(max_batch)
        self.max_wait_s = float(max_wait_s)
        self.length_ratio = float(length_ratio)
        self.kw = dict(fast_inference=fast_inference, speedup=speedup, seed=seed)
        self._solver = (solver, solver_steps, solver_spacing)
        self._solver_setting(None, None, None, None)  # ValueError here for bad defaults
        if pcm16:
            self.kw["pcm16"] = True
        cfg = pipeline.engine.cfg
        self._frames = lambda n: mel_frames(n, cfg.n_fft, cfg.hop_length)
        self._fs = getattr(cfg, "fs", None)  # the model rate file requests are resampled to
        self._float16k = wants_float16k(cfg)  # file requests are decoded with the float 16 kHz rows HuBERT reads
        self._ids = itertools.count()
        self._pending = []
        self._cv = threading.Condition()
        self._closed = False
        self.batches = collections.deque(maxlen=4096)  # utterance ids of the most recent batches (inspection, tests)
        self._device = getattr(pipeline.engine, "device", None)
        self._worker = threading.Thread(target=self._run, name="svc-server", daemon=True)
        self._worker.start()

    def _solver_setting(self, solver, solver_steps, solver_spacing, k_step):
        """A request's solver setting, each keyword None taking the server's default (solver "none": DDPM / PLMS on a
        server whose default is a solver), validated on the caller's thread -> (solver, solver_steps, solver_spacing),
        or None for no solver."""
        solver = self._solver[0] if solver is None else solver
        solver = None if solver == "none" else solver
        steps = self._solver[1] if solver_steps is None else solver_steps
        spacing = self._solver[2] if solver_spacing is None else solver_spacing
        if check_solver(solver, steps, spacing) is None:
            return None
        cfg = self.pipeline.engine.cfg
        if getattr(cfg, "mapper", None) is not None:
            solver_timesteps(cfg, k_step, steps, spacing)
        return (solver, steps, spacing)

    def _index_rate(self, index_rate):
        """A request's index_rate validated on the caller's thread (SVCPipeline's rule: bf16 content has no retrieval)."""
        index_rate = check_index_rate(index_rate)
        if index_rate is not None and getattr(self.pipeline.engine, "operands", "fp16") == "bf16":
            raise ValueError("index_rate: feature retrieval takes fp16 content (this engine runs operands='bf16')")
        return index_rate

    def submit(self, wav24, wav16, singer, utt_id=None, wav16_float=None, key_shift=0.0, k_step=None,
               k_step_mel="source", loudness_mix=None, solver=None, solver_steps=None, solver_spacing=None,
               index_rate=None) -> Future:
        """Queue one utterance (device tensors: 24 kHz f32 [N], 16 kHz [N16], optional float 16 kHz for
        ContentVec) -> Future resolving to its waveform f32 [T * hop] (int16 PCM with the server's pcm16=True).
        key_shift: semitones for this request, on top of the shift to its singer's F0 median.
        k_step: shallow diffusion for this request (SVCPipeline.convert_ragged(k_step=)); a batch holds requests of
        one k_step only, so the result is still the clip converted alone.
        k_step_mel: "source" or "shifted", shallow diffusion's start mel (SVCPipeline.convert(k_step_mel=)); a batch
        holds one value of it too.
        loudness_mix: loudness envelope transfer for this request (SVCPipeline.convert_ragged(loudness_mix=)); a batch
        holds requests of one value only (None, the stage not run, is a value of its own).
        solver, solver_steps, solver_spacing: this request's sampler instead of the server's default, each None: the
        server's (solver="none": DDPM / PLMS on a server whose default is a solver); a batch holds one setting only.
        index_rate: feature retrieval for this request (SVCPipeline.convert_ragged(index_rate=)); a batch holds
        requests of one value only (None, the stage not run, is a value of its own)."""
        n = int(wav24.shape[-1])
        if n < 1 or int(wav16.shape[-1]) < 1:
            raise ValueError("SVCServer.submit: empty audio")
        k_step = check_k_step(k_step, self.pipeline.engine.cfg)  # ValueError here, not in the worker
        check_k_step_mel(k_step_mel, k_step)
        loudness_mix = A.check_loudness_mix(loudness_mix)
        index_rate = self._index_rate(index_rate)
        sol = self._solver_setting(solver, solver_steps, solver_spacing, k_step)
        req = _Request(wav24=wav24.reshape(-1), wav16=wav16.reshape(-1), singer=int(singer),
                       utt_id=next(self._ids) if utt_id is None else int(utt_id),
                       wav16_float=None if wav16_float is None else wav16_float.reshape(-1),
                       frames=self._frames(n), t_submit=time.monotonic(), key_shift=float(key_shift), k_step=k_step,
                       k_step_mel=k_step_mel, loudness_mix=loudness_mix, solver=sol, index_rate=index_rate)
        if wav24.is_cuda:
            req.stream = torch.cuda.current_stream(wav24.device)
            req.ready = torch.cuda.Event()
            req.ready.record(req.stream)
        with self._cv:
            if self._closed:
                raise RuntimeError("SVCServer.submit: the server is closed")
            self._pending.append(req)
            self._cv.notify()
        return req.future

    def submit_file(self, src, singer, utt_id=None, key_shift=0.0, k_step=None, k_step_mel="source",
                    loudness_mix=None, solver=None, solver_steps=None, solver_spacing=None, index_rate=None) -> Future:
        """Queue one wav file (a path, bytes or a memoryview) -> Future, as submit(). Only the header is parsed here:
        the request's frame count for batching follows from its length and rate (svc_resample_len, mel_frames), and
        the worker decodes all the file requests of a batch in one audio.load_batch (they may share a batch with tensor
        requests). A bad file (unreadable header, <= 2 frames, non-finite samples) fails its own future only.
        When the configuration names a HuBERT / ContentVec content type the decode also gives the request its float
        16 kHz row (audio.load_contentvec_audio of the file), so for batching it counts as a request with `wav16_float`:
        it shares a batch with tensor requests that carry one, never with tensor requests that do not.
        k_step, k_step_mel, loudness_mix, solver, solver_steps, solver_spacing, index_rate: as in submit()."""
        k_step = check_k_step(k_step, self.pipeline.engine.cfg)  # ValueError here, not in the worker
        check_k_step_mel(k_step_mel, k_step)
        loudness_mix = A.check_loudness_mix(loudness_mix)
        index_rate = self._index_rate(index_rate)
        sol = self._solver_setting(solver, solver_steps, solver_spacing, k_step)
        req = self._file_request(src, singer, utt_id)
        req.solver = sol
        req.index_rate = index_rate
        req.loudness_mix = loudness_mix
        req.key_shift = float(key_shift)
        req.k_step = k_step
        req.k_step_mel = k_step_mel
        if req.future.done():
            return req.future
        if torch.cuda.is_available():
            req.stream = torch.cuda.current_stream(self._device)
        with self._cv:
            if self._closed:
                raise RuntimeError("SVCServer.submit_file: the server is closed")
            self._pending.append(req)
            self._cv.notify()
        return req.future

    def _file_request(self, src, singer, utt_id=None):
        """The request of one wav file from its header alone: frames = mel_frames(svc_resample_len(file frames, file
        rate, fs)), nothing decoded. A file that cannot be queued comes back with its future already failed."""
        req = _Request(wav24=None, wav16=None, singer=int(singer),
                       utt_id=next(self._ids) if utt_id is None else int(utt_id), t_submit=time.monotonic())
        try:
            info = A.parse_wav(src, None if isinstance(src, (str, os.PathLike)) else f"<request {req.utt_id}>")
            if info.n_frames <= 2:
                raise A.AudioError(f"{info.name}: {info.n_frames} samples")
        except Exception as exc:  # noqa: BLE001 - the caller sees it through the future, like a decode failure
            req.future.set_exception(exc)
            return req
        req.file = info
        req.float16k = self._float16k
        req.frames = self._frames(int(_lib.load().svc_resample_len(info.n_frames, info.sr, int(self._fs))))
        return req

    def enroll(self, singer, sources=None, wavs24=None, max_batch=16, **index_args):
        """SVCPipeline.enroll on the server's pipeline (it takes the engine's lock, so it runs between batches): the
        singer's F0 median from the singer's own recordings becomes the pitch target of later requests. index_args:
        SVCPipeline.enroll's index arguments (index, index_max_rows, index_compact, index_iters, wavs16, wavs16_float),
        passed through as given; any other name is a TypeError."""
        unknown = sorted(set(index_args) - {"index", "index_max_rows", "index_compact", "index_iters", "wavs16",
                                            "wavs16_float"})
        if unknown:
            raise TypeError(f"enroll: unexpected argument(s) {unknown}")
        return self.pipeline.enroll(singer, sources=sources, wavs24=wavs24, max_batch=max_batch, **index_args)

    def close(self, wait=True):
        """Stop accepting requests; the worker finishes every queued request first."""
        with self._cv:
            self._closed = True
            self._cv.notify()
        if wait:
            self._worker.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ worker
    def _take_batch(self):
        """The oldest request plus the pending ones of compatible length (within length_ratio, same ContentVec input
        form, same k_step, k_step_mel, loudness_mix, index_rate and solver setting), at most max_batch; called with the lock held."""
        head = self._pending[0]
        lo, hi = head.frames / self.length_ratio, head.frames * self.length_ratio
        batch = [head]
        for r in self._pending[1:]:
            if len(batch) == self.max_batch:
                break
            if (lo <= r.frames <= hi and self._has_float(r) == self._has_float(head) and r.k_step == head.k_step
                    and r.k_step_mel == head.k_step_mel and r.loudness_mix == head.loudness_mix
                    and r.solver == head.solver and r.index_rate == head.index_rate):
                batch.append(r)
        taken = set(map(id, batch))
        self._pending = [r for r in self._pending if id(r) not in taken]
        return batch

    @staticmethod
    def _has_float(r):
        """The request holds a float 16 kHz input, or will once the worker has decoded its file."""
        return r.wav16_float is not None or r.float16k

    def _ready(self):
        """A batch may run: it is full, the oldest request has waited max_wait_s, or the server is closing."""
        if not self._pending:
            return False
        if self._closed or len(self._pending) >= self.max_batch:
            return True
        return time.monotonic() - self._pending[0].t_submit >= self.max_wait_s

    def _run(self):
        if self._device is not None and torch.cuda.is_available():
            torch.cuda.set_device(self._device)
        while True:
            with self._cv:
                while not self._ready():
                    if self._closed and not self._pending:
                        return
                    timeout = None
                    if self._pending:
                        timeout = max(0.0, self.max_wait_s - (time.monotonic() - self._pending[0].t_submit))
                    self._cv.wait(timeout)
                batch = self._take_batch()
            self._convert(batch)

    def _decode_files(self, batch):
        """Decode the batch's file requests in one load_batch; a file that fails resolves its own future with the error
        and leaves the batch. -> the requests that go on."""
        files = [r for r in batch if r.file is not None]
        if not files:
            return batch
        w16f = [None] * len(files)
        try:
            if self._float16k:
                w24, w16, w16f, errors = A.load_batch([r.file for r in files], self._fs, self.pipeline.engine,
                                                      on_error="return", float16k=True)
            else:
                w24, w16, errors = A.load_batch([r.file for r in files], self._fs, self.pipeline.engine,
                                                on_error="return")
        except Exception as exc:  # noqa: BLE001 - the decode itself failed: every file request of the batch
            w24, w16, errors = [None] * len(files), [None] * len(files), {i: exc for i in range(len(files))}
        for i, r in enumerate(files):
            if i in errors:
                r.future.set_exception(errors[i])
            else:
                r.wav24, r.wav16, r.wav16_float = w24[i], w16[i], w16f[i]
        return [r for r in batch if r.wav24 is not None]

    def _convert(self, batch):
        batch = self._decode_files(batch)
        if not batch:
            return
        try:
            if torch.cuda.is_available():
                work = torch.cuda.current_stream()
                for r in batch:  # the inputs' producers on the submitting streams
                    if r.ready is not None:
                        work.wait_event(r.ready)
                    for t in (r.wav24, r.wav16, r.wav16_float):
                        if t is not None and t.is_cuda:
                            t.record_stream(work)
            w16f = [r.wav16_float for r in batch] if batch[0].wav16_float is not None else None
            kw = dict(self.kw)
            if any(r.key_shift for r in batch):  # one per request (none shifted: the call as before)
                kw["key_shift"] = [r.key_shift for r in batch]
            if batch[0].k_step is not None:  # the whole batch's (_take_batch)
                kw["k_step"] = batch[0].k_step
            if batch[0].k_step_mel != "source":
                kw["k_step_mel"] = batch[0].k_step_mel
            if batch[0].loudness_mix is not None:
                kw["loudness_mix"] = batch[0].loudness_mix
            if batch[0].index_rate is not None:
                kw["index_rate"] = batch[0].index_rate
            if batch[0].solver is not None:
                kw.update(zip(("solver", "solver_steps", "solver_spacing"), batch[0].solver))
            wavs = self.pipeline.convert_ragged([r.wav24 for r in batch], [r.wav16 for r in batch],
                                                [r.singer for r in batch], wavs16_float=w16f,
                                                utt_ids=[r.utt_id for r in batch], **kw)
            if torch.cuda.is_available():
                torch.cuda.current_stream().synchronize()
            self.batches.append([r.utt_id for r in batch])
            for r, w in zip(batch, wavs):
                if r.stream is not None and w.is_cuda:
                    w.record_stream(r.stream)  # the batch buffer outlives the consumer's use on its own stream
                r.future.set_result(w)
        except Exception as exc:  # noqa: BLE001 - every waiting caller gets the failure
            for r in batch:
                if not r.future.done():
                    r.future.set_exception(exc)
