"""Voice store: prompts prepared once on the GPU, used by handle afterwards.

A TTS server has a handful of voices and many requests per voice.  ``VoiceStore.register`` runs the
prompt front of ``infer.generate_batch`` once per voice and entirely on the device: upload -> resample
(``feature.Resample``) -> RMS (``zv_prompt_rms``) -> normalisation (``zv_prompt_scale``) -> fbank
(``extract_batch``) -> ``(feats + feat_bias) * feat_scale`` into the store's arena.  A ``Voice`` is the
handle of one stored prompt; ``generate_batch`` takes ``(tokens, Voice)`` items and
``serving.ContinuousBatcher.submit`` takes ``voice=``.  ``gather`` builds the speech condition of a group
of requests straight from the arena (``zv_voice_gather``) together with the gains that restore each
prompt's level on the output, all of it on the device: an admission reads nothing back.

The reference has no counterpart (it prepares the prompt of every sentence on the host,
``zipvoice/bin/infer_zipvoice.py:332-349``); ``include/zipvoice_hip.h`` defines the kernels.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as _eng
from .feature import compute_num_frames


class FrameAllocator:
    """First fit over the frame ranges of an arena of ``capacity`` frames, on the host.  The free list
    is kept sorted by offset and neighbours are merged on ``free``."""

    def __init__(self, capacity: int):
        if int(capacity) < 1:
            raise ValueError("capacity must be at least 1 frame")
        self.capacity = int(capacity)
        self._free: List[List[int]] = [[0, self.capacity]]        # [offset, frames], by offset
        self._used = {}                                          # offset -> frames

    def largest(self) -> int:
        return max((n for _, n in self._free), default=0)

    def free_ranges(self) -> List[Tuple[int, int]]:
        return [(o, n) for o, n in self._free]

    def alloc(self, frames: int) -> int:
        """The offset of the first free range that holds ``frames``; ValueError when none does."""
        frames = int(frames)
        if frames < 1:
            raise ValueError("a range holds at least 1 frame")
        for i, (o, n) in enumerate(self._free):
            if n >= frames:
                if n == frames:
                    del self._free[i]
                else:
                    self._free[i] = [o + frames, n - frames]
                self._used[o] = frames
                return o
        raise ValueError(f"the voice store is full: {frames} frames asked for, the largest free range "
                         f"has {self.largest()} (capacity {self.capacity})")

    def free(self, offset: int) -> None:
        """Give the range that starts at ``offset`` back and merge it with its free neighbours."""
        if offset not in self._used:
            raise ValueError(f"no range starts at frame {offset}")
        frames = self._used.pop(offset)
        i = 0
        while i < len(self._free) and self._free[i][0] < offset:
            i += 1
        self._free.insert(i, [offset, frames])
        if i + 1 < len(self._free) and offset + frames == self._free[i + 1][0]:
            self._free[i][1] += self._free.pop(i + 1)[1]
        if i > 0 and sum(self._free[i - 1]) == offset:
            self._free[i - 1][1] += self._free.pop(i)[1]


@dataclass(frozen=True, eq=False)
class Voice:
    """One registered prompt: ``frames`` feature frames at arena row ``offset`` of ``store``,
    ``samples`` prompt samples at the model's rate, and the prompt's tokens."""
    id: int
    offset: int
    frames: int
    samples: int
    prompt_tokens: Tuple[int, ...]
    store: "VoiceStore" = field(repr=False)


@dataclass(frozen=True, eq=False)
class Recording:
    """One registered recording to edit: ``frames`` feature frames (``compute_num_frames(samples, hop)``, the
    ``L`` of ``edit.sample_table``) at arena row ``offset`` of ``store`` and ``samples`` samples at the
    model's rate, whose un-normalised waveform the store keeps on the device (``VoiceStore.waveform``)."""
    id: int
    offset: int
    frames: int
    samples: int
    store: "VoiceStore" = field(repr=False)


def _check_rc(lib, rc: int):
    if rc != 0 and "voice table:" in lib.zv_last_error().decode():
        raise ValueError(lib.zv_last_error().decode())
    _eng._check(rc, lib)


def prompt_rms(wav: torch.Tensor, lens: Sequence[int], target_rms: float):
    """``zv_prompt_rms``: wav (B, ld) fp32 on the device, ``lens`` host sample counts ->
    (rms, gain_in, gain_out, lens int32 on the device), each (B,) on the device."""
    lib = _eng.load_library()
    B, ld = wav.shape
    hl = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    if hl.shape != (B,):
        raise ValueError(f"lens: expected shape ({B},), got {hl.shape}")
    ln = torch.from_numpy(hl).to(wav.device)
    out = torch.empty((3, B), dtype=torch.float32, device=wav.device)
    with torch.cuda.device(wav.device):
        _eng._check(lib.zv_prompt_rms(_eng._ptr(wav), ld, _eng._ptr(ln), hl.ctypes.data, B, float(target_rms),
                                      _eng._ptr(out[0]), _eng._ptr(out[1]), _eng._ptr(out[2]), _eng._stream()), lib)
    return out[0], out[1], out[2], ln


def prompt_scale(wav: torch.Tensor, lens: Sequence[int], lens_dev: torch.Tensor, rms: torch.Tensor,
                 target_rms: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``zv_prompt_scale``: the rows of wav (B, ld) below ``target_rms`` brought up to it, the others
    copied, zeros past each row's length."""
    lib = _eng.load_library()
    B, ld = wav.shape
    hl = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    out = torch.empty_like(wav) if out is None else out
    with torch.cuda.device(wav.device):
        _eng._check(lib.zv_prompt_scale(_eng._ptr(wav), ld, _eng._ptr(lens_dev), hl.ctypes.data, _eng._ptr(rms), B,
                                        float(target_rms), _eng._ptr(out), _eng._stream()), lib)
    return out


class VoiceGather:
    """The ``zv_voice`` handle: device table and pinned staging of ``zv_voice_gather``."""

    def __init__(self, device):
        self.lib, self.device = _eng.load_library(), torch.device(device)
        with torch.cuda.device(self.device):
            self.h = self.lib.zv_voice_create()
        if not self.h:
            raise RuntimeError(self.lib.zv_last_error().decode())

    def close(self) -> None:
        h = getattr(self, "h", None)
        if h:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            self.lib.zv_voice_destroy(h)
            self.h = None

    __del__ = close

    def device_bytes(self) -> int:
        return int(self.lib.zv_voice_device_bytes(self.h))

    def __call__(self, pool: torch.Tensor, table, T: int, gains_pool: Optional[torch.Tensor] = None):
        """pool (rows, F) fp32 on the device, ``table`` host rows (offset, frames) -> (out (n, T, F),
        gains (n,) or None).  A bad table is a ValueError and launches nothing."""
        tab = np.ascontiguousarray(np.asarray(table, dtype=np.int32).reshape(-1, 2))
        n, (rows, F) = tab.shape[0], pool.shape
        out = torch.empty((n, int(T), F), dtype=torch.float32, device=self.device)
        g = None if gains_pool is None else torch.empty((n,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _check_rc(self.lib, self.lib.zv_voice_gather(self.h, _eng._ptr(pool), rows, F, tab.ctypes.data, n, int(T),
                                                         _eng._ptr(out), _eng._ptr(gains_pool), _eng._ptr(g),
                                                         _eng._stream()))
        return out, g


class VoiceStore:
    """``capacity_frames`` feature frames of registered prompts on the device.

    ``register`` / ``register_batch`` prepare prompts and return their ``Voice`` handles, ``drop`` frees
    one (a ValueError while a ``ContinuousBatcher`` still has it queued; rows already admitted own a copy
    of their condition), ``gather`` builds a group's speech condition and output gains.  Everything
    after the upload of the samples stays on the device; registration is not the hot path and uploads
    from pageable memory, ``gather`` is: a warm call neither blocks the host nor reads from the device."""

    _serial = itertools.count()

    def __init__(self, feature_extractor, capacity_frames: int, target_rms: float = 0.1, feat_scale: float = 0.1,
                 feat_bias: float = 0.0, sampling_rate: int = 24000, device=None):
        self.fx = feature_extractor
        if feature_extractor.num_channels != 1:
            raise ValueError("the voice store holds one-channel prompts (the stereo model is out of scope)")
        if int(sampling_rate) != feature_extractor.config.sampling_rate:
            raise ValueError(f"sampling_rate {sampling_rate} is not the feature extractor's "
                             f"({feature_extractor.config.sampling_rate})")
        self.target_rms, self.feat_scale, self.feat_bias = float(target_rms), feat_scale, feat_bias
        self.sampling_rate = int(sampling_rate)
        self.alloc = FrameAllocator(capacity_frames)
        self.n_mels = feature_extractor.feature_dim(self.sampling_rate)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.arena = torch.zeros((self.alloc.capacity, self.n_mels), dtype=torch.float32, device=self.device)
        self.gains = torch.ones((self.alloc.capacity,), dtype=torch.float32, device=self.device)
        self._gather = VoiceGather(self.device)
        self._live = {}                       # voice id -> Voice
        self._uses = {}                       # voice id -> requests a batcher has queued
        self._wavs = {}                       # recording id -> its waveform at the model's rate, (samples,)
        self._ids = itertools.count()
        self.serial = next(VoiceStore._serial)

    # ------------------------------------------------------------------ registration
    def frames_of(self, samples: int, prompt_sampling_rate: Optional[int] = None) -> Tuple[int, int]:
        """(samples at the model's rate, feature frames) of a prompt of ``samples`` samples, by the
        host rules: ``ResamplePlan.out_len`` and ``compute_num_frames``."""
        from .infer import _resampler
        n = int(samples)
        if prompt_sampling_rate is not None and int(prompt_sampling_rate) != self.sampling_rate:
            n = _resampler(int(prompt_sampling_rate), self.sampling_rate).plan.out_len(n)
        return n, compute_num_frames(n, self.fx._hop)

    def _front(self, waves: Sequence, rates: Sequence[Optional[int]], what: str, keep_wav: bool = False):
        """The front of a registration: waveforms -> (arena offsets, frames, samples at the model's rate[,
        the resampled un-normalised waveforms on the device]).  Nothing is registered on an error."""
        from .infer import _prompts_at_rate
        dev, B = self.device, len(waves)
        wavs = [torch.as_tensor(np.asarray(w), dtype=torch.float32).reshape(-1) for w in waves]
        rates = [self.sampling_rate if r is None else int(r) for r in rates]
        sizes = [self.frames_of(len(w), r) for w, r in zip(wavs, rates)]
        lens, frames = [s[0] for s in sizes], [s[1] for s in sizes]
        pad = self.fx._n_fft // 2 if self.fx._frame_offset is None else self.fx._frame_offset
        if min(lens) <= pad:
            raise ValueError(f"reflect padding needs more than {pad} samples per {what}")
        offsets: List[int] = []
        try:
            for f in frames:
                offsets.append(self.alloc.alloc(f))
        except ValueError:
            for o in offsets:
                self.alloc.free(o)
            raise
        kept = []
        try:
            ld = (max(lens) + 3) // 4 * 4                 # (a multiple of 4: the 16-byte form of the scale pass)
            wb = torch.zeros((B, ld), dtype=torch.float32, device=dev)
            # (one upload and one resample per other rate; a prompt at the model's rate goes up here)
            for i, w in enumerate(_prompts_at_rate(wavs, rates, self.sampling_rate, dev)):
                wb[i, :lens[i]] = w
            if keep_wav:                                  # (before the normalisation below, which is in place)
                kept = [wb[i, :lens[i]].clone() for i in range(B)]
            rms, _, gain_out, ln = prompt_rms(wb, lens, self.target_rms)
            prompt_scale(wb, lens, ln, rms, self.target_rms, out=wb)
            feats, _ = self.fx.extract_batch(wb, torch.tensor(lens))
            feats = (feats + self.feat_bias) * self.feat_scale
            for i, (o, f) in enumerate(zip(offsets, frames)):
                self.arena[o:o + f] = feats[i, :f]
                self.gains[o:o + 1] = gain_out[i:i + 1]
        except Exception:
            for o in offsets:
                self.alloc.free(o)
            raise
        return offsets, frames, lens, kept

    @torch.inference_mode()
    def register_batch(self, prompts: Sequence[tuple]) -> List[Voice]:
        """``prompts`` = [(prompt_wav, prompt_tokens[, prompt_sampling_rate]), ...] -> their voices.
        A prompt the fbank cannot frame or a full arena is a ValueError and registers none."""
        if len(prompts) == 0:
            return []
        offsets, frames, lens, _ = self._front([p[0] for p in prompts],
                                               [None if len(p) < 3 else p[2] for p in prompts], "prompt")
        out = []
        for i, (o, f) in enumerate(zip(offsets, frames)):
            v = Voice(next(self._ids), o, f, lens[i], tuple(int(t) for t in prompts[i][1]), self)
            self._live[v.id], self._uses[v.id] = v, 0
            out.append(v)
        return out

    def register(self, prompt_wav, prompt_tokens, prompt_sampling_rate: Optional[int] = None) -> Voice:
        return self.register_batch([(prompt_wav, prompt_tokens, prompt_sampling_rate)])[0]

    @torch.inference_mode()
    def register_recording_batch(self, recordings: Sequence) -> List[Recording]:
        """``recordings`` = [wav or (wav, sampling_rate), ...] -> their ``Recording`` handles: the voices'
        front into the same arena (a range of whole rows each, the output gain at its first row), and the
        resampled, un-normalised waveform kept on the device for the splice (one tensor per recording).
        A recording the fbank cannot frame or a full arena is a ValueError and registers none."""
        if len(recordings) == 0:
            return []
        pairs = [r if isinstance(r, tuple) else (r, None) for r in recordings]
        offsets, frames, lens, kept = self._front([p[0] for p in pairs], [p[1] for p in pairs], "recording",
                                                  keep_wav=True)
        out = []
        for i, (o, f) in enumerate(zip(offsets, frames)):
            r = Recording(next(self._ids), o, f, lens[i], self)
            self._live[r.id], self._uses[r.id], self._wavs[r.id] = r, 0, kept[i]
            out.append(r)
        return out

    def register_recording(self, wav, sampling_rate: Optional[int] = None) -> Recording:
        return self.register_recording_batch([(wav, sampling_rate)])[0]

    def waveform(self, recording: Recording) -> torch.Tensor:
        """The recording at the model's rate, un-normalised, (samples,) on the device."""
        return self._wavs[self.check(recording).id]

    # ------------------------------------------------------------------ handles
    def check(self, voice):
        """``voice`` if it is a live voice (or recording) of this store; a ValueError otherwise."""
        if not isinstance(voice, (Voice, Recording)):
            raise ValueError(f"expected a Voice, got {type(voice).__name__}")
        kind = "recording" if isinstance(voice, Recording) else "voice"
        if voice.store is not self:
            raise ValueError(f"{kind} {voice.id} belongs to another store")
        if self._live.get(voice.id) is not voice:
            raise ValueError(f"{kind} {voice.id} has been dropped")
        return voice

    def hold(self, voice) -> None:
        """One more request uses ``voice``: a voice while the request is queued (``ContinuousBatcher.submit``),
        a recording from ``submit_edit`` until its row has been retired (retirement reads the arena again)."""
        self._uses[self.check(voice).id] += 1

    def release(self, voice) -> None:
        self._uses[voice.id] -= 1

    def uses(self, voice) -> int:
        """The requests that hold ``voice`` now."""
        return self._uses[self.check(voice).id]

    def drop(self, voice) -> None:
        self.check(voice)
        if self._uses[voice.id]:
            kind = "recording" if isinstance(voice, Recording) else "voice"
            raise ValueError(f"{kind} {voice.id} is still used by {self._uses[voice.id]} queued request(s)"
                             if kind == "voice" else
                             f"recording {voice.id} is still used by {self._uses[voice.id]} queued or in-flight "
                             f"request(s)")
        del self._live[voice.id], self._uses[voice.id]
        self._wavs.pop(voice.id, None)
        self.alloc.free(voice.offset)

    def device_bytes(self) -> int:
        return (self.arena.numel() * 4 + self.gains.numel() * 4 + self._gather.device_bytes()
                + sum(w.numel() * 4 for w in self._wavs.values()))

    # ------------------------------------------------------------------ the hot path
    def gather(self, voices: Sequence[Voice], T: int):
        """(speech condition (n, T, n_mels): row r the frames of ``voices[r]``, then zeros; gain_out
        (n,): the factor that restores row r's prompt level on its output).  One ``zv_voice_gather``."""
        table = [(self.check(v).offset, v.frames) for v in voices]
        return self._gather(self.arena, table, T, self.gains)
