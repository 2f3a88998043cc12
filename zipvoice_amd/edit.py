"""Speech editing: regenerate marked spans of a recording in place.

The model is trained to fill a masked interior span of the features from the audio on both
sides and the full transcript (``ZipVoice.forward``, zipvoice/models/zipvoice.py:358-363); the
reference exposes that as ``sample_intermediate`` (:488-534).  This module plans an edit on the
host and runs it end to end:

* ``plan_edit`` / ``plan_edit_batch``: a row of ``L`` original feature frames and edit spans
  ``(s, e, n)``, "replace original frames [s, e) by n generated frames" (``e == s``: an
  insertion, ``n == 0``: a deletion), become a frame table with rows ``(dst, src, len)`` in
  ``dst`` order, ``src = -1`` for a generated segment.  The table drives
  ``HipEngine.edit_gather`` (``zv_edit_gather``), which builds the speech condition and puts the
  original frames back over the solver's output (``ZipVoice.sample_edit``).
* ``sample_table``: the same plan in samples, rows ``(out, src, len, kind)``, for
  ``HipEngine.edit_splice`` (``zv_edit_splice``), which puts the vocoder's rendering of the
  generated spans between the pieces of the original waveform with short cross-fades.
* ``edit_batch`` / ``edit_sentence``: waveform in, edited waveform out.

Finding span times from text (forced alignment) is outside this module: callers give frames,
or seconds through ``seconds_to_frames``.  A recording has to fit one decoder pass.
"""
from __future__ import annotations

import datetime as dt
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

KEPT, GENERATED = 0, 1


def seconds_to_frames(seconds: float, sampling_rate: int = 24000, hop: int = 256) -> int:
    """The feature frame nearest to a time (half up), at ``hop`` samples per frame."""
    return int(math.floor(float(seconds) * sampling_rate / hop + 0.5))


def span_frames(old_frames: int, old_tokens: int, new_tokens: int, speed: float = 1.0,
                frames_per_token: Optional[float] = None) -> int:
    """How many frames to generate for ``new_tokens`` tokens that replace ``old_tokens`` tokens
    spoken over ``old_frames`` frames: the old span's rate (frames per token) times the new
    token count, over ``speed``, rounded half up.  An insertion (nothing replaced) has no rate
    of its own: give the recording's, ``frames_per_token = L / S``, which also wins when given
    for a replacement."""
    if frames_per_token is None:
        if old_frames <= 0 or old_tokens <= 0:
            raise ValueError("an insertion needs frames_per_token (the recording's L / S)")
        frames_per_token = old_frames / old_tokens
    if speed <= 0:
        raise ValueError("speed must be positive")
    return int(math.floor(frames_per_token * new_tokens / speed + 0.5))


def _merged_spans(L: int, spans, row: int) -> List[Tuple[int, int, int]]:
    """The spans of one row, validated, with touching neighbours merged."""
    out: List[Tuple[int, int, int]] = []
    prev_e = 0
    for k, sp in enumerate(spans):
        if len(sp) != 3 or any(int(v) != v for v in sp):
            raise ValueError(f"row {row} span {k}: expected three integers (s, e, n), got {sp!r}")
        s, e, n = (int(v) for v in sp)
        if not 0 <= s <= e <= L:
            raise ValueError(f"row {row} span {k}: need 0 <= s <= e <= L = {L}, got ({s}, {e})")
        if n < 0:
            raise ValueError(f"row {row} span {k}: n must be non-negative, got {n}")
        if s == e and n == 0:
            raise ValueError(f"row {row} span {k}: an empty span that generates nothing")
        if k and s < prev_e:
            raise ValueError(f"row {row} span {k}: spans must be sorted and disjoint "
                             f"(starts at {s}, the one before ends at {prev_e})")
        if out and out[-1][1] == s:                       # touching: one span
            ps, _, pn = out.pop()
            s, n = ps, pn + n
        out.append((s, e, n))
        prev_e = e
    return out


def plan_edit(L: int, spans: Sequence[Sequence[int]], row: int = 0) -> np.ndarray:
    """The frame table of one row: int32 rows ``(dst, src, len)`` in ``dst`` order that tile
    ``[0, T)``, ``T = L - sum(e - s) + sum(n)``; ``src = -1`` marks a generated segment, a kept
    segment copies original frames ``[src, src + len)``.  Zero-length segments are dropped.
    ``row`` only names the row in error messages."""
    L = int(L)
    if L < 0:
        raise ValueError(f"row {row}: L must be non-negative, got {L}")
    rows: List[Tuple[int, int, int]] = []
    dst = src = 0
    for s, e, n in _merged_spans(L, spans, row):
        if s > src:
            rows.append((dst, src, s - src))
            dst += s - src
        if n:
            rows.append((dst, -1, n))
            dst += n
        src = e
    if L > src:
        rows.append((dst, src, L - src))
    return np.asarray(rows, np.int32).reshape(-1, 3)


def table_length(table: np.ndarray) -> int:
    """The length a table's segments tile (new frames, or output samples)."""
    return int(table[-1, 0] + table[-1, 2]) if len(table) else 0


@dataclass
class EditPlan:
    """The frame tables of a batch: ``table`` (n, 3) int32, the rows' tables stacked;
    ``row_ptr`` (B + 1,) int32, row b owns ``table[row_ptr[b]:row_ptr[b + 1]]``; ``lens`` the
    original and ``new_lens`` the new frame counts, (B,) int32."""
    table: np.ndarray
    row_ptr: np.ndarray
    lens: np.ndarray
    new_lens: np.ndarray

    def row(self, b: int) -> np.ndarray:
        return self.table[self.row_ptr[b]:self.row_ptr[b + 1]]

    def generated(self, b: int) -> int:
        """Generated frames of row b."""
        t = self.row(b)
        return int(t[t[:, 1] < 0, 2].sum())


def _stack(tables: List[np.ndarray], width: int) -> Tuple[np.ndarray, np.ndarray]:
    row_ptr = np.zeros(len(tables) + 1, np.int32)
    row_ptr[1:] = np.cumsum([len(t) for t in tables])
    table = np.concatenate(tables) if tables else np.zeros((0, width), np.int32)
    return np.ascontiguousarray(table.reshape(-1, width), np.int32), row_ptr


def plan_edit_batch(lens: Sequence[int], spans: Sequence[Sequence[Sequence[int]]]) -> EditPlan:
    """``plan_edit`` per row, stacked."""
    lens = [int(v) for v in lens]
    if len(spans) != len(lens):
        raise ValueError(f"expected the spans of {len(lens)} rows, got {len(spans)}")
    tables = [plan_edit(L, sp, row=b) for b, (L, sp) in enumerate(zip(lens, spans))]
    table, row_ptr = _stack(tables, 3)
    return EditPlan(table, row_ptr, np.asarray(lens, np.int32),
                    np.asarray([table_length(t) for t in tables], np.int32))


def sample_table(plan: np.ndarray, N: int, hop: int, L: Optional[int] = None) -> np.ndarray:
    """A row's frame table in samples: int32 rows ``(out, src, len, kind)`` that tile the edited
    waveform.  ``N`` is the original's true sample count; its frame count is
    ``L = (N + hop // 2) // hop``, so ``L * hop`` lies within ``hop / 2`` of ``N`` on either side.
    A kept segment (kind 0) reads original samples ``[src * hop, (src + len) * hop)``, and the
    one that ends at frame ``L`` runs to sample ``N``; a generated segment (kind 1) reads
    ``[dst * hop, (dst + len) * hop)`` of the vocoder's output over the new frames."""
    N, hop = int(N), int(hop)
    L = (N + hop // 2) // hop if L is None else int(L)
    rows, out = [], 0
    for dst, src, ln in np.asarray(plan).reshape(-1, 3).tolist():
        if src < 0:
            s0, n, kind = dst * hop, ln * hop, GENERATED
        else:
            end = N if src + ln == L else (src + ln) * hop
            s0, n, kind = src * hop, end - src * hop, KEPT
        if n > 0:
            rows.append((out, s0, n, kind))
            out += n
    return np.asarray(rows, np.int32).reshape(-1, 4)


def sample_table_batch(plan: EditPlan, Ns: Sequence[int], hop: int) -> Tuple[np.ndarray, np.ndarray]:
    """``sample_table`` per row of a batch plan, stacked: (table (n, 4), row_ptr (B + 1,))."""
    return _stack([sample_table(plan.row(b), N, hop, int(plan.lens[b])) for b, N in enumerate(Ns)], 4)


def mask_spans(mask_row: np.ndarray, L: int) -> List[Tuple[int, int, int]]:
    """The runs of True in ``mask_row[:L]`` as spans ``(s, e, e - s)``: the spans a
    ``speech_condition_mask`` (``sample_intermediate``) stands for."""
    m = np.asarray(mask_row[:L], bool)
    edges = np.flatnonzero(np.diff(np.concatenate([[False], m, [False]]).astype(np.int8)))
    return [(int(s), int(e), int(e - s)) for s, e in zip(edges[::2], edges[1::2])]


def edit_batch(items: Sequence[tuple], model, vocoder, feature_extractor, num_step: int = 16,
               guidance_scale: float = 1.0, t_shift: float = 0.5, target_rms: float = 0.1,
               feat_scale: float = 0.1, feat_bias: float = 0.0, fade: int = 240,
               seeds: Optional[Sequence[int]] = None, keep_original_audio: bool = True):
    """Edit recordings: items = [(tokens, wav, spans[, rate]), ...], ``tokens`` the whole new
    transcript, ``wav`` the recording (mono samples, at ``rate`` or the model's rate), ``spans``
    the ``(s, e, n)`` spans in feature frames of the recording at the model's rate.

    Steps: resample per distinct rate -> RMS-normalise a copy for the features (as
    ``generate_batch``) -> ``extract_batch`` -> ``(feat + feat_bias) * feat_scale`` ->
    ``plan_edit_batch`` -> ``model.sample_edit`` -> ``vocoder.decode_features`` over all new
    frames -> ``edit_splice`` against the un-normalised resampled recording: everything outside
    the edits and the ``fade``-sample cross-fades around them is the recording's own samples,
    bit for bit, and a recording that was quieter than ``target_rms`` gets its level back on the
    generated side (gain ``infer.output_gain``).  ``keep_original_audio=False`` returns the
    vocoder's rendering of the whole row (one generated segment through the same splice).

    An item without spans comes back as its resampled input, bitwise, and is not sent to the
    decoder.  Returns ([(1, N_i)] waveforms on the device, {"t", "wav_seconds", "gen_seconds",
    "rtf"}), ``gen_seconds`` the generated audio and ``rtf = t / gen_seconds``.  Mono and
    one-channel Dialog models; the stereo model raises NotImplementedError.

    Items ``(tokens, Recording, spans)`` (``voices.VoiceStore.register_recording``; all of one store, not
    mixed with wav items: a ValueError) skip the front: the features come from one ``VoiceStore.gather`` of
    the recordings, the originals for the splice from the stored waveforms, the gains and ``target_rms`` /
    ``feat_scale`` / ``feat_bias`` from the store."""
    import torch

    from .infer import _prompt_rms_normalise, _prompts_at_rate, output_gain
    from .noise import check_keys

    from .voices import Recording

    if getattr(model.cfg, "stereo", False):
        raise NotImplementedError("edit_batch: the stereo dialog model is not supported")
    dev = model.device
    B = len(items)
    if seeds is not None:
        seeds, _ = check_keys(seeds, None, B)
    by_rec = [isinstance(it[1], Recording) for it in items]
    if any(by_rec):
        if not all(by_rec):
            raise ValueError("a batch is all (tokens, Recording, spans) items or all wavs, not a mix")
        return _edit_recordings(items, model, vocoder, num_step, guidance_scale, t_shift, fade, seeds,
                                keep_original_audio)
    sampling_rate = feature_extractor.config.sampling_rate
    hop = vocoder.cfg.hop_length
    with torch.inference_mode():
        wavs = [w.cpu() for w in _prompts_at_rate(
            [it[1] for it in items], [it[3] if len(it) > 3 else None for it in items], sampling_rate, dev)]
        res: List[Optional[torch.Tensor]] = [None] * B
        todo = [i for i, it in enumerate(items) if len(it[2]) > 0]
        for i in range(B):
            if i not in todo:
                res[i] = wavs[i].to(dev).unsqueeze(0)
        t = gen_samples = 0.0
        if todo:
            Ns = [len(wavs[i]) for i in todo]
            n = max(Ns)
            orig = torch.zeros((len(todo), n), dtype=torch.float32)
            norm = torch.zeros((len(todo), n), dtype=torch.float32)
            rms = []
            for r, i in enumerate(todo):
                orig[r, :Ns[r]] = wavs[i]
                w, v = _prompt_rms_normalise(wavs[i], target_rms)
                norm[r, :Ns[r]] = w
                rms.append(v)
            feats, nfr = feature_extractor.extract_batch(norm.to(dev), torch.tensor(Ns))
            features = (feats + feat_bias) * feat_scale
            L = [int(v) for v in nfr.tolist()]
            spans = [items[i][2] for i in todo]
            plan = plan_edit_batch(L, spans)                # (validates before any solve)
            orig = orig.to(dev)
            torch.cuda.synchronize(dev)
            t0 = dt.datetime.now()
            x1, new_lens, _ = model.sample_edit(
                tokens=[items[i][0] for i in todo], features=features, features_lens=nfr,
                spans=spans, num_step=num_step, guidance_scale=guidance_scale, t_shift=t_shift,
                seeds=None if seeds is None else [seeds[i] for i in todo])
            gen = vocoder.decode_features(x1, new_lens, feat_scale=feat_scale, feat_bias=feat_bias,
                                          clamp=True)
            gen_lens = [int(T) * hop for T in plan.new_lens]
            if keep_original_audio:
                table, row_ptr = sample_table_batch(plan, Ns, hop)
            else:
                table, row_ptr = _stack([np.asarray([(0, 0, g, GENERATED)] if g else [],
                                                    np.int32).reshape(-1, 4) for g in gen_lens], 4)
            gains = [output_gain(v, target_rms) for v in rms]
            out = model.engine.edit_splice(orig, Ns, gen, gen_lens, table, row_ptr, gains, fade)
            torch.cuda.synchronize(dev)
            t = (dt.datetime.now() - t0).total_seconds()
            for r, i in enumerate(todo):
                m = table_length(table[row_ptr[r]:row_ptr[r + 1]])
                res[i] = out[r, :, :m]
                gen_samples += (gen_lens[r] if not keep_original_audio else plan.generated(r) * hop)
    secs = sum(w.shape[-1] for w in res) / sampling_rate
    gsecs = gen_samples / sampling_rate
    return res, {"t": t, "wav_seconds": secs, "gen_seconds": gsecs,
                 "rtf": t / gsecs if gsecs else float("inf")}


def _edit_recordings(items, model, vocoder, num_step, guidance_scale, t_shift, fade, seeds, keep_original_audio):
    """``edit_batch`` over ``(tokens, Recording, spans)`` items: the steps from ``plan_edit_batch`` on, fed
    from the store (features: one gather at the longest recording; gains: the store's, applied to the
    generated waveform on the device before a splice with gains of 1, which evaluates the same product)."""
    import torch

    dev, B = model.device, len(items)
    store = items[0][1].store
    recs = [store.check(it[1]) for it in items]
    sampling_rate, hop = store.sampling_rate, vocoder.cfg.hop_length
    with torch.inference_mode():
        res: List[Optional[torch.Tensor]] = [None] * B
        todo = [i for i, it in enumerate(items) if len(it[2]) > 0]
        for i in range(B):
            if i not in todo:
                res[i] = store.waveform(recs[i]).clone().unsqueeze(0)
        t = gen_samples = 0.0
        if todo:
            sub = [recs[i] for i in todo]
            Ns, L = [r.samples for r in sub], [r.frames for r in sub]
            spans = [items[i][2] for i in todo]
            plan = plan_edit_batch(L, spans)                # (validates before any solve)
            features, gains = store.gather(sub, max(L))
            orig = torch.zeros((len(sub), max(Ns)), dtype=torch.float32, device=dev)
            for r, rec in enumerate(sub):
                orig[r, :Ns[r]] = store.waveform(rec)
            torch.cuda.synchronize(dev)
            t0 = dt.datetime.now()
            x1, new_lens, _ = model.sample_edit(
                tokens=[items[i][0] for i in todo], features=features, features_lens=L,
                spans=spans, num_step=num_step, guidance_scale=guidance_scale, t_shift=t_shift,
                seeds=None if seeds is None else [seeds[i] for i in todo])
            gen = vocoder.decode_features(x1, new_lens, feat_scale=store.feat_scale, feat_bias=store.feat_bias,
                                          clamp=True)
            gen = gen * gains.reshape((-1,) + (1,) * (gen.dim() - 1))
            gen_lens = [int(T) * hop for T in plan.new_lens]
            if keep_original_audio:
                table, row_ptr = sample_table_batch(plan, Ns, hop)
            else:
                table, row_ptr = _stack([np.asarray([(0, 0, g, GENERATED)] if g else [],
                                                    np.int32).reshape(-1, 4) for g in gen_lens], 4)
            out = model.engine.edit_splice(orig, Ns, gen, gen_lens, table, row_ptr, None, fade)
            torch.cuda.synchronize(dev)
            t = (dt.datetime.now() - t0).total_seconds()
            for r, i in enumerate(todo):
                m = table_length(table[row_ptr[r]:row_ptr[r + 1]])
                res[i] = out[r, :, :m]
                gen_samples += (gen_lens[r] if not keep_original_audio else plan.generated(r) * hop)
    secs = sum(w.shape[-1] for w in res) / sampling_rate
    gsecs = gen_samples / sampling_rate
    return res, {"t": t, "wav_seconds": secs, "gen_seconds": gsecs,
                 "rtf": t / gsecs if gsecs else float("inf")}


def edit_sentence(tokens: List[int], wav, spans, model, vocoder, feature_extractor,
                  sampling_rate: Optional[int] = None, seed: Optional[int] = None, **kw):
    """One recording through ``edit_batch``: (wav (1, N) on the device, metrics)."""
    item = (tokens, wav, spans) if sampling_rate is None else (tokens, wav, spans, sampling_rate)
    res, met = edit_batch([item], model, vocoder, feature_extractor,
                          seeds=None if seed is None else [seed], **kw)
    return res[0], met
