"""Continuous batching for serving: requests enter and leave a running solve between decoder steps.

``ContinuousBatcher`` keeps one ``engine.SolveSession`` of ``max_rows`` slots.  Every ``step()`` retires
the rows whose steps are done (prompt split, vocoder and RMS restore as one batch), admits queued
requests into the free slots in arrival order (prompt features, text and speech conditions and the
initial noise as one batch per admitted group) and runs one tick, in which every row in flight
advances one Euler step on its own grid.  A request therefore waits at most one decoder step before it
starts, whatever else is running, and the decoder batch stays as full as the queue allows.

Each request ends as ``infer.generate_sentence`` would leave it with the same initial noise; two
requests admitted together before the first tick run the decoder batches of ``infer.generate_batch``
with per-item settings.  The reference has no counterpart.
"""
from __future__ import annotations

import collections
from typing import List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from .common import predict_features_lens, to_device
from .feature import compute_num_frames
from .edit import GENERATED, _stack, plan_edit, sample_table, table_length
from .infer import _finish_row, _prepare_prompts, _resampler
from .models import per_row_schedule, split_prompt
from .noise import check_keys, initial_noise
from .voices import Recording, Voice


class _Request(NamedTuple):
    """Queued.  ``item``: (tokens, prompt_tokens, prompt_wav[, rate]) or (tokens, Voice); ``total``: ``_frames``'s."""
    ticket: int
    item: tuple
    num_step: int
    guidance_scale: float
    speed: float
    t_shift: float
    seed: Optional[int]
    total: int


class _EditRequest(NamedTuple):
    """A queued edit, and the same tuple in flight.  ``table``: the row's frame table (``edit.plan_edit``),
    ``total`` the new length it tiles."""
    ticket: int
    tokens: list
    recording: Recording
    table: np.ndarray
    total: int
    num_step: int
    guidance_scale: float
    t_shift: float
    seed: Optional[int]
    fade: int
    keep_original_audio: bool


def _kind(req) -> str:
    """The admission group a queued request belongs to."""
    if isinstance(req, _EditRequest):
        return "edit"
    return "voice" if isinstance(req.item[1], Voice) else "wav"


class _Row(NamedTuple):
    """In flight.  ``level`` (``infer._finish_row``): the prompt's RMS on the host, or a voice's gain on the device."""
    ticket: int
    frames: int
    prompt_frames: int
    level: Union[float, torch.Tensor]


class ContinuousBatcher:
    """``submit`` queues a request and returns its ticket; ``step`` retires, admits and ticks, returning
    ``[(ticket, wav (1, N))]`` of the requests that have finished; ``drain`` steps until nothing is left.
    ``last_mel`` holds ``(ticket, mel (T_i, n_mels))`` of the rows the last retiring step returned, before
    the vocoder.  ``max_frames`` bounds a request's prompt + generated frames.

    ``padding`` (``None``: leave the model's mode; ``"batch"`` / ``"row"``: set ``model.padding``, which is
    engine-wide, so it also holds for every other call on the model).  In ``"row"`` mode a request's
    features depend on its own frames only: the same request and seed give the same result, to rounding,
    whatever else is in flight.  In ``"batch"`` mode a row whose length is no multiple of 4 ends
    differently depending on the tick's length (``DESIGN.md`` section 3, "Padding").

    ``voices`` (a ``voices.VoiceStore``): ``submit(tokens, voice=...)`` then takes a registered voice in
    place of ``prompt_tokens`` and ``prompt_wav``.  A group of such requests is admitted without preparing
    a prompt and without reading anything back from the device: the speech condition and the output gains
    come from ``VoiceStore.gather``, the lengths from the host count ``submit`` made.  The store's
    ``target_rms`` / ``feat_scale`` / ``feat_bias`` must be the batcher's.

    ``submit_edit(tokens, recording, spans)`` queues a speech edit of a recording registered in the store
    (``VoiceStore.register_recording``): the edit joins the running solve like any other request.  Its row
    enters its slot straight from the store's arena (``SolveSession.admit_edit``) and leaves it the same
    way (``retire_edit``), the generated frames go through the vocoder and are spliced into the stored
    waveform (``edit_splice``); every length is known on the host from the plan, so nothing is read back.
    The recording is held from ``submit_edit`` until its row has been retired."""

    def __init__(self, model, vocoder, feature_extractor, max_rows: int, max_frames: int,
                 target_rms: float = 0.1, feat_scale: float = 0.1, feat_bias: float = 0.0,
                 padding: Optional[str] = None, voices=None):
        self.model, self.vocoder, self.fx = model, vocoder, feature_extractor
        if padding is not None:               # engine-wide: every other user of the model follows it
            model.padding = padding
        self.max_rows, self.max_frames = int(max_rows), int(max_frames)
        self.target_rms, self.feat_scale, self.feat_bias = target_rms, feat_scale, feat_bias
        if voices is not None and (voices.target_rms, voices.feat_scale, voices.feat_bias) != (
                float(target_rms), feat_scale, feat_bias):
            raise ValueError("the voice store was filled with another target_rms / feat_scale / feat_bias")
        self.voices = voices
        self.session = model.solver.open_session(self.max_rows, self.max_frames)
        self._queue = collections.deque()
        self._rows = {}                                      # slot -> _Row
        self._next_ticket = 0
        self._done: List[Tuple[int, torch.Tensor]] = []      # retired, not yet returned by step()
        self.last_mel: List[Tuple[int, torch.Tensor]] = []   # (ticket, mel (T_i, n_mels)) of the last retire

    def close(self) -> None:
        """Close the session; the requests still queued are given up (their voices are free to be dropped)."""
        while self._queue:
            req = self._queue.popleft()
            if isinstance(req, _EditRequest):
                self.voices.release(req.recording)
            elif isinstance(req.item[1], Voice):
                self.voices.release(req.item[1])
        for row in self._rows.values():                       # (edits in flight are given up too)
            if isinstance(row, _EditRequest):
                self.voices.release(row.recording)
        self._rows = {}
        self.session.close()

    def _frames(self, tokens, prompt_tokens, prompt_wav, prompt_sampling_rate, speed, voice=None) -> Tuple[int, int]:
        """(prompt frames, predicted frames of prompt + text) of a request, on the host."""
        if voice is not None:
            p = voice.frames
        else:
            cfg = self.fx.config
            n = int(np.asarray(prompt_wav).size) if not torch.is_tensor(prompt_wav) else int(prompt_wav.numel())
            if prompt_sampling_rate is not None and int(prompt_sampling_rate) != cfg.sampling_rate:
                n = _resampler(int(prompt_sampling_rate), cfg.sampling_rate).plan.out_len(n)
            p = compute_num_frames(n, cfg.hop_length)
        total = predict_features_lens(torch.tensor([p]), torch.tensor([len(prompt_tokens)]),
                                      torch.tensor([len(tokens)]), float(speed))
        return p, int(total[0])

    def submit(self, tokens, prompt_tokens=None, prompt_wav=None, prompt_sampling_rate=None, num_step: int = 16,
               guidance_scale: float = 1.0, speed: float = 1.0, t_shift: float = 0.5,
               seed: Optional[int] = None, voice: Optional[Voice] = None) -> int:
        """Queue one request, with its prompt (``prompt_tokens``, ``prompt_wav``) or a registered ``voice`` of
        the batcher's store; returns its ticket.  A request longer than ``max_frames`` is a ValueError."""
        if seed is not None:
            check_keys([seed], None, 1)
        if int(num_step) < 1:
            raise ValueError("num_step must be at least 1")
        if voice is not None:
            if prompt_tokens is not None or prompt_wav is not None:
                raise ValueError("give a voice or a prompt, not both")
            if self.voices is None:
                raise ValueError("this batcher has no voice store (ContinuousBatcher(voices=...))")
            self.voices.check(voice)
            p, total = self._frames(tokens, voice.prompt_tokens, None, None, speed, voice=voice)
        elif prompt_tokens is None or prompt_wav is None:
            raise ValueError("a request needs prompt_tokens and prompt_wav, or a voice")
        else:
            p, total = self._frames(tokens, prompt_tokens, prompt_wav, prompt_sampling_rate, speed)
        if total > self.max_frames:
            raise ValueError(f"request of {total} frames exceeds the batcher's max_frames ({self.max_frames})")
        ticket = self._next_ticket
        self._next_ticket += 1
        if voice is not None:
            item = (list(tokens), voice)
            self.voices.hold(voice)                       # (until admitted: drop() refuses meanwhile)
        else:
            item = (list(tokens), list(prompt_tokens), prompt_wav) + (
                () if prompt_sampling_rate is None else (int(prompt_sampling_rate),))
        self._queue.append(_Request(ticket, item, int(num_step), float(guidance_scale), float(speed), float(t_shift),
                                    seed, total))
        return ticket

    def submit_edit(self, tokens, recording: Recording, spans, num_step: int = 16, guidance_scale: float = 1.0,
                    t_shift: float = 0.5, seed: Optional[int] = None, fade: int = 240,
                    keep_original_audio: bool = True) -> int:
        """Queue one edit of ``recording`` (``VoiceStore.register_recording``): ``tokens`` the whole new
        transcript, ``spans`` the ``(s, e, n)`` spans in feature frames (``edit.plan_edit``); returns its
        ticket.  Everything the host can know is checked here: the spans, the new length against
        ``max_frames``, the recording, the seed.  A request without spans never reaches the session: the next
        ``step()`` returns the recording's waveform, bitwise."""
        if getattr(self.model.cfg, "stereo", False):
            raise NotImplementedError("submit_edit: the stereo dialog model is not supported")
        if seed is not None:
            check_keys([seed], None, 1)
        if int(num_step) < 1:
            raise ValueError("num_step must be at least 1")
        if int(fade) < 0:
            raise ValueError("fade must be non-negative")
        if self.voices is None:
            raise ValueError("this batcher has no voice store (ContinuousBatcher(voices=...))")
        if not isinstance(recording, Recording):
            raise ValueError(f"expected a Recording, got {type(recording).__name__}")
        self.voices.check(recording)
        table = plan_edit(recording.frames, spans)
        total = table_length(table)
        if total > self.max_frames:
            raise ValueError(f"edit of {total} frames exceeds the batcher's max_frames ({self.max_frames})")
        ticket = self._next_ticket
        self._next_ticket += 1
        if len(spans) == 0:
            self._done.append((ticket, self.voices.waveform(recording).clone().unsqueeze(0)))
            return ticket
        if total < 1:
            raise ValueError("the edit deletes the whole recording")
        self.voices.hold(recording)                       # (until retired: drop() refuses meanwhile)
        self._queue.append(_EditRequest(ticket, list(tokens), recording, table, total, int(num_step),
                                        float(guidance_scale), float(t_shift), seed, int(fade),
                                        bool(keep_original_audio)))
        return ticket

    def pending(self) -> Tuple[int, int]:
        """(queued, in-flight) request counts."""
        return len(self._queue), len(self._rows)

    @torch.inference_mode()
    def _retire(self) -> List[Tuple[int, torch.Tensor]]:
        left = self.session.steps_left()
        finished = [s for s in sorted(self._rows) if left[s] == 0]
        slots = [s for s in finished if not isinstance(self._rows[s], _EditRequest)]
        edits = [s for s in finished if isinstance(self._rows[s], _EditRequest)]
        self.last_mel = [] if finished else self.last_mel
        out = self._retire_generated(slots) if slots else []
        if edits:
            try:
                out += self._retire_edits(edits)
            except Exception:
                self._done += out                             # (retired already: the next step returns them)
                raise
        return out

    def _retire_generated(self, slots) -> List[Tuple[int, torch.Tensor]]:
        dev = self.model.device
        rows = [self._rows.pop(s) for s in slots]
        x1 = self.session.retire(slots)
        plens = to_device(torch.tensor([r.prompt_frames for r in rows]), dev)
        gen = [r.frames - r.prompt_frames for r in rows]
        pred, pred_lens, _ = split_prompt(x1, plens, to_device(torch.tensor(gen), dev), max(gen),
                                          max(r.prompt_frames for r in rows))
        wav = self.vocoder.decode_features(pred, pred_lens, feat_scale=self.feat_scale, feat_bias=self.feat_bias,
                                           clamp=True)
        self.last_mel = self.last_mel + [(r.ticket, pred[i, :n]) for i, (r, n) in enumerate(zip(rows, gen))]
        return [(r.ticket, _finish_row(wav[i], n * self.vocoder.cfg.hop_length, r.level, self.target_rms))
                for i, (r, n) in enumerate(zip(rows, gen))]

    def _edit_tables(self, rows):
        """(offsets, original lengths, frame table, row_ptr) of a group of edit rows, host arrays."""
        table, row_ptr = _stack([r.table for r in rows], 3)
        return [r.recording.offset for r in rows], [r.recording.frames for r in rows], table, row_ptr

    def _retire_edits(self, slots) -> List[Tuple[int, torch.Tensor]]:
        """The finished edit rows as one group: ``retire_edit`` from the arena, the vocoder over all new
        frames, the store's gain on the device, the splice against the stored waveforms."""
        rows = [self._rows[s] for s in slots]
        store, hop = self.voices, self.vocoder.cfg.hop_length
        offsets, lens, table, row_ptr = self._edit_tables(rows)
        # (the features keep the original frames whatever keep_original_audio says, as edit_batch's)
        x1, _ = self.session.retire_edit(slots, store.arena, offsets, lens, table, row_ptr)
        for s in slots:
            del self._rows[s]
        new_lens = [r.total for r in rows]
        gen = self.vocoder.decode_features(x1, to_device(torch.tensor(new_lens), self.model.device),
                                           feat_scale=self.feat_scale, feat_bias=self.feat_bias, clamp=True)
        # zv_edit_splice takes host gains; the store's are on the device, so the generated waveform is
        # scaled here and spliced with gains of 1 (its g * x * (1 - w) evaluates g * x first: the same bits)
        gains = torch.index_select(store.gains, 0, to_device(torch.tensor(offsets), store.gains.device))
        gen = gen * gains.reshape((-1,) + (1,) * (gen.dim() - 1))
        gen_lens = [n * hop for n in new_lens]
        Ns = [r.recording.samples for r in rows]
        tabs = [sample_table(r.table, N, hop, r.recording.frames) if r.keep_original_audio else
                np.asarray([(0, 0, g, GENERATED)], np.int32).reshape(-1, 4) for r, N, g in zip(rows, Ns, gen_lens)]
        stab, sptr = _stack(tabs, 4)
        orig = torch.zeros((len(rows), max(Ns)), dtype=torch.float32, device=self.model.device)
        for i, r in enumerate(rows):
            orig[i, :Ns[i]] = store.waveform(r.recording)
        fades = sorted(set(r.fade for r in rows))
        outs = {f: self.model.engine.edit_splice(orig, Ns, gen, gen_lens, stab, sptr, None, f) for f in fades}
        self.last_mel = self.last_mel + [(r.ticket, x1[i, :n]) for i, (r, n) in enumerate(zip(rows, new_lens))]
        res = []
        for i, r in enumerate(rows):
            store.release(r.recording)
            res.append((r.ticket, outs[r.fade][i, :, :table_length(tabs[i])]))
        return res

    def _admit_edits(self, free, reqs) -> None:
        """A group of edit requests into the free slots: the ground-truth-duration text condition over the
        plan's lengths, the seeded noise, and ``admit_edit`` straight from the store's arena."""
        m, dev, n = self.model, self.model.device, len(reqs)
        schedule, _ = per_row_schedule(n, num_step=[r.num_step for r in reqs],
                                       guidance_scale=[r.guidance_scale for r in reqs], speed=[1.0] * n,
                                       t_shift=[r.t_shift for r in reqs])
        new_lens = [r.total for r in reqs]
        embed, tokens_lens = m.forward_text_embed([r.tokens for r in reqs])
        tc, _ = m.forward_text_condition(embed, tokens_lens, to_device(torch.tensor(new_lens), dev),
                                         num_frames=max(new_lens))
        x0 = initial_noise(n, max(new_lens), self.voices.n_mels, dev, seeds=[r.seed for r in reqs])
        offsets, lens, table, row_ptr = self._edit_tables(reqs)
        self.session.admit_edit(free[:n], x0, tc, self.voices.arena, offsets, lens, table, row_ptr, schedule)
        for s, r in zip(free, reqs):
            self._queue.popleft()
            self._rows[s] = r                               # (the recording stays held until retirement)

    @torch.inference_mode()
    def _admit(self) -> None:
        left = self.session.steps_left()
        free = [s for s in range(self.max_rows) if left[s] < 0]
        n = min(len(free), len(self._queue))
        if n == 0:
            return
        # (a group is all voices, all wavs or all edits: the leading run of the kind at the head of the queue)
        kind = _kind(self._queue[0])
        by_voice = kind == "voice"
        n = next((i for i in range(n) if _kind(self._queue[i]) != kind), n)
        # (the requests stay queued until the session has taken them: a failure below loses none)
        reqs = [self._queue[i] for i in range(n)]
        if kind == "edit":
            return self._admit_edits(free, reqs)
        m, dev = self.model, self.model.device
        schedule, speeds = per_row_schedule(n, num_step=[r.num_step for r in reqs],
                                            guidance_scale=[r.guidance_scale for r in reqs],
                                            speed=[r.speed for r in reqs], t_shift=[r.t_shift for r in reqs])

        def text(prompt_tokens, prompt_frames, num_frames=None):
            return m.forward_text_inference_ratio_duration(
                tokens=[r.item[0] for r in reqs], prompt_tokens=prompt_tokens, prompt_features_lens=prompt_frames,
                speed=to_device(torch.tensor(speeds, dtype=torch.float32), dev), num_frames=num_frames)

        tc, sc, lens, prompt_frames, level = (self._voice_group if by_voice else self._wav_group)(reqs, text)
        x0 = initial_noise(n, tc.shape[1], sc.size(-1), dev, seeds=[r.seed for r in reqs])
        self.session.admit(free[:n], x0, tc, sc, lens, schedule)
        for i, (s, r) in enumerate(zip(free, reqs)):
            self._queue.popleft()
            if by_voice:
                self.voices.release(r.item[1])
            self._rows[s] = _Row(r.ticket, lens[i], prompt_frames[i], level[i])

    def _wav_group(self, reqs, text):
        """(text condition, speech condition, frames, prompt frames, the prompts' RMS) of a group whose
        requests carry prompt wavs: the prompts prepared as ``infer.generate_batch`` prepares them, the lengths
        read back from the text condition's mask."""
        items = [r.item for r in reqs]
        prompt_features, nfr, rms, _ = _prepare_prompts(items, self.fx, self.target_rms, self.feat_scale,
                                                        self.feat_bias, self.model.device)
        tc, pm = text([it[1] for it in items], nfr)
        sc = self.model.engine.speech_condition(prompt_features, nfr, tc.shape[1])
        lens = (~pm).sum(-1).tolist()
        long = [i for i, v in enumerate(lens) if v > self.max_frames]
        if long:                                          # submit's host count was short: drop it, keep the rest queued
            del self._queue[long[0]]
            raise ValueError(f"request {reqs[long[0]].ticket} has {lens[long[0]]} frames, more than max_frames "
                             f"({self.max_frames}); it was dropped")
        return tc, sc, lens, nfr.tolist(), rms

    def _voice_group(self, reqs, text):
        """The same of a group whose requests all carry voices, their output gains on the device as the level.
        Nothing is read back: the lengths are ``submit``'s host counts (the device evaluates the same fp32
        expression for the text condition), the speech condition and the gains come from the store, and every
        host value goes up through pinned memory."""
        voices = [r.item[1] for r in reqs]
        lens = [r.total for r in reqs]
        frames = [v.frames for v in voices]
        tc, _ = text([list(v.prompt_tokens) for v in voices], to_device(torch.tensor(frames), self.model.device),
                     max(lens))
        sc, gains = self.voices.gather(voices, max(lens))
        return tc, sc, lens, frames, gains

    def step(self) -> List[Tuple[int, torch.Tensor]]:
        """Retire the finished rows, admit queued requests into the free slots, run one tick.
        Returns [(ticket, wav (1, N) on the device)] of the requests finished by the previous ticks."""
        self._done += self._retire()                      # (kept if the admission below raises: the next step returns them)
        self._admit()
        self.session.step()
        done, self._done = self._done, []
        return done

    def drain(self) -> List[Tuple[int, torch.Tensor]]:
        """Step until the queue and the session are empty; every remaining result, in finishing order."""
        out = []
        while self._queue or self._rows or self._done:
            out += self.step()
        return out
