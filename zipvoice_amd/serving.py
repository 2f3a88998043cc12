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
from typing import List, Optional, Tuple

import numpy as np
import torch

from .common import predict_features_lens, to_device
from .feature import compute_num_frames
from .infer import _prepare_prompts, _resampler
from .models import per_row_schedule, split_prompt
from .noise import check_keys, seeded_normal, seeded_normal_into
from .voices import Voice


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
    ``target_rms`` / ``feat_scale`` / ``feat_bias`` must be the batcher's."""

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
        # slot -> (ticket, frames, prompt frames, prompt rms: a host float, or the output gain on the device)
        self._rows = {}
        self._next_ticket = 0
        self._done: List[Tuple[int, torch.Tensor]] = []      # retired, not yet returned by step()
        self.last_mel: List[Tuple[int, torch.Tensor]] = []   # (ticket, mel (T_i, n_mels)) of the last retire

    def close(self) -> None:
        """Close the session; the requests still queued are given up (their voices are free to be dropped)."""
        while self._queue:
            item = self._queue.popleft()[1]
            if isinstance(item[1], Voice):
                self.voices.release(item[1])
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
        self._queue.append((ticket, item, int(num_step), float(guidance_scale), float(speed), float(t_shift), seed,
                            total))
        return ticket

    def pending(self) -> Tuple[int, int]:
        """(queued, in-flight) request counts."""
        return len(self._queue), len(self._rows)

    @torch.inference_mode()
    def _retire(self) -> List[Tuple[int, torch.Tensor]]:
        left = self.session.steps_left()
        slots = [s for s in sorted(self._rows) if left[s] == 0]
        if not slots:
            return []
        dev = self.model.device
        rows = [self._rows.pop(s) for s in slots]
        x1 = self.session.retire(slots)
        plens = to_device(torch.tensor([r[2] for r in rows]), dev)
        glens = to_device(torch.tensor([r[1] - r[2] for r in rows]), dev)
        pred, pred_lens, _ = split_prompt(x1, plens, glens, max(r[1] - r[2] for r in rows), max(r[2] for r in rows))
        wav = self.vocoder.decode_features(pred, pred_lens, feat_scale=self.feat_scale, feat_bias=self.feat_bias,
                                           clamp=True)
        hop = self.vocoder.cfg.hop_length
        out, self.last_mel = [], []
        for i, (ticket, frames, p, rms) in enumerate(rows):
            w = wav[i, :(frames - p) * hop]
            if torch.is_tensor(rms):                      # a voice's row: its gain, already on the device
                w = w * rms
            elif rms < self.target_rms:
                w = w * rms / self.target_rms
            out.append((ticket, w.unsqueeze(0)))
            self.last_mel.append((ticket, pred[i, :frames - p]))
        return out

    @torch.inference_mode()
    def _admit(self) -> None:
        left = self.session.steps_left()
        free = [s for s in range(self.max_rows) if left[s] < 0]
        n = min(len(free), len(self._queue))
        if n == 0:
            return
        # (a group is all voices or all wavs: the leading run of the kind at the head of the queue)
        by_voice = isinstance(self._queue[0][1][1], Voice)
        n = next((i for i in range(n) if isinstance(self._queue[i][1][1], Voice) != by_voice), n)
        # (the requests stay queued until the session has taken them: a failure below loses none)
        reqs = [self._queue[i] for i in range(n)]
        if by_voice:
            return self._admit_voices(reqs, free[:n])
        m, dev = self.model, self.model.device
        items = [r[1] for r in reqs]
        feats, nfr, rms, _ = _prepare_prompts(items, self.fx, self.target_rms, dev)
        prompt_features = (feats + self.feat_bias) * self.feat_scale
        schedule, speeds = per_row_schedule(n, num_step=[r[2] for r in reqs], guidance_scale=[r[3] for r in reqs],
                                            speed=[r[4] for r in reqs], t_shift=[r[5] for r in reqs])
        tc, pm = m.forward_text_inference_ratio_duration(
            tokens=[it[0] for it in items], prompt_tokens=[it[1] for it in items], prompt_features_lens=nfr,
            speed=torch.tensor(speeds, dtype=torch.float32, device=dev))
        T_in = tc.shape[1]
        sc = m.engine.speech_condition(prompt_features, nfr, T_in)
        lens = (~pm).sum(-1).tolist()
        long = [i for i, v in enumerate(lens) if v > self.max_frames]
        if long:                                          # submit's host count was short: drop it, keep the rest queued
            del self._queue[long[0]]
            raise ValueError(f"request {reqs[long[0]][0]} has {lens[long[0]]} frames, more than max_frames "
                             f"({self.max_frames}); it was dropped")
        F = prompt_features.size(-1)
        seeds = [r[6] for r in reqs]
        if all(s is not None for s in seeds):
            x0 = seeded_normal(seeds, (T_in, F), device=dev)
        else:
            x0 = torch.randn(n, T_in, F, device=dev)
            keyed = [i for i, s in enumerate(seeds) if s is not None]
            if keyed:
                x0[keyed] = seeded_normal([seeds[i] for i in keyed], (T_in, F), device=dev)
        slots = free[:n]
        self.session.admit(slots, x0, tc, sc, lens, schedule)
        for _ in range(n):
            self._queue.popleft()
        for s, r, frames, p, q in zip(slots, reqs, lens, nfr.tolist(), rms):
            self._rows[s] = (r[0], frames, int(p), q)

    def _admit_voices(self, reqs, slots) -> None:
        """Admission of a group whose requests all carry voices.  Nothing is read back from the device:
        the lengths are ``submit``'s host counts (the device evaluates the same fp32 expression for the text
        condition), the speech condition and the gains come from the store, and every host value goes up
        through pinned memory."""
        m, dev, n = self.model, self.model.device, len(reqs)
        voices = [r[1][1] for r in reqs]
        lens = [r[7] for r in reqs]
        T_in = max(lens)
        schedule, speeds = per_row_schedule(n, num_step=[r[2] for r in reqs], guidance_scale=[r[3] for r in reqs],
                                            speed=[r[4] for r in reqs], t_shift=[r[5] for r in reqs])
        tc, _ = m.forward_text_inference_ratio_duration(
            tokens=[r[1][0] for r in reqs], prompt_tokens=[list(v.prompt_tokens) for v in voices],
            prompt_features_lens=to_device(torch.tensor([v.frames for v in voices]), dev),
            speed=to_device(torch.tensor(speeds, dtype=torch.float32), dev), num_frames=T_in)
        sc, gains = self.voices.gather(voices, T_in)
        seeds = [r[6] for r in reqs]
        if all(s is not None for s in seeds):
            x0 = seeded_normal(seeds, (T_in, sc.size(-1)), device=dev)
        else:
            x0 = torch.randn(n, T_in, sc.size(-1), device=dev)
            for i, s in enumerate(seeds):
                if s is not None:
                    seeded_normal_into(x0[i:i + 1], [s])
        self.session.admit(slots, x0, tc, sc, lens, schedule)
        for s, r, v, frames, i in zip(slots, reqs, voices, lens, range(n)):
            self._queue.popleft()
            self.voices.release(v)
            self._rows[s] = (r[0], frames, v.frames, gains[i])

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
