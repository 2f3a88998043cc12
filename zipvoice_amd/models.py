"""Drop-in mirrors of the reference's inference model classes.

Same class names, constructor keywords, method names, argument meanings and
return tuples as ``zipvoice/models/zipvoice.py`` (ZipVoice),
``zipvoice_distill.py`` (ZipVoiceDistill) and ``zipvoice_dialog.py``
(ZipVoiceDialog, ZipVoiceDialogStereo), restricted to inference.  The compute
of every method runs in the HIP engine (``engine.HipEngine``); this module only
does host-side integer glue (token lists -> padded ids / lengths / masks),
exactly where the reference does it on the host.

Usage (mirrors ``infer_zipvoice.py:549-577``)::

    model = ZipVoice(**model_json["model"], vocab_size=V, pad_id=0)
    model.load_state_dict(state_dict)        # reference key names, strict
    model = model.to("cuda:0").eval()
    pred, pred_lens, prompt, prompt_lens = model.sample(tokens=..., ...)
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .common import make_pad_mask, pad_labels, predict_features_lens, speaker_turn_indices, to_device
from .config import ModelConfig
from .engine import HipEngine, padding_id
from .noise import check_noise, initial_noise
from .solver import DistillEulerSolver, EulerSolver, RowSchedule
from .weights import check_state_dict, load_checkpoint_state_dict, synthetic_state_dict


class ZipVoice:
    """The ZipVoice model (inference), zipvoice.py:35-486."""

    variant = "zipvoice"
    solver_cls = EulerSolver

    def __init__(self, fm_decoder_downsampling_factor: List[int] = [1, 2, 4, 2, 1],
                 fm_decoder_num_layers: List[int] = [2, 2, 4, 4, 4],
                 fm_decoder_cnn_module_kernel: List[int] = [31, 15, 7, 15, 31],
                 fm_decoder_feedforward_dim: int = 1536, fm_decoder_num_heads: int = 4,
                 fm_decoder_dim: int = 512, text_encoder_num_layers: int = 4,
                 text_encoder_feedforward_dim: int = 512, text_encoder_cnn_module_kernel: int = 9,
                 text_encoder_num_heads: int = 4, text_encoder_dim: int = 192,
                 time_embed_dim: int = 192, text_embed_dim: int = 192, query_head_dim: int = 32,
                 value_head_dim: int = 12, pos_head_dim: int = 4, pos_dim: int = 48,
                 feat_dim: int = 100, vocab_size: int = 26, pad_id: int = 0,
                 precision: str = "fp32", padding: str = "batch", **extra):
        self.cfg = ModelConfig(
            fm_decoder_downsampling_factor=list(fm_decoder_downsampling_factor),
            fm_decoder_num_layers=list(fm_decoder_num_layers),
            fm_decoder_cnn_module_kernel=list(fm_decoder_cnn_module_kernel),
            fm_decoder_feedforward_dim=fm_decoder_feedforward_dim,
            fm_decoder_num_heads=fm_decoder_num_heads, fm_decoder_dim=fm_decoder_dim,
            text_encoder_num_layers=text_encoder_num_layers,
            text_encoder_feedforward_dim=text_encoder_feedforward_dim,
            text_encoder_cnn_module_kernel=text_encoder_cnn_module_kernel,
            text_encoder_num_heads=text_encoder_num_heads, text_encoder_dim=text_encoder_dim,
            time_embed_dim=time_embed_dim, text_embed_dim=text_embed_dim,
            query_head_dim=query_head_dim, value_head_dim=value_head_dim,
            pos_head_dim=pos_head_dim, pos_dim=pos_dim, feat_dim=feat_dim,
            vocab_size=vocab_size, pad_id=pad_id, variant=self.variant,
            **{k: v for k, v in extra.items() if k in ("spk_a_id", "spk_b_id")})
        unknown = set(extra) - {"spk_a_id", "spk_b_id"}
        if unknown:
            raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
        self.feat_dim = feat_dim
        self.text_embed_dim = text_embed_dim
        self.pad_id = pad_id
        self.precision = precision
        padding_id(padding)                    # (ValueError for anything but "batch" / "row")
        self._padding = padding                # remembered until the engine exists, and across rebuilds
        self._state: Optional[Dict[str, np.ndarray]] = None
        self.engine: Optional[HipEngine] = None
        self.device = torch.device("cpu")
        self.solver = self.solver_cls(self, func_name="forward_fm_decoder")

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict: bool = True):
        sd = {}
        for k, v in state_dict.items():
            if k.startswith("module."):
                k = k[len("module."):]
            if isinstance(v, torch.Tensor):
                v = v.detach().to("cpu", torch.float32).numpy()
            sd[k] = np.asarray(v, np.float32)
        if not strict:
            raise NotImplementedError("only strict=True loading is supported")
        check_state_dict(self.cfg, sd)
        self._state = sd
        if self.engine is not None:
            self._build_engine(self.engine.device)
        return self

    def load_checkpoint(self, path: str):
        """checkpoint.py:108-146 / infer_zipvoice.py:561-566 (.pt or .safetensors)."""
        return self.load_state_dict(load_checkpoint_state_dict(path))

    def load_synthetic(self, seed: int = 0):
        """Deterministic synthetic weights (no pretrained weights offline)."""
        return self.load_state_dict(synthetic_state_dict(self.cfg, seed))

    def _build_engine(self, device):
        if self._state is None:
            raise RuntimeError("load_state_dict() must be called before moving to a GPU")
        self.engine = HipEngine(self.cfg, self._state, precision=self.precision, device=device)
        self.engine.padding = self._padding
        self.device = self.engine.device

    @property
    def padding(self) -> str:
        """The decoder's padding mode, engine-wide (``HipEngine.padding``).  ``"batch"`` (default):
        the reference's behaviour on a padded batch, where a row whose length is no multiple of the
        decoder's downsampling factors depends on the padded length and on what lies past its end.
        ``"row"``: every row is integrated as it would be alone at its own length.  Every entry that
        runs the decoder follows it (``sample``, ``sample_edit``, ``sample_intermediate``,
        ``forward_fm_decoder``, the ``infer`` / ``longform`` / ``edit`` generators)."""
        return self._padding

    @padding.setter
    def padding(self, mode: str) -> None:
        padding_id(mode)
        if self.engine is not None:
            self.engine.padding = mode
        self._padding = mode

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("zipvoice_amd runs on ROCm GPUs only (no CPU fallback)")
        self._build_engine(device)
        self._state = self._state  # keep host copy for re-targeting
        return self

    def cuda(self, index: int = 0):
        return self.to(torch.device("cuda", index))

    def eval(self):
        return self

    def parameters_count(self) -> int:
        return int(sum(v.size for v in self._state.values())) if self._state else 0

    def _need_engine(self):
        if self.engine is None:
            raise RuntimeError("model is not on a GPU: call .to('cuda')")
        return self.engine

    # ------------------------------------------------------------------ decoder
    def forward_fm_decoder(self, t: torch.Tensor, xt: torch.Tensor, text_condition: torch.Tensor,
                           speech_condition: torch.Tensor,
                           padding_mask: Optional[torch.Tensor] = None,
                           guidance_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """zipvoice.py:135-185: velocity of the raw decoder (no CFG)."""
        eng = self._need_engine()
        if not torch.is_tensor(t):
            t = torch.tensor(float(t))
        assert t.dim() in (0, 1, 3)
        if guidance_scale is not None and not torch.is_tensor(guidance_scale):
            guidance_scale = torch.tensor(float(guidance_scale))
        if self.cfg.distill and guidance_scale is None:
            raise ValueError("ZipVoiceDistill.forward_fm_decoder needs guidance_scale")
        return eng.fm_decoder(t.reshape(-1), xt, text_condition, speech_condition, padding_mask,
                              guidance_scale.reshape(-1) if (guidance_scale is not None
                                                            and self.cfg.distill) else None)

    # ------------------------------------------------------------------ text side
    def forward_text_embed(self, tokens: List[List[int]]):
        """zipvoice.py:187-212 (dialog: + speaker-turn embeddings, zipvoice_dialog.py:127-159)."""
        eng = self._need_engine()
        tokens_padded = pad_labels(tokens, pad_id=self.pad_id, device=self.device)
        tokens_lens = to_device(torch.tensor([len(t) for t in tokens], dtype=torch.int64), self.device)
        # (make_pad_mask's values at the padded width, which is past every length, without its read
        # of the longest length back from the device)
        pm = torch.arange(tokens_padded.shape[1], device=self.device)[None] >= tokens_lens[:, None]
        spk = None
        if self.cfg.dialog:
            spk = speaker_turn_indices(tokens_padded, self.cfg.spk_a_id, self.cfg.spk_b_id,
                                       self.pad_id)
        embed = eng.text_encode(tokens_padded, pm, spk)
        return embed, tokens_lens

    def forward_text_condition(self, embed: torch.Tensor, tokens_lens: torch.Tensor,
                               features_lens: torch.Tensor, num_frames: Optional[int] = None):
        """zipvoice.py:214-251.  ``num_frames`` (extra, optional): the longest of ``features_lens`` when
        the caller knows it on the host; nothing is then read back from the device."""
        eng = self._need_engine()
        if num_frames is None:
            num_frames = int(features_lens.max())
            padding_mask = make_pad_mask(features_lens.to(self.device), max_len=num_frames)
        else:
            num_frames = int(num_frames)
            padding_mask = (torch.arange(num_frames, device=self.device)[None]
                            >= features_lens.to(self.device)[:, None])
        tc = eng.text_condition(embed, tokens_lens, features_lens, num_frames)
        return tc, padding_mask

    def forward_text_inference_gt_duration(self, tokens, features_lens, prompt_tokens,
                                           prompt_features_lens):
        """zipvoice.py:270-288."""
        tokens = [p + t for p, t in zip(prompt_tokens, tokens)]
        features_lens = prompt_features_lens.to(self.device) + features_lens.to(self.device)
        embed, tokens_lens = self.forward_text_embed(tokens)
        return self.forward_text_condition(embed, tokens_lens, features_lens)

    def forward_text_inference_ratio_duration(self, tokens, prompt_tokens, prompt_features_lens,
                                              speed: float, num_frames: Optional[int] = None):
        """zipvoice.py:290-330.  ``num_frames``: as ``forward_text_condition``."""
        cat_tokens = [p + t for p, t in zip(prompt_tokens, tokens)]
        ptl = to_device(torch.tensor([len(t) for t in prompt_tokens], dtype=torch.int64), self.device)
        tl = to_device(torch.tensor([len(t) for t in tokens], dtype=torch.int64), self.device)
        cat_embed, cat_tokens_lens = self.forward_text_embed(cat_tokens)
        features_lens = predict_features_lens(prompt_features_lens.to(self.device), ptl, tl, speed)
        return self.forward_text_condition(cat_embed, cat_tokens_lens, features_lens, num_frames)

    # ------------------------------------------------------------------ sampling
    def sample(self, tokens: List[List[int]], prompt_tokens: List[List[int]],
               prompt_features: torch.Tensor, prompt_features_lens: torch.Tensor,
               features_lens: Optional[torch.Tensor] = None, speed: float = 1.0,
               t_shift: float = 1.0, duration: str = "predict", num_step: int = 5,
               guidance_scale: float = 0.5, x0: Optional[torch.Tensor] = None,
               seeds: Optional[Sequence[int]] = None,
               seed_streams: Optional[Sequence[int]] = None):
        """zipvoice.py:388-486.  ``x0`` (extra, optional) supplies the initial noise
        explicitly; ``seeds`` (extra, optional; one int in [0, 2^64) per row, with
        ``seed_streams`` one int in [0, 2^32) per row, default 0) draws row b with
        ``noise.seeded_normal`` from (seeds[b], seed_streams[b]), so a row's noise does not
        depend on what it is batched with; otherwise the noise is drawn with torch.randn on
        the device as the reference does (:453-458).

        ``num_step``, ``t_shift``, ``guidance_scale`` and ``speed`` (extra) each also take a
        sequence of one value per row: the batch then runs as one scheduled solve
        (``solver.sample_rows``), every row with its own settings.  Scalars, and the
        reference's (batch, 1, 1) guidance tensor, take the unscheduled path."""
        check_noise(len(tokens), x0, seeds, seed_streams)
        eng = self._need_engine()
        # per-request settings: a sequence of one value per row for any of these four sends the
        # batch through the scheduled solve (solver.sample_rows), the others broadcast
        schedule = per_row_schedule(len(tokens), num_step=num_step, t_shift=t_shift,
                                    guidance_scale=guidance_scale, speed=speed)
        if schedule is not None:
            schedule, speed = schedule
            speed = torch.tensor(speed, dtype=torch.float32, device=self.device)
        assert duration in ["real", "predict"]
        prompt_features_lens = prompt_features_lens.to(self.device)
        if duration == "predict":
            text_condition, padding_mask = self.forward_text_inference_ratio_duration(
                tokens=tokens, prompt_tokens=prompt_tokens,
                prompt_features_lens=prompt_features_lens, speed=speed)
        else:
            assert features_lens is not None
            text_condition, padding_mask = self.forward_text_inference_gt_duration(
                tokens=tokens, features_lens=features_lens, prompt_tokens=prompt_tokens,
                prompt_features_lens=prompt_features_lens)
        batch_size, num_frames, _ = text_condition.shape
        speech_condition = eng.speech_condition(prompt_features, prompt_features_lens, num_frames)
        x0 = initial_noise(batch_size, num_frames, prompt_features.size(-1), self.device, x0, seeds,
                           seed_streams)
        # the output shapes are known before sampling: reading them here (the text path has
        # already synchronised for num_frames) keeps the host from waiting on the Euler loop,
        # so the prompt split and the vocoder are queued behind it without an idle gap
        x1_wo_prompt_lens = (~padding_mask).sum(-1) - prompt_features_lens
        Tg, Tp = (int(v) for v in torch.stack([x1_wo_prompt_lens.max(),
                                                prompt_features_lens.max()]).tolist())
        x1 = self._solve(x0, text_condition, speech_condition, padding_mask, schedule, num_step,
                         guidance_scale, t_shift)
        return split_prompt(x1, prompt_features_lens, x1_wo_prompt_lens, Tg, Tp) + (
            prompt_features_lens,)

    def _solve(self, x0, text_condition, speech_condition, padding_mask, schedule, num_step,
               guidance_scale, t_shift, t_start: float = 0.0, t_end: float = 1.0):
        """The solve of ``sample`` and ``sample_edit``: the scheduled one when ``schedule`` holds one
        ``RowSchedule`` per row, the plain one with the scalar settings when it is None."""
        if schedule is not None:
            return self.solver.sample_rows(x=x0, text_condition=text_condition,
                                           speech_condition=speech_condition,
                                           padding_mask=padding_mask, schedule=schedule)
        return self.solver.sample(x=x0, text_condition=text_condition,
                                  speech_condition=speech_condition, padding_mask=padding_mask,
                                  num_step=num_step, guidance_scale=guidance_scale,
                                  t_start=t_start, t_end=t_end, t_shift=t_shift)

    # ------------------------------------------------------------------ editing
    def sample_edit(self, tokens: List[List[int]], features: torch.Tensor,
                    features_lens: torch.Tensor, spans, num_step: int = 5,
                    guidance_scale: float = 0.5, t_shift: float = 1.0, t_start: float = 0.0,
                    t_end: float = 1.0, x0: Optional[torch.Tensor] = None,
                    seeds: Optional[Sequence[int]] = None,
                    seed_streams: Optional[Sequence[int]] = None, keep_original: bool = True):
        """Regenerate marked spans of ``features`` (B, Lmax, F; ``features_lens`` frames per row)
        and keep the rest: the infill the model is trained for (``forward``, zipvoice.py:358-363).
        No reference counterpart beyond ``sample_intermediate``.

        ``tokens`` is the whole new transcript of each row; ``spans[b]`` the row's edits
        ``(s, e, n)``, "replace original frames [s, e) by n generated ones" (``edit.plan_edit``;
        ``e == s`` inserts, ``n == 0`` deletes).  The text condition is the ground-truth-duration
        one over the new lengths (the reference's ``forward_text_train``), the speech condition
        the kept frames at their new places and zeros on the generated ones
        (``engine.edit_gather``).  ``num_step`` / ``t_shift`` / ``guidance_scale``, ``x0``,
        ``seeds`` and ``seed_streams`` are ``sample``'s.  With ``keep_original`` the kept frames
        of the result are the input's, bit for bit; without it they are the solver's.

        Returns (x1 (B, T, F), the new lengths (B,), mask (B, T) bool: True on generated
        frames)."""
        from .edit import plan_edit_batch
        B = len(tokens)
        check_noise(B, x0, seeds, seed_streams)
        eng = self._need_engine()
        schedule = per_row_schedule(B, num_step=num_step, t_shift=t_shift,
                                    guidance_scale=guidance_scale, speed=1.0)
        if features.dim() != 3 or features.size(0) != B:
            raise ValueError(f"features must be (B = {B}, L, F), got {tuple(features.shape)}")
        plan = plan_edit_batch(features_lens.tolist() if torch.is_tensor(features_lens)
                               else features_lens, spans)
        if int(plan.lens.max()) > features.size(1):
            raise ValueError("features_lens exceed the frames of features")
        new_lens = torch.from_numpy(plan.new_lens.astype(np.int64)).to(self.device)
        embed, tokens_lens = self.forward_text_embed(tokens)
        text_condition, padding_mask = self.forward_text_condition(embed, tokens_lens, new_lens)
        num_frames, F = text_condition.size(1), features.size(-1)
        speech_condition, mask = eng.edit_gather(features, plan.lens, plan.table, plan.row_ptr,
                                                 num_frames)
        x0 = initial_noise(B, num_frames, F, self.device, x0, seeds, seed_streams)
        if schedule is not None:                # (speed plays no part: the lengths are the plan's)
            schedule = [RowSchedule(num_step=r.num_step, guidance_scale=r.guidance_scale,
                                    t_start=float(t_start), t_end=float(t_end), t_shift=r.t_shift)
                        for r in schedule[0]]
        x1 = self._solve(x0, text_condition, speech_condition, padding_mask, schedule, num_step,
                         guidance_scale, t_shift, float(t_start), float(t_end))
        if keep_original:
            x1, _ = eng.edit_gather(features, plan.lens, plan.table, plan.row_ptr, num_frames,
                                    fill=x1)
        return x1, new_lens, mask

    def sample_intermediate(self, tokens: List[List[int]], features: torch.Tensor,
                            features_lens: torch.Tensor, noise: torch.Tensor,
                            speech_condition_mask: torch.Tensor, t_start: float, t_end: float,
                            num_step: int = 1, guidance_scale=None):
        """zipvoice.py:488-534: the solve from ``t_start`` to ``t_end`` with the speech condition
        ``where(speech_condition_mask, 0, features)``.  The same path as ``sample_edit`` driven
        by a mask: its runs of True inside a row's frames are spans with ``n = e - s``.
        ``guidance_scale`` is a float or the reference's (batch, 1, 1) tensor.  Returns
        (x_t_end (B, T, F), its lengths)."""
        from .edit import mask_spans
        lens = [int(v) for v in features_lens.tolist()]
        m = speech_condition_mask.cpu().numpy()
        spans = [mask_spans(m[b], lens[b]) for b in range(len(lens))]
        x, x_lens, _ = self.sample_edit(
            tokens=tokens, features=features, features_lens=features_lens, spans=spans,
            num_step=num_step, guidance_scale=0.0 if guidance_scale is None else guidance_scale,
            t_shift=1.0, t_start=t_start, t_end=t_end, x0=noise, keep_original=False)
        return x, x_lens


def per_row_schedule(B: int, **settings):
    """``sample``'s num_step / t_shift / guidance_scale / speed, each a scalar or a sequence of B
    values.  None when all are scalars (or the reference's (B, 1, 1) guidance tensor: the
    unscheduled path); else (one solver.RowSchedule per row, the B speeds) with the scalars
    broadcast.  A sequence of another length is a ValueError."""
    def is_seq(v):
        return isinstance(v, (list, tuple)) or (isinstance(v, np.ndarray) and v.ndim == 1)
    if not any(is_seq(v) for v in settings.values()):
        return None
    cols = {}
    for name, v in settings.items():
        if is_seq(v):
            if len(v) != B:
                raise ValueError(f"{name}: expected one value per row ({B}), got {len(v)}")
            cols[name] = list(v)
        elif torch.is_tensor(v) and v.numel() > 1:
            if v.numel() != B:
                raise ValueError(f"{name}: expected 1 or {B} values, got shape {tuple(v.shape)}")
            cols[name] = v.reshape(B).tolist()
        else:
            cols[name] = [float(v) if name != "num_step" else v] * B
    rows = [RowSchedule(num_step=int(n), guidance_scale=float(g), t_shift=float(s))
            for n, g, s in zip(cols["num_step"], cols["guidance_scale"], cols["t_shift"])]
    return rows, [float(s) for s in cols["speed"]]


def split_prompt(x1: torch.Tensor, prompt_lens: torch.Tensor, gen_lens: torch.Tensor,
                 Tg: Optional[int] = None, Tp: Optional[int] = None):
    """zipvoice.py:469-486 without the per-item python slicing loop: one gather.  Tg / Tp
    (the longest generated / prompt part) are read from the lengths when not given."""
    B, T, F = x1.shape
    dev = x1.device
    Tg = int(gen_lens.max()) if Tg is None else Tg
    Tp = int(prompt_lens.max()) if Tp is None else Tp
    ar_g = torch.arange(Tg, device=dev)[None]
    idx = (prompt_lens[:, None] + ar_g).clamp(max=T - 1)
    gen = torch.gather(x1, 1, idx[..., None].expand(B, Tg, F))
    gen = gen * (ar_g < gen_lens[:, None])[..., None]
    ar_p = torch.arange(Tp, device=dev)[None]
    prm = x1[:, :Tp] * (ar_p < prompt_lens[:, None])[..., None]
    return gen, gen_lens, prm


class ZipVoiceDistill(ZipVoice):
    """zipvoice_distill.py:27-94: guidance-scale embedding, no CFG doubling."""

    variant = "zipvoice_distill"
    solver_cls = DistillEulerSolver


class ZipVoiceDialog(ZipVoice):
    """zipvoice_dialog.py:28-215 (speaker-turn embeddings on the text encoder)."""

    variant = "zipvoice_dialog"

    def __init__(self, *args, spk_a_id: int = 360, spk_b_id: int = 361, **kw):
        super().__init__(*args, spk_a_id=spk_a_id, spk_b_id=spk_b_id, **kw)
        self.spk_a_id, self.spk_b_id = spk_a_id, spk_b_id


class ZipVoiceDialogStereo(ZipVoiceDialog):
    """zipvoice_dialog.py:218-256: two-stream decoder (500->512 / 512->200)."""

    variant = "zipvoice_dialog_stereo"


MODEL_CLASSES = {"zipvoice": ZipVoice, "zipvoice_distill": ZipVoiceDistill,
                 "zipvoice_dialog": ZipVoiceDialog,
                 "zipvoice_dialog_stereo": ZipVoiceDialogStereo}


def build_model(cfg: ModelConfig, precision: str = "fp32", padding: str = "batch"):
    cls = MODEL_CLASSES[cfg.variant]
    kw = cfg.model_kwargs()
    return cls(**kw, precision=precision, padding=padding)
