"""End-to-end generation on the engine: the reference's ``generate_sentence``
(``zipvoice/bin/infer_zipvoice.py:276-403``) from token ids to waveform, and a
batched form for serving.

Steps, as the reference: prompt resampling to the model's rate (torchaudio
``Resample``, :335-338; ``feature.Resample`` on the device) -> prompt RMS
normalisation to ``target_rms`` (:340-342) -> VocosFbank / BigVGANFbank prompt features (:345-347, :583-590) -> ``(feat + feat_bias) * feat_scale``
(:349) -> ``model.sample(duration="predict")`` (:355-371) -> ``pred /
feat_scale - feat_bias`` -> vocoder decode -> ``clamp(-1, 1)`` (:374-378) ->
RTF metrics (:381-396) -> RMS restore (:399-400).  Text normalisation /
tokenisation (jieba, pypinyin, piper) and audio file I/O (torchaudio.load) are
outside the ported path: callers pass token ids and the prompt's samples with
their rate.  ``prepare_prompt`` assembles the dialog / stereo prompts the way
``infer_zipvoice_dialog.py`` does after loading.
"""
from __future__ import annotations

import datetime as dt
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .common import to_device
from .models import per_row_schedule
from .noise import check_noise


def get_feature_extractor(feature_type: str, num_channels: int = 1):
    """The reference's feature-extractor choice by ``model_config["feature"]["type"]``
    (infer_zipvoice.py:583-590): "vocos" -> VocosFbank, "bigvgan_v2" -> BigVGANFbank."""
    from .feature import BigVGANFbank, VocosFbank
    if feature_type == "vocos":
        return VocosFbank(num_channels=num_channels)
    if feature_type == "bigvgan_v2":
        return BigVGANFbank(num_channels=num_channels)
    raise NotImplementedError(f"Unsupported feature type: {feature_type}")


def _prompt_rms_normalise(wav: torch.Tensor, target_rms: float) -> Tuple[torch.Tensor, float]:
    rms = float(torch.sqrt(torch.mean(torch.square(wav))))
    if rms < target_rms:
        wav = wav * target_rms / rms
    return wav, rms


def restore_level(wav: torch.Tensor, rms: float, target_rms: float) -> torch.Tensor:
    """The RMS restore (:399-400) on a waveform: two roundings per sample; ``wav`` itself at rms >= target."""
    return wav * rms / target_rms if rms < target_rms else wav


def output_gain(rms: float, target_rms: float) -> float:
    """The restore as one factor, rounded before the joiner or the splice multiplies by it: not
    ``restore_level``'s arithmetic."""
    return rms / target_rms if rms < target_rms else 1.0


def _finish_row(wav_row: torch.Tensor, n: int, level, target_rms: float) -> torch.Tensor:
    """A decoded row as its request gets it: its first ``n`` samples at the prompt's level, (1, n).
    ``level`` is the prompt's RMS on the host (a prompt wav) or its output gain on the device (a voice)."""
    w = wav_row[:n]
    return (w * level if torch.is_tensor(level) else restore_level(w, level, target_rms)).unsqueeze(0)


_resamplers: Dict[Tuple[int, int], object] = {}


def _resampler(orig_freq: int, new_freq: int):
    """One ``feature.Resample`` (filter table + engine handle) per rate pair."""
    from .feature import Resample
    key = (int(orig_freq), int(new_freq))
    if key not in _resamplers:
        _resamplers[key] = Resample(*key)
    return _resamplers[key]


@torch.inference_mode()
def prepare_prompt(wavs, rates, mode: str = "mono", sampling_rate: int = 24000, silence=None,
                   device=None) -> torch.Tensor:
    """The reference's prompt loading after ``torchaudio.load``: every wav (C, N) (or (N,)),
    with its own rate, is resampled per channel to ``sampling_rate`` on the device, then
    assembled into the (C, N) tensor ``feature_extractor.extract`` takes.

    "mono"   (infer_zipvoice.py:332-338): one wav; a two-channel prompt keeps its channels
             (the extractor averages them, as now).
    "dialog" (infer_zipvoice_dialog.py:268-282): one or two wavs, each averaged to one
             channel, concatenated in time.
    "stereo" (:415-442): one two-channel wav; or two two-channel wavs concatenated in
             time; or two one-channel wavs, the first on channel 0 over [0, n0) and the
             second on channel 1 over [n0, n0 + n1), on a background of ``silence``
             ((2, >= n0 + n1) samples at ``sampling_rate``, cut to n0 + n1) or zeros."""
    if mode not in ("mono", "dialog", "stereo"):
        raise ValueError(f"mode must be mono, dialog or stereo, not {mode!r}")
    if torch.is_tensor(wavs) or isinstance(wavs, np.ndarray):
        wavs = [wavs]
    if isinstance(rates, int):
        rates = [rates] * len(wavs)
    assert len(wavs) == len(rates) and 1 <= len(wavs) <= (1 if mode == "mono" else 2)
    dev = torch.device(device if device is not None else "cuda")
    loaded = []
    for w, rate in zip(wavs, rates):
        w = torch.as_tensor(np.asarray(w) if not torch.is_tensor(w) else w, dtype=torch.float32)
        w = (w.unsqueeze(0) if w.dim() == 1 else w).to(dev)
        assert w.dim() == 2 and w.shape[0] in (1, 2), w.shape
        if rate != sampling_rate:
            w = _resampler(rate, sampling_rate)(w)
        if mode == "dialog" and w.size(0) != 1:
            w = w.mean(0, keepdim=True)
        loaded.append(w)
    if mode == "stereo" and len(loaded) == 1:
        assert loaded[0].size(0) == 2, "Merged prompt wav must be stereo for stereo dialogue generation"
    if len(loaded) == 1:
        return loaded[0]
    if mode == "dialog" or loaded[0].size(0) == 2:
        assert loaded[0].size(0) == loaded[1].size(0), (loaded[0].shape, loaded[1].shape)
        return torch.cat(loaded, dim=1)
    assert loaded[0].size(0) == 1 and loaded[1].size(0) == 1
    n0, n1 = loaded[0].size(1), loaded[1].size(1)
    if silence is None:
        out = torch.zeros((2, n0 + n1), dtype=torch.float32, device=dev)
    else:
        out = torch.as_tensor(np.asarray(silence) if not torch.is_tensor(silence) else silence,
                              dtype=torch.float32).to(dev)[:, :n0 + n1].clone()
        assert out.shape == (2, n0 + n1), f"silence must be (2, >= {n0 + n1}), got {tuple(out.shape)}"
    out[0, :n0] = loaded[0][0]
    out[1, n0:] = loaded[1][0]
    return out


@torch.inference_mode()
def generate_sentence(tokens: List[int], prompt_tokens: List[int], prompt_wav, model, vocoder,
                      feature_extractor, num_step: int = 16, guidance_scale: float = 1.0,
                      speed: float = 1.0, t_shift: float = 0.5, target_rms: float = 0.1,
                      feat_scale: float = 0.1, feat_bias: float = 0.0,
                      sampling_rate: int = 24000, prompt_sampling_rate: int = 24000,
                      seed: Optional[int] = None) -> Tuple[torch.Tensor, Dict[str, float]]:
    """One sentence (infer_zipvoice.py:276-403).  Returns (wav (1, N) on the
    device, metrics with the reference's keys).  ``seed`` (an int in [0, 2^64); the
    reference's ``--seed``, :240) keys the initial noise to this request
    (``noise.seeded_normal``, stream 0): the same seed in a ``generate_batch`` row starts from
    the same noise.  Without it the noise comes from torch.randn, as before."""
    dev = model.device
    prompt_features, prompt_rms, _ = _prepare_prompt(
        prompt_wav, prompt_sampling_rate, feature_extractor, dev, target_rms, feat_scale, feat_bias,
        sampling_rate)
    prompt_features_lens = torch.tensor([prompt_features.size(1)], device=dev)
    torch.cuda.synchronize(dev)
    start_t = dt.datetime.now()
    pred, pred_lens, _, _ = model.sample(
        tokens=[tokens], prompt_tokens=[prompt_tokens], prompt_features=prompt_features,
        prompt_features_lens=prompt_features_lens, speed=speed, t_shift=t_shift,
        duration="predict", num_step=num_step, guidance_scale=guidance_scale,
        seeds=None if seed is None else [seed])
    torch.cuda.synchronize(dev)
    start_vocoder_t = dt.datetime.now()
    wav = vocoder.decode_features(pred, pred_lens, feat_scale=feat_scale, feat_bias=feat_bias,
                                  clamp=True)
    torch.cuda.synchronize(dev)
    t = (dt.datetime.now() - start_t).total_seconds()
    t_no_vocoder = (start_vocoder_t - start_t).total_seconds()
    t_vocoder = (dt.datetime.now() - start_vocoder_t).total_seconds()
    wav_seconds = wav.shape[-1] / sampling_rate
    metrics = {"t": t, "t_no_vocoder": t_no_vocoder, "t_vocoder": t_vocoder,
               "wav_seconds": wav_seconds, "rtf": t / wav_seconds,
               "rtf_no_vocoder": t_no_vocoder / wav_seconds, "rtf_vocoder": t_vocoder / wav_seconds}
    return restore_level(wav, prompt_rms, target_rms), metrics


def _prepare_prompt(prompt_wav, prompt_sampling_rate: int, feature_extractor, dev, target_rms: float,
                    feat_scale: float, feat_bias: float, sampling_rate: int):
    """One prompt as ``generate_sentence`` prepares it: resampled on the device when its rate is not
    the model's (:335-338, before the RMS, which is then taken on the device too), RMS-normalised,
    framed (a two-channel prompt keeps its channels for the extractor), scaled.  Returns
    (prompt_features (1, P, F) on the device, the RMS before normalisation, the samples per channel
    at the model's rate)."""
    w = torch.as_tensor(np.asarray(prompt_wav) if not torch.is_tensor(prompt_wav) else prompt_wav,
                        dtype=torch.float32)
    if w.dim() == 1:
        w = w.unsqueeze(0)
    if prompt_sampling_rate != sampling_rate:
        w = _resampler(prompt_sampling_rate, sampling_rate)(w.to(dev))
    w, rms = _prompt_rms_normalise(w, target_rms)
    feats = feature_extractor.extract(w.to(dev), sampling_rate=sampling_rate)
    return ((feats.unsqueeze(0) + feat_bias) * feat_scale).to(dev), rms, w.shape[-1]


def _prompts_at_rate(wavs: Sequence, rates: Sequence[Optional[int]], sampling_rate: int, dev
                     ) -> List[torch.Tensor]:
    """Host prompts (mono samples; ``rates[i]`` None: at ``sampling_rate``) -> one 1-D float32 row each
    at ``sampling_rate``, where it already is: a prompt at the model's rate stays on the host (no GPU is
    touched if all are), the others go up padded, one ``resample_batch`` per distinct rate, and are
    returned as views of its output on ``dev``, cut to their lengths."""
    rows = [torch.as_tensor(np.asarray(w), dtype=torch.float32).reshape(-1) for w in wavs]
    by_rate: Dict[int, List[int]] = {}
    for i, rate in enumerate(rates):
        if rate is not None and int(rate) != sampling_rate:
            by_rate.setdefault(int(rate), []).append(i)
    for rate, idx in by_rate.items():
        lens = [len(rows[i]) for i in idx]
        rb = torch.zeros((len(idx), max(lens)), dtype=torch.float32)
        for r, i in enumerate(idx):
            rb[r, :lens[r]] = rows[i]
        out, olens = _resampler(rate, sampling_rate).resample_batch(rb.to(dev), lens)
        for r, (i, n) in enumerate(zip(idx, olens.tolist())):
            rows[i] = out[r, :n]
    return rows


def _prepare_prompts(items: Sequence[tuple], feature_extractor, target_rms: float, feat_scale: float,
                     feat_bias: float, dev):
    """The prompts of items = [(tokens, prompt_tokens, prompt_wav[, prompt_sampling_rate]), ...]
    as ``generate_batch`` prepares them: one batched resample per distinct rate, host RMS
    normalisation, one ``extract_batch``, scale and bias.  Returns (prompt features (B, T, n_mels),
    frame counts (B,) on the device, the prompts' RMS before normalisation, their sample counts at
    the model's rate)."""
    rows = _prompts_at_rate([it[2] for it in items], [it[3] if len(it) > 3 else None for it in items],
                            feature_extractor.config.sampling_rate, dev)
    # (resampled rows come back: RMS + padding are the 24 kHz items' host path)
    wavs, rms = zip(*[_prompt_rms_normalise(w.cpu(), target_rms) for w in rows])
    n = max(len(w) for w in wavs)
    wb = torch.zeros((len(wavs), n), dtype=torch.float32)
    for i, w in enumerate(wavs):
        wb[i, :len(w)] = w
    lens = torch.tensor([len(w) for w in wavs])
    feats, nfr = feature_extractor.extract_batch(wb.to(dev), lens)
    return (feats + feat_bias) * feat_scale, nfr, list(rms), [len(w) for w in wavs]


@torch.inference_mode()
def generate_batch(items: Sequence[tuple], model, vocoder,
                   feature_extractor, num_step: int = 16, guidance_scale: float = 1.0,
                   speed: float = 1.0, t_shift: float = 0.5, target_rms: float = 0.1,
                   feat_scale: float = 0.1, feat_bias: float = 0.0, x0=None,
                   remove_long_sil: bool = False, joiner=None,
                   seeds: Optional[Sequence[int]] = None
                   ) -> Tuple[List[torch.Tensor], Dict[str, float]]:
    """Batched serving form: items = [(tokens, prompt_tokens, prompt_wav), ...] with 24 kHz
    prompts, or (tokens, prompt_tokens, prompt_wav, prompt_sampling_rate); prompts at
    other rates are resampled on the device, one batched call per distinct rate.
    Each output equals what ``generate_sentence`` would produce for that item with
    the same initial noise (per-utterance lengths and masks throughout).  To rounding that holds
    in ``model.padding == "row"``, where every row is integrated as it would be alone; in the
    default ``"batch"`` mode it holds for the items whose total length is the batch's longest or a
    multiple of 4 (the decoder's largest downsampling factor), and the others end as the
    reference's batched ``sample`` leaves them (``DESIGN.md`` section 3, "Padding").

    ``seeds`` (one int in [0, 2^64) per item; not together with ``x0``) keys every item's
    initial noise to the item (``noise.seeded_normal``, stream 0): item i then starts from the
    noise ``generate_sentence(seed=seeds[i])`` starts from, whatever it is batched with.

    ``num_step``, ``guidance_scale``, ``speed`` and ``t_shift`` each also take a sequence of one
    value per item (a ValueError at any other length): the pool then runs as one scheduled solve
    (``ZipVoice.sample``), every item integrated with its own settings.

    ``remove_long_sil`` (upstream ZipVoice's ``--remove-long-sil``; mono and one-channel
    Dialog models, stereo is out of scope): every decoded row goes through
    ``longform.WavJoiner.trim`` (``joiner``, default ``WavJoiner()``), which drops the
    silence at its edges and cuts over-long pauses inside, with the RMS restore folded in
    as the row's gain; each waveform is then (1, N_i) and ``wav_seconds`` / ``rtf`` use
    the trimmed lengths.

    Items ``(tokens, Voice)`` (``voices.VoiceStore.register``; all of one store, not mixed with wav
    items: a ValueError) take the prompt features from the store and its ``target_rms`` / ``feat_scale``
    / ``feat_bias``: no prompt is resampled, measured or framed, and the RMS restore is one multiply by
    the store's gains on the device (the row's gain of ``WavJoiner.trim`` under ``remove_long_sil``)."""
    dev = model.device
    B = len(items)
    seeds, _ = check_noise(B, x0, seeds)
    # (per-item settings are checked for their length here, before any GPU work)
    per_row_schedule(B, num_step=num_step, t_shift=t_shift, guidance_scale=guidance_scale, speed=speed)
    from .voices import Voice
    by_voice = [len(it) == 2 and isinstance(it[1], Voice) for it in items]
    if any(by_voice):
        if not all(by_voice):
            raise ValueError("a batch is all (tokens, Voice) items or all prompt wavs, not a mix")
        store = items[0][1].store
        voices = [store.check(it[1]) for it in items]
        # the store holds (feats + feat_bias) * feat_scale of the normalised prompts: nothing to prepare
        # (level: the output gains on the device; the wav items' is their prompts' RMS on the host)
        prompt_features, level = store.gather(voices, max(v.frames for v in voices))
        nfr = to_device(torch.tensor([v.frames for v in voices]), dev)
        prompt_tokens = [list(v.prompt_tokens) for v in voices]
    else:
        prompt_features, nfr, level, _ = _prepare_prompts(items, feature_extractor, target_rms, feat_scale,
                                                          feat_bias, dev)
        prompt_tokens = [it[1] for it in items]
    if remove_long_sil:
        from .longform import WavJoiner
        joiner = joiner if joiner is not None else WavJoiner()
        gains = level if torch.is_tensor(level) else torch.tensor(
            [output_gain(r, target_rms) for r in level], dtype=torch.float32).to(dev)
    torch.cuda.synchronize(dev)
    t0 = dt.datetime.now()
    pred, pred_lens, _, _ = model.sample(
        tokens=[it[0] for it in items], prompt_tokens=prompt_tokens,
        prompt_features=prompt_features, prompt_features_lens=nfr, speed=speed,
        t_shift=t_shift, duration="predict", num_step=num_step, guidance_scale=guidance_scale,
        x0=x0, seeds=seeds)
    out = vocoder.decode_features(pred, pred_lens, feat_scale=feat_scale, feat_bias=feat_bias,
                                  clamp=True)
    if remove_long_sil:
        out, out_lens = joiner.trim(out, (pred_lens * vocoder.cfg.hop_length).to(torch.int32),
                                    gains)
    torch.cuda.synchronize(dev)
    t = (dt.datetime.now() - t0).total_seconds()
    if remove_long_sil:
        ns = out_lens.tolist()
        secs = sum(ns) / 24000
        return ([out[i, :ns[i]].unsqueeze(0) for i in range(B)],
                {"t": t, "wav_seconds": secs, "rtf": t / secs if secs else float("inf")})
    hop = vocoder.cfg.hop_length
    res = [_finish_row(out[i], n * hop, level[i], target_rms) for i, n in enumerate(pred_lens.tolist())]
    secs = float(pred_lens.sum()) * hop / 24000
    return res, {"t": t, "wav_seconds": secs, "rtf": t / secs}
