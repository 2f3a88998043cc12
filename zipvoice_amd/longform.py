"""Long-form synthesis: text longer than the model speaks in one pass.

The reference has no long-form path, so nothing here mirrors it; the behaviour is this
module's own (and ``include/zipvoice_hip.h`` for the join).  Its parts:

* ``chunk_tokens`` / ``chunk_budget``: split a token list at the caller's sentence-end ids
  into chunks whose predicted duration fits the model (host, pure Python; the engine takes
  token ids and knows no tokenizer).
* ``WavJoiner``: the engine's ``zv_wavjoin_*`` kernels: trim the pauses the model puts at
  chunk edges (and over-long pauses inside), then glue the trimmed chunks with linear
  cross-fades, all on the device.  ``join_docs`` joins the chunks of several documents in
  one call, each document into its own waveform; ``trim`` is the one-chunk-per-document
  case, a pause trim per row.
* ``generate_long``: prompt -> chunks -> ``model.sample`` in batches that share the one
  prompt -> vocoder -> one join.
* ``WavJoiner.stream`` / ``WavJoinStream``: the same join push by push (``zv_wavjoin_stream_*``);
  ``generate_long_stream`` / ``stream_groups``: ``generate_long`` as a generator that yields
  the audio group by group, bitwise the samples of the one-call join.
* ``plan_long_batch`` / ``generate_long_batch``: several texts with their own prompts; the
  chunks of all of them are pooled into the ``model.sample`` batches, and one ``join_docs``
  writes one waveform per text.
"""
from __future__ import annotations

import collections
import ctypes
import datetime as dt
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as _eng
from .noise import check_keys, check_noise


# ------------------------------------------------------------------------------ chunker
def _split_after(tokens: Sequence[int], ids) -> List[List[int]]:
    """Split after every token in ``ids`` (the break token stays with its piece)."""
    out, cur = [], []
    for t in tokens:
        cur.append(t)
        if t in ids:
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def _even_parts(piece: List[int], max_tokens: int) -> List[List[int]]:
    """k = ceil(n / max_tokens) consecutive parts whose sizes differ by at most 1."""
    n = len(piece)
    k = -(-n // max_tokens)
    out, pos = [], 0
    for i in range(k):
        size = n // k + (1 if i < n % k else 0)
        out.append(piece[pos:pos + size])
        pos += size
    return out


def chunk_tokens(tokens: Sequence[int], break_ids, max_tokens: int,
                 soft_break_ids=()) -> List[List[int]]:
    """Token list -> list of chunks of at most ``max_tokens`` tokens, in order (their
    concatenation is the input).

    The text is split after every token in ``break_ids`` (sentence ends).  A sentence longer
    than ``max_tokens`` is split the same way at ``soft_break_ids`` (commas and the like),
    and a piece that is still too long, of length n, is cut into ceil(n / max_tokens)
    consecutive parts whose sizes differ by at most 1.  The resulting pieces merge greedily,
    left to right, while the merged length stays <= ``max_tokens``."""
    max_tokens = int(max_tokens)
    if max_tokens < 1:
        raise ValueError("max_tokens must be at least 1")
    hard, soft = frozenset(break_ids), frozenset(soft_break_ids)
    pieces: List[List[int]] = []
    for sentence in _split_after(list(tokens), hard):
        if len(sentence) <= max_tokens:
            pieces.append(sentence)
            continue
        for part in _split_after(sentence, soft):
            pieces.extend([part] if len(part) <= max_tokens else _even_parts(part, max_tokens))
    chunks: List[List[int]] = []
    for p in pieces:
        if chunks and len(chunks[-1]) + len(p) <= max_tokens:
            chunks[-1] = chunks[-1] + p
        else:
            chunks.append(list(p))
    return chunks


def chunk_budget(prompt_tokens_len: int, prompt_seconds: float, max_seconds: float = 25.0,
                 speed: float = 1.0) -> int:
    """The token count whose predicted duration fills the time left beside the prompt:
    ``common.predict_features_lens`` gives a chunk of n tokens
    n * prompt_seconds / prompt_tokens_len / speed seconds, so
    max(1, floor((max_seconds - prompt_seconds) * prompt_tokens_len / prompt_seconds * speed))
    tokens fit ``max_seconds`` of prompt plus speech.  ``max_seconds`` is the caller's limit
    for one pass (25 s is a default, not a tuned value)."""
    if not prompt_seconds > 0 or prompt_tokens_len < 1:
        raise ValueError("the prompt must have a positive duration and at least one token")
    if prompt_seconds >= max_seconds:
        raise ValueError(f"the prompt ({prompt_seconds:.2f} s) leaves no room within "
                         f"max_seconds = {max_seconds}")
    return max(1, math.floor((max_seconds - prompt_seconds) * prompt_tokens_len
                             / prompt_seconds * speed))


# ------------------------------------------------------------------------------ joiner
class WavJoiner:
    """Trim and join on the device (``zv_wavjoin_*``, definition in include/zipvoice_hip.h).

    ``frame`` samples per energy frame (240 = 10 ms at 24 kHz); a frame is quiet below
    ``threshold_db`` dBFS RMS; ``keep_edge`` quiet frames stay around the speech (10 =
    100 ms); a pause inside longer than ``max_gap`` frames (50 = 500 ms) is cut to
    ``max_gap`` frames; neighbouring chunks overlap by up to ``fade`` samples (2400 =
    100 ms) of linear cross-fade.  One engine handle per device, freed in ``__del__``."""

    def __init__(self, frame: int = 240, threshold_db: float = -42.0, keep_edge: int = 10,
                 max_gap: int = 50, fade: int = 2400):
        self.frame, self.threshold_db = int(frame), float(threshold_db)
        self.keep_edge, self.max_gap, self.fade = int(keep_edge), int(max_gap), int(fade)
        self.thr = 10.0 ** (self.threshold_db / 20.0)
        self._lib = None
        self._handles: Dict[torch.device, int] = {}

    def _handle(self, device: torch.device):
        if not torch.cuda.is_available():
            raise RuntimeError("zipvoice_amd long-form join needs a ROCm GPU; no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._handles:
            self._lib = _eng.load_library()
            h = self._lib.zv_wavjoin_create(self.frame, self.thr, self.keep_edge, self.max_gap,
                                            self.fade)
            if not h:
                raise ValueError(self._lib.zv_last_error().decode())
            self._handles[device] = h
        return self._handles[device]

    def __del__(self):
        for dev, h in list(getattr(self, "_handles", {}).items()):
            try:
                torch.cuda.synchronize(dev)
            except Exception:
                pass
            self._lib.zv_wavjoin_destroy(h)
        self._handles = {}

    def device_bytes(self) -> int:
        """Scratch the handles hold (0 before the first call)."""
        return sum(int(self._lib.zv_wavjoin_device_bytes(h)) for h in self._handles.values())

    def _prepare(self, wavs, lens, gains):
        """The arguments of one call on the device: (handle, wavs (B, C, n) fp32, host lens or
        None for a device ``lens``, lens int32 on the device, gains fp32 on the device or
        None).  Host values are checked; tensors already on the device are taken as they
        are (the kernels clamp every length into [0, n]), so they cost no host wait."""
        if wavs.dim() == 2:
            wavs = wavs.unsqueeze(1)
        if wavs.dim() != 3 or wavs.shape[1] not in (1, 2):
            raise ValueError(f"wavs must be (B, n) or (B, C, n) with C in (1, 2), got "
                             f"{tuple(wavs.shape)}")
        dev = wavs.device if wavs.is_cuda else torch.device("cuda")
        h = self._handle(dev)
        wavs = wavs.to(dev, torch.float32).contiguous()
        B, C, n = wavs.shape
        if torch.is_tensor(lens) and lens.is_cuda:
            if lens.shape != (B,):
                raise ValueError("lens must hold B sample counts in [0, n]")
            lens_host, ln = None, lens.to(dev, torch.int32).contiguous()
        else:
            lens_host = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
            if len(lens_host) != B or (B and (min(lens_host) < 0 or max(lens_host) > n)):
                raise ValueError("lens must hold B sample counts in [0, n]")
            ln = torch.tensor(lens_host, dtype=torch.int32, device=dev)
        g = None
        if gains is not None:
            g = torch.as_tensor(gains, dtype=torch.float32).to(dev).contiguous()
            if g.shape != (B,):
                raise ValueError("gains must have shape (B,)")
        return h, dev, wavs, lens_host, ln, g

    @torch.inference_mode()
    def __call__(self, wavs: torch.Tensor, lens, gains=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """wavs (B, n) or (B, C, n) fp32 (C in {1, 2}), lens (B,) sample counts (host
        values), gains (B,) or None -> (out (C, N) on the device, spans (B, 3) int32 on the
        device: trimmed length m_b, start off_b in ``out`` (-1 for an empty chunk), overlap
        F_b with the previous non-empty chunk).  Allocates cap = sum(lens) columns and waits
        for the host once, to read N."""
        if torch.is_tensor(lens):
            lens = lens.tolist()
        h, dev, wavs, lens_host, ln, g = self._prepare(wavs, lens, gains)
        B, C, n = wavs.shape
        cap = sum(lens_host)
        out = torch.empty((C, max(cap, 1)), dtype=torch.float32, device=dev)
        out_len = torch.empty(1, dtype=torch.int64, device=dev)
        spans = torch.empty((max(B, 1), 3), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _eng._check(self._lib.zv_wavjoin_apply(
                h, _eng._ptr(wavs), n, _eng._ptr(ln), _eng._ptr(g), B, C, _eng._ptr(out),
                out.shape[1], cap, _eng._ptr(out_len), _eng._ptr(spans), _eng._stream()),
                self._lib)
        N = int(out_len.item())                       # the one host wait: N depends on the data
        if N > cap:
            raise RuntimeError(f"joined length {N} exceeds the allocated {cap} samples")
        return out[:, :N], spans[:B]

    @torch.inference_mode()
    def join_docs(self, wavs: torch.Tensor, lens, doc_sizes, gains=None
                  ) -> Tuple[List[torch.Tensor], torch.Tensor]:
        """The chunks of D documents in one call (``zv_wavjoin_apply_docs``): wavs, lens and
        gains as in ``__call__``; ``doc_sizes`` a host list of D non-negative chunk counts
        that sum to B, document d owning the next ``doc_sizes[d]`` chunks.  Every document
        is trimmed and joined on its own, as a separate ``__call__`` on its chunks would do
        it.  Returns (outs: D views (C, N_d) of one (D, C, cap) device tensor, cap = the
        largest per-document sum of lens; spans (B, 3) int32 on the device, with off_b
        relative to the chunk's document).  Waits for the host once, to read the D lengths
        in one transfer."""
        if torch.is_tensor(lens):
            lens = lens.tolist()
        h, dev, wavs, lens_host, ln, g = self._prepare(wavs, lens, gains)
        B, C, n = wavs.shape
        sizes = [int(v) for v in (doc_sizes.tolist() if torch.is_tensor(doc_sizes) else doc_sizes)]
        if any(v < 0 for v in sizes) or sum(sizes) != B:
            raise ValueError(f"doc_sizes must hold non-negative chunk counts that sum to B = {B}, "
                             f"got {sizes}")
        D = len(sizes)
        ptr = [0]
        for v in sizes:
            ptr.append(ptr[-1] + v)
        cap = max([sum(lens_host[ptr[d]:ptr[d + 1]]) for d in range(D)] + [1])
        doc_ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)
        out = torch.empty((D, C, cap), dtype=torch.float32, device=dev)
        out_len = torch.empty(max(D, 1), dtype=torch.int64, device=dev)
        spans = torch.empty((max(B, 1), 3), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _eng._check(self._lib.zv_wavjoin_apply_docs(
                h, _eng._ptr(wavs), n, _eng._ptr(ln), _eng._ptr(g), B, C, _eng._ptr(doc_ptr), D,
                _eng._ptr(out), cap, cap, _eng._ptr(out_len), _eng._ptr(spans), _eng._stream()),
                self._lib)
        Ns = out_len[:D].tolist()                     # the one host wait: N_d depends on the data
        if Ns and max(Ns) > cap:
            raise RuntimeError(f"joined length {max(Ns)} exceeds the allocated {cap} samples")
        return [out[d, :, :Ns[d]] for d in range(D)], spans[:B]

    @torch.inference_mode()
    def trim(self, wavs: torch.Tensor, lens, gains=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """A pause trim per row: every row is its own document (D = B), so nothing is
        cross-faded; the silence at a row's edges goes and over-long pauses inside are cut
        (usable on decoded batches and on prompts).  wavs (B, n) or (B, C, n), lens and
        gains as in ``__call__`` or tensors on the device -> (out of the input's shape on
        the device, row b holding its N_b kept samples times its gain, then zeros; out_lens
        (B,) int64 on the device).  No host wait: with ``lens`` and ``gains`` already on
        the device nothing here blocks the host, and the lengths stay there."""
        squeeze = wavs.dim() == 2
        h, dev, wavs, _, ln, g = self._prepare(wavs, lens, gains)
        B, C, n = wavs.shape
        doc_ptr = torch.arange(B + 1, dtype=torch.int32, device=dev)
        out = torch.empty((B, C, n), dtype=torch.float32, device=dev)
        out_len = torch.empty(B, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _eng._check(self._lib.zv_wavjoin_apply_docs(
                h, _eng._ptr(wavs), n, _eng._ptr(ln), _eng._ptr(g), B, C, _eng._ptr(doc_ptr), B,
                _eng._ptr(out), n, n, _eng._ptr(out_len), None, _eng._stream()), self._lib)
        return (out[:, 0] if squeeze else out), out_len

    def stream(self, channels: int = 1, device=None) -> "WavJoinStream":
        """A stateful join on this joiner's parameters (``zv_wavjoin_stream_*``): chunks go in
        push by push, and the pieces that come out, concatenated, are bitwise ``__call__``
        on all of them.  ``device``: the GPU it lives on (default: the current one)."""
        return WavJoinStream(self, channels, device)


class _PendingPiece:
    """A queued push of a ``WavJoinStream``.  ``wait()`` blocks until the push has run and
    returns (piece (C, n) on the device, spans (B, 3) int32 on the device, off_b relative to
    the piece); ``position`` is then the stream position of the piece's first sample."""

    def __init__(self, stream, out, spans, host_len, event, cap):
        self._stream, self._out, self._spans = stream, out, spans
        self._host_len, self._event, self._cap = host_len, event, cap
        self.position, self._n = None, None

    def wait(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._host_len is not None:
            # the one host wait: n depends on the data.  Ask first: waiting on an event that is
            # done was seen to last until the work queued after it had drained
            if not self._event.query():
                self._event.synchronize()
            self._n, self.position = (int(v) for v in self._host_len.tolist())
            self._stream._pinned.append(self._host_len)   # back to the stream for a later push
            self._host_len = None
            self._stream.position = max(self._stream.position, self.position + self._n)
        if self._n > self._cap:
            raise RuntimeError(f"piece of {self._n} samples exceeds the allocated {self._cap}")
        return self._out[:, :self._n], self._spans


class WavJoinStream:
    """One open document of a stateful join (a D = 1 ``zv_wavjoin_stream``; definition in
    include/zipvoice_hip.h).  Between pushes the device keeps the last min(fade, m / 2)
    samples of the last non-empty chunk, because their cross-fade depends on the chunk that
    comes next; ``final`` releases them.  Keeps its ``WavJoiner`` alive; calls on the two are
    ordered on the current device stream."""

    def __init__(self, joiner: WavJoiner, channels: int = 1, device=None):
        self.joiner, self.channels = joiner, int(channels)
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._h = None
        jh = joiner._handle(dev)
        self._lib = joiner._lib
        with torch.cuda.device(dev):
            self._h = self._lib.zv_wavjoin_stream_create(jh, self.channels, 1)
        if not self._h:
            raise ValueError(self._lib.zv_last_error().decode())
        self.position = 0                             # samples emitted by the pieces waited for
        self.closed = False
        # pinned {n, pos} buffers: a pending piece borrows one and hands it back in wait(), so
        # a warm push does not go to the pinned-memory allocator
        self._pinned: List[torch.Tensor] = []

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            self._lib.zv_wavjoin_stream_destroy(self._h)
            self._h = None

    def device_bytes(self) -> int:
        """The held tail and the slot's words on the device."""
        return int(self._lib.zv_wavjoin_stream_device_bytes(self._h))

    @torch.inference_mode()
    def push_async(self, wavs: torch.Tensor, lens, gains=None, final: bool = False
                   ) -> _PendingPiece:
        """Queue a push and return without waiting: arguments as ``push``.  The piece's
        length comes back through a pinned, non-blocking copy and an event, so work queued
        between this call and ``wait()`` overlaps the wait."""
        if self.closed:
            raise RuntimeError("the stream is closed; reset() it first")
        if wavs.dim() == 2:
            wavs = wavs.unsqueeze(1)
        if wavs.dim() == 3 and wavs.shape[1] != self.channels:
            raise ValueError(f"the stream has {self.channels} channel(s), got "
                             f"{tuple(wavs.shape)}")
        if wavs.is_cuda and wavs.device != self.device:
            raise ValueError(f"the stream lives on {self.device}, got wavs on {wavs.device}")
        _, dev, wavs, lens_host, ln, g = self.joiner._prepare(wavs.to(self.device), lens, gains)
        B, C, n = wavs.shape
        # a slot emits at most its held tail (<= fade) and its chunks; lens on the device are
        # not read here, so the padded length bounds them
        cap = self.joiner.fade + (sum(lens_host) if lens_host is not None else B * n)
        out = torch.empty((C, max(cap, 1)), dtype=torch.float32, device=dev)
        out_len = torch.empty(2, dtype=torch.int64, device=dev)
        spans = torch.empty((max(B, 1), 3), dtype=torch.int32, device=dev)
        host_len = (self._pinned.pop() if self._pinned
                    else torch.empty(2, dtype=torch.int64, pin_memory=True))
        fin = (ctypes.c_uint8 * 1)(1 if final else 0)
        with torch.cuda.device(dev):
            _eng._check(self._lib.zv_wavjoin_stream_push(
                self._h, _eng._ptr(wavs), n, _eng._ptr(ln), _eng._ptr(g), B, None, fin,
                _eng._ptr(out), out.shape[1], cap, _eng._ptr(out_len), _eng._ptr(spans),
                _eng._stream()), self._lib)
            host_len.copy_(out_len, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        self.closed = bool(final)
        return _PendingPiece(self, out, spans[:B], host_len, event, cap)

    def push(self, wavs: torch.Tensor, lens, gains=None, final: bool = False
             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """wavs (B, n) or (B, C, n), lens and gains as in ``WavJoiner.__call__`` (lens may
        also be a device tensor, which costs no host wait but allocates for the padded
        length) -> (piece (C, n) on the device, spans (B, 3): m_b, off_b relative to the
        piece, F_b).  Allocates fade + sum(lens) columns, or fade + B * n with ``lens`` on the
        device; the piece is a view of that buffer and keeps all of it alive (``clone()`` a
        piece that is kept for long).  ``final`` also emits the held tail and closes the
        stream."""
        return self.push_async(wavs, lens, gains, final).wait()

    def close(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """A final push of no chunks: the held tail, gained."""
        empty = torch.empty((0, self.channels, 0), dtype=torch.float32, device=self.device)
        return self.push(empty, [], None, final=True)

    def reset(self) -> None:
        """Forget the held tail and the position (ordered on the current stream) and reopen."""
        with torch.cuda.device(self.device):
            _eng._check(self._lib.zv_wavjoin_stream_reset(self._h, 0, _eng._stream()), self._lib)
        self.position, self.closed = 0, False


# ------------------------------------------------------------------------------ pipeline
def _long_prepare(tokens, prompt_tokens, prompt_wav, model, feature_extractor, break_ids,
                  soft_break_ids, max_seconds, speed, target_rms, feat_scale, feat_bias,
                  sampling_rate, prompt_sampling_rate):
    """What ``generate_long`` and ``generate_long_stream`` do before the first chunk runs:
    the prompt, prepared once as ``infer.generate_sentence`` does, and the text cut by
    ``chunk_budget`` and ``chunk_tokens``.  Returns (prompt_features (1, P, F) on the device,
    the prompt's RMS before normalisation, the chunks)."""
    from .infer import _prepare_prompt
    prompt_features, prompt_rms, samples = _prepare_prompt(
        prompt_wav, prompt_sampling_rate, feature_extractor, model.device, target_rms, feat_scale,
        feat_bias, sampling_rate)
    budget = chunk_budget(len(prompt_tokens), samples / sampling_rate, max_seconds, speed)
    chunks = chunk_tokens(tokens, break_ids, budget, soft_break_ids)
    if not chunks:
        raise ValueError("no tokens to synthesise")
    return prompt_features, prompt_rms, chunks


def _long_group(model, vocoder, tokens, prompt_tokens, prompt_features, prompt_frames, seeds,
                streams, x0, feat_scale, feat_bias, **settings):
    """One group of chunks, whose rows may belong to different requests: row i speaks ``tokens[i]``
    after the prompt ``prompt_tokens[i]`` / ``prompt_features[i, :prompt_frames[i]]`` (frames on the
    device) and, with ``seeds``, draws from (seeds[i], streams[i]).  One ``model.sample`` with ``settings``
    (speed, t_shift, num_step, guidance_scale), then the vocoder.  Returns (wavs (nb, n), frames (nb,))."""
    pred, pred_lens, _, _ = model.sample(
        tokens=tokens, prompt_tokens=prompt_tokens, prompt_features=prompt_features,
        prompt_features_lens=prompt_frames, duration="predict", x0=x0, seeds=seeds,
        seed_streams=streams, **settings)
    wav = vocoder.decode_features(pred, pred_lens, feat_scale=feat_scale, feat_bias=feat_bias,
                                  clamp=True)
    return wav, pred_lens


def _long_run(model, vocoder, plan, prompt_tokens, prompt_features, prompt_frames, seeds, x0,
              feat_scale, feat_bias, **settings):
    """The groups of ``plan`` through ``_long_group``.  Request d has the prompt ``prompt_tokens[d]`` /
    ``prompt_features[d]`` of ``prompt_frames[d]`` frames (host ints) and the seed ``seeds[d]`` (``seeds``
    None: torch.randn); chunk k of a request, in text order, draws from stream k; ``x0`` is None or one
    tensor per group.  Returns (the decoded rows as one (K, n) batch in join order, their host lengths)."""
    if x0 is not None and len(x0) != len(plan.groups):
        raise ValueError(f"x0 must hold one tensor per sample() call ({len(plan.groups)}), got {len(x0)}")
    dev = model.device
    nfr = torch.tensor(prompt_frames, dtype=torch.int64, device=dev)
    # chunk i is chunk i - first[doc_of[i]] of its request (join order is text by text)
    first = [sum(plan.doc_sizes[:d]) for d in range(len(plan.doc_sizes))]
    wavs, lens, rows = [], [], []
    for gi, grp in enumerate(plan.groups):
        docs = [plan.doc_of[i] for i in grp]
        di = torch.tensor(docs, dtype=torch.int64, device=dev)
        wav, pred_lens = _long_group(
            model, vocoder, [plan.chunks[i] for i in grp], [prompt_tokens[d] for d in docs],
            prompt_features.index_select(0, di)[:, :max(prompt_frames[d] for d in docs)].contiguous(),
            nfr.index_select(0, di), None if seeds is None else [seeds[d] for d in docs],
            None if seeds is None else [i - first[plan.doc_of[i]] for i in grp],
            None if x0 is None else x0[gi], feat_scale, feat_bias, **settings)
        wavs.append(wav)
        lens.append(pred_lens)
        rows.append(torch.tensor(grp, dtype=torch.int64, device=dev))
    K, n = len(plan.chunks), max(x.shape[1] for x in wavs)
    batch = torch.zeros((K, n), dtype=torch.float32, device=dev)
    for x, r in zip(wavs, rows):                      # group order -> join order
        batch[:, :x.shape[1]].index_copy_(0, r, x)
    lens_dev = torch.empty(K, dtype=torch.int64, device=dev).index_copy_(
        0, torch.cat(rows), torch.cat(lens).to(torch.int64))
    return batch, [int(v) * vocoder.cfg.hop_length for v in lens_dev.tolist()]


@torch.inference_mode()
def generate_long(tokens: List[int], prompt_tokens: List[int], prompt_wav, model, vocoder,
                  feature_extractor, break_ids, soft_break_ids=(), max_seconds: float = 25.0,
                  batch_size: int = 32, joiner: Optional[WavJoiner] = None, x0=None,
                  return_chunks: bool = False, num_step: int = 16, guidance_scale: float = 1.0,
                  speed: float = 1.0, t_shift: float = 0.5, target_rms: float = 0.1,
                  feat_scale: float = 0.1, feat_bias: float = 0.0, sampling_rate: int = 24000,
                  prompt_sampling_rate: int = 24000, seed: Optional[int] = None):
    """A text of any length with one prompt (mono and one-channel Dialog models).

    ``seed`` (an int in [0, 2^64); not together with ``x0``) keys the noise to the request:
    chunk k of the text, in text order, draws with ``noise.seeded_normal`` from
    (seed, stream = k), whatever group it falls into, so ``generate_long_batch`` with the
    same seed for this request starts every chunk from the same noise.

    The prompt is prepared once, as ``infer.generate_sentence`` does; ``chunk_budget`` and
    ``chunk_tokens`` cut the text into K chunks that each fit ``max_seconds`` together with
    the prompt; the chunks run through ``model.sample`` in text order, in consecutive groups
    of at most ``batch_size`` rows that repeat the prompt (``x0``: None, or one initial-noise
    tensor per group), and through ``vocoder.decode_features``; one ``WavJoiner`` call trims
    and joins the K waveforms, with ``generate_sentence``'s RMS restore folded in as the
    per-chunk gain.  Returns (wav (1, N) on the device, metrics with t, wav_seconds, rtf,
    num_chunks, num_batches); with ``return_chunks`` also the list of per-chunk waveforms
    (untrimmed, before the gain) and the joiner's spans."""
    from .infer import output_gain
    if seed is not None:
        if x0 is not None:
            raise ValueError("give x0 or seed, not both")
        seed = check_keys([seed])[0][0]
    dev = model.device
    prompt_features, prompt_rms, chunks = _long_prepare(
        tokens, prompt_tokens, prompt_wav, model, feature_extractor, break_ids, soft_break_ids,
        max_seconds, speed, target_rms, feat_scale, feat_bias, sampling_rate, prompt_sampling_rate)
    # the one-text plan: ``plan_long_batch``'s without sorting (frames are not needed: nothing is sorted)
    K, bs = len(chunks), int(batch_size)
    plan = LongPlan(chunks, [K], [0] * K, None, [list(range(i, min(i + bs, K))) for i in range(0, K, bs)])
    joiner = joiner if joiner is not None else WavJoiner()

    torch.cuda.synchronize(dev)
    t0 = dt.datetime.now()
    batch, lens_host = _long_run(
        model, vocoder, plan, [prompt_tokens], prompt_features, [prompt_features.size(1)],
        None if seed is None else [seed], x0, feat_scale, feat_bias, speed=speed, t_shift=t_shift,
        num_step=num_step, guidance_scale=guidance_scale)
    gains = [output_gain(prompt_rms, target_rms)] * K if prompt_rms < target_rms else None
    out, spans = joiner(batch, lens_host, gains)
    torch.cuda.synchronize(dev)
    t = (dt.datetime.now() - t0).total_seconds()
    secs = out.shape[1] / sampling_rate
    metrics = {"t": t, "wav_seconds": secs, "rtf": t / secs if secs else float("inf"),
               "num_chunks": K, "num_batches": len(plan.groups)}
    if return_chunks:
        return out, metrics, [batch[i, :lens_host[i]] for i in range(K)], spans
    return out, metrics


def stream_groups(K: int, first_batch: int = 1, batch_size: int = 32) -> List[List[int]]:
    """The ``model.sample`` calls of ``generate_long_stream`` over K chunks (host only): the
    first group takes min(first_batch, K) chunks, so the first audio waits for a small
    batch; the rest follow in text order in groups of ``batch_size``."""
    K, first_batch, batch_size = int(K), int(first_batch), int(batch_size)
    if K < 0 or first_batch < 1 or batch_size < 1:
        raise ValueError("K must be non-negative, first_batch and batch_size at least 1")
    first = min(first_batch, K)
    groups = [list(range(first))] if first else []
    return groups + [list(range(i, min(i + batch_size, K))) for i in range(first, K, batch_size)]


@torch.inference_mode()
def generate_long_stream(tokens: List[int], prompt_tokens: List[int], prompt_wav, model, vocoder,
                         feature_extractor, break_ids, soft_break_ids=(),
                         max_seconds: float = 25.0, first_batch: int = 1, batch_size: int = 32,
                         seed: Optional[int] = None, joiner: Optional[WavJoiner] = None,
                         return_chunks: bool = False, num_step: int = 16,
                         guidance_scale: float = 1.0, speed: float = 1.0, t_shift: float = 0.5,
                         target_rms: float = 0.1, feat_scale: float = 0.1, feat_bias: float = 0.0,
                         sampling_rate: int = 24000, prompt_sampling_rate: int = 24000):
    """``generate_long`` as a generator that hands the audio over group by group (mono and
    one-channel Dialog models; no ``x0``: seeds are the batch-invariant path).

    The prompt, the chunks and the per-chunk seeding (chunk k draws from (seed, stream = k))
    are ``generate_long``'s; ``stream_groups`` forms the groups.  Every group runs
    ``model.sample`` and ``vocoder.decode_features`` and is then pushed into one
    ``WavJoinStream`` with the RMS restore as its chunks' gain; the last group's push is
    final.  Streaming changes when samples are handed over, never their value: the pieces,
    concatenated, are bitwise the ``WavJoiner`` join of all chunks in one call.

    Yields one (piece (1, n) on the device, info) per group, n >= 0.  Piece g is handed over
    as soon as its length is back (a pinned copy and an event); group g + 1 is queued when
    the consumer asks for the next piece.  Queueing it first was measured and is worse:
    ``model.sample`` reads its frame count back at its start and holds the host through most
    of its solve, so piece 0, ready after 83 ms, left the generator after 270 ms (DESIGN.md
    §3a).  ``WavJoinStream.push_async`` is there for a caller whose producer does not block.
    The price of this order: the GPU is idle for as long as the consumer keeps piece g before
    it asks for the next one, so a consumer hands the piece on (to a queue, a socket writer)
    and comes straight back.  A push gets ``lens`` on the device, so each piece is a view of a
    buffer of fade + (rows * padded length) columns, which it keeps alive.
    info: group, chunks_done, num_chunks, position (samples emitted, this piece included),
    final, t (seconds on the host clock from the first group's start, taken as
    ``generate_long`` takes its ``t``, to this piece's completion: the first yield's ``t`` is
    the time to first audio); with ``return_chunks`` also chunks (the group's waveforms,
    untrimmed, before the gain) and spans (m_b, off_b relative to the piece, F_b)."""
    from .infer import output_gain
    if seed is not None:
        seed = check_keys([seed])[0][0]
    dev = model.device
    prompt_features, prompt_rms, chunks = _long_prepare(
        tokens, prompt_tokens, prompt_wav, model, feature_extractor, break_ids, soft_break_ids,
        max_seconds, speed, target_rms, feat_scale, feat_bias, sampling_rate, prompt_sampling_rate)
    K = len(chunks)
    groups = stream_groups(K, first_batch, batch_size)
    joiner = joiner if joiner is not None else WavJoiner()
    hop = vocoder.cfg.hop_length
    gain = output_gain(prompt_rms, target_rms) if prompt_rms < target_rms else None
    P = prompt_features.size(1)

    js = joiner.stream(1, device=dev)
    torch.cuda.synchronize(dev)
    t0 = dt.datetime.now()

    def queue(gi):
        idx = groups[gi]
        nb = len(idx)                                        # rows that repeat the one prompt
        wav, pred_lens = _long_group(
            model, vocoder, [chunks[i] for i in idx], [prompt_tokens] * nb,
            prompt_features.expand(nb, -1, -1).contiguous(),
            torch.full((nb,), P, dtype=torch.int64, device=dev),
            None if seed is None else [seed] * nb, None if seed is None else idx, None,
            feat_scale, feat_bias, speed=speed, t_shift=t_shift, num_step=num_step,
            guidance_scale=guidance_scale)
        lens = pred_lens.to(dev, torch.int32) * hop          # stays on the device: no wait here
        return wav, lens, js.push_async(wav, lens, None if gain is None else [gain] * len(idx),
                                        final=gi == len(groups) - 1)

    for gi, idx in enumerate(groups):
        wav, lens, pending = queue(gi)
        piece, spans = pending.wait()
        info = {"group": gi, "chunks_done": idx[-1] + 1, "num_chunks": K,
                "position": pending.position + piece.shape[1], "final": gi == len(groups) - 1,
                "t": (dt.datetime.now() - t0).total_seconds()}
        if return_chunks:
            info["chunks"] = [wav[i, :n] for i, n in enumerate(lens.tolist())]
            info["spans"] = spans
        yield piece, info


# ------------------------------------------------------------------------------ pooled
LongPlan = collections.namedtuple("LongPlan", "chunks doc_sizes doc_of frames groups")


def plan_long_batch(texts: Sequence[Sequence[int]], prompt_tokens_lens: Sequence[int],
                    prompt_samples: Sequence[int], break_ids, soft_break_ids=(),
                    max_seconds: float = 25.0, batch_size: int = 32, speed: float = 1.0,
                    sort_by_length: bool = True, sampling_rate: int = 24000,
                    hop: int = 256) -> LongPlan:
    """The chunks of several texts and the ``model.sample`` calls that speak them (host only).

    Text d, with a prompt of ``prompt_tokens_lens[d]`` tokens and ``prompt_samples[d]``
    samples at ``sampling_rate``, is cut by ``chunk_budget`` and ``chunk_tokens`` as
    ``generate_long`` cuts it.  Returns LongPlan(chunks: all chunks in join order, text by
    text; doc_sizes: chunks per text; doc_of: the text of every chunk; frames: the total
    frames (prompt + speech) ``model.sample`` will use for every chunk, from
    ``feature.compute_num_frames`` and ``common.predict_features_lens``; groups: the
    ``model.sample`` calls in order, as lists of indices into ``chunks``).

    With ``sort_by_length`` the indices are sorted by ``frames`` descending (ties by index
    ascending) and cut into consecutive groups of ``batch_size``: rows of like length share a
    batch, so less attention and feed-forward work goes to padding, and the first call has
    the largest shape, so the engine's workspace grows once.  Without it the groups are
    consecutive in join order; for a single text these are ``generate_long``'s groups."""
    from .common import predict_features_lens
    from .feature import compute_num_frames
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    if not len(texts) == len(prompt_tokens_lens) == len(prompt_samples):
        raise ValueError("texts, prompt_tokens_lens and prompt_samples must have one entry per "
                         "text")
    chunks: List[List[int]] = []
    doc_sizes, doc_of = [], []
    for d, text in enumerate(texts):
        try:
            budget = chunk_budget(int(prompt_tokens_lens[d]),
                                  int(prompt_samples[d]) / sampling_rate, max_seconds, speed)
        except ValueError as e:
            raise ValueError(f"text {d}: {e}") from None
        cs = chunk_tokens(text, break_ids, budget, soft_break_ids)
        if not cs:
            raise ValueError(f"text {d}: no tokens to synthesise")
        chunks += cs
        doc_sizes.append(len(cs))
        doc_of += [d] * len(cs)
    frames: List[int] = []
    if chunks:
        P = torch.tensor([compute_num_frames(int(prompt_samples[d]), hop) for d in doc_of],
                         dtype=torch.int64)
        ptl = torch.tensor([int(prompt_tokens_lens[d]) for d in doc_of], dtype=torch.int64)
        tl = torch.tensor([len(c) for c in chunks], dtype=torch.int64)
        frames = [int(v) for v in predict_features_lens(P, ptl, tl, speed).tolist()]
    order = list(range(len(chunks)))
    if sort_by_length:
        order.sort(key=lambda i: (-frames[i], i))
    groups = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
    return LongPlan(chunks, doc_sizes, doc_of, frames, groups)


@torch.inference_mode()
def generate_long_batch(requests: Sequence[tuple], model, vocoder, feature_extractor, break_ids,
                        soft_break_ids=(), max_seconds: float = 25.0, batch_size: int = 32,
                        joiner: Optional[WavJoiner] = None, x0=None, return_chunks: bool = False,
                        sort_by_length: bool = True, num_step: int = 16,
                        guidance_scale: float = 1.0, speed: float = 1.0, t_shift: float = 0.5,
                        target_rms: float = 0.1, feat_scale: float = 0.1, feat_bias: float = 0.0,
                        seeds: Optional[Sequence[int]] = None):
    """Several texts of any length, each with its own prompt, with their chunks pooled into
    shared ``model.sample`` batches (mono and one-channel Dialog models; stereo is out of
    scope).

    ``seeds`` (one int in [0, 2^64) per request; not together with ``x0``) keys the noise to
    the requests: chunk k of request d, in text order and before any sorting or grouping,
    draws with ``noise.seeded_normal`` from (seeds[d], stream = k), as
    ``generate_long(seed=seeds[d])`` draws it, so a request's noise does not depend on the
    other requests' texts.

    requests = [(tokens, prompt_tokens, prompt_wav), ...] with prompts at the model's rate, or
    (tokens, prompt_tokens, prompt_wav, prompt_sampling_rate).  The prompts are prepared as
    ``infer.generate_batch`` prepares its items (one batched resample per distinct rate, host
    RMS normalisation, one ``extract_batch``); ``plan_long_batch`` cuts the texts and forms
    the groups; every group is one ``model.sample`` call whose rows carry their own request's
    prompt features, prompt length and prompt tokens (``x0``: None, or one initial-noise
    tensor per group in plan order), then ``vocoder.decode_features``; the decoded rows go
    into one (K, n) batch in join order, and one ``WavJoiner.join_docs`` call trims and joins
    them per request, with each request's RMS restore folded in as its chunks' gain.
    Returns (a list of R waveforms (1, N_d) on the device, metrics with t, wav_seconds, rtf,
    num_chunks, num_batches, num_requests); with ``return_chunks`` also the per-chunk
    waveforms in join order (untrimmed, before the gain), the joiner's spans and the plan."""
    from .infer import _prepare_prompts, output_gain
    dev = model.device
    R = len(requests)
    if R == 0:
        raise ValueError("no requests to synthesise")
    seeds, _ = check_noise(R, x0, seeds)
    sampling_rate = feature_extractor.config.sampling_rate
    prompt_features, nfr, rms, nsamp = _prepare_prompts(requests, feature_extractor, target_rms,
                                                        feat_scale, feat_bias, dev)
    plan = plan_long_batch([r[0] for r in requests], [len(r[1]) for r in requests], nsamp,
                           break_ids, soft_break_ids, max_seconds, batch_size, speed,
                           sort_by_length, sampling_rate, feature_extractor.config.hop_length)
    joiner = joiner if joiner is not None else WavJoiner()
    K = len(plan.chunks)
    P = [int(v) for v in nfr.tolist()]

    torch.cuda.synchronize(dev)
    t0 = dt.datetime.now()
    batch, lens_host = _long_run(
        model, vocoder, plan, [r[1] for r in requests], prompt_features, P, seeds, x0, feat_scale,
        feat_bias, speed=speed, t_shift=t_shift, num_step=num_step, guidance_scale=guidance_scale)
    gains = None
    if any(r < target_rms for r in rms):
        gains = [output_gain(rms[d], target_rms) for d in plan.doc_of]
    outs, spans = joiner.join_docs(batch, lens_host, plan.doc_sizes, gains)
    torch.cuda.synchronize(dev)
    t = (dt.datetime.now() - t0).total_seconds()
    secs = sum(o.shape[1] for o in outs) / sampling_rate
    metrics = {"t": t, "wav_seconds": secs, "rtf": t / secs if secs else float("inf"),
               "num_chunks": K, "num_batches": len(plan.groups), "num_requests": R}
    if return_chunks:
        return outs, metrics, [batch[i, :lens_host[i]] for i in range(K)], spans, plan
    return outs, metrics
