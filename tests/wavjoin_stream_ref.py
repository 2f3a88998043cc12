"""Float64 restatement of the stateful long-form join (include/zipvoice_hip.h, the
zv_wavjoin_stream_* block), in numpy only and written as the definition reads: a slot
carries the samples of its last non-empty chunk that are not emitted yet, and a push walks
its chunks one by one, finishing the predecessor when the next non-empty chunk tells how
much of it fades.  Nothing here slices a one-shot result; only the trim of a single chunk
(frames, kept frames, y_b: unchanged by streaming) comes from tests/wavjoin_ref.py.
tests/test_longform_stream_plan.py checks it against wavjoin_ref.wavjoin on the CPU, the GPU
tests compare the engine with it."""
from collections import namedtuple

import numpy as np

import wavjoin_ref as ref

Piece = namedtuple("Piece", "out n pos spans margin")

THR = 10.0 ** (-42.0 / 20.0)
SMALL = dict(frame=16, thr=THR, keep_edge=1, max_gap=2, fade=24)
LOUD, QUIET = 0.1, 1e-4
SPLITS = ([8, 0], [1] * 8, [3, 0, 5], [1, 7], [2, 1, 1, 1, 3], [0, 8])


class Slot:
    """One open document.  m, g: the held chunk p (m == 0: none); tail (C, H) float64: its raw
    samples y_p[m - H, m), H = min(fade, m / 2); pos: the samples emitted so far."""

    def __init__(self, C, frame, thr, keep_edge, max_gap, fade):
        self.C, self.fade = C, fade
        self.params = dict(frame=frame, thr=thr, keep_edge=keep_edge, max_gap=max_gap, fade=fade)
        self.reset()

    def reset(self):
        self.m, self.g, self.tail, self.pos, self.closed = 0, 1.0, np.zeros((self.C, 0)), 0, False

    def push(self, wavs, lens, gains=None, final=False):
        """wavs: B arrays (C, n_b) or (n_b,) (or one (B, C, n) array), lens, gains (B,) or None
        -> Piece(out (C, n) float64, n, pos before the push, spans (B, 3) int64 {m_b, off_b
        relative to the piece, F_b}, margin of the chunks' frames from the threshold)."""
        assert not self.closed, "push to a closed slot"
        B = len(lens)
        g = np.ones(B) if gains is None else np.asarray(gains, np.float64)
        fade, margin = self.fade, np.inf
        parts, col = [], 0                      # the columns written so far, in order
        spans = np.zeros((B, 3), np.int64)
        # the chain's current chunk: its length, its gain, and its raw samples not yet emitted
        cur_m, cur_g, pending = self.m, self.g, self.tail
        for b in range(B):
            x = np.asarray(wavs[b], np.float64)
            x = (x[None] if x.ndim == 1 else x)[:, :int(lens[b])]
            one = ref.wavjoin([x], [x.shape[1]], None, **self.params)
            margin = min(margin, one.margin)
            y = x[:, one.kept[0]]                # the trimmed chunk y_b
            mb = y.shape[1]
            if mb == 0:
                spans[b] = (0, -1, 0)
                continue
            F = min(fade, cur_m // 2, mb // 2) if cur_m else 0
            k = pending.shape[1]
            assert F <= k
            parts.append(cur_g * pending[:, :k - F])      # final now: p fades over F samples only
            col += k - F
            spans[b] = (mb, col, F)
            for j in range(F):
                w = (j + 1) / (F + 1)
                parts.append((cur_g * pending[:, k - F + j] * (1 - w) + g[b] * y[:, j] * w)[:, None])
            col += F
            cur_m, cur_g, pending = mb, float(g[b]), y[:, F:]
        if final:
            parts.append(cur_g * pending)
            cur_m, cur_g, pending = 0, 1.0, np.zeros((self.C, 0))
        else:                                    # hold the last H samples back, raw
            H = min(fade, cur_m // 2)
            k = pending.shape[1]
            parts.append(cur_g * pending[:, :k - H])
            pending = pending[:, k - H:]
        out = np.concatenate(parts, axis=1) if parts else np.zeros((self.C, 0))
        pos = self.pos
        self.m, self.g, self.tail, self.pos, self.closed = cur_m, cur_g, pending, pos + out.shape[1], final
        return Piece(out, out.shape[1], pos, spans, margin)


def noise(rng, C, *segments):
    """segments: (amplitude, samples), ... -> one (C, n) float32 chunk of Gaussian noise."""
    return np.concatenate([(a * rng.standard_normal((C, n))).astype(np.float32)
                           for a, n in segments], axis=1)


def eight_chunks(C=1, seed=0):
    """The chunks of the split-invariance cases (frame 16, fade 24): loud / quiet / loud, all
    quiet (empty), 1 sample, 9 samples, zero length, shorter than 2 * fade, 300 loud samples,
    quiet then loud; gains 1, 0.5 and 0.25 mixed."""
    rng = np.random.default_rng(seed)
    chunks = [noise(rng, C, (LOUD, 403), (QUIET, 331), (LOUD, 1210)),
              noise(rng, C, (QUIET, 500)),
              noise(rng, C, (1.0, 1)),
              noise(rng, C, (LOUD, 9)),
              np.zeros((C, 0), np.float32),
              noise(rng, C, (LOUD, 41)),
              noise(rng, C, (LOUD, 300)),
              noise(rng, C, (QUIET, 215), (LOUD, 2049))]
    gains = [1.0, 1.0, 0.5, 1.0, 1.0, 0.25, 1.0, 0.5]
    return chunks, gains


def cut(seq, sizes):
    """seq cut into consecutive parts of the given sizes."""
    assert sum(sizes) == len(seq)
    out, i = [], 0
    for s in sizes:
        out.append(seq[i:i + s])
        i += s
    return out
