"""Float64 restatement of the long-form trim and join (include/zipvoice_hip.h, the
zv_wavjoin_* block; zipvoice_amd/csrc/zv_wavjoin.inc), in numpy only and written as the
definition reads: frame by frame, run by run, chunk by chunk.  The GPU tests compare the
engine with this; tests/test_longform_plan.py checks it against hand-made cases."""
from collections import namedtuple

import numpy as np

Joined = namedtuple("Joined", "out m off F margin kept")


def kept_frames(loud, keep_edge, max_gap):
    """loud: bool per frame -> bool per frame (the kept ones)."""
    nf = len(loud)
    keep = np.zeros(nf, bool)
    idx = np.flatnonzero(loud)
    if len(idx) == 0:
        return keep
    first, last = int(idx[0]), int(idx[-1])
    keep[max(0, first - keep_edge):min(nf - 1, last + keep_edge) + 1] = True
    f = first + 1
    while f < last:
        if loud[f]:
            f += 1
            continue
        e = f
        while not loud[e]:                      # ends at or before `last`, which is loud
            e += 1
        r = e - f                               # the maximal quiet run [f, e)
        if r > max_gap:
            head, tail = (max_gap + 1) // 2, max_gap // 2
            keep[f + head:e - tail] = False
        f = e
    return keep


def wavjoin(wavs, lens, gains, frame, thr, keep_edge, max_gap, fade):
    """wavs: (B, C, n) or (B, n) array (or a list of (C, n_b) / (n_b,) arrays), lens: (B,)
    sample counts, gains: (B,) or None.  Returns Joined(out (C, N) float64, m, off, F (B,)
    int64, margin = min over all frames of |e / (thr^2 * count) - 1|, kept = the list of
    per-chunk sample-index arrays of the trimmed chunks)."""
    xs = []
    for b, x in enumerate(wavs):
        x = np.asarray(x, np.float64)
        xs.append((x[None] if x.ndim == 1 else x)[:, :int(lens[b])])
    B = len(xs)
    C = xs[0].shape[0] if B else 1
    g = np.ones(B) if gains is None else np.asarray(gains, np.float64)
    margin = np.inf
    kept, ys = [], []
    for x in xs:
        n = x.shape[1]
        nf = -(-n // frame)
        loud = np.zeros(nf, bool)
        for f in range(nf):
            seg = x[:, f * frame:min((f + 1) * frame, n)]
            e, lim = float((seg * seg).sum()), thr * thr * seg.size
            loud[f] = not e < lim
            if lim > 0:
                margin = min(margin, abs(e / lim - 1.0))
        keep = kept_frames(loud, keep_edge, max_gap)
        idx = [np.arange(f * frame, min((f + 1) * frame, n)) for f in range(nf) if keep[f]]
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        kept.append(idx)
        ys.append(x[:, idx])
    m = np.array([y.shape[1] for y in ys], np.int64)
    off = np.full(B, -1, np.int64)
    F = np.zeros(B, np.int64)
    p = -1
    for b in range(B):
        if m[b] == 0:
            continue
        if p < 0:
            off[b] = 0
        else:
            F[b] = min(fade, m[p] // 2, m[b] // 2)
            off[b] = off[p] + m[p] - F[b]
        p = b
    N = int(off[p] + m[p]) if p >= 0 else 0
    out = np.zeros((C, N))
    p = -1
    for b in range(B):
        if m[b] == 0:
            continue
        o, Fb = int(off[b]), int(F[b])
        out[:, o + Fb:o + m[b]] = g[b] * ys[b][:, Fb:]
        for j in range(Fb):
            w = (j + 1) / (Fb + 1)
            out[:, o + j] = g[p] * ys[p][:, m[p] - Fb + j] * (1 - w) + g[b] * ys[b][:, j] * w
        p = b
    return Joined(out, m, off, F, margin, kept)
