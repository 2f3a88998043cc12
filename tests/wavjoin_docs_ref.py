"""The segmented join (include/zipvoice_hip.h, zv_wavjoin_apply_docs) in float64:
tests/wavjoin_ref.wavjoin called once per document on that document's chunks, as the
definition reads.  Numpy only."""
from collections import namedtuple

import numpy as np

import wavjoin_ref as ref

JoinedDocs = namedtuple("JoinedDocs", "outs N m off F margin kept")


def wavjoin_docs(wavs, lens, gains, doc_ptr, frame, thr, keep_edge, max_gap, fade):
    """wavs, lens, gains as in wavjoin_ref.wavjoin; doc_ptr: D + 1 chunk bounds.  Returns
    JoinedDocs(outs: D arrays (C, N_d) float64, N (D,), m / off / F (B,) int64 with off
    relative to the chunk's document, margin = the smallest over all documents, kept = the
    per-chunk sample-index arrays).  An empty document has N = 0."""
    B, D = len(lens), len(doc_ptr) - 1
    assert doc_ptr[0] == 0 and doc_ptr[-1] == B
    assert all(a <= b for a, b in zip(doc_ptr, doc_ptr[1:]))
    C = 1 if B == 0 or np.asarray(wavs[0]).ndim == 1 else np.asarray(wavs[0]).shape[0]
    g = None if gains is None else np.asarray(gains, np.float64)
    outs, kept = [], []
    m, off, F = (np.zeros(B, np.int64) for _ in range(3))
    margin = np.inf
    for d in range(D):
        lo, hi = int(doc_ptr[d]), int(doc_ptr[d + 1])
        if lo == hi:
            outs.append(np.zeros((C, 0)))
            continue
        r = ref.wavjoin([wavs[b] for b in range(lo, hi)], lens[lo:hi],
                        None if g is None else g[lo:hi], frame, thr, keep_edge, max_gap, fade)
        outs.append(r.out)
        m[lo:hi], off[lo:hi], F[lo:hi] = r.m, r.off, r.F
        margin = min(margin, r.margin)
        kept += r.kept
    return JoinedDocs(outs, np.array([o.shape[1] for o in outs], np.int64), m, off, F, margin, kept)
