"""The host half of streaming long-form synthesis, without a GPU: the float64 restatement of
the stateful join (tests/wavjoin_stream_ref.py) against the one-shot reference
(tests/wavjoin_ref.py) for every way of cutting a chunk sequence into pushes that the GPU
tests use, and the grouping rule of generate_long_stream (longform.stream_groups)."""
import numpy as np
import pytest

import wavjoin_ref as ref
import wavjoin_stream_ref as sref
from zipvoice_amd.longform import stream_groups

P = sref.SMALL


def run_split(chunks, gains, sizes, C, params=P):
    """Push the chunks in parts of the given sizes, the last one final -> (the pieces
    concatenated, absolute spans, the Piece of every push)."""
    slot = sref.Slot(C, **params)
    pieces, spans = [], []
    parts = list(zip(sref.cut(chunks, sizes), sref.cut(gains, sizes)))
    for i, (cs, gs) in enumerate(parts):
        r = slot.push(cs, [c.shape[1] for c in cs], gs, final=i == len(parts) - 1)
        assert r.pos == sum(p.n for p in pieces)
        pieces.append(r)
        sp = r.spans.copy()
        sp[sp[:, 1] >= 0, 1] += r.pos
        spans.append(sp)
    return np.concatenate([p.out for p in pieces], axis=1), np.concatenate(spans), pieces


def random_splits(n, total, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cuts = np.sort(rng.integers(0, total + 1, rng.integers(1, 6)))
        out.append(np.diff(np.concatenate([[0], cuts, [total]])).tolist())
    return out


@pytest.mark.parametrize("C", [1, 2])
def test_every_split_reproduces_the_one_shot_reference(C):
    chunks, gains = sref.eight_chunks(C)
    lens = [c.shape[1] for c in chunks]
    whole = ref.wavjoin(chunks, lens, gains, **P)
    assert whole.margin >= 1e-3, whole.margin
    # the cases the chunk list is meant to hold
    assert whole.m[1] == 0 and whole.m[2] == 1 and whole.m[3] == 9 and lens[4] == 0
    assert 0 < whole.m[5] < 2 * P["fade"] and whole.m[6] == 300 and 0 < whole.m[0] < lens[0]
    want = np.stack([whole.m, whole.off, whole.F], 1)
    for sizes in list(sref.SPLITS) + random_splits(6, 8, 1):
        out, spans, pieces = run_split(chunks, gains, sizes, C)
        assert np.array_equal(out, whole.out), sizes      # the same float64 expression
        assert np.array_equal(spans, want), sizes
        assert min(p.margin for p in pieces) >= 1e-3


def test_held_tail_rule():
    chunks, gains = sref.eight_chunks(1)
    slot = sref.Slot(1, **P)
    whole = ref.wavjoin(chunks, [c.shape[1] for c in chunks], gains, **P)
    last = 0
    for b, c in enumerate(chunks):
        r = slot.push([c], [c.shape[1]], [gains[b]])
        if whole.m[b]:
            last = int(whole.m[b])
        N = int(ref.wavjoin(chunks[:b + 1], [x.shape[1] for x in chunks[:b + 1]], gains[:b + 1],
                            **P).out.shape[1])
        assert r.pos + r.n == N - min(P["fade"], last // 2), b
        assert slot.tail.shape[1] == min(P["fade"], last // 2)
    assert whole.m[2] == 1
    one = sref.Slot(1, **P)
    r = one.push([chunks[2]], [1], [0.5])
    assert r.n == 1 and one.tail.shape[1] == 0             # a 1-sample chunk holds nothing
    # a closing push without chunks emits exactly the held samples, gained
    slot2 = sref.Slot(1, **P)
    slot2.push([chunks[5]], [chunks[5].shape[1]], [0.25])
    held = slot2.tail.copy()
    r = slot2.push([], [], None, final=True)
    assert r.n == held.shape[1] > 0 and np.array_equal(r.out, 0.25 * held) and slot2.closed


def test_stream_groups():
    assert stream_groups(0, 1, 4) == []
    assert stream_groups(2, 4, 32) == [[0, 1]]                       # K < first_batch
    assert stream_groups(4, 4, 32) == [[0, 1, 2, 3]]                 # K = first_batch
    assert stream_groups(8, 1, 32) == [[0], list(range(1, 8))]
    assert stream_groups(8, 1, 3) == [[0], [1, 2, 3], [4, 5, 6], [7]]   # a remainder
    assert stream_groups(7, 1, 3) == [[0], [1, 2, 3], [4, 5, 6]]
    assert stream_groups(7, 2, 2) == [[0, 1], [2, 3], [4, 5], [6]]
    for K, fb, bs in ((13, 3, 4), (5, 5, 1), (1, 1, 1)):
        g = stream_groups(K, fb, bs)
        assert [i for grp in g for i in grp] == list(range(K))
        assert len(g[0]) == min(fb, K) and all(0 < len(x) <= bs for x in g[1:])
    for bad in ((-1, 1, 1), (3, 0, 1), (3, 1, 0)):
        with pytest.raises(ValueError):
            stream_groups(*bad)
