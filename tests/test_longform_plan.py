"""Host side of long-form synthesis (zipvoice_amd/longform.py): the chunker's properties,
the token budget, and self-checks of the float64 join restatement (tests/wavjoin_ref.py)
that the GPU tests compare the engine with.  No GPU needed."""
import math

import numpy as np
import pytest

import wavjoin_ref as ref
from zipvoice_amd.longform import chunk_budget, chunk_tokens

HARD, SOFT = (1, 2), (3,)


def pieces_between(tokens, ids):
    """Lengths of the maximal pieces that end on a token of `ids`, by end position."""
    out, start = {}, 0
    for i, t in enumerate(tokens):
        if t in ids or i == len(tokens) - 1:
            out[i] = i + 1 - start
            start = i + 1
    return out


def check_properties(tokens, max_tokens, hard=HARD, soft=SOFT):
    chunks = chunk_tokens(tokens, hard, max_tokens, soft)
    assert [t for c in chunks for t in c] == list(tokens)
    assert all(1 <= len(c) <= max_tokens for c in chunks)
    # a chunk ends on a break id unless it is the last one or a forced cut, and a cut is
    # forced only inside a break-free piece longer than max_tokens
    every = tuple(hard) + tuple(soft)
    ends, pos = pieces_between(tokens, every), 0
    for c in chunks[:-1]:
        pos += len(c)
        if c[-1] not in every:
            end = min(e for e in ends if e >= pos - 1)
            assert ends[end] > max_tokens, (pos, c)
    # a soft break ends a chunk only inside a sentence longer than max_tokens
    sent, pos = pieces_between(tokens, hard), 0
    for c in chunks[:-1]:
        pos += len(c)
        if c[-1] not in hard:
            end = min(e for e in sent if e >= pos - 1)
            assert sent[end] > max_tokens, (pos, c)
    # greedy: two neighbours that both end on a hard break do not fit one chunk
    for a, b in zip(chunks, chunks[1:]):
        if a[-1] in hard and b[-1] in hard:
            assert len(a) + len(b) > max_tokens
    return chunks


def test_chunker_hand_made():
    t = [5, 6, 1, 7, 1, 8, 9, 10, 2, 11]
    assert chunk_tokens(t, HARD, 5) == [[5, 6, 1, 7, 1], [8, 9, 10, 2, 11]]
    assert chunk_tokens(t, HARD, 4) == [[5, 6, 1], [7, 1], [8, 9, 10, 2], [11]]
    assert chunk_tokens(t, HARD, 100) == [t]
    assert chunk_tokens([], HARD, 4) == []
    # a long sentence: soft breaks first, then the forced cut of what is still too long
    s = [5, 5, 3, 6, 6, 6, 6, 6, 6, 6, 3, 7, 1, 8, 1]
    assert chunk_tokens(s, HARD, 4, SOFT) == [[5, 5, 3], [6, 6, 6, 6], [6, 6, 6, 3],
                                              [7, 1, 8, 1]]
    # without soft ids the sentence is cut evenly: 13 tokens -> 4 parts of 4, 3, 3, 3
    assert [len(c) for c in chunk_tokens(s, HARD, 4)] == [4, 3, 3, 3, 2]
    with pytest.raises(ValueError):
        chunk_tokens(t, HARD, 0)


@pytest.mark.parametrize("seed", range(8))
def test_chunker_properties_random(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    # ids 1, 2 hard, 3 soft, the rest plain; densities vary with the seed
    tokens = rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9], n,
                        p=np.array([1, 1, 3, 5, 5, 5, 5, 5, 5 + 10 * (seed % 3)], float)
                        / (35 + 10 * (seed % 3))).tolist()
    for max_tokens in (1, 2, 3, 7, 20, 64, 1000):
        check_properties(tokens, max_tokens)


def test_chunker_without_breaks_cuts_evenly():
    tokens = list(range(10, 1010))
    for max_tokens in (1, 7, 64, 333, 999, 1000):
        chunks = check_properties(tokens, max_tokens)
        k = math.ceil(1000 / max_tokens)
        sizes = [len(c) for c in chunks]
        assert len(sizes) == k and max(sizes) - min(sizes) <= 1 and sum(sizes) == 1000
        assert sizes == sorted(sizes, reverse=True)


def test_chunker_max_tokens_one():
    t = [5, 1, 6, 7, 2]
    assert chunk_tokens(t, HARD, 1, SOFT) == [[5], [1], [6], [7], [2]]


def test_chunk_budget():
    # 10 tokens in 2 s = 5 tokens/s; 23 s left -> 115 tokens
    assert chunk_budget(10, 2.0) == 115
    assert chunk_budget(10, 2.0, max_seconds=12.0) == 50
    assert chunk_budget(10, 2.0, max_seconds=12.0, speed=1.5) == 75
    assert chunk_budget(7, 3.0, max_seconds=10.0) == 16            # 7 * 7 / 3 = 16.33
    assert chunk_budget(1, 9.0, max_seconds=10.0) == 1             # 0.11 -> at least 1
    assert chunk_budget(12, 1.0, max_seconds=4.0) == 36
    with pytest.raises(ValueError):
        chunk_budget(10, 25.0)
    with pytest.raises(ValueError):
        chunk_budget(10, 30.0, max_seconds=25.0)


# ------------------------------------------------------------------ reference self-checks
P = dict(frame=240, thr=10 ** (-42 / 20), keep_edge=2, max_gap=4, fade=480)


def noise(rng, *segments):
    """segments: (amplitude, samples), ... -> one float32 chunk."""
    return np.concatenate([(a * rng.standard_normal(n)).astype(np.float32) for a, n in segments])


def batch(chunks):
    lens = [len(c) for c in chunks]
    x = np.zeros((len(chunks), max(lens)), np.float32)
    for b, c in enumerate(chunks):
        x[b, :lens[b]] = c
    return x, lens


def test_ref_kept_frames_by_hand():
    L, q = True, False
    # edges: keep_edge frames around first / last loud, clipped to the chunk
    assert ref.kept_frames(np.array([q, q, q, L, q, q, q, q]), 2, 4).tolist() == \
        [q, L, L, L, L, L, q, q]
    assert ref.kept_frames(np.array([q, L, q]), 5, 4).tolist() == [L, L, L]
    assert not ref.kept_frames(np.array([q, q, q]), 2, 4).any()
    # a run of exactly max_gap stays, max_gap + 1 loses its middle frame; odd max_gap keeps
    # ceil(max_gap / 2) at the front
    assert ref.kept_frames(np.array([L, q, q, q, q, L]), 0, 4).all()
    assert ref.kept_frames(np.array([L, q, q, q, q, q, L]), 0, 4).tolist() == \
        [L, L, L, q, L, L, L]
    assert ref.kept_frames(np.array([L, q, q, q, q, q, L]), 0, 3).tolist() == \
        [L, L, L, q, q, L, L]
    assert ref.kept_frames(np.array([L, q, q, L]), 0, 0).tolist() == [L, q, q, L]


def test_ref_length_is_sum_m_minus_sum_f():
    rng = np.random.default_rng(0)
    x, lens = batch([noise(rng, (1e-4, 1000), (0.1, 3001), (1e-4, 5003), (0.1, 777), (1e-4, 2500)),
                     noise(rng, (1e-4, 4000)), noise(rng, (0.1, 100)),
                     noise(rng, (0.1, 1203), (1e-4, 700), (0.1, 1500))])
    r = ref.wavjoin(x, lens, None, **P)
    assert r.out.shape == (1, int(r.m.sum() - r.F.sum()))
    assert r.m[1] == 0 and r.off[1] == -1 and r.F[1] == 0
    assert r.F.tolist() == [0, 0, 50, 50]                  # floor(100 / 2) limits both fades
    # chunk 0: loud frames 4..16 and 37..40, 2 + 2 of the 20 quiet frames between, 2 + 2 at the edges
    assert r.m[0] == 240 * (2 + 13 + 4 + 4 + 2) and r.m[3] == 3403


def test_ref_single_loud_chunk_unchanged():
    rng = np.random.default_rng(1)
    x, lens = batch([noise(rng, (0.1, 5003))])
    r = ref.wavjoin(x, lens, None, **P)
    assert r.m.tolist() == [5003] and r.off.tolist() == [0] and r.F.tolist() == [0]
    assert np.array_equal(r.out[0], x[0].astype(np.float64))


def test_ref_all_quiet_is_empty():
    rng = np.random.default_rng(2)
    x, lens = batch([noise(rng, (1e-4, 3000)), noise(rng, (1e-4, 10)), np.zeros(0, np.float32)])
    r = ref.wavjoin(x, lens, None, **P)
    assert r.out.shape == (1, 0) and not r.m.any() and (r.off == -1).all() and not r.F.any()


def test_ref_constant_chunks_join_to_a_constant():
    x, lens = batch([np.ones(2000, np.float32), np.ones(700, np.float32), np.ones(1500, np.float32)])
    r = ref.wavjoin(x, lens, None, **P)
    assert r.F.tolist() == [0, 350, 350] and r.out.shape == (1, 4200 - 700)
    assert np.abs(r.out - 1.0).max() < 1e-15              # the fade weights sum to 1
    g = ref.wavjoin(x, lens, [1.0, 0.5, 1.0], **P)
    assert abs(g.out[0, 1650] - (1.0 - 0.5 / 351)) < 1e-15
    assert abs(g.out[0, 2000 + 349] - (0.5 + 0.5 * 350 / 351)) < 1e-15
