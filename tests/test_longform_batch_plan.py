"""The host half of pooled long-form synthesis (zipvoice_amd/longform.py plan_long_batch):
several texts are cut as generate_long cuts one, and their chunks are pooled into
model.sample groups.  No GPU.

Hand numbers.  Prompt A: 24000 samples, 12 tokens -> P = (24000 + 128) // 256 = 94 frames;
with max_seconds = 5 the budget is floor(4 * 12 / 1) = 48 tokens and a chunk of n tokens has
94 + ceil(94 / 12 * n) frames.  Prompt B: 18000 samples, 9 tokens -> P = 70, budget
floor(4.25 * 9 / 0.75) = 51, 70 + ceil(70 / 9 * n) frames."""
import pytest

torch = pytest.importorskip("torch")

from zipvoice_amd.common import predict_features_lens  # noqa: E402
from zipvoice_amd.longform import chunk_budget, chunk_tokens, plan_long_batch  # noqa: E402

BREAK, SOFT = (3, 4), (5,)
A, B = (12, 24000), (9, 18000)                           # (prompt tokens, prompt samples)


def sentence(n, start=10):
    """n tokens, the last a sentence end."""
    return [start + i % 70 for i in range(n - 1)] + [BREAK[n % 2]]


TEXTS = [sentence(48) + sentence(30) + sentence(20),     # 48 | 30 | 20 (30 + 20 > 48)
         sentence(25) + sentence(26) + sentence(10),     # 25 + 26 = 51 | 10
         sentence(48, 20)]
PROMPTS = [A, B, A]


def plan(texts=TEXTS, prompts=PROMPTS, **kw):
    kw = dict(dict(max_seconds=5.0, batch_size=4), **kw)
    return plan_long_batch(texts, [p[0] for p in prompts], [p[1] for p in prompts], BREAK, SOFT,
                           **kw)


def test_hand_numbers():
    assert chunk_budget(12, 1.0, 5.0) == 48 and chunk_budget(9, 0.75, 5.0) == 51
    p = plan()
    assert [len(c) for c in p.chunks] == [48, 30, 20, 51, 10, 48]
    assert p.doc_sizes == [3, 2, 1] and p.doc_of == [0, 0, 0, 1, 1, 2]
    # 94 + ceil(7.8333 * 48 = 376), ceil(235), ceil(156.67); 70 + ceil(7.7778 * 51 = 396.67),
    # ceil(77.78)
    assert p.frames == [470, 329, 251, 467, 148, 470]
    # descending, the tie 470 / 470 by index; then consecutive groups of 4
    assert p.groups == [[0, 5, 3, 1], [2, 4]]


def test_chunks_are_the_texts_cut_as_generate_long_cuts_them():
    p = plan()
    pos = 0
    for d, text in enumerate(TEXTS):
        own = p.chunks[pos:pos + p.doc_sizes[d]]
        assert [t for c in own for t in c] == text
        budget = chunk_budget(PROMPTS[d][0], PROMPTS[d][1] / 24000, 5.0)
        assert own == chunk_tokens(text, BREAK, budget, SOFT)
        assert p.doc_of[pos:pos + p.doc_sizes[d]] == [d] * p.doc_sizes[d]
        pos += p.doc_sizes[d]
    assert pos == len(p.chunks) == len(p.doc_of) == len(p.frames) == sum(p.doc_sizes)


@pytest.mark.parametrize("batch_size", [1, 2, 4, 6, 32])
@pytest.mark.parametrize("sort_by_length", [True, False])
def test_groups_partition_the_chunks(batch_size, sort_by_length):
    p = plan(batch_size=batch_size, sort_by_length=sort_by_length)
    K = len(p.chunks)
    flat = [i for g in p.groups for i in g]
    assert sorted(flat) == list(range(K))
    assert all(1 <= len(g) <= batch_size for g in p.groups)
    assert all(len(g) == batch_size for g in p.groups[:-1])
    if sort_by_length:
        for a, b in zip(flat, flat[1:]):
            assert p.frames[a] > p.frames[b] or (p.frames[a] == p.frames[b] and a < b)
        assert p.frames[flat[0]] == max(p.frames)        # the first call has the largest shape
    else:
        assert flat == list(range(K))


def test_one_text_unsorted_gives_generate_longs_groups():
    text = TEXTS[0] + TEXTS[2] + sentence(7)
    for bs in (1, 2, 3, 32):
        p = plan([text], [A], batch_size=bs, sort_by_length=False)
        chunks = chunk_tokens(text, BREAK, 48, SOFT)
        assert len(chunks) >= 4 and p.chunks == chunks
        assert [[p.chunks[i] for i in g] for g in p.groups] == \
            [chunks[i:i + bs] for i in range(0, len(chunks), bs)]


@pytest.mark.parametrize("speed", [1.0, 1.3])
def test_frames_are_what_sample_will_use(speed):
    p = plan(speed=speed)
    P = torch.tensor([94 if PROMPTS[d] is A else 70 for d in p.doc_of])
    ptl = torch.tensor([PROMPTS[d][0] for d in p.doc_of])
    tl = torch.tensor([len(c) for c in p.chunks])
    assert p.frames == predict_features_lens(P, ptl, tl, speed).tolist()
    assert all(isinstance(f, int) for f in p.frames)


def test_other_rate_and_hop():
    p = plan_long_batch([sentence(30)], [12], [16000], BREAK, SOFT, max_seconds=5.0,
                        sampling_rate=16000, hop=160)
    assert p.frames == [100 + 250] and p.groups == [[0]]  # P = 100, 100 / 12 * 30 = 250


def test_rejections():
    with pytest.raises(ValueError, match="text 1"):
        plan([TEXTS[0], [], TEXTS[2]])                   # an empty text, named by its index
    with pytest.raises(ValueError, match="text 2.*no room"):
        plan(prompts=[A, B, (12, 5 * 24000)])            # a prompt of max_seconds
    with pytest.raises(ValueError, match="text 0"):
        plan(prompts=[(0, 24000), B, A])                 # a prompt without tokens
    with pytest.raises(ValueError, match="batch_size"):
        plan(batch_size=0)
    with pytest.raises(ValueError):
        plan_long_batch(TEXTS, [12, 9], [24000, 18000, 24000], BREAK)
    p = plan([], [])
    assert p.chunks == [] and p.groups == [] and p.doc_sizes == [] and p.frames == []
