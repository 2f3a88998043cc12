"""The host half of speech editing (zipvoice_amd/edit.py): spans -> frame table -> sample table,
against the frame-by-frame restatement in tests/edit_ref.py and against tables written out by
hand.  No GPU."""
import numpy as np
import pytest

import edit_ref
from zipvoice_amd.edit import (mask_spans, plan_edit, plan_edit_batch, sample_table,
                               sample_table_batch, seconds_to_frames, span_frames, table_length)

L = 20
CASES = {
    "no spans": ([], [(0, 0, 20)]),
    "span at frame 0": ([(0, 4, 6)], [(0, -1, 6), (6, 4, 16)]),
    "span ending at L": ([(15, 20, 3)], [(0, 0, 15), (15, -1, 3)]),
    "insertion": ([(7, 7, 5)], [(0, 0, 7), (7, -1, 5), (12, 7, 13)]),
    "insertion at 0": ([(0, 0, 2)], [(0, -1, 2), (2, 0, 20)]),
    "insertion at L": ([(20, 20, 2)], [(0, 0, 20), (20, -1, 2)]),
    "deletion": ([(5, 9, 0)], [(0, 0, 5), (5, 9, 11)]),
    "deletion at 0": ([(0, 3, 0)], [(0, 3, 17)]),
    "touching spans merged": ([(3, 6, 2), (6, 8, 0), (8, 8, 4)], [(0, 0, 3), (3, -1, 6), (9, 8, 12)]),
    "1-frame segments": ([(1, 2, 1), (3, 4, 1), (5, 5, 1)],
                         [(0, 0, 1), (1, -1, 1), (2, 2, 1), (3, -1, 1), (4, 4, 1), (5, -1, 1), (6, 5, 15)]),
    "everything replaced": ([(0, 20, 7)], [(0, -1, 7)]),
    "everything deleted": ([(0, 20, 0)], []),
}


@pytest.mark.parametrize("name", list(CASES))
def test_tables(name):
    spans, want = CASES[name]
    tab = plan_edit(L, spans)
    assert tab.dtype == np.int32 and tab.shape == (len(want), 3)
    assert tab.tolist() == [list(r) for r in want]
    assert np.array_equal(tab, edit_ref.plan(L, spans))
    T = L - sum(e - s for s, e, _ in spans) + sum(n for _, _, n in spans)
    assert table_length(tab) == T
    # the segments tile [0, T) and none is empty
    assert (tab[:, 2] > 0).all()
    assert np.array_equal(tab[:, 0], np.concatenate([[0], np.cumsum(tab[:, 2])[:-1]])[:len(tab)])


def test_random_plans_match_the_reference():
    rng = np.random.default_rng(0)
    for _ in range(200):
        Lr = int(rng.integers(0, 30))
        cuts = np.sort(rng.integers(0, Lr + 1, 2 * int(rng.integers(0, 4))))
        spans = []
        for s, e in zip(cuts[::2], cuts[1::2]):
            n = int(rng.integers(0, 5))
            if s == e and n == 0:
                n = 1
            spans.append((int(s), int(e), n))
        assert np.array_equal(plan_edit(Lr, spans), edit_ref.plan(Lr, spans)), (Lr, spans)


def test_prefix_prompt_table():
    P, G = 33, 41
    assert plan_edit(P, [(P, P, G)]).tolist() == [[0, 0, P], [P, -1, G]]
    # the same over features padded to L > P: the padding is what the span replaces
    assert plan_edit(P + 9, [(P, P + 9, G)]).tolist() == [[0, 0, P], [P, -1, G]]


def test_batch_stacks_rows():
    plan = plan_edit_batch([20, 5, 8], [[(7, 7, 5)], [], [(0, 8, 0)]])
    assert plan.row_ptr.tolist() == [0, 3, 4, 4]
    assert plan.lens.tolist() == [20, 5, 8] and plan.new_lens.tolist() == [25, 5, 0]
    assert plan.row(1).tolist() == [[0, 0, 5]] and plan.row(2).shape == (0, 3)
    assert plan.generated(0) == 5 and plan.generated(1) == 0
    assert plan.table.dtype == np.int32 and plan.row_ptr.dtype == np.int32
    with pytest.raises(ValueError, match="rows"):
        plan_edit_batch([20], [[], []])


@pytest.mark.parametrize("spans,msg", [
    ([(-1, 3, 1)], "row 4 span 0: need 0 <= s <= e <= L"),
    ([(5, 3, 1)], "row 4 span 0: need 0 <= s <= e <= L"),
    ([(5, 21, 1)], "row 4 span 0: need 0 <= s <= e <= L"),
    ([(2, 6, 1), (5, 8, 1)], "row 4 span 1: spans must be sorted and disjoint"),
    ([(10, 12, 1), (2, 4, 1)], "row 4 span 1: spans must be sorted and disjoint"),
    ([(2, 4, -1)], "row 4 span 0: n must be non-negative"),
    ([(2, 4, 1), (9, 9, 0)], "row 4 span 1: an empty span that generates nothing"),
    ([(2, 4)], "row 4 span 0: expected three integers"),
    ([(2, 4, 1.5)], "row 4 span 0: expected three integers"),
])
def test_validation_errors_name_row_and_span(spans, msg):
    with pytest.raises(ValueError, match=msg):
        plan_edit(L, spans, row=4)
    with pytest.raises(ValueError, match=msg):
        plan_edit_batch([3, 3, 3, 3, L], [[], [], [], [], spans])


@pytest.mark.parametrize("delta", [-100, 100])
def test_sample_table_runs_to_the_true_sample_count(delta):
    hop = 256
    N = L * hop + delta
    assert (N + hop // 2) // hop == L
    # the last kept segment ends at frame L: it runs to sample N, short or long of L * hop
    tab = sample_table(plan_edit(L, [(7, 9, 5)]), N, hop)
    assert tab.dtype == np.int32
    assert tab.tolist() == [[0, 0, 7 * hop, 0], [7 * hop, 7 * hop, 5 * hop, 1],
                            [12 * hop, 9 * hop, N - 9 * hop, 0]]
    assert table_length(tab) == N + 3 * hop
    # a kept segment that stops before L ends on a frame edge; the generated tail reads the
    # vocoder's output at the new frame positions
    tab = sample_table(plan_edit(L, [(0, 0, 2), (15, 20, 3)]), N, hop)
    assert tab.tolist() == [[0, 0, 2 * hop, 1], [2 * hop, 0, 15 * hop, 0], [17 * hop, 17 * hop, 3 * hop, 1]]
    # a deletion: two kept segments meet
    tab = sample_table(plan_edit(L, [(5, 9, 0)]), N, hop)
    assert tab.tolist() == [[0, 0, 5 * hop, 0], [5 * hop, 9 * hop, N - 9 * hop, 0]]
    # no spans: the recording itself
    assert sample_table(plan_edit(L, []), N, hop).tolist() == [[0, 0, N, 0]]
    for spans in ([(7, 9, 5)], [(19, 20, 1)], [(0, 1, 0), (19, 19, 1)]):
        p = plan_edit(L, spans)
        assert np.array_equal(sample_table(p, N, hop), edit_ref.sample_table(p, N, hop, L))
    plan = plan_edit_batch([L, L], [[(7, 9, 5)], []])
    table, ptr = sample_table_batch(plan, [N, N - 3], hop)
    assert ptr.tolist() == [0, 3, 4] and table[3].tolist() == [0, 0, N - 3, 0]


def test_span_frames_rounds_half_up():
    assert span_frames(30, 10, 10) == 30
    assert span_frames(30, 10, 5) == 15
    assert span_frames(25, 10, 1) == 3                  # 2.5 -> 3
    assert span_frames(35, 10, 1) == 4                  # 3.5 -> 4 (not to even)
    assert span_frames(24, 10, 1) == 2                  # 2.4 -> 2
    assert span_frames(30, 10, 10, speed=2.0) == 15
    assert span_frames(30, 10, 5, speed=0.8) == 19      # 18.75 -> 19
    assert span_frames(30, 10, 0) == 0
    # an insertion has no rate of its own: the recording's L / S
    assert span_frames(0, 0, 4, frames_per_token=200 / 80) == 10
    assert span_frames(0, 0, 3, frames_per_token=2.5) == 8           # 7.5 -> 8
    with pytest.raises(ValueError):
        span_frames(0, 0, 4)
    with pytest.raises(ValueError):
        span_frames(30, 10, 4, speed=0.0)


def test_seconds_to_frames():
    assert seconds_to_frames(0.0) == 0
    assert seconds_to_frames(1.0) == 94                 # 93.75 -> 94
    assert seconds_to_frames(0.016) == 2                # 1.5 -> 2
    assert seconds_to_frames(1.0, sampling_rate=16000, hop=160) == 100


def test_mask_spans():
    m = np.zeros(12, bool)
    m[[0, 1, 4, 5, 6, 9, 11]] = True
    assert mask_spans(m, 12) == [(0, 2, 2), (4, 7, 3), (9, 10, 1), (11, 12, 1)]
    assert mask_spans(m, 10) == [(0, 2, 2), (4, 7, 3), (9, 10, 1)]    # the padding is no span
    assert mask_spans(np.zeros(5, bool), 5) == []
