"""Host-only checks of a solve session's tick plan (no GPU): zv_session_plan, the function
zv_session_step itself runs, against session_ref.tick_plan and against zv_sched_plan.

A slot state is (rows, done, lens): rows[b].num_step == 0 marks a free slot, an occupied slot is active
while done[b] < num_step and runs step done[b] of its own grid.  The tick is the scheduled solve's step rule
over the active slots in slot order (tests/test_sched_plan.py), T_k the longest active row."""
import ctypes

import numpy as np
import pytest

import session_ref as sr
from test_sched_plan import SCHEDULES, bits, call_plan, row

F32 = np.float32
FREE = (0, 0.0, 0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def lib():
    from zipvoice_amd.csrc.build import build
    build(verbose=False)
    from zipvoice_amd import engine
    return engine.load_library()


def call_session_plan(lib, rows, done, lens, distill, expect_ok=True):
    from zipvoice_amd.engine import ZvSchedPlanOut, row_schedule_array
    S = len(rows)
    arr = dict(dec_src=np.full(2 * S + 1, -7, np.int32), dec_zero_text=np.full(2 * S + 1, 7, np.uint8),
               dec_zero_speech=np.full(2 * S + 1, 7, np.uint8), dec_t=np.full(2 * S + 1, -7, F32),
               act_row=np.full(S + 1, -7, np.int32), act_dt=np.full(S + 1, -7, F32),
               act_scale=np.full(S + 1, -7, F32), act_cond=np.full(S + 1, -7, np.int32),
               act_uncond=np.full(S + 1, -7, np.int32))
    out = ZvSchedPlanOut()
    for k, v in arr.items():
        setattr(out, k, v.ctypes.data)
    Tk = ctypes.c_int32(-7)
    d, ln = np.asarray(done, np.int32), np.asarray(lens, np.int32)
    rc = lib.zv_session_plan(ctypes.cast(row_schedule_array(rows if rows else [FREE]), ctypes.c_void_p), d.ctypes.data,
                             ln.ctypes.data, S, distill, ctypes.byref(out), ctypes.byref(Tk))
    if not expect_ok:
        return rc, lib.zv_last_error().decode()
    assert rc == 0, lib.zv_last_error().decode()
    A, U = out.active, out.copies
    for k, v in arr.items():                       # nothing past the tick's entries is written
        n = U + A if k.startswith("dec_") else A
        assert (v[n:] == v.dtype.type(7 if v.dtype == np.uint8 else -7)).all(), k
        arr[k] = v[:n]
    return out.steps, int(out.total_rows), A, U, arr, Tk.value


def assert_plan(got, want, what):
    for key, w in want.items():
        dtype = got[key].dtype.type
        assert np.array_equal(bits(got[key], dtype), bits(w, dtype)), (what, key, got[key], w)


@pytest.mark.parametrize("distill", [0, 1])
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_fresh_state_is_the_scheduled_solves_step_0(lib, name, distill):
    """Every slot at done == 0: zv_sched_plan's step 0 verbatim (arrays, steps, total rows), T_k = max len."""
    sched = SCHEDULES[name]
    lens = [33 + 7 * b for b in range(len(sched))][::-1]
    steps, total, A, U, got, Tk = call_session_plan(lib, sched, [0] * len(sched), lens, distill)
    wsteps, wtotal, wA, wU, want = call_plan(lib, sched, distill, 0)
    assert (steps, total, A, U, Tk) == (wsteps, wtotal, wA, wU, max(lens)), name
    assert_plan(got, want, name)
    ref, rA, rU, rT = sr.tick_plan(sched, [0] * len(sched), lens, distill)
    assert (A, U, Tk) == (rA, rU, rT)
    assert_plan(got, ref, name + " vs session_ref")


# slots 0 .. 5: at k = 0 (guided), free, at k = 2 of 4 and past t = 0.5 (guided), at k = 1 of 4 and before
# t = 0.5 (guided), unguided at k = 0, done (awaiting retire; the longest row: it must not set T_k)
MIXED_ROWS = [row(3, 1.0, 0.5), FREE, row(4, 0.7, 2.0), row(4, 2.5, 0.5), row(2, 0.0), row(1, 1.0)]
MIXED_DONE = [0, 0, 2, 1, 0, 1]
MIXED_LENS = [50, 0, 71, 33, 64, 97]


@pytest.mark.parametrize("distill", [0, 1])
def test_mixed_state(lib, distill):
    from oracle import zipvoice_np as zvo
    steps, total, A, U, got, Tk = call_session_plan(lib, MIXED_ROWS, MIXED_DONE, MIXED_LENS, distill)
    want, wA, wU, wT = sr.tick_plan(MIXED_ROWS, MIXED_DONE, MIXED_LENS, distill)
    assert (A, U, Tk) == (wA, wU, wT) == (4, 0 if distill else 3, 71)
    assert_plan(got, want, "mixed")
    assert list(got["act_row"]) == [0, 2, 3, 4]                     # slot order; the free and the done slot skipped
    assert steps == 3                                               # slot 3 has 3 steps left
    # each row's t and dt from its own grid at its own index
    for i, b in enumerate(got["act_row"]):
        r, k = MIXED_ROWS[b], MIXED_DONE[b]
        ts = zvo.get_time_steps(r[1], r[2], r[0], r[3])
        assert got["dec_t"][got["act_cond"][i]].view(np.uint32) == ts[k].view(np.uint32)
        assert got["act_dt"][i].view(np.uint32) == F32(ts[k + 1] - ts[k]).view(np.uint32)
    if not distill:
        # the copy rule per row: slot 0 at t = 0 and slot 3 at t = 0.25 * 0.5 / (1 - 0.5 * 0.25) keep the speech
        # and double the scale; slot 2 (t_shift 2 at u = 0.5: t = 2/3) zeroes it and keeps the scale
        assert list(got["dec_src"][:U]) == [0, 2, 3]
        assert list(got["dec_zero_speech"][:U]) == [0, 1, 0] and list(got["dec_zero_text"][:U]) == [1, 1, 1]
        assert np.array_equal(got["act_scale"].view(np.uint32), np.array([2.0, 0.7, 5.0, 0.0], F32).view(np.uint32))
        assert list(got["act_uncond"]) == [0, 1, 2, -1]
        # the ticks to come with nothing admitted: (4 + 3) + (3 + 2: slot 4 and slots 0, 2, 3) ...
        left = [(r[0] - d) if r[0] else 0 for r, d in zip(MIXED_ROWS, MIXED_DONE)]
        guided = [F32(r[4]) != 0 for r in MIXED_ROWS]
        assert total == sum(sum(1 + int(guided[b]) for b in range(6) if left[b] > j) for j in range(3))
    else:
        assert np.array_equal(got["act_scale"].view(np.uint32), np.array([1.0, 0.7, 2.5, 0.0], F32).view(np.uint32))
        assert list(got["act_uncond"]) == [-1] * 4 and list(got["act_cond"]) == [0, 1, 2, 3]


def test_ticks_walk_each_rows_grid(lib):
    """Stepping the state by hand (done += 1 on the active slots), with a row entering a freed slot midway:
    every row's collected t and dt are its own grid, whatever ran beside it."""
    from oracle import zipvoice_np as zvo
    rows, done, lens = [row(3, 1.0, 0.5), FREE, row(1, 2.5, 0.7, 0.25, 0.9)], [0, 0, 0], [50, 0, 33]
    late = {1: (1, row(2, 0.0)), 2: (2, row(2, 0.7))}                # tick -> (slot, row): slot 2 is reused
    seen = {}
    for tick in range(5):
        if tick in late:
            b, r = late[tick]
            assert rows[b][0] == 0 or done[b] == rows[b][0]
            rows[b], done[b], lens[b] = r, 0, 40 + tick
        _, _, A, U, got, Tk = call_session_plan(lib, rows, done, lens, 0)
        assert Tk == max([lens[b] for b in range(3) if rows[b][0] and done[b] < rows[b][0]] + [0])
        for i, b in enumerate(got["act_row"]):
            seen.setdefault((b, rows[b]), []).append((got["dec_t"][got["act_cond"][i]], got["act_dt"][i]))
            done[b] += 1
    assert len(seen) == 4
    for (b, r), td in seen.items():
        ts = zvo.get_time_steps(r[1], r[2], r[0], r[3])
        assert np.array_equal(np.asarray([t for t, _ in td], F32).view(np.uint32), ts[:-1].view(np.uint32)), (b, r)
        assert np.array_equal(np.asarray([d for _, d in td], F32).view(np.uint32),
                              np.diff(ts).astype(F32).view(np.uint32)), (b, r)


def test_no_active_slot(lib):
    steps, total, A, U, got, Tk = call_session_plan(lib, [FREE, row(2, 1.0)], [0, 2], [0, 50], 0)
    assert (steps, total, A, U, Tk) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("rows,done,lens,word", [
    ([], [0], [1], "slots"),
    ([row(-1)], [0], [5], "num_step"),
    ([row(2, float("nan"))], [0], [5], "finite"),
    ([row(2, 1.0, 0.0)], [0], [5], "t_shift"),
    ([row(2, 1.0, 1.0, float("inf"))], [0], [5], "finite"),
    ([row(2), row(2)], [0, 3], [5, 5], "done"),
    ([row(2), row(2)], [-1, 0], [5, 5], "done"),
    ([row(2)], [0], [0], "length"),
])
def test_rejections(lib, rows, done, lens, word):
    rc, msg = call_session_plan(lib, rows, done, lens, 0, expect_ok=False)
    assert rc != 0 and word in msg, msg
