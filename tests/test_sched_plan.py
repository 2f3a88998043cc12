"""Host-only checks of the scheduled solve's plan (no GPU): zv_sched_plan, the function
zv_euler_sample_sched itself runs, against a numpy restatement of the rules written here.

Row b of a schedule integrates its own grid get_time_steps(t_start, t_end, num_step, t_shift) with its own
scale g, as EulerSolver.sample would on that row alone.  Step k of the solve (K = max num_step steps):
  active rows: those with k < num_step, in input order;
  not distilled: a row has an unconditional copy iff it is active and g != 0; at the row's own t = ts[k]
    (float32): t > 0.5 zeroes the copy's speech and keeps g, else the speech stays and the scale is
    fl32(2 g); the copy's text is always zeroed; a row without a copy has scale 0 and no unconditional row;
  the decoder batch: the copies in active order, then the conditional rows in active order;
  distilled: no copies, the row's g as it is (the guidance embedding's input);
  dt = ts[k + 1] - ts[k] in float32; the whole solve launches sum_k (copies_k + active_k) decoder rows."""
import ctypes

import numpy as np
import pytest

from oracle import zipvoice_np as zvo

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from zipvoice_amd.csrc.build import build
    build(verbose=False)
    from zipvoice_amd import engine
    return engine.load_library()


def row(num_step, g=0.0, t_shift=1.0, t_start=0.0, t_end=1.0):
    return (num_step, t_start, t_end, t_shift, g)


SCHEDULES = {
    "one": [row(3, 1.0, 0.5)],
    "one_unguided": [row(2)],
    "equal": [row(3, 1.0, 0.5)] * 3,
    "steps": [row(3, 1.0), row(1, 1.0), row(2, 1.0), row(3, 1.0)],
    "shifts": [row(4, 0.7, 0.5), row(4, 0.7, 1.0, 0.25, 0.9), row(3, 0.7, 0.7, 0.25, 0.9), row(5, 0.7, 2.0)],
    "scales": [row(2, 0.0), row(2, -0.5), row(2, 2.5), row(2, 0.0), row(2, 1e-30)],
    # the pool of the issue: a draft next to a final render, guided next to unguided
    "mixed": [row(3, 1.0, 0.5), row(1, 0.0, 1.0), row(2, 2.5, 0.7, 0.25, 0.9), row(3, 0.0, 0.5)],
    # ts = [0, 0.5, 1]: a step exactly at 0.5 (speech kept, scale doubled) next to its neighbours
    "half": [row(2, 0.7), row(4, 0.7), row(2, -3.0)],
    "last_row_longest": [row(1, 1.0), row(1, 0.0), row(6, 0.3, 0.5)],
}


def call_plan(lib, sched, distill, step):
    from zipvoice_amd.engine import ZvSchedPlanOut, row_schedule_array
    B = len(sched)
    rows = row_schedule_array(sched)
    arr = dict(dec_src=np.full(2 * B + 1, -7, np.int32), dec_zero_text=np.full(2 * B + 1, 7, np.uint8),
               dec_zero_speech=np.full(2 * B + 1, 7, np.uint8), dec_t=np.full(2 * B + 1, -7, F32),
               act_row=np.full(B + 1, -7, np.int32), act_dt=np.full(B + 1, -7, F32),
               act_scale=np.full(B + 1, -7, F32), act_cond=np.full(B + 1, -7, np.int32),
               act_uncond=np.full(B + 1, -7, np.int32))
    out = ZvSchedPlanOut()
    for k, v in arr.items():
        setattr(out, k, v.ctypes.data)
    rc = lib.zv_sched_plan(ctypes.cast(rows, ctypes.c_void_p), B, distill, step, ctypes.byref(out))
    assert rc == 0, lib.zv_last_error().decode()
    A, U = out.active, out.copies
    for k, v in arr.items():                       # nothing past the step's entries is written
        n = U + A if k.startswith("dec_") else A
        assert (v[n:] == v.dtype.type(7 if v.dtype == np.uint8 else -7)).all(), k
        arr[k] = v[:n]
    return out.steps, int(out.total_rows), A, U, arr


def restate(sched, distill, k):
    """The rules of the module docstring, in numpy."""
    ts = [zvo.get_time_steps(r[1], r[2], r[0], r[3]) for r in sched]
    active = [b for b, r in enumerate(sched) if k < r[0]]
    guided = [b for b in active if not distill and F32(sched[b][4]) != 0]
    U, A = len(guided), len(active)
    dec_src = guided + active
    zt = [1] * U + [0] * A
    zs = [int(ts[b][k] > F32(0.5)) for b in guided] + [0] * A
    t = [ts[b][k] for b in dec_src]
    dt = [F32(ts[b][k + 1] - ts[b][k]) for b in active]
    scale, unc = [], []
    for b in active:
        g = F32(sched[b][4])
        if distill:
            scale.append(g)
            unc.append(-1)
        elif b in guided:
            scale.append(g if ts[b][k] > F32(0.5) else F32(g * F32(2.0)))
            unc.append(guided.index(b))
        else:
            scale.append(F32(0.0))
            unc.append(-1)
    cond = [U + i for i in range(A)]
    return dict(dec_src=dec_src, dec_zero_text=zt, dec_zero_speech=zs, dec_t=t, act_row=active, act_dt=dt,
                act_scale=scale, act_cond=cond, act_uncond=unc), A, U


def bits(a, dtype):
    a = np.asarray(a, dtype)
    return a.view(np.uint32) if dtype == F32 else a


@pytest.mark.parametrize("distill", [0, 1])
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_plan_matches_restatement(lib, name, distill):
    sched = SCHEDULES[name]
    K = max(r[0] for r in sched)
    total = 0
    for k in range(K):
        steps, total_rows, A, U, got = call_plan(lib, sched, distill, k)
        want, wA, wU = restate(sched, distill, k)
        assert (steps, A, U) == (K, wA, wU), (name, k)
        for key, w in want.items():
            dtype = got[key].dtype.type
            assert np.array_equal(bits(got[key], dtype), bits(w, dtype)), (name, k, key, got[key], w)
        # input order, and the copy set exactly {active, g != 0} (none in distill)
        assert list(got["act_row"]) == sorted(got["act_row"])
        guided = [b for b in got["act_row"] if not distill and F32(sched[b][4]) != 0]
        assert list(got["dec_src"][:U]) == guided
        total += U + A
    assert total_rows == total


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_rows_follow_their_own_grid(lib, name):
    """Collected over the steps, each row's t and dt are its own get_time_steps grid, bit for bit."""
    sched = SCHEDULES[name]
    K = max(r[0] for r in sched)
    t_of, dt_of = {b: [] for b in range(len(sched))}, {b: [] for b in range(len(sched))}
    for k in range(K):
        _, _, A, U, got = call_plan(lib, sched, 0, k)
        for i, b in enumerate(got["act_row"]):
            t_of[b].append(got["dec_t"][got["act_cond"][i]])
            dt_of[b].append(got["act_dt"][i])
            if got["act_uncond"][i] >= 0:
                assert got["dec_t"][got["act_uncond"][i]].view(np.uint32) == t_of[b][-1].view(np.uint32)
    for b, r in enumerate(sched):
        ts = zvo.get_time_steps(r[1], r[2], r[0], r[3])
        assert ts.dtype == F32
        assert np.array_equal(np.asarray(t_of[b], F32).view(np.uint32), ts[:-1].view(np.uint32)), (name, b)
        assert np.array_equal(np.asarray(dt_of[b], F32).view(np.uint32), np.diff(ts).astype(F32).view(np.uint32)), (name, b)


def test_speech_zeroed_strictly_above_half(lib):
    sched = SCHEDULES["half"]
    ts = zvo.get_time_steps(0.0, 1.0, 2, 1.0)
    assert ts[1] == F32(0.5)
    _, _, A, U, got = call_plan(lib, sched, 0, 1)
    assert list(got["dec_src"][:U]) == [0, 1, 2]
    # rows 0 and 2 sit exactly at 0.5: speech kept, scale 2 g; row 1 (4 steps) is at 0.25
    assert list(got["dec_zero_speech"][:U]) == [0, 0, 0] and list(got["dec_zero_text"][:U]) == [1, 1, 1]
    assert np.array_equal(got["act_scale"].view(np.uint32), np.array([1.4, 1.4, -6.0], F32).view(np.uint32))
    _, _, _, U3, got3 = call_plan(lib, sched, 0, 3)         # only row 1 is left, at t = 0.75
    assert U3 == 1 and list(got3["dec_zero_speech"][:1]) == [1] and got3["act_scale"][0] == F32(0.7)


@pytest.mark.parametrize("t_shift,g", [(0.5, 1.0), (1.0, 0.7), (0.7, -0.5)])
def test_fully_guided_and_active_is_cfg_plans_layout(lib, t_shift, g):
    """Every row active and guided: [uncond B | cond B] with zv_cfg_plan's flag and scale at the step's t."""
    B, n = 3, 4
    sched = [row(n, g, t_shift)] * B
    for k in range(n):
        _, total, A, U, got = call_plan(lib, sched, 0, k)
        assert (A, U, total) == (B, B, 2 * B * n)
        assert list(got["dec_src"]) == list(range(B)) * 2
        assert list(got["act_cond"]) == [B + b for b in range(B)] and list(got["act_uncond"]) == list(range(B))
        copies, zs, go, gm = ctypes.c_int(), ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
        assert lib.zv_cfg_plan(float(got["dec_t"][0]), g, 0, 0, 0, ctypes.byref(copies), ctypes.byref(zs),
                               ctypes.byref(go), ctypes.byref(gm)) == 0
        assert copies.value == 2
        assert list(got["dec_zero_speech"]) == [zs.value] * B + [0] * B
        assert list(got["dec_zero_text"]) == [1] * B + [0] * B
        assert (got["act_scale"] == F32(go.value)).all()


def test_totals_of_the_mixed_pool(lib):
    """The mixed pool: active rows 4 + 3 + 2 and copies 2 + 2 + 1 = 14 decoder rows over 3 steps, where the
    most expensive setting for every row would launch 2 * 4 * 3 = 24."""
    steps, total, _, _, _ = call_plan(lib, SCHEDULES["mixed"], 0, 0)
    assert (steps, total) == (3, 14)
    steps, total, A, U, _ = call_plan(lib, SCHEDULES["mixed"], 1, 0)
    assert (steps, total, A, U) == (3, 9, 4, 0)


@pytest.mark.parametrize("bad,word", [
    ([], "B must be"),
    ([row(0)], "num_step"),
    ([row(2), row(-1)], "num_step"),
    ([row(2, float("nan"))], "finite"),
    ([row(2, 1.0, float("inf"))], "finite"),
    ([row(2, 1.0, 1.0, float("nan"))], "finite"),
    ([row(2, 1.0, 1.0, 0.0, float("-inf"))], "finite"),
    ([row(2, 1.0, 0.0)], "t_shift"),
    ([row(2, 1.0, -0.5)], "t_shift"),
])
def test_rejections(lib, bad, word):
    from zipvoice_amd.engine import ZvSchedPlanOut, row_schedule_array
    rows = row_schedule_array(bad if bad else [row(1)])
    out = ZvSchedPlanOut()
    rc = lib.zv_sched_plan(ctypes.cast(rows, ctypes.c_void_p), len(bad), 0, 0, ctypes.byref(out))
    assert rc != 0
    msg = lib.zv_last_error().decode()
    assert msg and word in msg, msg


def test_step_outside_the_schedule_is_rejected(lib):
    from zipvoice_amd.engine import ZvSchedPlanOut, row_schedule_array
    rows = row_schedule_array([row(2), row(3)])
    out = ZvSchedPlanOut()
    for step in (-1, 3):
        assert lib.zv_sched_plan(ctypes.cast(rows, ctypes.c_void_p), 2, 0, step, ctypes.byref(out)) != 0
        assert "step" in lib.zv_last_error().decode()
    assert lib.zv_sched_plan(ctypes.cast(rows, ctypes.c_void_p), 2, 0, 2, ctypes.byref(out)) == 0
    assert (out.steps, out.active, out.copies) == (3, 1, 0)
