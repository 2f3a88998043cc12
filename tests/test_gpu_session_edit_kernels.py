"""The two kernels of a session's edit rows (csrc/zv_session.inc: zv_session_admit_edit_kernel and
zv_session_retire_edit_kernel), each launched through the rules, the table layout and the launch function
zv_engine::session_admit_edit / session_retire_edit run (zv_session_edit_check), against
tests/session_edit_ref.py.  Everything is bit for bit: both kernels only copy and zero-fill.

Shapes (tests/session_edit_cases.py): 3 slots of max_frames = 23, a pool of 64 rows, guards of 2 elements;
(Fx, Ft) = (100, 100) the quad kernels, (6, 5) the scalar ones; two calls whose tables have 7, 1 and 2, 5, 1
segments.  The pool is NaN outside the ranges some row names, so a read outside them shows in the output;
slot buffers, out and mask_out are canary-filled, and the slots a call does not name and the guard elements
must keep their canaries.  Rejections: every rule once, outputs and the session state untouched."""
import ctypes

import numpy as np
import pytest

import session_edit_cases as sc
import session_edit_ref as ser

pytestmark = pytest.mark.gpu

S, MAXT, GUARD, CAN32, CAN8 = sc.SLOTS, sc.MAXT, sc.GUARD, sc.CAN32, sc.CAN8


@pytest.fixture(scope="module")
def lib0():
    from zipvoice_amd import engine
    return engine.load_library()


def rng_for(*key):
    return np.random.default_rng([ord(c) for c in "session edit " + " ".join(map(str, key))])


def interior(buf, n, what):
    can = CAN8 if buf.dtype == np.uint8 else CAN32
    assert (buf[:GUARD] == can).all() and (buf[GUARD + n:] == can).all(), what + ": guard elements written"
    return buf[GUARD:GUARD + n]


def run(lib0, kind, Fx, Ft, **fields):
    a = sc.check_args(kind, Fx, Ft, **fields)
    assert lib0.zv_session_edit_check(ctypes.byref(a)) == 0, lib0.zv_last_error().decode()
    assert a.launch[0] == {"admit": 0, "retire": 1}[kind] and a.launch[3] == 256
    return list(a.launch)


def sched_rows(n):
    from zipvoice_amd.engine import row_schedule_array
    return row_schedule_array([sc.SCHED] * n)


@pytest.mark.parametrize("call", sorted(sc.CALLS))
@pytest.mark.parametrize("widths", sorted(sc.WIDTHS))
def test_admit_edit(lib0, widths, call):
    Fx, Ft = sc.WIDTHS[widths]
    names, slots, T_in, _ = sc.CALLS[call]
    tabs, offsets, lens, table, ptr = sc.call_tables(call)
    n = len(names)
    rng = rng_for("admit", widths, call)
    pool = sc.pool_for(rng, Fx)
    x0 = rng.standard_normal((n, T_in, Fx)).astype(np.float32)
    tc0 = (8.0 + rng.standard_normal((n, T_in, Ft))).astype(np.float32)
    ox, ot, os_ = (np.full(S * MAXT * F + 2 * GUARD, CAN32, np.uint32) for F in (Fx, Ft, Fx))
    om = np.full(S * MAXT + 2 * GUARD, CAN8, np.uint8)
    left, cur = sc.i32([-1] * S), sc.i32([0] * S)
    rows = sched_rows(n)
    rec = run(lib0, "admit", Fx, Ft, n=n, T_io=T_in, slot=sc.i32(slots), offsets=sc.i32(offsets), lens=sc.i32(lens),
              table=table, row_ptr=ptr, rows=ctypes.cast(rows, ctypes.c_void_p).value, state_left=left, state_len=cur,
              x=x0, tc=tc0, pool=pool, out=ox, out_tc=ot, out_sc=os_, mout=om)
    what = f"admit_edit {widths} call {call}"
    assert rec[1] == int(Fx % 4 == 0 and Ft % 4 == 0) and rec[4] == n, (what, rec)
    can = lambda F: np.full((S, MAXT, F), CAN32, np.uint32).view(np.float32)
    wx, wt, ws, wm = ser.admit_edit_ref(can(Fx), can(Ft), can(Fx), np.full((S, MAXT), CAN8, np.uint8), slots, x0, tc0,
                                        pool, offsets, tabs)
    idle = [s for s in range(S) if s not in slots]
    for got, want, F, name in ((ox, wx, Fx, "x"), (ot, wt, Ft, "tc"), (os_, ws, Fx, "sc")):
        g = interior(got, S * MAXT * F, what).reshape(S, MAXT, F)
        assert np.array_equal(g, want.view(np.uint32)), f"{what}: {name}"
        assert (g[idle] == CAN32).all(), f"{what}: {name} of a slot not named was written"
        assert not np.isnan(g[slots].view(np.float32)).any(), f"{what}: {name} holds a pool row no case names"
    gm = interior(om, S * MAXT, what).reshape(S, MAXT)
    assert np.array_equal(gm, wm) and (gm[idle] == CAN8).all(), what + ": pad"
    Ts = [ser.new_length(t) for t in tabs]
    for s, T in zip(slots, Ts):
        assert gm[s].sum() == MAXT - T and not gm[s, :T].any()
    # the host state is the engine's after an admission
    want_left, want_cur = [-1] * S, [0] * S
    for s, T in zip(slots, Ts):
        want_left[s], want_cur[s] = sc.SCHED[0], T
    assert left.tolist() == want_left and cur.tolist() == want_cur


@pytest.mark.parametrize("keep", [1, 0])
@pytest.mark.parametrize("call", sorted(sc.CALLS))
@pytest.mark.parametrize("widths", sorted(sc.WIDTHS))
def test_retire_edit(lib0, widths, call, keep):
    Fx, Ft = sc.WIDTHS[widths]
    names, slots, _, T_out = sc.CALLS[call]
    tabs, offsets, lens, table, ptr = sc.call_tables(call)
    n = len(names)
    rng = rng_for("retire", widths, call)
    pool = sc.pool_for(rng, Fx)
    x = rng.standard_normal((S, MAXT, Fx)).astype(np.float32)
    Ts = [ser.new_length(t) for t in tabs]
    left, cur = sc.i32([-1] * S), sc.i32([0] * S)
    for s, T in zip(slots, Ts):
        left[s], cur[s] = 0, T
    out = np.full(n * T_out * Fx + 2 * GUARD, CAN32, np.uint32)
    mout = np.full(n * T_out + 2 * GUARD, CAN8, np.uint8)
    rec = run(lib0, "retire", Fx, Ft, n=n, T_io=T_out, keep_original=keep, slot=sc.i32(slots), offsets=sc.i32(offsets),
              lens=sc.i32(lens), table=table, row_ptr=ptr, state_left=left, state_len=cur, x=x, pool=pool, out=out,
              mout=mout)
    what = f"retire_edit {widths} call {call} keep={keep}"
    assert rec[1] == int(Fx % 4 == 0) and rec[4] == n, (what, rec)
    want, wmask = ser.retire_edit_ref(x, slots, pool, offsets, tabs, T_out, keep_original=bool(keep))
    got = interior(out, n * T_out * Fx, what).reshape(n, T_out, Fx)
    assert np.array_equal(got, want.view(np.uint32)), what
    assert not np.isnan(got.view(np.float32)).any(), what + ": a pool row no case names was read"
    assert np.array_equal(interior(mout, n * T_out, what).reshape(n, T_out), wmask), what + ": mask"
    if not keep:                                                       # the slot rows, as a plain retirement
        for i, (s, T) in enumerate(zip(slots, Ts)):
            assert np.array_equal(got[i, :T], x[s, :T].view(np.uint32)) and (got[i, T:] == 0).all()
    else:
        assert any(not np.array_equal(got[i, :T], x[s, :T].view(np.uint32)) for i, (s, T) in enumerate(zip(slots, Ts)))
    assert left.tolist() == [-1] * S and cur.tolist() == [0] * S       # the slots are free afterwards
    # without a mask: the same rows
    left[:], cur[:] = -1, 0
    for s, T in zip(slots, Ts):
        left[s], cur[s] = 0, T
    out2 = np.full(n * T_out * Fx + 2 * GUARD, CAN32, np.uint32)
    run(lib0, "retire", Fx, Ft, n=n, T_io=T_out, keep_original=keep, slot=sc.i32(slots), offsets=sc.i32(offsets),
        lens=sc.i32(lens), table=table, row_ptr=ptr, state_left=left, state_len=cur, x=x, pool=pool, out=out2)
    assert np.array_equal(out2, out)


REJECTIONS, GOOD, PTR = sc.rejections()


@pytest.mark.parametrize("widths", sorted(sc.WIDTHS))
def test_rejections_launch_nothing_and_change_nothing(lib0, widths):
    """Each rule once, at both widths: return 1, the row named, every output canary and the state arrays as
    they were; then the good request the rejections were cut from goes through."""
    Fx, Ft = sc.WIDTHS[widths]
    for what, kind, fields, row in REJECTIONS:
        sc.run_rejection(lib0, what, kind, fields, row, GOOD, PTR, Fx, Ft)
    rng = rng_for("good", widths)
    pool = sc.pool_for(rng, Fx)
    left, cur = sc.i32([-1, -1, 3]), sc.i32([0, 0, 9])
    rows = sched_rows(2)
    outs = [np.full(S * MAXT * F + 2 * GUARD, CAN32, np.uint32) for F in (Fx, Ft, Fx)]
    run(lib0, "admit", Fx, Ft, n=2, T_io=23, slot=sc.i32([1, 0]), offsets=sc.i32([10, 30]), lens=sc.i32([9, 6]),
        table=GOOD, row_ptr=PTR, rows=ctypes.cast(rows, ctypes.c_void_p).value, state_left=left, state_len=cur,
        x=rng.standard_normal((2, 23, Fx)).astype(np.float32), tc=rng.standard_normal((2, 23, Ft)).astype(np.float32),
        pool=pool, out=outs[0], out_tc=outs[1], out_sc=outs[2], mout=np.full(S * MAXT + 2 * GUARD, CAN8, np.uint8))
    assert left.tolist() == [2, 2, 3] and cur.tolist() == [1, 7, 9]
    assert (interior(outs[0], S * MAXT * Fx, "good").reshape(S, MAXT, Fx)[2] == CAN32).all()
