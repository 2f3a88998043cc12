"""The cases of the edit rows' kernel tests (tests/test_gpu_session_edit_kernels.py) and of the host-only
tests of the same rules (tests/test_session_edit_plan.py): 3 slots of max_frames = 23, a pool of 64 rows.

A session of 3 slots takes at most 3 rows per call, so the five rows below go through two calls.  Call A
leaves slot 1 alone (its canaries must survive), call B fills every slot and names one pool range twice.
Between them the tables have 7, 1, 2, 5 and 1 segments (the bisection's depths 0 to 3) and hold: an insertion
at frame 0 (a generated segment first), a deletion that leaves a kept | kept junction, a replacement with a
1-frame kept segment between two generated ones, a row that is one generated segment, a row of exactly
max_frames frames, a row of 1 frame, T_in above every other T_i, two rows on one pool range, and a range
that ends at pool_rows."""
import numpy as np

import edit_ref

SLOTS, MAXT, POOL_ROWS, GUARD = 3, 23, 64, 2
WIDTHS = {"quad": (100, 100), "scalar": (6, 5)}

# name: (pool offset, L, spans)
ROWS = {
    "seven": (44, 20, [(0, 0, 6), (2, 4, 2), (5, 7, 3), (10, 14, 0)]),   # T = 23; the range ends at pool_rows
    "generated": (3, 4, [(0, 4, 5)]),                                     # one generated segment, T = 5
    "two": (10, 9, [(4, 9, 3)]),                                          # kept | generated, T = 7
    "five": (10, 9, [(1, 2, 2), (5, 6, 1)]),                              # the same pool range, T = 10
    "one": (30, 6, [(0, 5, 0)]),                                          # one kept frame, T = 1
}
# call: (rows, their slots, T_in of the admission, T_out of the retirement)
CALLS = {"A": (["seven", "generated"], [2, 0], 23, 23), "B": (["two", "five", "one"], [1, 2, 0], 23, 12)}
SCHED = (2, 0.0, 1.0, 0.5, 1.0)          # every admitted row's (num_step, t_start, t_end, t_shift, guidance_scale)


def table(name):
    _, L, spans = ROWS[name]
    return edit_ref.plan(L, spans)


def call_tables(call):
    """(tables, offsets, lens, stacked table, row_ptr) of a call's rows."""
    names = CALLS[call][0]
    tabs = [table(n) for n in names]
    stacked, ptr = edit_ref.stack(tabs, 3)
    return tabs, [ROWS[n][0] for n in names], [ROWS[n][1] for n in names], stacked, ptr


def pool_for(rng, F):
    """Full-mantissa values on the rows some case names, NaN everywhere else: a stray read shows."""
    pool = np.full((POOL_ROWS, F), np.nan, np.float32)
    for off, L, _ in ROWS.values():
        pool[off:off + L] = (-8.0 + rng.standard_normal((L, F))).astype(np.float32)
    return pool


def i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32))


def rejections():
    """(what, kind, fields that replace those of a good two-row request, the row the error must name or None).
    The good request: rows "two" and "one" into slots 1 and 0 (admit: both free, T_in = 23; retire: both done
    with lengths 7 and 1, T_out = 12); slot 2 is occupied with 3 steps left and 9 frames."""
    tabs = [table("two"), table("one")]
    good, ptr = edit_ref.stack(tabs, 3)

    def tab(fn):
        t = good.copy()
        fn(t)
        return t
    both = [
        ("a segment of length 0", dict(table=tab(lambda t: t.__setitem__((1, 2), 0))), 0),
        ("segments that do not tile", dict(table=tab(lambda t: t.__setitem__((1, 0), 5))), 0),
        ("a first segment not at 0", dict(table=tab(lambda t: t.__setitem__((2, 0), 1))), 1),
        ("a kept segment past L", dict(lens=i32([9, 5])), 1),
        ("a kept segment from a negative frame", dict(table=tab(lambda t: t.__setitem__((0, 1), -2))), 0),
        ("a negative offset", dict(offsets=i32([-1, 30])), 0),
        ("a range past pool_rows", dict(offsets=i32([10, 59])), 1),
        ("a negative L", dict(lens=i32([9, -1])), 1),
        ("row_ptr not from 0", dict(row_ptr=i32([1, 2, 3])), None),
        ("row_ptr falling", dict(row_ptr=i32([0, 3, 2])), 1),
        ("no rows", dict(n=0), None),
        ("a slot outside the session", dict(slot=i32([1, SLOTS])), 1),
        ("a negative slot", dict(slot=i32([-1, 0])), 0),
        ("a slot named twice", dict(slot=i32([1, 1])), 1),
    ]
    admit = [
        ("a slot that is not free", dict(slot=i32([1, 2])), 1),
        ("an empty row", dict(table=np.ascontiguousarray(good[:2]), row_ptr=i32([0, 2, 2])), 1),
        ("a row longer than T_in", dict(T_io=6), 0),
        ("a row longer than max_frames", dict(table=tab(lambda t: t.__setitem__((1, 2), 20))), 0),
        ("a schedule without steps", dict(sched=[SCHED, (0,) + SCHED[1:]]), 1),
        ("a schedule with t_shift 0", dict(sched=[(2, 0.0, 1.0, 0.0, 1.0), SCHED]), 0),
    ]
    retire = [
        ("a free slot", dict(free=[0]), 1),
        ("a slot with steps left", dict(slot=i32([1, 2])), 1),
        ("T_out shorter than a row", dict(T_io=6), 0),
        ("a table whose length is not the slot's", dict(table=tab(lambda t: t.__setitem__((1, 2), 4))), 0),
    ]
    return ([(w, "admit", f, r) for w, f, r in both + admit] + [(w, "retire", f, r) for w, f, r in both + retire],
            good, ptr)


CAN32, CAN8 = np.uint32(0x7FC5A5A5), np.uint8(0xA5)


def check_args(kind, Fx, Ft, **fields):
    """A zv_session_edit_check_args over numpy arrays (kept alive by the caller) and plain values."""
    from zipvoice_amd.engine import ZvSessionEditCheckArgs
    a = ZvSessionEditCheckArgs()
    a.kind, a.guard, a.slots, a.max_frames, a.pool_rows = {"admit": 0, "retire": 1}[kind], GUARD, SLOTS, MAXT, POOL_ROWS
    a.Fx, a.Ft, a.keep_original = Fx, Ft, 1
    for k, v in fields.items():
        if v is None:
            continue
        if isinstance(v, np.ndarray):
            assert v.flags["C_CONTIGUOUS"], k
            setattr(a, k, v.ctypes.data)
        else:
            setattr(a, k, v)
    return a


def run_rejection(lib, what, kind, fields, row, good, ptr, Fx=6, Ft=5):
    """One rejected call of zv_session_edit_check: it returns 1 with a message that names the row, leaves
    every output canary and the session's state arrays as they were.  Nothing here needs a device: the
    rules run on the host before anything is allocated or queued."""
    import ctypes

    from zipvoice_amd.engine import row_schedule_array
    rng = np.random.default_rng(len(what))
    fields = dict(fields)
    sched = row_schedule_array(fields.pop("sched", [SCHED, SCHED]))
    left, cur = i32([-1, -1, 3]), i32([0, 0, 9])
    if kind == "retire":
        left[:2], cur[:2] = 0, (1, 7)
        for s in fields.pop("free", []):
            left[s], cur[s] = -1, 0
    left0, cur0 = left.copy(), cur.copy()
    T_io = fields.pop("T_io", 23 if kind == "admit" else 12)
    n = fields.pop("n", 2)
    st = SLOTS * MAXT
    req = dict(slot=i32([1, 0]), offsets=i32([10, 30]), lens=i32([9, 6]), table=good, row_ptr=ptr)
    req.update(fields)
    pool = pool_for(rng, Fx)
    if kind == "admit":
        data = dict(x=rng.standard_normal((2, T_io, Fx)).astype(np.float32),
                    tc=rng.standard_normal((2, T_io, Ft)).astype(np.float32))
        outs = dict(out=np.full(st * Fx + 2 * GUARD, CAN32, np.uint32), out_tc=np.full(st * Ft + 2 * GUARD, CAN32, np.uint32),
                    out_sc=np.full(st * Fx + 2 * GUARD, CAN32, np.uint32), mout=np.full(st + 2 * GUARD, CAN8, np.uint8))
    else:
        data = dict(x=rng.standard_normal((SLOTS, MAXT, Fx)).astype(np.float32))
        outs = dict(out=np.full(2 * T_io * Fx + 2 * GUARD, CAN32, np.uint32), mout=np.full(2 * T_io + 2 * GUARD, CAN8, np.uint8))
    a = check_args(kind, Fx, Ft, n=n, T_io=T_io, pool=pool, state_left=left, state_len=cur,
                   rows=ctypes.cast(sched, ctypes.c_void_p).value, **req, **data, **outs)
    assert lib.zv_session_edit_check(ctypes.byref(a)) == 1, f"{kind}: {what} was accepted"
    msg = lib.zv_last_error().decode()
    assert f"session: {kind}_edit" in msg, (what, msg)
    if row is not None:
        assert f"row {row}:" in msg, (what, msg)
    for name, buf in outs.items():
        assert (buf == (CAN8 if buf.dtype == np.uint8 else CAN32)).all(), f"{kind}: {what}: {name} was written"
    assert np.array_equal(left, left0) and np.array_equal(cur, cur0), f"{kind}: {what}: the state changed"
    assert list(a.launch) == [0] * 8, f"{kind}: {what}: a launch was recorded"
    return msg
