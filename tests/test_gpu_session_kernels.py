"""The solve session's kernels (csrc/zv_session.inc: admit, retire and the operand build, mask gather and
Euler update at the session's two strides), each launched through the launch function zv_engine::session_*
calls (zv_session_check), against tests/session_ref.py.

Everything is bit for bit: admit, retire and the mask gather are copies and zero fills; the operand build is
a copy through kr.split16 (both operand libraries, with and without the lo half); the update is compared with
session_ref.euler_update_ref on dyadic operands (every fp32 step exact, so the comparison does not depend on
how the compiler contracts the two expressions) and, on general operands, with the scheduled solve's kernel
(zv_sched_check on the same rows: both inline euler_combine / euler_step).  Slots that a call does not
name, the frames >= T_k of a slot the update does name, guard elements and pad columns keep their canaries.

Shapes: 4 slots of max_frames = 97; (Fx, Ft) = (100, 100) the quad kernels, (200, 100) stereo, (6, 5) the
scalar kernels; T_in in {97, 40}; lens and T_k in {1, 40, 97}."""
import ctypes

import numpy as np
import pytest

import kernel_ref as kr
import session_ref as sr

pytestmark = pytest.mark.gpu

ADMIT, RETIRE, BUILD, GATHER, EULER = range(5)
CAN32, CAN16, CAN8 = np.uint32(0x7FC5A5A5), np.uint16(0x7FA5), np.uint8(0xA5)
GUARD = 2
S, MAXT = 4, 97
WIDTHS = {"quad": (100, 100), "stereo": (200, 100), "scalar": (6, 5)}


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=request.param)


@pytest.fixture(scope="module")
def lib0():
    from zipvoice_amd import engine
    return engine.load_library()


def call(Lb, kind, **fields):
    from zipvoice_amd.engine import ZvSessionCheckArgs
    a = ZvSessionCheckArgs()
    a.kind, a.guard, a.slots, a.max_frames = kind, GUARD, S, MAXT
    for k, v in fields.items():
        if v is None:
            continue
        if isinstance(v, np.ndarray):
            assert v.flags["C_CONTIGUOUS"]
            setattr(a, k, v.ctypes.data)
        else:
            setattr(a, k, v)
    rc = Lb.zv_session_check(ctypes.byref(a))
    assert rc == 0, Lb.zv_last_error().decode()
    assert a.launch[0] == kind and a.launch[3] == 256
    return list(a.launch)


def rng_for(*key):
    return np.random.default_rng([ord(c) for c in "session " + " ".join(map(str, key))])


def i32(a):
    return np.asarray(a, np.int32)


def flat_canary(n):
    return np.full(n + 2 * GUARD, CAN32, np.uint32)


def flat_interior(buf, n, what):
    assert (buf[:GUARD] == buf.dtype.type(CAN32 if buf.dtype == np.uint32 else CAN8)).all() and \
        (buf[GUARD + n:] == buf.dtype.type(CAN32 if buf.dtype == np.uint32 else CAN8)).all(), what + ": guard elements written"
    return buf[GUARD:GUARD + n]


def slot_state(rng, Fx, Ft):
    """Slot buffers with full-mantissa values, the three tensors far apart."""
    x = rng.standard_normal((S, MAXT, Fx)).astype(np.float32)
    tc = (8.0 + rng.standard_normal((S, MAXT, Ft))).astype(np.float32)
    sc = (-8.0 + rng.standard_normal((S, MAXT, Fx))).astype(np.float32)
    return x, tc, sc


# (T_in, slots, lens): out of slot order; the full, the one-frame and a middle length; slot 1 is never named
ADMITS = {97: (97, [3, 0, 2], [97, 1, 40]), 40: (40, [2, 0], [40, 1])}


@pytest.mark.parametrize("T_in", sorted(ADMITS))
@pytest.mark.parametrize("widths", sorted(WIDTHS))
def test_admit(lib0, widths, T_in):
    Fx, Ft = WIDTHS[widths]
    _, slots, lens = ADMITS[T_in]
    n = len(slots)
    rng = rng_for("admit", widths, T_in)
    x0 = rng.standard_normal((n, T_in, Fx)).astype(np.float32)
    tc0 = (8.0 + rng.standard_normal((n, T_in, Ft))).astype(np.float32)
    sc0 = (-8.0 + rng.standard_normal((n, T_in, Fx))).astype(np.float32)
    ox, ot, os_ = flat_canary(S * MAXT * Fx), flat_canary(S * MAXT * Ft), flat_canary(S * MAXT * Fx)
    om = np.full(S * MAXT + 2 * GUARD, CAN8, np.uint8)
    rec = call(lib0, ADMIT, n=n, T_io=T_in, Fx=Fx, Ft=Ft, Fs=Fx, slot=i32(slots), len=i32(lens), x=x0, tc=tc0, sc=sc0,
               out=ox, out_tc=ot, out_sc=os_, mout=om)
    what = f"admit {widths} T_in={T_in}"
    assert rec[1] == int(Fx % 4 == 0 and Ft % 4 == 0) and rec[4] == n, (what, rec)
    can = lambda F: np.full((S, MAXT, F), CAN32, np.uint32).view(np.float32)
    wx, wt, ws, wm = sr.admit_ref(can(Fx), can(Ft), can(Fx), np.full((S, MAXT), CAN8, np.uint8), slots, lens, x0, tc0, sc0)
    for got, want, F, name in ((ox, wx, Fx, "x"), (ot, wt, Ft, "tc"), (os_, ws, Fx, "sc")):
        g = flat_interior(got, S * MAXT * F, what).reshape(S, MAXT, F)
        assert np.array_equal(g, want.view(np.uint32)), f"{what}: {name}"
        assert (g[1] == CAN32).all(), f"{what}: {name} of a slot not named was written"
    gm = flat_interior(om, S * MAXT, what).reshape(S, MAXT)
    assert np.array_equal(gm, wm) and (gm[1] == CAN8).all(), what + ": pad"
    for s, ln in zip(slots, lens):
        assert gm[s].sum() == MAXT - ln and not gm[s, :ln].any()


@pytest.mark.parametrize("T_out", [97, 41])
@pytest.mark.parametrize("widths", sorted(WIDTHS))
def test_retire(lib0, widths, T_out):
    Fx, Ft = WIDTHS[widths]
    slots, lens = ([3, 0, 2], [97, 1, 40]) if T_out == 97 else ([2, 0], [40, 1])
    n = len(slots)
    x, _, _ = slot_state(rng_for("retire", widths), Fx, Ft)
    out = flat_canary(n * T_out * Fx)
    rec = call(lib0, RETIRE, n=n, T_io=T_out, Fx=Fx, slot=i32(slots), len=i32(lens), x=x, out=out)
    what = f"retire {widths} T_out={T_out}"
    assert rec[1] == int(Fx % 4 == 0) and rec[4] == n, (what, rec)
    got = flat_interior(out, n * T_out * Fx, what).reshape(n, T_out, Fx)
    assert np.array_equal(got, sr.retire_ref(x, slots, lens, T_out).view(np.uint32)), what


# decoder rows over the slots {0, 2, 3} (slot 1 idle): copies of 2 and 3 with different speech flags, then the rows
MAP = ([2, 3, 0, 2, 3], [1, 1, 0, 0, 0], [1, 0, 0, 0, 0])


@pytest.mark.parametrize("Tk", [1, 40, 97])
@pytest.mark.parametrize("widths", sorted(WIDTHS))
def test_build_input(lib, widths, Tk):
    fmt, Lb = lib
    Fx, Ft = WIDTHS[widths]
    src, zt, zs = MAP
    N, Fin = len(src), 2 * Fx + Ft
    ld = -(-Fin // 64) * 64 if Fx % 4 == 0 else Fin + 2
    x, tc, sc = slot_state(rng_for("build", widths), Fx, Ft)
    hi, lw = kr.split16(sr.build_input_ref(x, tc, sc, src, zt, zs, Tk).astype(np.float64), fmt)
    assert np.abs(lw).max() > 0
    for lo in (True, False):
        oh = np.full((N * Tk + 2 * GUARD, ld), CAN16, np.uint16)
        ol = np.full((N * Tk + 2 * GUARD, ld), CAN16, np.uint16) if lo else None
        rec = call(Lb, BUILD, T_k=Tk, N=N, Fx=Fx, Ft=Ft, Fs=Fx, ld=ld, x=x, tc=tc, sc=sc, src=i32(src),
                   zero_text=np.asarray(zt, np.uint8), zero_speech=np.asarray(zs, np.uint8), oh=oh, ol=ol)
        what = f"{fmt} session build {widths} T_k={Tk} lo={lo}"
        assert rec[1] == int(Fx % 4 == 0 and Ft % 4 == 0 and ld % 4 == 0) and rec[4] == N, (what, rec)
        for buf, want, half in ((oh, hi, "hi"), (ol, lw, "lo")):
            if buf is None:
                continue
            mask = np.ones(buf.shape, bool)
            mask[GUARD:GUARD + N * Tk, :Fin] = False
            assert (buf[mask] == CAN16).all(), f"{what}: {half} written outside the output"
            assert np.array_equal(kr.decode16(buf[GUARD:GUARD + N * Tk, :Fin], fmt), want), f"{what}: {half}"


@pytest.mark.parametrize("Tk", [1, 40, 97])
def test_mask_gather(lib0, Tk):
    src = MAP[0]
    N = len(src)
    m = rng_for("mask", Tk).integers(0, 2, (S, MAXT)).astype(np.uint8)
    mout = np.full(N * Tk + 2 * GUARD, CAN8, np.uint8)
    rec = call(lib0, GATHER, T_k=Tk, N=N, mask=m, src=i32(src), mout=mout)
    assert rec[4] == N and rec[2] == 1, rec
    got = flat_interior(mout, N * Tk, f"mask T_k={Tk}").reshape(N, Tk)
    assert np.array_equal(got, sr.mask_gather_ref(m, src, Tk))


# the update of MAP's tick: slots 0, 2, 3 active, 2 and 3 guided; slot 1 is not listed
UPD = ([0, 2, 3], [2, 3, 4], [-1, 0, 1])


def euler_case(rng, Fx, Tk, klass):
    row, cond, unc = UPD
    N = 5
    if klass == "exact":                 # small integers, dyadic scales and steps: every fp32 step is exact
        x = rng.integers(-8, 9, (S, MAXT, Fx)).astype(np.float32)
        v = rng.integers(-8, 9, (N, Tk, Fx)).astype(np.float32)
        scale, dt = [1.5, -0.5, 6.0], [0.125, 0.25, -0.5]
    else:
        x = rng.standard_normal((S, MAXT, Fx)).astype(np.float32)
        v = (3.0 * rng.standard_normal((N, Tk, Fx))).astype(np.float32)
        scale, dt = [0.7, 5.0, -0.3], [0.0625, 0.337, 0.1]
    # canaries where the update must not write: the slot not listed, and the frames >= T_k of the listed ones
    xu = x.view(np.uint32)
    xu[1] = CAN32
    xu[:, Tk:] = CAN32
    return x, v, row, cond, unc, np.asarray(scale, np.float32), np.asarray(dt, np.float32)


def run_session_euler(lib0, x, v, row, cond, unc, scale, dt, Fx, Tk, what):
    out = flat_canary(S * MAXT * Fx)
    rec = call(lib0, EULER, T_k=Tk, N=v.shape[0], A=len(row), Fx=Fx, x=x, v=v, row=i32(row), dt=dt, scale=scale,
               cond=i32(cond), uncond=i32(unc), out=out)
    assert rec[4] == len(row) and rec[2] == min(-(-Tk * Fx // 256), 1024), (what, rec)
    got = flat_interior(out, S * MAXT * Fx, what).reshape(S, MAXT, Fx)
    assert (got[1] == CAN32).all(), what + ": the slot not listed was written"
    assert (got[:, Tk:] == CAN32).all(), what + ": frames >= T_k were written"
    return got


@pytest.mark.parametrize("Tk", [1, 40, 97])
@pytest.mark.parametrize("widths", sorted(WIDTHS))
def test_euler_update_exact(lib0, widths, Tk):
    Fx, _ = WIDTHS[widths]
    x, v, row, cond, unc, scale, dt = euler_case(rng_for("euler exact", widths, Tk), Fx, Tk, "exact")
    what = f"session euler exact {widths} T_k={Tk}"
    got = run_session_euler(lib0, x, v, row, cond, unc, scale, dt, Fx, Tk, what)
    with np.errstate(invalid="ignore"):
        want = sr.euler_update_ref(x, v, row, dt, scale, cond, unc, Tk)
    want.view(np.uint32)[1] = CAN32                # (the canary NaNs' payload need not survive numpy's copy)
    want.view(np.uint32)[:, Tk:] = CAN32
    assert np.array_equal(got, want.view(np.uint32)), what
    assert not np.array_equal(got[0, :Tk], x.view(np.uint32)[0, :Tk])


@pytest.mark.parametrize("Tk", [1, 40, 97])
@pytest.mark.parametrize("widths", sorted(WIDTHS))
def test_euler_update_equals_the_scheduled_kernel(lib0, widths, Tk):
    """General operands: the strided update leaves, bit for bit, what the scheduled solve's kernel leaves on
    the same rows packed at stride T_k (zv_sched_check; pinned against float64 by tests/test_gpu_sched_ref.py)."""
    from zipvoice_amd.engine import ZvSchedCheckArgs
    Fx, _ = WIDTHS[widths]
    x, v, row, cond, unc, scale, dt = euler_case(rng_for("euler general", widths, Tk), Fx, Tk, "general")
    what = f"session euler general {widths} T_k={Tk}"
    got = run_session_euler(lib0, x, v, row, cond, unc, scale, dt, Fx, Tk, what)
    A, per_row = len(row), Tk * Fx
    packed = np.ascontiguousarray(x[row, :Tk].reshape(A, per_row))
    out = np.full(A * per_row + 2 * GUARD, CAN32, np.uint32)
    a = ZvSchedCheckArgs()
    a.kind, a.guard, a.B, a.N, a.A, a.per_row = 2, GUARD, A, v.shape[0], A, per_row
    keep = dict(x=packed, v=v, row=i32(range(A)), dt=dt, scale=scale, cond=i32(cond), uncond=i32(unc), out=out)
    for k, val in keep.items():
        setattr(a, k, val.ctypes.data)
    assert lib0.zv_sched_check(ctypes.byref(a)) == 0, lib0.zv_last_error().decode()
    want = out[GUARD:GUARD + A * per_row].reshape(A, Tk, Fx)
    assert np.array_equal(got[row, :Tk], want), what
    assert not np.array_equal(want, packed.view(np.uint32).reshape(A, Tk, Fx))


def test_rejects_what_would_read_or_write_out_of_bounds(lib0):
    """Indices are checked on the host before any launch."""
    from zipvoice_amd.engine import ZvSessionCheckArgs
    Fx = 4
    z = lambda *s: np.zeros(s, np.float32)
    keep = dict(x=z(S, MAXT, Fx), out=z(S * MAXT * Fx + 2 * GUARD), v=z(2, 5, Fx), m=np.zeros((S, MAXT), np.uint8),
                mout=np.zeros(2 * MAXT + 2 * GUARD, np.uint8), f2=z(2), req=z(2, 9, Fx))
    ret = dict(kind=RETIRE, n=2, T_io=9, Fx=Fx, x=keep["x"], out=keep["out"])
    eul = dict(kind=EULER, T_k=5, N=2, A=2, Fx=Fx, x=keep["x"], v=keep["v"], out=keep["out"], dt=keep["f2"], scale=keep["f2"])
    bad = [
        dict(ret, slot=i32([0, S]), len=i32([1, 1])),                 # a slot outside the session
        dict(ret, slot=i32([-1, 0]), len=i32([1, 1])),
        dict(ret, slot=i32([2, 2]), len=i32([1, 1])),                 # named twice
        dict(ret, slot=i32([0, 1]), len=i32([1, 10])),                # longer than T_out
        dict(ret, slot=i32([0, 1]), len=i32([0, 1])),
        dict(kind=GATHER, T_k=MAXT + 1, N=2, mask=keep["m"], mout=keep["mout"], src=i32([0, 1])),
        dict(kind=GATHER, T_k=5, N=2, mask=keep["m"], mout=keep["mout"], src=i32([0, S])),
        dict(eul, row=i32([0, 1]), cond=i32([0, 2]), uncond=i32([-1, -1])),
        dict(eul, row=i32([1, 1]), cond=i32([0, 1]), uncond=i32([-1, -1])),
        dict(eul, row=i32([0, S]), cond=i32([0, 1]), uncond=i32([-1, -1])),
        dict(eul, T_k=MAXT + 1, row=i32([0, 1]), cond=i32([0, 1]), uncond=i32([-1, -1])),
    ]
    for f in bad:
        a = ZvSessionCheckArgs()
        a.guard, a.slots, a.max_frames = GUARD, S, MAXT
        for k, v in f.items():
            setattr(a, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        assert lib0.zv_session_check(ctypes.byref(a)) == 1, {k: v for k, v in f.items() if not isinstance(v, np.ndarray) or v.size < 4}
        assert b"zv_session_check" in lib0.zv_last_error()
