"""The scheduled solve's three kernels (csrc/zv_elem.inc: operand build through the row map, mask gather,
the scattered Euler update), each launched through the launch function zv_engine::euler_sample_sched
calls (zv_sched_check), against references composed from tests/kernel_ref.py's solve-boundary functions:
a decoder batch is gathered row by row from kr.build_input_ref / kr.euler_ref of the single rows.

Exact classes (bit for bit): the operand build against kr.split16 of the gathered float64 reference, in
both operand libraries, quad and scalar form, with and without the lo half; the mask gather; the update on
dyadic operands (kr.euler_ref(exact=True) asserts every fp32 step exact).  General class: the update
within kr.euler_ref's tolerance (one fp32 rounding per operation, weighted by that operation's float64
result), each row with its own scale and dt.  Input rows outside the active list come back bit-identical;
canary guard rows and pad columns come back untouched.  The launches cap a row's blocks at 1024 (262144
threads): one case of each kernel runs a row one element past that.  Each general test prints its max
|err| / tolerance (MI355X: 0.70 ... 0.91 over the small cases, 0.99 over the 262221-value rows of the cap
case; the unscheduled kernel reaches 0.93 of the same bound in tests/test_gpu_solve_ref.py)."""
import ctypes

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

BUILD, GATHER, EULER = range(3)
CAN32, CAN16, CAN8 = np.uint32(0x7FC5A5A5), np.uint16(0x7FA5), np.uint8(0xA5)
GUARD = 2
ROW_CAP = 1024 * 256                   # threads over one row: one more element takes a second trip


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=request.param)


@pytest.fixture(scope="module")
def lib0():
    from zipvoice_amd import engine
    return engine.load_library()


def f32(x):
    k = np.ascontiguousarray(x, np.float32)
    assert np.array_equal(k.astype(np.float64), x), "inputs must be fp32 values"
    return k


def call(Lb, kind, **fields):
    from zipvoice_amd.engine import ZvSchedCheckArgs
    a = ZvSchedCheckArgs()
    a.kind, a.guard = kind, GUARD
    for k, v in fields.items():
        if v is None:
            continue
        if isinstance(v, np.ndarray):
            assert v.flags["C_CONTIGUOUS"]
            setattr(a, k, v.ctypes.data)
        else:
            setattr(a, k, v)
    rc = Lb.zv_sched_check(ctypes.byref(a))
    assert rc == 0, Lb.zv_last_error().decode()
    assert a.launch[0] == kind and a.launch[3] == 256
    return list(a.launch)


def canary(rows, ld, can):
    return np.full((rows + 2 * GUARD, ld), can, can.dtype)


def interior(buf, rows, width, what):
    can = {2: CAN16, 1: CAN8}[buf.dtype.itemsize]
    mask = np.ones(buf.shape, bool)
    mask[GUARD:GUARD + rows, :width] = False
    touched = int((buf[mask] != can).sum())
    assert touched == 0, f"{what}: {touched} elements outside the output were written"
    return buf[GUARD:GUARD + rows, :width]


def rng_for(*key):
    return np.random.default_rng([ord(c) for c in "sched " + " ".join(map(str, key))])


def sources(rng, B, T, Fx, Ft):
    """fp32 values with a full mantissa (a nonzero lo half), the three sources far apart."""
    x = rng.standard_normal((B * T, Fx)).astype(np.float32).astype(np.float64)
    tc = (8.0 + rng.standard_normal((B * T, Ft))).astype(np.float32).astype(np.float64)
    sc = (-8.0 + rng.standard_normal((B * T, Fx))).astype(np.float32).astype(np.float64)
    return x, tc, sc


def gathered_build_ref(x, tc, sc, B, T, src, zt, zs):
    """Decoder row j = kr.build_input_ref of input row src[j] alone: the unconditional copy (rows [0, T) of two
    copies, speech zeroed iff zs[j]) where zt[j], else the conditional row (zs is 0 there)."""
    out = []
    for j, b in enumerate(src):
        r = slice(b * T, (b + 1) * T)
        if zt[j]:
            out.append(kr.build_input_ref(x[r], tc[r], sc[r], 1, T, 2, int(zs[j]))[:T])
        else:
            assert not zs[j]
            out.append(kr.build_input_ref(x[r], tc[r], sc[r], 1, T, 1, 0))
    return np.concatenate(out, axis=0)


# B = 5, T = 7: active rows {0, 2, 4}, copies for {2, 4} with different speech flags, then the conditional rows
MAP_5 = (5, [2, 4, 0, 2, 4], [1, 1, 0, 0, 0], [1, 0, 0, 0, 0])
MAP_1 = (1, [0], [0], [0])
MAP_1C = (1, [0, 0], [1, 0], [1, 0])


@pytest.mark.parametrize("B,src,zt,zs", [MAP_5, MAP_1, MAP_1C], ids=["B5", "B1", "B1copy"])
@pytest.mark.parametrize("Fx,Ft,ld", [(100, 100, 320), (3, 5, 13)], ids=["quad", "scalar"])
def test_build_input_map(lib, Fx, Ft, ld, B, src, zt, zs):
    fmt, Lb = lib
    T, N, Fin = 7, len(src), 2 * Fx + Ft
    assert ld > Fin
    x, tc, sc = sources(rng_for("build", Fx, B), B, T, Fx, Ft)
    hi, lw = kr.split16(gathered_build_ref(x, tc, sc, B, T, src, zt, zs), fmt)
    assert np.abs(lw).max() > 0
    for lo in (True, False):
        oh, ol = canary(N * T, ld, CAN16), canary(N * T, ld, CAN16) if lo else None
        rec = call(Lb, BUILD, B=B, T=T, N=N, Fx=Fx, Ft=Ft, Fs=Fx, ld=ld, x=f32(x), tc=f32(tc), sc=f32(sc),
                   src=np.asarray(src, np.int32), zero_text=np.asarray(zt, np.uint8),
                   zero_speech=np.asarray(zs, np.uint8), oh=oh, ol=ol)
        what = f"{fmt} sched build Fx={Fx} B={B} lo={lo}"
        assert rec[1] == int(Fx % 4 == 0 and Ft % 4 == 0 and ld % 4 == 0) and rec[4] == N, (what, rec)
        assert np.array_equal(kr.decode16(interior(oh, N * T, Fin, what), fmt), hi), what + ": hi"
        if lo:
            assert np.array_equal(kr.decode16(interior(ol, N * T, Fin, what), fmt), lw), what + ": lo"


def decode16_f32(u, fmt):
    return u.view(np.float16).astype(np.float32) if fmt == "f16" else (u.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("quad", [0, 1])
def test_build_input_map_past_the_row_cap(lib, quad):
    """One row of more elements (quads) than a row's capped blocks have threads, plus a tail: the stride
    loop's second trip.  Integers the 16-bit formats hold exactly, so the operand is the value itself.
    The second decoder row is the copy of the same input row with its speech kept."""
    fmt, Lb = lib
    Fx, Ft, ld = (4, 4, 16) if quad else (3, 5, 13)
    Fin = 2 * Fx + Ft
    per = Fin // 4 if quad else Fin
    T = ROW_CAP // per + 3
    assert T * per > ROW_CAP and (T * per - ROW_CAP) % 256 != 0
    rng = rng_for("build cap", quad)
    x = rng.integers(-8, 9, (2 * T, Fx)).astype(np.float32)
    tc = (64 + rng.integers(0, 9, (2 * T, Ft))).astype(np.float32)
    s = (-64 - rng.integers(0, 9, (2 * T, Fx))).astype(np.float32)
    oh = canary(2 * T, ld, CAN16)
    rec = call(Lb, BUILD, B=2, T=T, N=2, Fx=Fx, Ft=Ft, Fs=Fx, ld=ld, x=x, tc=tc, sc=s,
               src=np.array([1, 1], np.int32), zero_text=np.array([1, 0], np.uint8),
               zero_speech=np.array([0, 0], np.uint8), oh=oh)
    assert rec[1] == quad and rec[2] == 1024 and rec[4] == 2, rec
    got = decode16_f32(interior(oh, 2 * T, Fin, "build cap"), fmt)
    cond = np.concatenate([x[T:], tc[T:], s[T:]], axis=1)
    unc = np.concatenate([x[T:], np.zeros_like(tc[T:]), s[T:]], axis=1)
    assert np.array_equal(got, np.concatenate([unc, cond]))


@pytest.mark.parametrize("B,src,T", [(5, [2, 4, 0, 2, 4], 7), (1, [0], 7), (1, [0, 0], 301),
                                      (3, [2, 0, 2, 1], ROW_CAP + 77)], ids=["B5", "B1", "B1copy", "cap"])
def test_mask_gather(lib0, B, src, T):
    N = len(src)
    m = rng_for("mask", B, T).integers(0, 2, (B, T)).astype(np.uint8)
    mout = np.full(N * T + 2 * GUARD, CAN8, np.uint8)
    rec = call(lib0, GATHER, B=B, T=T, N=N, mask=m, src=np.asarray(src, np.int32), mout=mout)
    assert rec[4] == N and rec[2] == min(-(-T // 256), 1024), rec
    assert (mout[:GUARD] == CAN8).all() and (mout[GUARD + N * T:] == CAN8).all()
    assert np.array_equal(mout[GUARD:GUARD + N * T].reshape(N, T), m[src])


def euler_operands(rng, B, N, per_row, klass):
    if klass == "exact":                 # small integers, dyadic scales and steps: every fp32 step is exact
        x = rng.integers(-8, 9, B * per_row).astype(np.float64)
        v = rng.integers(-8, 9, N * per_row).astype(np.float64)
        scale, dt = [1.5, -0.5, 6.0, 0.25, 3.0], [0.125, 0.25, -0.5, 0.0625, 0.5]
    else:
        x = rng.standard_normal(B * per_row).astype(np.float32).astype(np.float64)
        v = (3.0 * rng.standard_normal(N * per_row)).astype(np.float32).astype(np.float64)
        scale, dt = [0.7, 5.0, -0.3, 1.4, 2.5], [0.0625, 0.337, 0.1, 0.21, 0.05]
    f = lambda a: [float(np.float32(t)) for t in a]
    return x, v, f(scale), f(dt)


def run_euler(lib0, klass, B, N, per_row, row, cond, unc, what):
    A = len(row)
    x, v, scale, dt = euler_operands(rng_for("euler", klass, B, per_row), B, N, per_row, klass)
    scale, dt = scale[:A], dt[:A]
    out = np.full(B * per_row + 2 * GUARD, CAN32, np.uint32)
    rec = call(lib0, EULER, B=B, N=N, A=A, per_row=per_row, x=f32(x), v=f32(v), row=np.asarray(row, np.int32),
               dt=np.asarray(dt, np.float32), scale=np.asarray(scale, np.float32),
               cond=np.asarray(cond, np.int32), uncond=np.asarray(unc, np.int32), out=out)
    assert rec[4] == A and rec[2] == min(-(-per_row // 256), 1024), rec
    assert (out[:GUARD] == CAN32).all() and (out[GUARD + B * per_row:] == CAN32).all(), what + ": guard elements written"
    got = out[GUARD:GUARD + B * per_row].view(np.float32).reshape(B, per_row)
    xs, vs = x.reshape(B, per_row), v.reshape(N, per_row)
    ratio = 0.0
    for i, b in enumerate(row):
        if unc[i] >= 0:                  # euler_ref's v = [uncond | cond] of this row alone
            ref, tol = kr.euler_ref(xs[b], np.concatenate([vs[unc[i]], vs[cond[i]]]), 1, scale[i], dt[i],
                                    exact=klass == "exact")
        else:
            ref, tol = kr.euler_ref(xs[b], vs[cond[i]], 0, 0.0, dt[i], exact=klass == "exact")
        g = got[b].astype(np.float64)
        if klass == "exact":
            assert np.array_equal(g, ref), f"{what} row {b}: {int((g != ref).sum())} values differ"
        else:
            err = np.abs(g - ref)
            assert np.isfinite(g).all() and (err <= tol).all(), f"{what} row {b}: max |err| / tol = {(err / tol).max():.3f}"
            ratio = max(ratio, float((err / np.maximum(tol, 1e-300)).max()))
    for b in set(range(B)) - set(row):   # not in the list: not written
        assert np.array_equal(got[b].view(np.uint32), f32(xs[b]).view(np.uint32)), f"{what}: inactive row {b} changed"
    return ratio


# B = 5: rows {0, 2, 4} active, {2, 4} guided (decoder batch: copies of 2, 4, then 0, 2, 4); rows 1, 3 finished
UPD_5 = (5, 5, [0, 2, 4], [2, 3, 4], [-1, 0, 1])
UPD_ALL = (3, 6, [0, 1, 2], [3, 4, 5], [0, 1, 2])          # today's [uncond B | cond B]
UPD_1 = (1, 1, [0], [0], [-1])
UPD_1C = (1, 2, [0], [1], [0])


@pytest.mark.parametrize("klass", ["exact", "general"])
@pytest.mark.parametrize("B,N,row,cond,unc", [UPD_5, UPD_ALL, UPD_1, UPD_1C], ids=["B5", "all", "B1", "B1copy"])
def test_euler_update_sched(lib0, B, N, row, cond, unc, klass):
    per_row = 7 * 100 + 1                  # no multiple of the block
    ratio = run_euler(lib0, klass, B, N, per_row, row, cond, unc, f"sched euler B={B} {klass}")
    if klass == "general":
        print(f"PIN SCHED_EULER B={B} N={N}: max |err| / tol = {ratio:.3f}")


@pytest.mark.parametrize("klass", ["exact", "general"])
def test_euler_update_sched_past_the_row_cap(lib0, klass):
    """A row of 1024 x 256 + 77 values: the stride loop's second trip; the middle row stays as it was."""
    ratio = run_euler(lib0, klass, 3, 3, ROW_CAP + 77, [0, 2], [1, 2], [-1, 0], f"sched euler cap {klass}")
    if klass == "general":
        print(f"PIN SCHED_EULER cap: max |err| / tol = {ratio:.3f}")


def test_rejects_what_would_read_or_write_out_of_bounds(lib0):
    """Indices are checked on the host before any launch: a source row outside the input, a velocity row
    outside the decoder batch, an input row listed twice."""
    from zipvoice_amd.engine import ZvSchedCheckArgs
    keep = dict(m=np.zeros((2, 7), np.uint8), mout=np.zeros(2 * 7 + 2 * GUARD, np.uint8), x=np.zeros(2 * 8, np.float32),
                v=np.zeros(2 * 8, np.float32), out=np.zeros(2 * 8 + 2 * GUARD, np.float32),
                dt=np.zeros(2, np.float32))
    i32 = lambda *a: np.asarray(a, np.int32)
    eul = dict(kind=EULER, B=2, N=2, A=2, per_row=8, x=keep["x"], v=keep["v"], out=keep["out"], dt=keep["dt"], scale=keep["dt"])
    bad = [
        dict(kind=GATHER, B=2, T=7, N=2, mask=keep["m"], mout=keep["mout"], src=i32(0, 2)),
        dict(kind=GATHER, B=2, T=7, N=2, mask=keep["m"], mout=keep["mout"], src=i32(-1, 0)),
        dict(eul, row=i32(0, 1), cond=i32(0, 2), uncond=i32(-1, -1)),
        dict(eul, row=i32(0, 1), cond=i32(0, 1), uncond=i32(-2, -1)),
        dict(eul, row=i32(1, 1), cond=i32(0, 1), uncond=i32(-1, -1)),
        dict(eul, row=i32(0, 2), cond=i32(0, 1), uncond=i32(-1, -1)),
    ]
    for f in bad:
        a = ZvSchedCheckArgs()
        a.guard = GUARD
        for k, v in f.items():
            setattr(a, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        assert lib0.zv_sched_check(ctypes.byref(a)) == 1, f
        assert b"zv_sched_check" in lib0.zv_last_error()
