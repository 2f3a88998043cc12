"""The kernels at the stack boundaries (csrc/zv_elem.inc), each launched as zv_engine launches it
(zv_stackedge_check), against float64 references of the same operations (tests/kernel_ref.py
downsample_ref / upsample_combine_ref / mask_downsample_ref after zipformer.py:887-935 and :857-858,
biasnorm_bypass), in both operand libraries.

zv_downsample_kernel, zv_upsample_combine_kernel (row-blocked, C = 512) / _any_kernel (grid-stride,
C = 384), zv_mask_downsample_kernel: dyadic weights and scales and small-integer inputs make every
step exact in fp32 (asserted by the reference), so the comparison is array_equal; the utterances'
edge frames hold +-1000, so a frame taken from the neighbouring utterance (a clamp to L instead of
L - 1, l / ds against the wrong dL) is off by hundreds.  The general class (Gaussian inputs) allows
one fp32 rounding per operation.
zv_stack_entry_kernel: one fp32 addition and the hi / lo splits: equal to numpy's fp32 bit for bit
in both classes.
zv_biasnorm_bypass_v_kernel<2> (C = 512) and zv_biasnorm_bypass_kernel (C = 384, and C = 256 with
the fp8 copy): kernel_ref.biasnorm_bypass with tol_x = 0; the 16-bit copies within half an ulp more,
the second output out + rowvec, its fp8 copy equal to oracle/mx8_np.py's packing of the returned
16-bit values.  zv_biasnorm_bypass_pair_kernel has no launch site in zv_engine.hip and is not
tested.

Every output has canary-filled guard rows (the 16-bit ones also a row stride larger than the width)
which must come back intact."""
import ctypes
import zlib

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

DOWN, UP, MASK, ENTRY, NORM = range(5)
CAN32, CAN16, CAN8 = np.uint32(0x7FC5A5A5), np.uint16(0x7FA5), np.uint8(0xA5)
GUARD = 2


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=request.param)


def _interior(buf, rows, width, can, what):
    mask = np.ones(buf.shape, bool)
    mask[GUARD:GUARD + rows, :width] = False
    touched = int((buf[mask] != can).sum())
    assert touched == 0, f"{what}: {touched} elements outside the output were written"
    return buf[GUARD:GUARD + rows, :width]


def f32(x):
    k = np.ascontiguousarray(x, np.float32)
    assert np.array_equal(k.astype(np.float64), x), "inputs must be fp32 values"
    return k


def run(lib, fmt, kind, B, L, C, ds=1, x=None, w=None, nb=None, orig=None, rowvec=None, mask=None, rpg=1,
        log_scale=0.0, rows_out=0, want=(), q8=False):
    """One zv_stackedge_check call.  want: which of out / l / h2 / l2 to ask for besides the kind's
    own.  Returns (dict of outputs, launch record)."""
    from zipvoice_amd.engine import ZvStackedgeCheckArgs
    a = ZvStackedgeCheckArgs()
    a.kind, a.B, a.L, a.C, a.ds, a.guard, a.rows_per_group, a.log_scale = kind, B, L, C, ds, GUARD, rpg, log_scale
    keep = {}
    for name, arr in (("x", x), ("w", w), ("nb", nb), ("orig", orig), ("rowvec", rowvec)):
        if arr is not None:
            keep[name] = f32(arr)
            setattr(a, name, keep[name].ctypes.data)
    bufs = {}
    if mask is not None:
        keep["mask"] = np.ascontiguousarray(mask, np.uint8)
        a.mask = keep["mask"].ctypes.data
        bufs["mout"] = np.full((rows_out + 2 * GUARD, 1), CAN8, np.uint8)
        a.mout = bufs["mout"].ctypes.data
    if "out" in want:
        bufs["out"] = np.full((rows_out + 2 * GUARD, C), CAN32, np.uint32)
        a.out = bufs["out"].ctypes.data
    a.ldact = C + 8
    for name in ("h", "l", "h2", "l2"):
        if name in want:
            bufs[name] = np.full((rows_out + 2 * GUARD, a.ldact), CAN16, np.uint16)
            setattr(a, name, bufs[name].ctypes.data)
    if q8:
        a.ldq = C + 128
        bufs["q2"] = np.full((rows_out + 2 * GUARD, a.ldq), CAN8, np.uint8)
        bufs["qs2"] = np.full((rows_out + 2 * GUARD, a.ldq // 32), CAN8, np.uint8)
        a.q2, a.qs2 = bufs["q2"].ctypes.data, bufs["qs2"].ctypes.data
    rc = lib.zv_stackedge_check(ctypes.byref(a))
    assert rc == 0, lib.zv_last_error().decode()
    out = {}
    for name, buf in bufs.items():
        if name == "out":
            out[name] = _interior(buf, rows_out, C, CAN32, name).view(np.float32).astype(np.float64)
        elif name == "mout":
            out[name] = _interior(buf, rows_out, 1, CAN8, name)[:, 0]
        elif name == "q2":
            out[name] = _interior(buf, rows_out, C, CAN8, name)
        elif name == "qs2":
            out[name] = _interior(buf, rows_out, C // 32, CAN8, name)
        else:
            out[name] = kr.decode16(_interior(buf, rows_out, C, CAN16, name), fmt)
    return out, list(a.launch)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def edges(x, B, L, rng):
    return kr.put_edges(x, B, L, rng)


RESAMPLE = [(ds, L, C) for ds in (2, 4) for L in (1, 2, 5, 9, 64, 65) for C in (512, 384)]


@pytest.mark.parametrize("ds,L,C", RESAMPLE)
def test_downsample_upsample_mask(lib, ds, L, C):
    fmt, Lb = lib
    B, dL = 2, -(-L // ds)
    figs = []
    for klass in ("exact", "general"):
        rng = rng_for("resample", ds, L, C, klass)
        if klass == "exact":
            x = edges(rng.integers(-64, 65, (B * L, C)).astype(np.float64), B, L, rng)
            w = kr.ds_weights(ds)
            d = edges(rng.integers(-64, 65, (B * dL, C)).astype(np.float64), B, dL, rng)
            sc = rng.choice([0.0, 0.25, 0.5, 1.0], C)
        else:
            g = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
            x, d = edges(g(B * L, C), B, L, rng), edges(g(B * dL, C), B, dL, rng)
            w = np.exp(g(ds))
            w = (w / w.sum()).astype(np.float32).astype(np.float64)
            sc = rng.random(C).astype(np.float32).astype(np.float64)
        ex = klass == "exact"
        # downsample
        out, rec = run(Lb, fmt, DOWN, B, L, C, ds, x=x, w=w, rows_out=B * dL, want=("out",))
        ref = kr.downsample_ref(x, w, B, L, ds, exact=ex)
        mag = kr.downsample_ref(np.abs(x), np.abs(w), B, L, ds)
        if ex:
            assert np.array_equal(out["out"], ref), f"downsample: {int((out['out'] != ref).sum())} values differ"
        else:                                             # ds products and ds additions, one rounding each
            assert (np.abs(out["out"] - ref) <= 2 * ds * kr.U32 * mag).all(), "downsample"
        figs.append(float(np.abs(out["out"] - ref).max()))
        # upsample + combine, in place over orig
        out, rec = run(Lb, fmt, UP, B, L, C, ds, x=d, w=sc, orig=x, rows_out=B * L, want=("out",))
        assert rec[1] == (0 if 256 % (C // 4) == 0 else 1), rec
        ref = kr.upsample_combine_ref(x, d, sc, B, L, ds, exact=ex)
        if ex:
            assert np.array_equal(out["out"], ref), f"upsample: {int((out['out'] != ref).sum())} values differ"
        else:                                             # u - o, * sc, o + ...: three roundings
            up = np.repeat(d.reshape(B, dL, C), ds, axis=1)[:, :L].reshape(B * L, C)
            assert (np.abs(out["out"] - ref) <= 3 * kr.U32 * (np.abs(up) + 2 * np.abs(x))).all(), "upsample"
        figs.append(float(np.abs(out["out"] - ref).max()))
    m = rng_for("mask", ds, L).integers(0, 2, B * L).astype(np.uint8)
    out, _ = run(Lb, fmt, MASK, B, L, 0, ds, mask=m, rows_out=B * dL)
    assert np.array_equal(out["mout"], kr.mask_downsample_ref(m, B, L, ds))
    print(f"{fmt} ds={ds} L={L} C={C}: max |err| exact / general down, up = {figs}")


@pytest.mark.parametrize("C", [512, 384])
@pytest.mark.parametrize("L", [1, 5, 33])
def test_stack_entry(lib, L, C):
    """cur = src + rowvec[utterance] (or src), and the hi / lo copies of both: bitwise numpy's fp32."""
    fmt, Lb = lib
    B = 2
    for klass in ("exact", "general"):
        for with_rv in (True, False):
            rng = rng_for("entry", L, C, klass, with_rv)
            if klass == "exact":
                src, rv = rng.integers(-256, 257, (B * L, C)) / 64.0, rng.integers(-128, 129, (B, C)) / 64.0
            else:
                src = rng.standard_normal((B * L, C)).astype(np.float32).astype(np.float64)
                rv = rng.standard_normal((B, C)).astype(np.float32).astype(np.float64)
            out, _ = run(Lb, fmt, ENTRY, B, L, C, x=src, rowvec=rv if with_rv else None, rpg=L, rows_out=B * L,
                         want=("out", "h", "l", "h2", "l2"))
            cur = src.astype(np.float32)
            if with_rv:
                cur = cur + np.repeat(rv, L, axis=0).astype(np.float32)
            cur = cur.astype(np.float64)
            assert np.array_equal(out["out"], cur), "cur"
            for v, hn, ln in ((src, "h", "l"), (cur, "h2", "l2")):
                hi, lo = kr.split16(v, fmt)
                assert np.array_equal(out[hn], hi), hn
                assert np.array_equal(out[ln], lo), ln
            out, _ = run(Lb, fmt, ENTRY, B, L, C, x=src, rowvec=rv if with_rv else None, rpg=L, rows_out=B * L,
                         want=("h", "h2"))               # the engine's call: no fp32 cur, no lo halves
            assert np.array_equal(out["h"], kr.round16(src, fmt)) and np.array_equal(out["h2"], kr.round16(cur, fmt))


def near16(got, ref, tol, fmt, what):
    lim = tol + 0.5 * kr.ulp16(np.abs(ref) + tol, fmt)
    err = np.abs(got - ref)
    assert np.isfinite(got).all() and (err <= lim).all(), f"{what}: max |err| / allowed = {(err / lim).max():.3f}"
    return float((err / lim).max())


def near_pair(hi, lo, ref, tol, fmt, what):
    lo_max = 0.5 * kr.ulp16(np.abs(ref) + tol, fmt)
    lim = tol + 0.5 * kr.ulp16(lo_max, fmt)
    err = np.abs(hi + lo - ref)
    assert (err <= lim).all(), f"{what}: max |hi + lo - ref| / allowed = {(err / lim).max():.3f}"


@pytest.mark.parametrize("C", [512, 384, 256])
@pytest.mark.parametrize("M", [1, 7, 8, 9, 33])
def test_biasnorm_bypass(lib, M, C):
    """One utterance of M rows (rowvec per utterance, as the engine's temb): the plain call (out, h),
    the split-mode call (l too), and the call with the next layer's stream h2 (/ l2) = out + rowvec,
    with its fp8 copy where C % 256 == 0."""
    fmt, Lb = lib
    from oracle import mx8_np
    ratios = []
    for klass in ("integer", "general"):
        rng = rng_for("norm", M, C, klass)
        g = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
        if klass == "integer":
            x, orig = rng.integers(-8, 9, (M, C)).astype(np.float64), rng.integers(-8, 9, (M, C)).astype(np.float64)
        else:
            x, orig = 2.0 * g(M, C), g(M, C)
        nb, rv = 0.25 * g(C), g(1, C)
        byp = rng.random(C).astype(np.float32).astype(np.float64)
        log_scale = float(np.float32(0.3))
        ref, tol = kr.biasnorm_bypass(x, np.zeros_like(x), nb, log_scale, orig, byp)     # asserts rms(x - nb) >= 1
        ref2, tol2 = ref + rv, tol + kr.U32 * (np.abs(ref) + np.abs(rv))
        for want, rowvec in ((("out", "h"), None), (("out", "h", "l"), None), (("out", "h", "h2"), rv),
                             (("out", "h", "l", "h2", "l2"), rv), (("out", "h", "h2"), None)):
            q8 = "h2" in want and rowvec is not None and C % 256 == 0 and "l" not in want
            out, rec = run(Lb, fmt, NORM, 1, M, C, x=x, w=byp, nb=nb, orig=orig, rowvec=rowvec, rpg=M,
                           log_scale=log_scale, rows_out=M, want=want, q8=q8)
            assert rec[1] == (1 if C == 512 else 0), rec
            tag = f"{fmt} BiasNorm M={M} C={C} {klass} {want}"
            err = np.abs(out["out"] - ref)
            ratio = float((err / np.maximum(tol, 1e-300)).max())
            assert (err <= tol).all(), f"{tag}: max |err| / tol = {ratio:.3f}"
            ratios.append(ratio)
            near16(out["h"], ref, tol, fmt, tag + " h")
            if "l" in out:
                near_pair(out["h"], out["l"], ref, tol, fmt, tag + " h + l")
            if "h2" in out:
                r2, t2 = (ref2, tol2) if rowvec is not None else (ref, tol)
                near16(out["h2"], r2, t2, fmt, tag + " h2")
                if "l2" in out:
                    near_pair(out["h2"], out["l2"], r2, t2, fmt, tag + " h2 + l2")
            if q8:
                rq, rs = mx8_np.quantize(out["h2"].astype(np.float32), C)
                assert np.array_equal(out["qs2"], rs), f"{tag}: fp8 scales"
                assert np.array_equal(out["q2"], rq), f"{tag}: fp8 codes"
    print(f"{fmt} BiasNorm M={M} C={C}: max |err| / tol = {max(ratios):.3f}")
