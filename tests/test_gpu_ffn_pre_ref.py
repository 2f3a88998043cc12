"""The fused FeedForward kernel's pre-projection form (csrc/zv_ffn.inc, PRE) against float64, in both
operand libraries (zv_ffn_check with K > 0; reference, input classes and tolerance in
tests/ffn_pre_ref.py, which builds on tests/kernel_ref.py):

    cur1 = resid + (A . Wp^T + bp) [+ rowvec];  x = round16(cur1);  v = cur1 + FF(x);
    then the bypass epilogue, or the BiasNorm + bypass epilogue with its optional outputs.

cur1 is exact by construction and equals the x of kernel_ref.ffn_inputs, so the module's reference
and tolerance are test_gpu_ffn_ref.py's, plus one fp32 ulp per added operation.  A wrong K order in
the pre-projection, or a wrong register order of x against the re-packed W1, moves outputs by whole
units (tests/test_ffn_pre_ref.py asserts the first on the CPU).  Outputs are canary-guarded."""
import ctypes
import functools

import numpy as np
import pytest

import ffn_pre_ref as pr
import kernel_ref as kr
import test_gpu_ffn_ref as base

pytestmark = pytest.mark.gpu

D, GUARD, LDC, LDCH = base.D, base.GUARD, base.LDC, base.LDCH
LOG_SCALE = base.LOG_SCALE
PRE_BIT = 16
# form name -> (zv_ffn_check form, row-vector rows per group, launch flags | PRE << 4, NORM, optional outputs)
FORMS = {"bypass": (2, 203, 2 | 4 | 8 | PRE_BIT, 0, ()), "bypass_norv": (2, 0, 2 | 4 | 8 | PRE_BIT, 0, ()),
         "bypass_rv7": (2, 7, 2 | 4 | 8 | PRE_BIT, 0, ()),
         "norm_all": (3, 0, 4 | 8 | PRE_BIT, 1, ("Cl", "C2h", "C2l")),
         "norm_rv203": (3, 203, 4 | 8 | PRE_BIT, 1, ("Cl", "C2h", "C2l")),
         "norm_rv7": (3, 7, 4 | PRE_BIT, 1, ("C2h",)), "norm_rv7_all": (3, 7, 4 | PRE_BIT, 1, ("Cl", "C2h", "C2l"))}


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=request.param)


def run_pre(lib, fmt, form, H, W1, b1, W2, b2, A, Wp, bp, resid, rowvec, rpg, orig, byp, nb=None, part_slots=0,
            extra=()):
    from zipvoice_amd.engine import ZvFfnCheckArgs
    M, K = A.shape
    f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
    names = ("W1", "b1", "W2", "b2", "resid", "rowvec", "orig", "byp", "nb", "A", "Wp", "bp")
    keep = [f32(v) for v in (W1, b1, W2, b2, resid, rowvec, orig, byp, nb, A, Wp, bp)]
    a = ZvFfnCheckArgs()
    a.M, a.H, a.form, a.rows_per_group, a.part_slots, a.guard, a.K = M, H, form, rpg, part_slots, GUARD, K
    a.log_scale = LOG_SCALE if form == 3 else 0.0
    for n, v in zip(names, keep):
        setattr(a, n, None if v is None else v.ctypes.data)
    a.ldc, a.ldch = LDC, LDCH
    bufs = {"C": np.full((M + 2 * GUARD, LDC), base.CAN32, np.uint32),
            "Ch": np.full((M + 2 * GUARD, LDCH), base.CAN16, np.uint16)}
    for n in extra:
        bufs[n] = np.full((M + 2 * GUARD, LDCH), base.CAN16, np.uint16)
    for n, b in bufs.items():
        setattr(a, n, b.ctypes.data)
    rc = lib.zv_ffn_check(ctypes.byref(a))
    assert rc == 0, lib.zv_last_error().decode()
    out, raw = {}, {}
    for n, b in bufs.items():
        can = base.CAN32 if b.dtype == np.uint32 else base.CAN16
        raw[n] = base._interior(b, M, can, n).copy()
        out[n] = raw[n].view(np.float32).astype(np.float64) if b.dtype == np.uint32 else kr.decode16(raw[n], fmt)
    return out, raw, tuple(a.launch)


@functools.lru_cache(maxsize=None)
def module_ref(M, H, fmt):
    """The module's inputs (x = cur1) and float64 output with tolerance, once per shape."""
    x, W1, b1, W2, b2, _ = kr.ffn_inputs(M, H, fmt, seed=1000 * H + M)
    ff, tol, mag = pr.pre_ref(x, W1, b1, W2, b2, fmt)
    rng = np.random.default_rng(M + H + 5)
    f = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
    ex = dict(orig=f(M, D), byp=rng.random(D).astype(np.float32).astype(np.float64), nb=0.1 * f(D))
    for v in (x, ff, tol, mag, *ex.values()):
        v.setflags(write=False)
    return (ff, tol, mag), ex


@functools.lru_cache(maxsize=None)
def pre_case(M, H, K, fmt, rpg):
    mod, pre = pr.pre_inputs(M, H, K, fmt, rpg, seed=1000 * H + M)
    assert np.array_equal(pr.cur1_of(*pre, rpg), mod[0])
    return mod, pre


def check_form(lib, fmt, name, M, H, K, part_slots=0):
    form, rpg, flags, norm, extra = FORMS[name]
    (x, W1, b1, W2, b2), (A, Wp, bp, resid, rv) = pre_case(M, H, K, fmt, rpg)
    (ff, tol_ff, mag), ex = module_ref(M, H, fmt)
    out, raw, rec = run_pre(lib, fmt, form, H, W1, b1, W2, b2, A, Wp, bp, resid, rv, rpg, ex["orig"], ex["byp"],
                            nb=ex["nb"] if norm else None, part_slots=part_slots, extra=extra)
    assert rec[:6] == (128, D, 1, flags, norm, 0), (name, rec)
    if part_slots == 0:
        assert rec[6:] == (base.cdiv(M, 128), H // 32), (name, rec)
    what = f"{fmt} pre {name} M={M} H={H} K={K}"
    within, half16 = base.within, base.half16
    if not norm:
        ref, tol, _ = kr.ffn_epilogue(ff, tol_ff, mag, x, orig=ex["orig"], byp=ex["byp"])
        ratios = [within(out["C"], ref, tol, what + " C"), within(out["Ch"], ref, half16(ref, tol, fmt), what + " Ch")]
    else:
        xm, tol_x, _ = kr.ffn_epilogue(ff, tol_ff, mag, x)
        ref, tol = kr.biasnorm_bypass(xm, tol_x, ex["nb"], LOG_SCALE, ex["orig"], ex["byp"])
        ratios = [within(out["C"], ref, tol, what + " C"), within(out["Ch"], ref, half16(ref, tol, fmt), what + " Ch")]
        p = kr.PREC[fmt]
        if "Cl" in out:
            ratios.append(within(out["Ch"] + out["Cl"], ref, tol + 2.0 ** -p * kr.ulp16(np.abs(ref) + tol, fmt),
                                 what + " Ch + Cl"))
        ref2 = ref if rv is None else ref + rv[np.arange(M) // rpg]
        tol2 = tol + 2 * kr.U32 * (np.abs(ref) + np.abs(ref2))
        if "C2h" in out:
            ratios.append(within(out["C2h"], ref2, half16(ref2, tol2, fmt), what + " C2h"))
        if "C2l" in out:
            ratios.append(within(out["C2h"] + out["C2l"], ref2,
                                 tol2 + 2.0 ** -p * kr.ulp16(np.abs(ref2) + tol2, fmt), what + " C2h + C2l"))
    return max(ratios), raw, rec


@pytest.mark.parametrize("M", [1, 31, 33, 127, 128, 129, 623])
@pytest.mark.parametrize("H", [64, 192])
def test_ffn_pre_every_form(lib, H, M):
    fmt, L = lib
    for K in (48, 560, 656):
        line = [f"{name} {check_form(L, fmt, name, M, H, K)[0]:.3f}" for name in FORMS]
        print(f"{fmt} ffn pre M={M} H={H} K={K}: max |err| / tol: " + ", ".join(line))


def test_ffn_pre_wide_hidden(lib):
    """H = 1920 (FF3's width: the BiasNorm form's LDS is nearly full)."""
    fmt, L = lib
    line = [f"{name} {check_form(L, fmt, name, 129, 1920, 560)[0]:.3f}" for name in ("bypass", "norm_rv203", "norm_rv7")]
    print(f"{fmt} ffn pre M=129 H=1920 K=560: " + ", ".join(line))


@pytest.mark.parametrize("name", ["bypass", "norm_rv203", "norm_rv7"])
def test_ffn_pre_persistent_schedule(lib, name):
    """Five row blocks on three and four lines: a cut row block's P item runs the pre-projection and
    hands x over through Ch.  Bitwise equal to one row block per block; within tolerance of float64."""
    fmt, L = lib
    M, H, K = 623, 192, 560
    r0, raw0, rec0 = check_form(L, fmt, name, M, H, K, part_slots=0)
    for slots in (3, 4):
        r, raw, rec = check_form(L, fmt, name, M, H, K, part_slots=slots)
        assert rec[6] == slots and rec[7] > H // 32, rec
        for n in raw0:
            assert np.array_equal(raw[n], raw0[n]), f"{fmt} {name} {n}: {slots} lines differ from one block per row block"
        print(f"{fmt} ffn pre {name} persistent {slots} lines (w = {rec[7]}): bitwise equal, max |err| / tol = {r:.3f}")
