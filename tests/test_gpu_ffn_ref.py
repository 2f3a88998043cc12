"""The fused FeedForward kernel (csrc/zv_ffn.inc) alone against float64, every form launch_ffn can
dispatch, in both operand libraries (zv_ffn_check; reference and tolerance derivation in
tests/kernel_ref.py ffn_ref / ffn_epilogue / biasnorm_bypass).

The hidden pre-activations come from the exact class (x in {-3..3}, W1 in {-4..4}/64, b1 in
{-16..16}/8), so u is known exactly and the reference hidden value is round16(SwooshL(u)); a
hidden value whose transcendental tolerance (4x the fp32 formula's error) straddles a 16-bit
rounding boundary may be one ulp off.  Per output the tolerance is
    sum over ambiguous k of |w2_nk| ulp16(h_k) + (H + 8) 2^-23 sum_k |w2_nk||h_k|
    + one fp32 ulp per epilogue operation,
propagated through the BiasNorm epilogue as kernel_ref.biasnorm_bypass derives; a 16-bit output
adds half an ulp of its format.  tests/test_kernel_ref.py asserts that this stays below 2 % of
the FeedForward contribution's RMS and that a dropped 32-wide hidden chunk is far outside it.
Outputs are canary-guarded as in test_gpu_linear_ref.py."""
import ctypes
import functools

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

D = 512
CAN32, CAN16 = np.uint32(0x7FC5A5A5), np.uint16(0x7FA5)
GUARD = 2
LDC, LDCH = D + 4, D + 8


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=request.param)


def cdiv(a, b):
    return -(-a // b)


def _interior(buf, M, can, what):
    mask = np.ones(buf.shape, bool)
    mask[GUARD:GUARD + M, :D] = False
    touched = int((buf[mask] != can).sum())
    assert touched == 0, f"{what}: {touched} elements outside the output were written"
    return buf[GUARD:GUARD + M, :D]


def run_ffn(lib, fmt, form, x, W1, b1, W2, b2, resid, rowvec=None, rpg=0, orig=None, byp=None, nb=None,
            log_scale=0.0, part_slots=0, copy=True, extra=()):
    """One zv_ffn_check call; extra: which of Cl / C2h / C2l to ask for (NORM)."""
    from zipvoice_amd.engine import ZvFfnCheckArgs
    M, H = x.shape[0], W1.shape[0]
    f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
    names = ("x", "W1", "b1", "W2", "b2", "resid", "rowvec", "orig", "byp", "nb")
    keep = [f32(v) for v in (x, W1, b1, W2, b2, resid, rowvec, orig, byp, nb)]
    a = ZvFfnCheckArgs()
    a.M, a.H, a.form, a.rows_per_group, a.part_slots, a.guard = M, H, form, rpg, part_slots, GUARD
    a.log_scale = log_scale
    for n, v in zip(names, keep):
        setattr(a, n, None if v is None else v.ctypes.data)
    a.ldc, a.ldch = LDC, LDCH
    bufs = {"C": np.full((M + 2 * GUARD, LDC), CAN32, np.uint32)}
    if copy:
        bufs["Ch"] = np.full((M + 2 * GUARD, LDCH), CAN16, np.uint16)
    for n in extra:
        bufs[n] = np.full((M + 2 * GUARD, LDCH), CAN16, np.uint16)
    for n, b in bufs.items():
        setattr(a, n, b.ctypes.data)
    rc = lib.zv_ffn_check(ctypes.byref(a))
    assert rc == 0, lib.zv_last_error().decode()
    out, raw = {}, {}
    for n, b in bufs.items():
        if b.dtype == np.uint32:
            raw[n] = _interior(b, M, CAN32, n).copy()
            out[n] = raw[n].view(np.float32).astype(np.float64)
        else:
            raw[n] = _interior(b, M, CAN16, n).copy()
            out[n] = kr.decode16(raw[n], fmt)
    return out, raw, tuple(a.launch), a.num_cus


@functools.lru_cache(maxsize=None)
def reference(M, H, fmt):
    """Inputs and the float64 module output with its tolerance, computed once per shape."""
    x, W1, b1, W2, b2, resid = kr.ffn_inputs(M, H, fmt, seed=1000 * H + M)
    ff, tol, mag = kr.ffn_ref(x, W1, b1, W2, b2, fmt)
    rng = np.random.default_rng(M + H)
    f = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
    ex = dict(orig=f(M, D), byp=rng.random(D).astype(np.float32).astype(np.float64), nb=0.1 * f(D),
              rv203=f(cdiv(M, 203), D), rv7=f(cdiv(M, 7), D))
    for v in (x, W1, b1, W2, b2, resid, ff, tol, mag, *ex.values()):
        v.setflags(write=False)
    return (x, W1, b1, W2, b2, resid), (ff, tol, mag), ex


def within(got, ref, tol, what):
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), what
    r = float((err / tol).max())
    assert (err <= tol).all(), f"{what}: max |err| / tol = {r:.3f}, {int((err > tol).sum())} outside"
    return r


def half16(ref, tol, fmt):
    return tol + 0.5 * kr.ulp16(np.abs(ref) + tol, fmt)


LOG_SCALE = 0.125
# form name -> (zv_ffn_check form, row-vector rows per group, launch flags RV | ORIG << 1 | COPY << 2 | TP << 3, NORM)
FORMS = {"plain_copy": (0, 0, 4 | 8, 0), "plain_nocopy": (0, 0, 0 | 8, 0), "rv203": (1, 203, 1 | 4 | 8, 0),
         "rv7": (1, 7, 1 | 4, 0), "bypass": (2, 0, 2 | 4 | 8, 0),
         "norm": (3, 0, 4 | 8, 1), "norm_all": (3, 0, 4 | 8, 1), "norm_rv203": (3, 203, 4 | 8, 1),
         "norm_rv7": (3, 7, 4, 1), "norm_rv7_all": (3, 7, 4, 1)}
# the optional outputs each BiasNorm form asks for (Ch always)
NORM_EXTRA = {"norm": (), "norm_all": ("Cl", "C2h", "C2l"), "norm_rv203": ("Cl", "C2h", "C2l"),
              "norm_rv7": ("C2h",), "norm_rv7_all": ("Cl", "C2h", "C2l")}


def check_form(lib, fmt, name, M, H, part_slots=0):
    """Run one form and compare every output with float64.  Returns (max ratio, raw outputs)."""
    form, rpg, flags, norm = FORMS[name]
    (x, W1, b1, W2, b2, resid), (ff, tol_ff, mag), ex = reference(M, H, fmt)
    rv = ex["rv203"] if rpg == 203 else ex["rv7"] if rpg == 7 else None
    kw = dict(rowvec=rv, rpg=rpg, part_slots=part_slots)
    extra = ()
    if form >= 2:
        kw.update(orig=ex["orig"], byp=ex["byp"])
    if form == 3:
        kw.update(nb=ex["nb"], log_scale=LOG_SCALE)
        extra = NORM_EXTRA[name]
    out, raw, rec, cus = run_ffn(lib, fmt, form, x, W1, b1, W2, b2, resid, copy=name != "plain_nocopy",
                                 extra=extra, **kw)
    assert rec[:6] == (128, D, 1, flags, norm, 0), (name, rec)
    if part_slots == 0:
        assert rec[6:] == (cdiv(M, 128), H // 32), (name, rec)
    what = f"{fmt} {name} M={M} H={H}"
    ratios = []
    if form < 3:
        ref, tol, _ = kr.ffn_epilogue(ff, tol_ff, mag, resid, rowvec=rv, rows_per_group=max(rpg, 1),
                                      orig=kw.get("orig"), byp=kw.get("byp"))
        ratios.append(within(out["C"], ref, tol, what + " C"))
        if "Ch" in out:
            ratios.append(within(out["Ch"], ref, half16(ref, tol, fmt), what + " Ch"))
    else:
        xm, tol_x, _ = kr.ffn_epilogue(ff, tol_ff, mag, resid)
        ref, tol = kr.biasnorm_bypass(xm, tol_x, ex["nb"], LOG_SCALE, ex["orig"], ex["byp"])
        ratios.append(within(out["C"], ref, tol, what + " C"))
        ratios.append(within(out["Ch"], ref, half16(ref, tol, fmt), what + " Ch"))
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
@pytest.mark.parametrize("H", [64, 192, 1536])
def test_ffn_every_form(lib, H, M):
    fmt, L = lib
    line = []
    for name in FORMS:
        r, _, _ = check_form(L, fmt, name, M, H)
        line.append(f"{name} {r:.3f}")
    print(f"{fmt} ffn M={M} H={H}: max |err| / tol: " + ", ".join(line))


@pytest.mark.parametrize("name", ["plain_copy", "rv203", "bypass", "norm_all", "norm_rv7"])
def test_ffn_persistent_schedule(lib, name):
    """Five row blocks on three and four lines: row blocks are cut into P and C items
    (launch record: blocks = lines, more chunk steps per block than the row block's chunks).
    Bitwise equal to one row block per block, and within tolerance of float64."""
    fmt, L = lib
    M, H = 623, 192
    r0, raw0, rec0 = check_form(L, fmt, name, M, H, part_slots=0)
    for slots in (3, 4):
        r, raw, rec = check_form(L, fmt, name, M, H, part_slots=slots)
        assert rec[6] == slots and rec[7] > H // 32, rec
        for n in raw0:
            assert np.array_equal(raw[n], raw0[n]), f"{fmt} {name} {n}: {slots} lines differ from one block per row block"
        print(f"{fmt} ffn {name} persistent {slots} lines (w = {rec[7]}): bitwise equal, max |err| / tol = {r:.3f}")


def test_ffn_swoosh_l_sweep(lib):
    """SwooshL through the fused kernel's hand-written micro-ops: H = 512, W2 the identity, two
    unit columns in W1 and b1 = n / 8, so output n of row m is exactly round16(SwooshL(u_m + n / 8));
    u_m + n / 8 covers [-120, 120] in steps of 1 / 64 (and beyond, up to 184)."""
    fmt, L = lib
    H = 512
    # rows: u_m = a0 + a1 with a0 an integer and a1 a multiple of 1/64 in [0, 1/8): with b1 = n/8
    # (n = 0..511) every multiple of 1/64 in [-120, 120] appears
    a0 = np.repeat(np.arange(-120, 121, 3), 8)          # integers (exact in both formats)
    a1 = np.tile(np.arange(8) / 64.0, a0.size // 8)
    M = a0.size
    x = np.zeros((M, D))
    x[:, 0], x[:, 1] = a0, a1
    W1 = np.zeros((H, D))
    W1[:, :2] = 1.0
    b1 = np.arange(H) / 8.0
    W2, b2, resid = np.eye(D), np.zeros(D), np.zeros((M, D))
    out, _, rec, _ = run_ffn(L, fmt, 0, x, W1, b1, W2, b2, resid, copy=True)
    pre = kr.assert_fp32_exact(kr.assert_exact_dot(kr.round16(x, fmt), W1) + b1)
    covered = np.unique(pre[(pre >= -120) & (pre <= 120)])
    assert covered.size == 240 * 64 + 1, "the sweep covers [-120, 120] in steps of 1/64"
    ref = kr.swoosh_l(pre)
    # the fp32 output is the 16-bit hidden value itself (identity W2, zero bias and residual)
    assert np.isfinite(out["C"]).all()
    bad, amb, r, multi = kr.check16(out["C"], ref, kr.tol_swoosh_l(pre), fmt)
    print(f"{fmt} fused SwooshL sweep: launch {rec}, {int(amb.sum())} ambiguous of {amb.size} "
          f"({multi} of them multi-ulp, next to SwooshL's zero), max |err| / allowed = {r:.3f}")
    assert not bad.any(), f"{int(bad.sum())} hidden values outside 4x the fp32 formula's error, " \
                          f"first at u = {pre[bad][:5]}"
