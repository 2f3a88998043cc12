"""The BigVGAN kernels (csrc/zv_bigvgan.inc), the implicit-conv A loader of zv_gemm_kernel and
conv_pre's im2col, one launch at a time through zv_bigvgan_check -- the launches and weight relayouts
zv_bigvgan::finalize / decode use -- against the float64 references of tests/kernel_ref.py (checked
on the CPU in tests/test_kernel_ref.py), in both operand libraries and both splits.

Classes, bounds and the stale-memory rule are stated in kernel_ref.py's BigVGAN section; the case
lists live in bigvgan_cases below and are shared with the CPU tests.  Every output has canary-filled
guard rows which must come back intact; rows [len, Lp) of every input stream hold junk (a read past
an utterance's end is off by hundreds), the utterances' edge frames hold large values.

Measured on an MI355X (profiles/bigvgan_ref_pin.txt): max |err| / bound of the general classes ACT
0.075, CONV 0.09, CONVT 0.012, STEP 0.002; the sine term 1.29e-6 up to 16 rad and 3.50e-5 up to 64
turns, against allowances of twice that."""
import ctypes
import zlib

import numpy as np
import pytest

import kernel_ref as kr
from bigvgan_cases import (ACT_C, ACT_LMAX, CONVT_UK, CONV_C, POST_LMAX, act_case, act_lens, conv_cases,
                           conv_inputs, conv_predict, convt_inputs, needed_rows, post_inputs, step_inputs)

pytestmark = pytest.mark.gpu

FILTER, ACT, CONV, CONVT, AVG, POST, IM2COL, STEP = range(8)
CAN32, CAN16 = np.uint32(0x7FC5A5A5), np.uint16(0x7FA5)
GUARD = 2
F32 = ("x", "x1", "x2", "w", "bias", "alpha", "ibeta", "w2", "bias2", "alpha2", "ibeta2", "taps", "resid")


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=request.param)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def f32(x):
    k = np.ascontiguousarray(x, np.float32)
    assert np.array_equal(k.astype(np.float64), np.asarray(x, np.float64)), "inputs must be fp32 values"
    return k


def can32(rows, cols):
    return np.full((rows + 2 * GUARD, cols), CAN32, np.uint32)


def interior(buf, rows, can, what):
    """The output's rows, after asserting that the guard rows are intact."""
    g = np.concatenate([buf[:GUARD], buf[GUARD + rows:]])
    assert (g == can).all(), f"{what}: {int((g != can).sum())} guard elements were written"
    return buf[GUARD:GUARD + rows]


def call(L, kind, expect_error=None, **kw):
    """One zv_bigvgan_check call; keyword = field.  fp32 inputs are checked to be fp32 values."""
    from zipvoice_amd.engine import ZvBigvganCheckArgs
    a = ZvBigvganCheckArgs()
    a.kind, a.split, a.guard, a.scale, a.div = kind, 1, GUARD, 1, 1.0
    keep = []
    for k, v in kw.items():
        if v is None:
            continue
        if k in F32:
            v = f32(v)
        elif k == "lens":
            v = np.ascontiguousarray(v, np.int32)
        if isinstance(v, np.ndarray):
            assert v.flags.c_contiguous
            keep.append(v)
            setattr(a, k, v.ctypes.data)
        else:
            setattr(a, k, v)
    rc = L.zv_bigvgan_check(ctypes.byref(a))
    if expect_error is not None:
        assert rc != 0 and expect_error in L.zv_last_error().decode(), (rc, L.zv_last_error().decode())
        return None
    assert rc == 0, L.zv_last_error().decode()
    return a


def as64(buf):
    return buf.view(np.float32).astype(np.float64)


def within(got, ref, tol, what, mask=None):
    err = np.abs(got - ref)
    ok = np.isfinite(got) & (err <= tol)
    if mask is not None:
        ok = ok | ~mask
    ratio = float((err / np.maximum(tol, 1e-300))[mask if mask is not None else slice(None)].max()) if err.size else 0.0
    assert ok.all(), f"{what}: {int((~ok).sum())} values outside the bound, max |err| / tol = {ratio:.3f}"
    return ratio


# --------------------------------------------------------------------------- FILTER
def test_filter(lib):
    fmt, L = lib
    from oracle.bigvgan_np import anti_alias_filter
    f = anti_alias_filter(2).astype(np.float32).astype(np.float64)
    for taps in (None, kr.BV_TAPS_EXACT):
        out = np.zeros(24, np.float32)
        call(L, FILTER, out=out, taps=taps)
        want = kr.bv_filter_ref(f if taps is None else taps)
        if taps is None:            # the engine evaluates the Bessel window itself: the last bit may differ
            assert np.abs(out - want).max() <= 2.0 ** -23 * np.abs(want).max()
        else:
            assert np.array_equal(out.astype(np.float64), want)


# --------------------------------------------------------------------------- ACT
def run_act(L, fmt, mode, split, x, lens, scale, B, Lmax, halo, C, alpha, ibeta, taps, stale=1):
    Lp, Cp = kr.bv_rows(Lmax, halo), -(-C // 32) * 32
    M = B * Lp
    if mode == 0:
        out = can32(M, C)
        call(L, ACT, mode=0, split=split, B=B, Lmax=Lmax, halo=halo, C=C, scale=scale, lens=lens, x=x, alpha=alpha,
             ibeta=ibeta, taps=taps, out=out, stale=stale)
        return as64(interior(out, M, CAN32, "act out")), None
    rows = M + 2 * halo
    bufs = []
    for _ in range(2 if split == 3 else 1):
        b = np.full((rows + 2 * GUARD, Cp), CAN16, np.uint16)
        b[GUARD + halo + M:GUARD + rows] = np.uint16(0x3C55)       # the trailing halo: never written
        bufs.append(b)
    call(L, ACT, mode=2, split=split, B=B, Lmax=Lmax, halo=halo, C=C, scale=scale, lens=lens, x=x, alpha=alpha,
         ibeta=ibeta, taps=taps, oh=bufs[0], ol=bufs[1] if split == 3 else None, stale=stale)
    outs = []
    for b in bufs:
        r = interior(b, rows, CAN16, "act operand")
        assert (r[halo + M:] == 0x3C55).all(), "the trailing halo rows were written"
        assert (r[:halo] == 0).all(), "the halo rows before utterance 0 must be zero"
        outs.append(kr.decode16(r[halo:halo + M], fmt))
    return outs[0], outs[1] if split == 3 else None


def check_operand(hi, lo, z, tol, C, fmt, what):
    """The MODE 2 operand against the reference: pad channels zero, hi by the ambiguity rule, hi + lo
    against the fp32 value."""
    assert (hi[:, C:] == 0).all() and (lo is None or (lo[:, C:] == 0).all()), f"{what}: pad channels not zero"
    bad, amb, _, _ = kr.check16(hi[:, :C], z, tol, fmt)
    assert not bad.any(), f"{what}: {int(bad.sum())} hi values off (of {bad.size}, {int(amb.sum())} ambiguous)"
    if lo is not None:
        lim = tol + 2.0 ** -24 * np.abs(z) + 0.5 * kr.ulp16(0.5 * kr.ulp16(np.abs(z) + tol, fmt), fmt)
        err = np.abs(hi[:, :C] + lo[:, :C] - z)
        assert (err <= lim).all(), f"{what}: max |hi + lo - ref| / allowed = {(err / lim).max():.3f}"


@pytest.mark.parametrize("C", ACT_C)
@pytest.mark.parametrize("Lmax", ACT_LMAX + ["scaled"])
def test_act(lib, Lmax, C):
    fmt, L = lib
    ratios = []
    for halo in (8, 32):
        for klass in ("exact", "general", "wide"):
            c = act_case(Lmax, C, halo, klass)
            z, tol = kr.bv_act_ref(c["x"], c["lens"], c["scale"], c["B"], c["Lmax"], c["Lp"], c["alpha"], c["ibeta"],
                                   c["f"], klass)
            args = (c["x"], c["lens"], c["scale"], c["B"], c["Lmax"], halo, C, c["alpha"], c["ibeta"], c["taps"])
            tag = f"{fmt} ACT {klass} Lmax={Lmax} C={C} halo={halo}"
            out, _ = run_act(L, fmt, 0, 1, *args)
            if klass == "exact":
                assert np.array_equal(out, z), f"{tag}: {int((out != z).sum())} values differ"
            else:
                valid = tol > 0
                assert (out[~valid] == 0).all(), f"{tag}: rows outside the utterances must be zero"
                ratios.append(within(out, z, tol, tag))
            if klass == "wide":         # (its allowance is past the fp16 ulp: the fp32 output only)
                continue
            for split in (1, 3):
                hi, lo = run_act(L, fmt, 2, split, *args, stale=split)
                if klass == "exact":
                    rh, rl = kr.split16(z, fmt)
                    assert np.array_equal(hi[:, :C], rh) and (hi[:, C:] == 0).all(), f"{tag} split {split}: hi"
                    if lo is not None:
                        assert np.array_equal(lo[:, :C], rl) and (lo[:, C:] == 0).all(), f"{tag}: lo"
                else:
                    check_operand(hi, lo, z, tol, C, fmt, f"{tag} split {split}")
    print(f"{fmt} ACT Lmax={Lmax} C={C}: general max |err| / tol = {max(ratios):.3f}")


def sine_sweep(L, klass, n=4096, C=16):
    """The sine term alone: with the one-tap filter z[t] = 2 x[t] + ib sin^2(2 a x[t]).  |y| <= 2^-6,
    alpha spreads |alpha y| over the class's range; returns (max |err| of the term, max |arg|)."""
    rng = rng_for("sine", klass)
    top = kr.BV_ARG_GENERAL if klass == "general" else kr.BV_ARG_WIDE
    taps = np.zeros(12)
    taps[5] = 1.0
    x = (rng.integers(1, 2 ** 10, (n, C)) * 2.0 ** -17 * rng.choice([-1.0, 1.0], (n, C)))
    halo, Lp = 8, kr.bv_rows(n, 8)
    xs = np.zeros((Lp, C))
    xs[:n] = x
    alpha = (np.geomspace(1.0, top, C) / 2.0 ** -6).astype(np.float32).astype(np.float64)
    ibeta = np.ones(C)
    out, _ = run_act(L, "bf16", 0, 1, xs, None, 1, 1, n, halo, C, alpha, ibeta, taps)
    y = 2.0 * x
    arg = (y * alpha).astype(np.float32).astype(np.float64)     # the kernel's fp32 product, exact here or not
    ref = y + np.sin(y * alpha) ** 2
    return float(np.abs(out[:n] - ref).max()), float(np.abs(arg).max())


def test_act_sine_term(lib):
    """The hardware sine behind __sinf over the general class's range and over 64 turns: its measured
    error against float64 stays inside the allowance each class's tolerance carries for it."""
    fmt, L = lib
    for klass in ("general", "wide"):
        err, top = sine_sweep(L, klass)
        print(f"{fmt} sine term {klass}: max |err| = {err:.3e} up to |arg| = {top:.1f} rad "
              f"(allowance {kr.BV_ETERM[klass]:.3e})")
        assert err <= kr.BV_ETERM[klass]


# --------------------------------------------------------------------------- CONV
def run_conv(L, fmt, split, c, hi, lo):
    out = can32(c["M"], c["C"])
    a = call(L, CONV, split=split, B=c["B"], Lmax=c["Lmax"], halo=c["halo"], C=c["C"], Cout=c["C"], ks=c["ks"],
             d=c["d"], w=c["w"], bias=c["bias"], resid=c["resid"], ah=hi, al=lo, out=out)
    return as64(interior(out, c["M"], CAN32, "conv out")), list(a.launch)


@pytest.mark.parametrize("C", CONV_C)
def test_conv(lib, C):
    fmt, L = lib
    ratios = []
    for case in conv_cases(C):
        for split in (1, 3):
            for klass in ("exact", "general"):
                c = conv_inputs(case, klass, split, fmt)
                ref, tol, valid = kr.bv_conv_ref(c["a"], c["w"], c["bias"], c["d"], c["lens"], 1, c["B"], c["Lmax"],
                                                 c["Lp"], split, fmt, c["resid"], klass)
                need = needed_rows(c)
                outs = []
                for fill in ("stale", "zero"):
                    ops = []
                    for half, sd in zip(c["operand"], (11, 12)):
                        buf = np.zeros((c["M"] + 2 * c["halo"], c["Cp"]), np.uint16)
                        if fill == "stale":
                            r = rng_for("stale", sd, buf.shape)
                            buf[:] = 0x3C00 | r.integers(0, 0x400, buf.shape).astype(np.uint16)
                        buf[need] = 0
                        rows = c["halo"] + np.flatnonzero(valid)
                        buf[rows, :C] = kr.encode16(half[valid], fmt)
                        ops.append(buf)
                    out, rec = run_conv(L, fmt, split, c, ops[0], ops[1] if split == 3 else None)
                    want = conv_predict(C, split)
                    assert rec[:3] + [rec[5]] == want, (rec, want)
                    outs.append(out)
                tag = f"{fmt} CONV {klass} {case} split {split}"
                assert np.array_equal(outs[0][valid], outs[1][valid]), f"{tag}: valid rows depend on unread rows"
                if klass == "exact":
                    assert np.array_equal(outs[0][valid], ref[valid]), \
                        f"{tag}: {int((outs[0][valid] != ref[valid]).sum())} values differ"
                else:
                    ratios.append(within(outs[0][valid], ref[valid], tol[valid], tag))
    print(f"{fmt} CONV C={C}: general max |err| / tol = {max(ratios):.3f}")


def test_conv_cases_reach_every_arm():
    arms = {tuple(conv_predict(C, s)) for C in CONV_C for s in (1, 3)}
    want = {(bm, bn, s, bk) for s in (1, 3) for bm, bn, bk in
            ((256, 32, 32), (256, 48, 64), (64, 64, 64), (128, 96, 32), (128, 128, 32), (128, 128, 64))}
    assert arms == want


# --------------------------------------------------------------------------- CONVT
@pytest.mark.parametrize("u,k", CONVT_UK)
def test_convt(lib, u, k):
    fmt, L = lib
    ratios = []
    for Lin in (1, 2, 5):
        for Cout in (8, 24):
            for stage0 in (True, False):
                c = convt_inputs(u, k, Lin, Cout, stage0)
                B, halo, Ls, Lo = c["B"], c["halo"], c["Ls"], c["Lo"]
                kw = dict(B=B, Lmax=Lin, Ls=Ls, halo=halo, Cout=Cout, ks=k, u=u, scale=c["scale"], lens=c["lens"],
                          bias=c["bias"])
                # the gather alone, exact: small-integer P
                ref, _ = kr.bv_convt_ref(c["P"], c["eye"], c["bias"], u, c["lens"], c["scale"], B, Lin, Ls, Lo,
                                         klass="exact")
                out = can32(B * Lo, Cout)
                call(L, CONVT, flag=0, C=k * Cout, x=c["P"], out=out, **kw)
                got = as64(interior(out, B * Lo, CAN32, "convt out"))
                assert np.array_equal(got, ref), f"{fmt} gather u={u} k={k} Lin={Lin} Cout={Cout} stage0={stage0}"
                # with the relayout and the GEMM
                for split in (1, 3):
                    for klass in ("exact", "general"):
                        x, w = c["x"][klass], c["w"][klass]
                        ref, tol = kr.bv_convt_ref(x, w, c["bias"], u, c["lens"], c["scale"], B, Lin, Ls, Lo, split,
                                                   fmt, klass)
                        out = can32(B * Lo, Cout)
                        a = call(L, CONVT, flag=1, split=split, C=c["Cin"], x=x, w=w, out=out, **kw)
                        got = as64(interior(out, B * Lo, CAN32, "convt out"))
                        assert list(a.launch)[:3] + [a.launch[5]] == [128, 128, split, 64]
                        tag = f"{fmt} CONVT {klass} u={u} k={k} Lin={Lin} Cout={Cout} stage0={stage0} split {split}"
                        if klass == "exact":
                            assert np.array_equal(got, ref), tag
                        else:
                            assert (got[tol == 0] == 0).all(), f"{tag}: rows past len_in * u must be zero"
                            ratios.append(within(got, ref, tol, tag, tol > 0))
    print(f"{fmt} CONVT u={u} k={k}: general max |err| / tol = {max(ratios):.3f}")


# --------------------------------------------------------------------------- POST
@pytest.mark.parametrize("C", [16, 24])
@pytest.mark.parametrize("Lmax", POST_LMAX)
def test_post(lib, Lmax, C):
    fmt, L = lib
    for klass in ("exact", "general"):
        for use_tanh in (0, 1):
            c = post_inputs(Lmax, C, klass)
            ref, tol = kr.bv_post_ref(c["a"], c["w"], c["bias0"], c["lens"], c["scale"], c["B"], Lmax, c["Ls"],
                                      use_tanh, klass)
            out = can32(c["B"] * Lmax, 1)
            call(L, POST, B=c["B"], Lmax=Lmax, Ls=c["Ls"], C=C, scale=c["scale"], lens=c["lens"], x=c["a"], w=c["w"],
                 bias0=c["bias0"], flag=use_tanh, out=out)
            got = as64(interior(out, c["B"] * Lmax, CAN32, "wav"))[:, 0]
            tag = f"{fmt} POST {klass} tanh={use_tanh} Lmax={Lmax} C={C}"
            if not use_tanh and Lmax >= 3:
                assert (np.abs(ref) == 1.0).any(), f"{tag}: the inputs must drive outputs past +-1"
            if klass == "exact" and not use_tanh:
                assert np.array_equal(got, ref), f"{tag}: {int((got != ref).sum())} samples differ"
            else:
                assert (got[tol == 0] == 0).all(), f"{tag}: samples past the utterance must be zero"
                within(got, ref, tol, tag, tol > 0)


def test_post_rejects_wide_channels(lib):
    """(256 + 6) * C * 4 bytes of LDS: C = 64 is past the 64 KiB window; the call fails before any launch."""
    fmt, L = lib
    C = 64
    call(L, POST, expect_error="too wide for the LDS window", B=1, Lmax=4, Ls=4, C=C, x=np.zeros((4, C)),
         w=np.zeros((C, 7)), out=can32(4, 1))


# --------------------------------------------------------------------------- AVG, IM2COL
@pytest.mark.parametrize("n", [1, 2, 3])
def test_avg(lib, n):
    fmt, L = lib
    for C, ld, M in ((24, 0, 7), (24, 64, 7), (48, 64, 300), (96, 128, 33)):
        for split in (1, 3):
            rng = rng_for("avg", n, C, ld, split)
            ys = [(3 * rng.standard_normal((M, C))).astype(np.float32).astype(np.float64) for _ in range(n)]
            ref, tol = kr.bv_avg_ref(ys)
            out = can32(M, C)
            o16 = [np.full((M + 2 * GUARD, ld), CAN16, np.uint16) for _ in range(2)] if ld else [None, None]
            call(L, AVG, split=split, B=1, Lmax=M, C=C, n=n, x=ys[0], x1=ys[1] if n > 1 else None,
                 x2=ys[2] if n > 2 else None, out=out, oh=o16[0], ol=o16[1] if split == 3 else None, ld=ld)
            got = as64(interior(out, M, CAN32, "avg"))
            within(got, ref, tol, f"{fmt} AVG n={n} C={C}")
            if ld:
                hi = interior(o16[0], M, CAN16, "avg hi")
                assert (hi[:, C:] == CAN16).all(), "AVG writes C columns only"
                rh, rl = kr.split16(got, fmt)            # the copies of the kernel's own fp32 value
                assert np.array_equal(kr.decode16(hi[:, :C], fmt), rh)
                if split == 3:
                    lo = interior(o16[1], M, CAN16, "avg lo")
                    assert np.array_equal(kr.decode16(lo[:, :C], fmt), rl) and (lo[:, C:] == CAN16).all()


@pytest.mark.parametrize("layout", [0, 1])
def test_im2col(lib, layout):
    """C = 100 mel channels, 7 taps: K = 700 of a row stride 704; columns [700, 704) keep the stale
    pattern the caller put there, and conv_pre's GEMM must not see it."""
    fmt, L = lib
    C, ks, B, Co = 100, 7, 3, 40
    K, ld = C * ks, 704
    for T, lens in ((1, [1, 1, 1]), (5, [5, 1, 3]), (9, [9, 2, 8])):
        for div, sub in ((1.0, 0.0), (0.1, -4.5)):
            for split in (1, 3):
                rng = rng_for("im2col", layout, T, div, split)
                x = rng.standard_normal((B, C, T) if layout == 0 else (B, T, C)) * 1.5 - 4.0
                x = x.astype(np.float32).astype(np.float64)
                w = (rng.standard_normal((Co, C, ks)) / np.sqrt(K)).astype(np.float32).astype(np.float64)
                bias = rng.standard_normal(Co).astype(np.float32).astype(np.float64)
                A, tolA, zero = kr.im2col_ref(x, layout, np.float32(div).astype(np.float64),
                                              np.float32(sub).astype(np.float64), lens, B, T, C, ks)
                M = B * T
                bufs = [np.full((M + 2 * GUARD, ld), CAN16, np.uint16) for _ in range(2)]
                stale = 0x3C00 | rng.integers(0, 0x400, (M, ld - K)).astype(np.uint16)
                for b in bufs:
                    b[GUARD:GUARD + M, K:] = stale
                out = can32(M, Co)
                call(L, IM2COL, split=split, B=B, Lmax=T, C=C, ks=ks, layout=layout, div=div, sub=sub, lens=lens,
                     x=x.reshape(-1), oh=bufs[0], ol=bufs[1] if split == 3 else None, flag=1, Cout=Co, w=w, bias=bias,
                     out=out)
                hi = interior(bufs[0], M, CAN16, "im2col hi")
                assert np.array_equal(hi[:, K:], stale), "columns [700, 704) are not the kernel's to write"
                hv = kr.decode16(hi[:, :K], fmt)
                tag = f"{fmt} IM2COL layout {layout} T={T} div={div} split {split}"
                assert (hv[zero] == 0).all() and (hi[:, :K][zero] == 0).all(), f"{tag}: zero taps"
                assert kr.amb16(A[~zero], tolA[~zero], fmt)[0].mean() <= kr.AMB_CAP      # from the reference alone
                bad, _, _, _ = kr.check16(hv, A, tolA, fmt)
                assert not (bad & ~zero).any(), f"{tag}: {int((bad & ~zero).sum())} hi values off"
                val = hv
                if split == 3:
                    lv = kr.decode16(interior(bufs[1], M, CAN16, "im2col lo")[:, :K], fmt)
                    assert (lv[zero] == 0).all()
                    val = hv + lv
                    lim = tolA + 0.5 * kr.ulp16(0.5 * kr.ulp16(np.abs(A) + tolA, fmt), fmt)
                    assert (np.abs(val - A) <= lim).all(), f"{tag}: hi + lo"
                # conv_pre on the operand the kernel wrote
                As = [hv] if split == 1 else [hv, lv]
                wm = np.concatenate([w[:, :, t] for t in range(ks)], 1)
                Ws = kr.operands(val, wm, split, fmt)[1]
                ref = kr.dot_kernel(As, Ws) + bias
                tol = kr.dot_tol(val, wm, split) + 2 * kr.U32 * (np.abs(val) @ np.abs(wm).T + np.abs(bias))
                got = as64(interior(out, M, CAN32, "conv_pre"))
                within(got, ref, tol, tag + " + GEMM")


# --------------------------------------------------------------------------- STEP
@pytest.mark.parametrize("C", [24, 64])
@pytest.mark.parametrize("ks,d", [(11, 5), (3, 1)])
def test_step(lib, ks, d, C):
    fmt, L = lib
    for split in (1, 3):
        c = step_inputs(C, ks, d)
        ref, tol, valid = kr.bv_step_ref(c, split, fmt)
        outs = []
        for stale in (1, 2):
            out = can32(c["M"], C)
            call(L, STEP, split=split, B=c["B"], Lmax=c["Lmax"], halo=c["halo"], C=C, Cout=C, ks=ks, d=d,
                 lens=c["lens"], x=c["x"], alpha=c["alpha"], ibeta=c["ibeta"], w=c["w"], bias=c["bias"],
                 alpha2=c["alpha2"], ibeta2=c["ibeta2"], w2=c["w2"], bias2=c["bias2"], out=out, stale=stale)
            outs.append(as64(interior(out, c["M"], CAN32, "step out")))
        tag = f"{fmt} STEP C={C} ks={ks} d={d} split {split}"
        assert np.array_equal(outs[0][valid], outs[1][valid]), f"{tag}: valid rows depend on stale memory"
        r = within(outs[0][valid], ref[valid], tol[valid], tag)
        print(f"{tag}: max |err| / tol = {r:.2e}")
