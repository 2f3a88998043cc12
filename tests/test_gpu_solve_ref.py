"""The kernels around the decoder (csrc/zv_elem.inc: operand build, Euler update / CFG combine, mask
copy, fill, timestep embedding, the small fp32 linear, the positional projection, embedding lookup,
speaker add, text and speech condition), each launched through the launch function zv_engine calls
(zv_solve_check), against float64 references written from the model's definition (tests/kernel_ref.py,
"solve boundary"; inputs and case lists in tests/solve_cases.py, which tests/test_kernel_ref.py's
visibility checks share).

Exact classes (bit for bit): the operand build and the embedding against kr.split16 (the two kernels
that write 16-bit operands, run in both operand libraries); Euler / combine, the small linear without
activation (dyadic operands: every fp32 step is exact, asserted by the reference); mask copy, fill,
speaker add, text and speech condition (copies, or one exact addition).
General classes: Euler / combine: one fp32 rounding per operation weighted by that operation's float64
result (kr.euler_ref); the small linear: (ceil(K / 64) + 8) 2^-24 (sum |x w| + |b| + |add|), plus
sum |w| times SwooshR's tolerance under pre = 1 (kr.small_linear_ref); the timestep embedding and the
positional projection: the kernels' fp32 formulas restated in numpy, their error against float64
measured on the CPU over these tests' arguments (kr.ERR_SINCOS, kr.err_posp_angle, kr.err_swoosh_r_lae;
tests/test_kernel_ref.py recomputes them), times kr.TRANS_FACTOR, propagated through a = xa (k + 1) and
the D-term dot product (kr.posp_table, kr.posp_ref).  None is tuned against a kernel's output.

Every output has canary-filled guard rows (16-bit outputs and the small linear's also a row stride
larger than the width) which must come back intact.  Each test prints its max |err| / tolerance
(profiles/solve_ref_pin.txt)."""
import ctypes

import numpy as np
import pytest

import kernel_ref as kr
import solve_cases as sc

pytestmark = pytest.mark.gpu

(BUILD, EULER, COMBINE, MASKCOPY, FILL, TEMB, LINEAR, POSP, EMBED, SPK, TEXT, SPEECH) = range(12)
CAN32, CAN16, CAN8 = np.uint32(0x7FC5A5A5), np.uint16(0x7FA5), np.uint8(0xA5)
GUARD = 2
CAP = 65536 * 256                      # grid1d's cap in threads: one more element takes a second trip


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
    """One zv_solve_check call; arrays are passed by address (and kept alive).  Returns the launch record."""
    from zipvoice_amd.engine import ZvSolveCheckArgs
    a = ZvSolveCheckArgs()
    a.kind, a.guard, a.form = kind, GUARD, -1
    for k, v in fields.items():
        if v is None:
            continue
        if isinstance(v, np.ndarray):
            assert v.flags["C_CONTIGUOUS"]
            setattr(a, k, v.ctypes.data)
        else:
            setattr(a, k, v)
    rc = Lb.zv_solve_check(ctypes.byref(a))
    assert rc == 0, Lb.zv_last_error().decode()
    assert a.launch[0] == kind and a.launch[3] == 256
    return list(a.launch)


def canary(rows, ld, can):
    return np.full((rows + 2 * GUARD, ld), can, can.dtype)


def interior(buf, rows, width, what):
    """The (rows, width) interior of a canary-filled output; everything around it must be untouched."""
    can = {4: CAN32, 2: CAN16, 1: CAN8}[buf.dtype.itemsize]
    mask = np.ones(buf.shape, bool)
    mask[GUARD:GUARD + rows, :width] = False
    touched = int((buf[mask] != can).sum())
    assert touched == 0, f"{what}: {touched} elements outside the output were written"
    got = buf[GUARD:GUARD + rows, :width]
    return got.view(np.float32).astype(np.float64) if buf.dtype == np.uint32 else got


def flat_out(n):
    """A flat fp32 output with GUARD guard elements at both ends."""
    return np.full(n + 2 * GUARD, CAN32, np.uint32)


def flat_interior(buf, n, what):
    assert (buf[:GUARD] == CAN32).all() and (buf[GUARD + n:] == CAN32).all(), f"{what}: guard elements written"
    return buf[GUARD:GUARD + n].view(np.float32)


def within(got, ref, tol, what):
    err = np.abs(got - ref)
    ok = np.isfinite(got).all() and (err <= tol).all()
    ratio = float((err / np.maximum(tol, 1e-300)).max())
    assert ok, f"{what}: max |err| / tol = {ratio:.3f}, max |err| = {err.max():.3e}"
    return ratio


# --------------------------------------------------------------------------- build input
@pytest.mark.parametrize("T", sc.BUILD_T)
@pytest.mark.parametrize("Fx,Ft,ld", sc.BUILD_SHAPES)
def test_build_input(lib, Fx, Ft, ld, T):
    """cat[x, text, speech] with the CFG copies, bit for bit kr.split16 of the float64 reference, through
    the policy's kernel; pad columns [Fin, ld) and guard rows stay canary."""
    fmt, Lb = lib
    B, Fin = sc.BUILD_B, 2 * Fx + Ft
    x, tc, s = sc.build_inputs(Fx, Ft, T)
    kx, kt, ks = f32(x), f32(tc), f32(s)
    for copies in (1, 2):
        for zs in (0, 1):
            for lo in (True, False):
                rows = copies * B * T
                oh, ol = canary(rows, ld, CAN16), canary(rows, ld, CAN16) if lo else None
                rec = call(Lb, BUILD, B=B, T=T, Fx=Fx, Ft=Ft, Fs=Fx, copies=copies, zero_speech=zs, ld=ld, x=kx,
                           tc=kt, sc=ks, oh=oh, ol=ol)
                what = f"{fmt} build ({Fx}, {Ft}, ld {ld}) T={T} copies={copies} zs={zs} lo={lo}"
                assert rec[1] == int(sc.build_quad(Fx, Ft, ld)), what
                hi, lw = kr.split16(kr.build_input_ref(x, tc, s, B, T, copies, zs), fmt)
                assert np.array_equal(kr.decode16(interior(oh, rows, Fin, what), fmt), hi), what + ": hi"
                if lo:
                    assert np.array_equal(kr.decode16(interior(ol, rows, Fin, what), fmt), lw), what + ": lo"


def decode16_f32(u, fmt):
    return u.view(np.float16).astype(np.float32) if fmt == "f16" else (u.astype(np.uint32) << 16).view(np.float32)


def test_build_input_second_trip(lib):
    """The scalar kernel with more elements than grid1d's cap has threads (65536 x 256) plus a tail: the
    grid-stride loop's second trip.  Values are integers the 16-bit formats hold exactly (the three
    sources 64 apart), so the expected operand is the value itself."""
    fmt, Lb = lib
    Fx = Ft = 10
    Fin, ld, T = 30, 32, CAP // 30 + 3
    assert T * Fin > CAP and (T * Fin - CAP) % 256 != 0
    rng = sc.rng_for("build big")
    x = rng.integers(-8, 9, (T, Fx)).astype(np.float32)
    tc = (64 + rng.integers(0, 9, (T, Ft))).astype(np.float32)
    s = (-64 - rng.integers(0, 9, (T, Fx))).astype(np.float32)
    oh = canary(T, ld, CAN16)
    rec = call(Lb, BUILD, B=1, T=T, Fx=Fx, Ft=Ft, Fs=Fx, copies=1, zero_speech=0, ld=ld, x=x, tc=tc, sc=s, oh=oh)
    assert rec[1] == 0 and rec[2] == 65536, rec
    got = decode16_f32(interior(oh, T, Fin, "build big"), fmt)
    assert np.array_equal(got, np.concatenate([x, tc, s], axis=1))


# --------------------------------------------------------------------------- Euler / combine
@pytest.mark.parametrize("klass", ["exact", "general"])
@pytest.mark.parametrize("T", sc.EULER_T)
def test_euler_and_combine(lib0, T, klass):
    """x += ((1 + g) v_cond - g v_uncond) dt in place over x, and the combine alone; scalar and per-row g
    (rows (0, 3, -0.5), doubled where gmul = 2), with and without CFG."""
    B, per_row = sc.EULER_B, T * sc.EULER_FX
    n = B * per_row
    assert per_row % 256 != 0
    x, v, g, dt = sc.euler_inputs(T, klass)
    ratios = []
    for mode, grows, gmul in sc.EULER_MODES:
        cfg = int(mode != "nocfg")
        vk = v if cfg else v[:n]
        gr = None if grows is None else np.asarray(grows, np.float64)
        kw = dict(n=n, v=f32(vk), g=g, dt=dt, gmul=gmul, per_row=per_row, B=B, grows=None if gr is None else f32(gr))
        what = f"euler T={T} {klass} {mode} gmul={gmul}"
        jobs = [(EULER, x)] + ([(COMBINE, None)] if cfg else [])
        for kind, xin in jobs:
            out = flat_out(n)
            call(lib0, kind, cfg=cfg, x=None if xin is None else f32(xin), out=out, **kw)
            got = flat_interior(out, n, what).astype(np.float64)
            ref, tol = kr.euler_ref(xin, vk, cfg, g, dt, gr, gmul, per_row, exact=klass == "exact")
            if klass == "exact":
                assert np.array_equal(got, ref), f"{what} kind {kind}: {int((got != ref).sum())} values differ"
            else:
                ratios.append(within(got, ref, tol, f"{what} kind {kind}"))
    if ratios:
        print(f"PIN EULER T={T}: max |err| / tol = {max(ratios):.3f}")


def test_euler_second_trip(lib0):
    """n = 65536 x 256 + 77 values, three rows with their own scales: the grid-stride second trip and
    i / per_row at a large i.  Integers in [-8, 8], g in {0, 6, -1}, dt = 1/8: every intermediate is a
    multiple of 1/8 below 2^10, exact in fp32, so numpy's fp32 evaluation is the exact value."""
    B, per_row = 3, (CAP + 77) // 3
    n = B * per_row
    assert n == CAP + 77
    rng = sc.rng_for("euler big")
    x = rng.integers(-8, 9, n).astype(np.float32)
    v = rng.integers(-8, 9, 2 * n).astype(np.float32)
    grows = np.asarray(sc.EULER_GROWS, np.float32)
    out = flat_out(n)
    rec = call(lib0, EULER, cfg=1, n=n, x=x, v=v, g=0.0, dt=0.125, gmul=2.0, per_row=per_row, B=B, grows=grows, out=out)
    assert rec[2] == 65536, rec
    gi = np.repeat(grows * np.float32(2), per_row)
    ref = x + ((np.float32(1) + gi) * v[n:] - gi * v[:n]) * np.float32(0.125)
    got = flat_interior(out, n, "euler big")
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} values differ"


# --------------------------------------------------------------------------- mask copy, fill
@pytest.mark.parametrize("n", [1, 255, 1000])
def test_mask_copy_and_fill(lib0, n):
    m = sc.rng_for("mask", n).integers(0, 2, n).astype(np.uint8)
    for copies in (1, 2):
        mout = np.full(n * copies + 2 * GUARD, CAN8, np.uint8)
        call(lib0, MASKCOPY, n=n, copies=copies, mask=m, mout=mout)
        assert (mout[:GUARD] == CAN8).all() and (mout[GUARD + n * copies:] == CAN8).all()
        assert np.array_equal(mout[GUARD:GUARD + n * copies], np.tile(m, copies))
    out = flat_out(n)
    call(lib0, FILL, n=n, value=0.3, out=out)
    assert np.array_equal(flat_interior(out, n, "fill"), np.full(n, np.float32(0.3)))


# --------------------------------------------------------------------------- timestep embedding
@pytest.mark.parametrize("dim", sc.TEMB_DIMS)
@pytest.mark.parametrize("M", [1, 3])
def test_timestep_embed(lib0, M, dim):
    fr = kr.temb_freqs(dim)
    ratios = []
    for which in ("t", "g"):
        t = sc.temb_t(M, which)
        out = canary(M, dim, CAN32)
        call(lib0, TEMB, M=M, N=dim, x=f32(t), W=f32(fr), out=out)
        got = interior(out, M, dim, f"temb M={M} dim={dim}")
        ref, tol = kr.temb_ref(t, fr, dim)
        if dim % 2:
            assert (got[:, -1] == 0).all(), "the odd dim's last column is zero"
        ratios.append(within(got, ref, tol, f"temb M={M} dim={dim} {which}"))
    print(f"PIN TEMB M={M} dim={dim}: max |err| / tol = {max(ratios):.3f}")


# --------------------------------------------------------------------------- small linear
@pytest.mark.parametrize("M,N,K,pre,bias,add", sc.SMALL_LINEAR)
def test_small_linear(lib0, M, N, K, pre, bias, add):
    """out = act(x) W^T + b + add through the policy (the row-staged kernel up to K = 8192), and each
    kernel forced where both take the shape: bitwise equal, as zv_elem.inc claims."""
    ldin, ldw, ld = K + 3, K + 5, N + 7
    ratios = []
    for klass in (("exact", "general") if not pre else ("general",)):
        x, W, b, a = sc.small_linear_inputs(M, N, K, pre, bias, add, klass)
        xp, Wp = np.zeros((M, ldin)), np.zeros((N, ldw))
        xp[:, :K], Wp[:, :K] = x, W
        xp[:, K:], Wp[:, K:] = 1e6, -1e6                # a read past the width is off by far
        ref, tol = kr.small_linear_ref(x, W, b, a, pre, exact=klass == "exact")
        outs = {}
        for form in (-1, 0, 1) if K <= 8192 else (-1, 1):
            out = canary(M, ld, CAN32)
            rec = call(lib0, LINEAR, M=M, N=N, K=K, pre=pre, form=form, ldin=ldin, ldw=ldw, ld=ld, x=f32(xp), W=f32(Wp),
                       bias=None if b is None else f32(b), add=None if a is None else f32(a), inplace=int(add == "out"),
                       out=out)
            assert rec[1] == ((0 if K <= 8192 else 1) if form < 0 else form), rec
            what = f"small linear {M}x{N}x{K} pre={pre} {klass} form={form}"
            got = outs[form] = interior(out, M, N, what)
            if klass == "exact":
                assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} values differ"
            else:
                ratios.append(within(got, ref, tol, what))
        if 0 in outs:
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[-1], outs[0]), "the two kernels differ"
    print(f"PIN SMALL_LINEAR {M}x{N}x{K} pre={pre}: max |err| / tol = {max(ratios):.3f}")


# --------------------------------------------------------------------------- posP
@pytest.mark.parametrize("L,nl,HPD,D", sc.POSP)
def test_posp(lib0, L, nl, HPD, D):
    """One-hot weights: every output is a single entry of the table, so each column's placement and
    accuracy shows on its own; Gaussian weights: the D-term dot product."""
    rows = nl * (2 * L - 1)
    ratios = {}
    for klass, shifts in (("onehot", sc.posp_shifts(nl, HPD, D)), ("general", (0,))):
        for sh in shifts:
            W = sc.posp_weights(L, nl, HPD, D, klass, sh)
            out = canary(rows, HPD, CAN32)
            call(lib0, POSP, T=L, M=nl, N=HPD, K=D, W=f32(W), out=out)
            what = f"posP L={L} nl={nl} HPD={HPD} D={D} {klass} shift={sh}"
            got = interior(out, rows, HPD, what)
            ref, tol = kr.posp_ref(W, L, nl, HPD, D)
            if klass == "onehot":                         # the constant column is exact
                one = np.tile(((np.arange(nl * HPD) + sh) % D == D - 1).reshape(nl, 1, HPD), (1, 2 * L - 1, 1)).reshape(rows, HPD)
                assert (got[one] == 1.0).all(), what + ": pe[D - 1] = 1"
            ratios[klass] = max(ratios.get(klass, 0.0), within(got, ref, tol, what))
    print(f"PIN POSP L={L} nl={nl} HPD={HPD} D={D}: max |err| / tol one-hot {ratios['onehot']:.3f}, general {ratios['general']:.3f}")


# --------------------------------------------------------------------------- the text side
@pytest.mark.parametrize("C", sc.TEXT_C)
def test_embed(lib, C):
    """nn.Embedding into the 16-bit operand: bit for bit kr.split16 of the table's rows."""
    fmt, Lb = lib
    V, n, ld = 11, 2 * 7, C + 3
    tab = sc.table(1, V, C)[0]
    tok = sc.rng_for("embed", C).integers(0, V, n).astype(np.int64)
    tok[0], tok[-1] = V - 1, 0
    hi, lw = kr.split16(kr.embed_ref(tok, tab), fmt)
    for lo in (True, False):
        oh, ol = canary(n, ld, CAN16), canary(n, ld, CAN16) if lo else None
        call(Lb, EMBED, n=n, C=C, N=V, ld=ld, tok=tok, W=f32(tab), oh=oh, ol=ol)
        assert np.array_equal(kr.decode16(interior(oh, n, C, "embed"), fmt), hi)
        if lo:
            assert np.array_equal(kr.decode16(interior(ol, n, C, "embed lo"), fmt), lw)


@pytest.mark.parametrize("C", sc.TEXT_C)
def test_spk_add(lib0, C):
    B, S = 2, 9
    emb = sc.table(B, S, C).reshape(B * S, C)
    tab = np.stack([0.5 + np.arange(C) / 4.0, -300.0 - np.arange(C) / 8.0])
    spk = np.array([0, 0, 1, 1, -1, 0, 1, -1, -1, 1, 0, -1, 1, 0, 0, 1, -1, -1], np.int8)   # -1, 0, 1 inside a row
    out = canary(B * S, C, CAN32)
    call(lib0, SPK, n=B * S, C=C, x=f32(emb), spk=spk, W=f32(tab), out=out)
    assert np.array_equal(interior(out, B * S, C, "spk add"), kr.spk_add_ref(emb, spk, tab))


@pytest.mark.parametrize("case", range(len(sc.TEXT_COND)))
@pytest.mark.parametrize("C", sc.TEXT_C)
def test_text_condition(lib0, C, case):
    T, tl, fl, S = sc.TEXT_COND[case]
    B = len(tl)
    emb = sc.table(B, S, C)
    out = canary(B * T, C, CAN32)
    call(lib0, TEXT, B=B, T=T, S=S, C=C, x=f32(emb), lens=np.asarray(tl, np.int32), lens2=np.asarray(fl, np.int32), out=out)
    got, ref = interior(out, B * T, C, "text condition"), kr.text_cond_ref(emb, tl, fl, T)
    assert np.array_equal(got, ref), f"{int((got != ref).any(1).sum())} frames differ"


@pytest.mark.parametrize("case", range(len(sc.SPEECH_COND)))
@pytest.mark.parametrize("C", sc.TEXT_C)
def test_speech_condition(lib0, C, case):
    T, Tp, plen = sc.SPEECH_COND[case]
    B = len(plen)
    pf = sc.table(B, Tp, C) + 1.0                         # no zero entry: a kept frame is never 0
    out = canary(B * T, C, CAN32)
    call(lib0, SPEECH, B=B, T=T, S=Tp, C=C, x=f32(pf), lens=np.asarray(plen, np.int32), out=out)
    got, ref = interior(out, B * T, C, "speech condition"), kr.speech_cond_ref(pf, plen, T)
    assert np.array_equal(got, ref), f"{int((got != ref).any(1).sum())} frames differ"


def test_rejects_what_would_read_out_of_bounds(lib0):
    """The entry checks on the host what the kernels take on trust: a token outside the table, a token
    count that leaves no pad slot, a speaker code outside {-1, 0, 1}, per-row scales that do not cover n.
    Each is an error return before any launch."""
    from zipvoice_amd.engine import ZvSolveCheckArgs
    C = 5
    keep = dict(tab=f32(sc.table(1, 11, C)[0]), oh=canary(2, C, CAN16), out=canary(46, C, CAN32),
                emb=f32(sc.table(2, 8, C)), v=np.zeros(40, np.float32), gr=np.zeros(3, np.float32))
    bad = [
        dict(kind=EMBED, n=2, C=C, N=11, ld=C, tok=np.array([0, 11], np.int64), W=keep["tab"], oh=keep["oh"]),
        dict(kind=TEXT, B=2, T=23, S=8, C=C, x=keep["emb"], lens=np.array([8, 3], np.int32),
             lens2=np.array([23, 23], np.int32), out=keep["out"]),
        dict(kind=TEXT, B=2, T=23, S=8, C=C, x=keep["emb"], lens=np.array([0, 3], np.int32),
             lens2=np.array([23, 23], np.int32), out=keep["out"]),
        dict(kind=SPK, n=2, C=C, x=keep["tab"], spk=np.array([0, 2], np.int8), W=keep["tab"], out=keep["out"]),
        dict(kind=COMBINE, n=20, v=keep["v"], grows=keep["gr"], B=3, per_row=7, gmul=1.0, out=keep["out"]),
    ]
    for f in bad:
        a = ZvSolveCheckArgs()
        a.guard, a.form = GUARD, -1
        for k, v in f.items():
            setattr(a, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        assert lib0.zv_solve_check(ctypes.byref(a)) == 1, f
        assert b"zv_solve_check" in lib0.zv_last_error()
