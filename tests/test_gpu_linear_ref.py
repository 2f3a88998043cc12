"""The engine's linears (csrc/zv_gemm.inc, zv_gemm256.inc) against a float64 reference of the same
operation, launched through the engine's own dispatch (zv_linear_check: linear16<1>, linear16<3>,
attn_in_wsplit and the fused TRANS / NA / GLU launch choices of zv_engine::layer), in both operand
libraries.  tests/kernel_ref.py holds the reference and the derivation of the bounds:

exact class    small dyadic operands for which every product, partial sum (in any order) and
               epilogue step is exact in fp32 (asserted by the reference itself): the fp32 output
               equals float64 bit for bit and the 16-bit copy is its round-to-nearest-even;
               tolerance 0.  Split products: one operand carries p + 3 significant bits (a non-zero,
               exact lo half), the other is exact in hi alone, both assignments.
general class  Gaussian operands; |err| <= (K + 8) 2^-23 sum_k |a_k||w_k| (fp32 accumulation in any
               order, factor 2 over the unit roundoff for the MFMA's internal accumulation),
               + 2^-16 sum_k |a_k||w_k| for the split products (dropped lo lo term, the lo halves'
               rounding), + 2^-24 per epilogue operation on the magnitude of its operands,
               + half a 16-bit ulp at the reference value for a 16-bit output.
transcendental 4x the error of the same formula in fp32 numpy (v_exp_f32 / v_log_f32 / v_rcp_f32
               are 1-ulp instructions); a 16-bit output may be one ulp off only where that
               tolerance straddles a rounding boundary (kernel_ref.check16).

Every output buffer has a row stride larger than its width and guard rows on both sides, filled
with a canary bit pattern that must come back intact (the counted epilogues store unconditionally
and send what is outside the output to a sink).  The launch record tells which instantiation the
dispatch chose; each case asserts the one predicted from the reported CU count, and
test_dispatch_coverage that the case list reaches every instantiation linear16 can choose."""
import ctypes
import zlib

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

PLAIN, PLAIN_F32, RESID, RESID_BYP, RESID_RV, RV_COPY, TRANS, NA, GLU = range(9)
FORM_NAME = ["plain", "plain_f32", "resid", "resid_byp", "resid_rv", "rv_copy", "trans", "na", "glu"]
CAN32, CAN16 = np.uint32(0x7FC5A5A5), np.uint16(0x7FA5)     # NaN patterns in fp32 / bf16 / fp16
GUARD = 2
OPERAND = {"bf16": "bf16", "f16": "f16"}


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=OPERAND[request.param])


def _buf32(rows, ld):
    return np.full((rows + 2 * GUARD, ld), CAN32, np.uint32)


def _buf16(rows, ld):
    return np.full((rows + 2 * GUARD, ld), CAN16, np.uint16)


def _interior(buf, rows, width, can, what):
    """The (rows, width) output of a canary-guarded buffer; everything else must be untouched."""
    mask = np.ones(buf.shape, bool)
    mask[GUARD:GUARD + rows, :width] = False
    touched = int((buf[mask] != can).sum())
    assert touched == 0, f"{what}: {touched} elements outside the output were written"
    return buf[GUARD:GUARD + rows, :width]


def run_linear(lib, fmt, form, split, A, W, bias, act=0, resid=None, orig=None, byp=None, rowvec=None,
               rpg=1, rpb=0, rowmask=None, with_copy=True):
    """One zv_linear_check call.  Returns (outputs dict of float64 arrays, launch record)."""
    from zipvoice_amd.engine import ZvLinearCheckArgs
    M, K = A.shape
    N = W.shape[0]
    f32 = lambda x: None if x is None else np.ascontiguousarray(x, np.float32)
    keep = [f32(A), f32(W), f32(bias), f32(resid), f32(orig), f32(byp), f32(rowvec),
            None if rowmask is None else np.ascontiguousarray(rowmask, np.uint8)]
    for k, src in zip(keep[:7], (A, W, bias, resid, orig, byp, rowvec)):
        assert k is None or np.array_equal(k.astype(np.float64), src), "inputs must be fp32 values"
    a = ZvLinearCheckArgs()
    a.M, a.N, a.K, a.split, a.form, a.act = M, N, K, split, form, act
    a.rows_per_group, a.rpb, a.guard = rpg, rpb, GUARD
    for name, arr in zip(("A", "W", "bias", "resid", "orig", "byp", "rowvec", "rowmask"), keep):
        setattr(a, name, None if arr is None else arr.ctypes.data)
    wch = N // 3 if form == NA else N // 2 if form == GLU else N
    C = Ch = Cl = Cth = Ctl = None
    a.ldc = cdiv(N, 4) * 4 + 4
    a.ldch = cdiv(wch, 8) * 8 + 8
    if form in (PLAIN_F32, RESID, RESID_BYP, RESID_RV):
        C = _buf32(M, a.ldc)
    if form in (PLAIN, RV_COPY, NA, GLU) or (form in (RESID, RESID_BYP, RESID_RV) and with_copy):
        Ch = _buf16(M, a.ldch)
        Cl = _buf16(M, a.ldch) if split == 3 else None
    if form in (TRANS, NA):
        nt = (N // 3 if form == NA else N) * cdiv(M, rpb)
        a.ldct = cdiv(rpb, 8) * 8 + 8
        Cth = _buf16(nt, a.ldct)
        Ctl = _buf16(nt, a.ldct) if split == 3 else None
    for name, arr in (("C", C), ("Ch", Ch), ("Cl", Cl), ("Cth", Cth), ("Ctl", Ctl)):
        setattr(a, name, None if arr is None else arr.ctypes.data)
    rc = lib.zv_linear_check(ctypes.byref(a))
    assert rc == 0, lib.zv_last_error().decode()
    out = {}
    tag = f"{FORM_NAME[form]} {M}x{N}x{K} split {split}"
    if C is not None:
        out["C"] = _interior(C, M, N, CAN32, tag + " C").view(np.float32).astype(np.float64)
    if Ch is not None:
        out["Ch"] = kr.decode16(_interior(Ch, M, wch, CAN16, tag + " Ch"), fmt)
    if Cl is not None:
        out["Cl"] = kr.decode16(_interior(Cl, M, wch, CAN16, tag + " Cl"), fmt)
    for name, buf in (("Cth", Cth), ("Ctl", Ctl)):
        if buf is None:
            continue
        B, rows_t = cdiv(M, rpb), (N // 3 if form == NA else N)
        inner = buf[GUARD:GUARD + B * rows_t].reshape(B, rows_t, a.ldct)
        assert (buf[:GUARD] == CAN16).all() and (buf[GUARD + B * rows_t:] == CAN16).all(), tag + " guard rows"
        out[name] = (inner, a.ldct)
    rec = tuple(a.launch)
    return out, rec, a.num_cus


# --------------------------------------------------------------------------- inputs
def exact_inputs(rng, M, N, K, fmt, wide):
    """Exact-class operands.  wide None: A in {-3..3}, W in {-4..4}/64 (exact in hi alone).
    wide "A" / "W": that operand's non-zero entries are odd p + 3-bit significands in [1, 2)
    (/ 64 for W), thinned so that sum |products| stays below 2^20 lsb units (headroom for the
    epilogue's additions and the bypass scale's two extra bits)."""
    p = kr.PREC[fmt]
    A = rng.integers(-3, 4, (M, K)).astype(np.float64)
    W = rng.integers(-4, 5, (N, K)) / 64.0
    if wide:
        other = 4 if wide == "A" else 3
        d = min(1.0, 2.0 ** 20 / (K * 2.0 ** (p + 3) * other))
        shape = (M, K) if wide == "A" else (N, K)
        m = (2 * rng.integers(2 ** (p + 1), 2 ** (p + 2), shape) + 1) * rng.choice([-1.0, 1.0], shape)
        v = m * 2.0 ** -(p + 2) * (rng.random(shape) < d)
        if wide == "A":
            A = v
        else:
            W = v / 64.0
    return A, W


def exact_epilogue_inputs(rng, M, N, rpg):
    return dict(bias=rng.integers(-16, 17, N) / 8.0, resid=rng.integers(-256, 257, (M, N)) / 64.0,
                orig=rng.integers(-256, 257, (M, N)) / 64.0, byp=rng.choice([0.0, 0.25, 0.5, 1.0], N),
                rowvec=rng.integers(-128, 129, (cdiv(M, rpg), N)) / 64.0)


def general_inputs(rng, M, N, K, fmt, split, rpg):
    f = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
    A, W = f(M, K), f(N, K) / np.sqrt(K)
    if split != 3:
        A = kr.round16(A, fmt)
    if split == 1:
        W = kr.round16(W, fmt)
    W = W.astype(np.float32).astype(np.float64)
    return A, W, dict(bias=f(N), resid=f(M, N), orig=f(M, N), byp=rng.random(N).astype(np.float32).astype(np.float64),
                      rowvec=f(cdiv(M, rpg), N))


def form_kwargs(form, e):
    kw = {}
    if form in (RESID, RESID_BYP, RESID_RV, RV_COPY):
        kw["resid"] = e["resid"]
    if form == RESID_BYP:
        kw.update(orig=e["orig"], byp=e["byp"])
    if form in (RESID_RV, RV_COPY):
        kw["rowvec"] = e["rowvec"]
    return kw


# --------------------------------------------------------------------------- dispatch mirror
def predict(M, N, split, form, act, cus, with_copy=True):
    """The instantiation zv_engine::linear16 / attn_in_wsplit chooses: (BM, BN, SPLIT, ROLE, 256x256,
    STAGES * 16 + OCC), from the CU count the library reports."""
    t = cdiv(M, 128) * cdiv(N, 128)
    if split == 2:
        return (128, 64, 2, 3, 0, 34)
    if N <= 64:
        return (128, 64, split, 0, 0, 34)
    if form in (RESID, RESID_BYP, RESID_RV, RV_COPY):
        if form == RV_COPY and split != 1:
            return (128, 128, split, 0, 0, 34)
        role = {RESID: 1, RESID_BYP: 2, RESID_RV: 4, RV_COPY: 5}[form]
        if split == 1 and t < cus // 2:
            return (64, 64, 1, role, 0, 66)
        if split == 1 and t < cus * 3 // 2:
            return (128, 64, 1, role, 0, 35)
        return (128, 128, split, role, 0, 34)
    counted = form == PLAIN
    if cdiv(N, 96) * 96 < cdiv(N, 128) * 128:
        if counted and not act:
            return (128, 64, 1, 3, 0, 35) if split == 1 else (128, 128, split, 3, 0, 34)
        return (128, 96, split, 0, 0, 34)
    if not counted:
        return (128, 128, split, 0, 0, 34)
    if split == 1 and cdiv(M, 256) * cdiv(N, 256) >= 256:
        return (256, 256, 1, 3, 1, 0)
    if split == 1 and t < cus * 3 // 2:
        return (128, 64, 1, 3, 0, 35)
    return (128, 128, split, 3, 0, 34)


def rec_key(rec):
    return (rec[0], rec[1], rec[2], rec[4], rec[5], rec[7])


# --------------------------------------------------------------------------- the case list
SMALL = [(1, 8, 48), (63, 48, 64), (65, 64, 300), (127, 72, 512), (129, 200, 560), (257, 272, 1920),
         (517, 512, 64), (517, 520, 300), (129, 512, 1920), (65, 272, 48)]
SMALL_SPLIT = [(63, 48, 64), (129, 200, 560), (257, 272, 300), (65, 520, 512), (127, 72, 1920)]
# tile regimes on 256 CUs: 64x64, 128x64 and 128x128 residual tiles; the 256x256 kernel with ragged
# M and (N = 1528) ragged N.  N = 520 takes the 96-wide-tile branch of linear16 at every size (576
# computed columns against 640): the 256x256 kernel is not reachable there
REGIMES = [(517, 512, 64), (4100, 512, 64), (12300, 512, 64), (10760, 1536, 64), (21765, 520, 64),
           (10760, 1528, 64)]
STD_FORMS = [(PLAIN, 0), (PLAIN, 1), (PLAIN_F32, 0), (RESID, 0), (RESID_BYP, 0), (RESID_RV, 0), (RV_COPY, 0)]
# residual forms without the 16-bit copy (the !Ch arm of the counted residual epilogue): these shapes
NOCOPY = [(129, 200, 560), (517, 512, 64), (4100, 512, 64), (12300, 512, 64)]


def std_cases():
    """(split, form, act, M, N, K, copy): copy False = a residual form without its 16-bit copy."""
    cases = []
    for M, N, K in SMALL + [r for r in REGIMES if r not in SMALL]:
        for form, act in STD_FORMS:
            if (M, N, K) in REGIMES[3:] and form not in (PLAIN, RESID):
                continue                           # the large launches: the plain forms and one residual
            cases.append((1, form, act, M, N, K, True))
            if (M, N, K) in NOCOPY and form in (RESID, RESID_BYP, RESID_RV):
                cases.append((1, form, act, M, N, K, False))
    for M, N, K in SMALL_SPLIT:
        for form, act in STD_FORMS:
            if form != RV_COPY:                    # the copy-only form exists in the 16-bit mode only
                cases.append((3, form, act, M, N, K, True))
            if (M, N, K) in NOCOPY and form in (RESID, RESID_BYP, RESID_RV):
                cases.append((3, form, act, M, N, K, False))
        cases.append((2, PLAIN, 0, M, N, K, True))
    return cases


def pick_rpg(M, i):
    for k in range(3):
        r = (7, 203, 1)[(i + k) % 3]
        if r == 1 or M % r:
            return r


def case_id(c):
    split, form, act, M, N, K, copy = c
    return f"s{split}-{FORM_NAME[form]}{'-swoosh' if act else ''}{'' if copy else '-nocopy'}-{M}x{N}x{K}"


def check_fp32(got, ref, tol, what):
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(tol, 1e-300)).max()) if np.any(tol > 0) else float(err.max() > 0)
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), f"{what}: max |err| / tol = {ratio:.3f}, {int((err > tol).sum())} outside"
    return ratio


def check_16(got, ref, tol, fmt, what):
    """General class: |got - ref| <= tol + half a 16-bit ulp at the reference value."""
    return check_fp32(got, ref, tol + 0.5 * kr.ulp16(np.abs(ref) + tol, fmt), what)


def check_pair(hi, lo, ref, tol, fmt, what):
    """A hi / lo pair whose value is not known exactly: hi + lo is the kernel's fp32 value up to the
    lo half's own rounding: half an ulp of lo, |lo| <= half an ulp of hi (the ulp of a subnormal lo
    is the format's smallest)."""
    lo_max = 0.5 * kr.ulp16(np.abs(ref) + tol, fmt)
    return check_fp32(hi + lo, ref, tol + 0.5 * kr.ulp16(lo_max, fmt), what)


def exact_lo(ref, fmt):
    """The lo half of an exactly known fp32 value."""
    return kr.round16((ref - kr.round16(ref, fmt)).astype(np.float32).astype(np.float64), fmt)


@pytest.mark.parametrize("klass", ["exact", "general"])
@pytest.mark.parametrize("case", std_cases(), ids=case_id)
def test_std_forms(lib, case, klass):
    fmt, L = lib
    split, form, act, M, N, K, copy = case
    rng = np.random.default_rng(zlib.crc32(repr((case, klass)).encode()))
    rpg = pick_rpg(M, M + N + K)
    wides = [None] if split == 1 else ["W"] if split == 2 else ["A", "W"]
    ratios = []
    for wide in (wides if klass == "exact" else [None]):
        if klass == "exact":
            A, W = exact_inputs(rng, M, N, K, fmt, wide)
            e = exact_epilogue_inputs(rng, M, N, rpg)
        else:
            A, W, e = general_inputs(rng, M, N, K, fmt, split, rpg)
        kw = form_kwargs(form, e)
        out, rec, cus = run_linear(L, fmt, form, split, A, W, e["bias"], act=act, rpg=rpg, with_copy=copy, **kw)
        assert rec_key(rec) == predict(M, N, split, form, act, cus), (rec, cus)
        assert copy or ("Ch" not in out and "Cl" not in out)
        As, Ws = kr.operands(A, W, split, fmt)
        rkw = dict(kw, rows_per_group=rpg) if "rowvec" in kw else kw
        if klass == "exact":
            # the operands are exactly representable, one side in hi alone: nothing is dropped
            assert np.array_equal(sum(As), A) and np.array_equal(sum(Ws), W)
            assert len(As) == 1 or len(Ws) == 1 or not As[1].any() or not Ws[1].any()
            if wide:
                assert (As[1] if wide == "A" else Ws[1]).any()
            acc = kr.assert_exact_dot(As, Ws)
            pre, _, _ = kr.std_epilogue(acc, e["bias"], exact=True, **rkw)
            tol = np.zeros_like(pre)
        else:
            acc = A @ W.T
            pre, mag, nops = kr.std_epilogue(acc, e["bias"], **rkw)
            tol = kr.dot_tol(A, W, split) + nops * kr.U32 * mag
        if act:                                        # SwooshL: |d/dx| < 1, + the formula's own error
            ref, tol = kr.swoosh_l(pre), tol + kr.tol_swoosh_l(pre) + kr.U32 * np.abs(kr.swoosh_l(pre))
        else:
            ref = pre
        tag = f"{fmt} {case_id(case)} {klass} wide={wide}"
        if "C" in out:
            if klass == "exact" and not act:
                assert np.array_equal(out["C"], ref), f"{tag}: fp32 output differs from float64 " \
                    f"({int((out['C'] != ref).sum())} elements, max {np.abs(out['C'] - ref).max():.3e})"
                ratios.append(0.0)
            else:
                ratios.append(check_fp32(out["C"], ref, tol, tag + " C"))
        if "Ch" in out:
            if klass == "exact" and not act:
                assert np.array_equal(out["Ch"], kr.round16(ref, fmt)), \
                    f"{tag}: 16-bit copy is not round16 of the exact value"
                if "Cl" in out:
                    assert np.array_equal(out["Cl"], exact_lo(ref, fmt)), f"{tag}: lo half"
                ratios.append(0.0)
            elif klass == "exact":
                bad, amb, r, _ = kr.check16(out["Ch"], ref, tol, fmt)
                assert not bad.any(), f"{tag}: {int(bad.sum())} 16-bit values off ({int(amb.sum())} ambiguous)"
                ratios.append(r)
                if "Cl" in out:
                    check_pair(out["Ch"], out["Cl"], ref, tol, fmt, tag + " Ch + Cl")
            else:
                ratios.append(check_16(out["Ch"], ref, tol, fmt, tag + " Ch"))
                if "Cl" in out:
                    check_pair(out["Ch"], out["Cl"], ref, tol, fmt, tag + " Ch + Cl")
    print(f"{fmt} {case_id(case)} {klass}: launch {rec}, max |err| / tol = {max(ratios):.3f}")


def test_dispatch_coverage(lib):
    """Every instantiation linear16 / launch_resid / attn_in_wsplit can choose is reached by the
    case list (each case asserts that the launch record equals this prediction)."""
    fmt, L = lib
    A, W = np.ones((1, 64)), np.ones((8, 64))
    _, _, cus = run_linear(L, fmt, PLAIN, 1, A, W, np.zeros(8))
    seen = {predict(c[3], c[4], c[0], c[1], c[2], cus) for c in std_cases()}
    want = {(128, 64, 1, 0, 0, 34), (128, 64, 3, 0, 0, 34), (128, 64, 2, 3, 0, 34),            # N <= 64, wsplit
            (128, 64, 1, 3, 0, 35), (128, 128, 3, 3, 0, 34),                                    # 96-wide branch
            (128, 96, 1, 0, 0, 34), (128, 96, 3, 0, 0, 34),
            (128, 128, 1, 0, 0, 34), (128, 128, 3, 0, 0, 34),                                   # general epilogue
            (256, 256, 1, 3, 1, 0), (128, 128, 1, 3, 0, 34)}                                    # plain counted
    for role in (1, 2, 4, 5):
        want |= {(64, 64, 1, role, 0, 66), (128, 64, 1, role, 0, 35), (128, 128, 1, role, 0, 34)}
    for role in (1, 2, 4):
        want.add((128, 128, 3, role, 0, 34))
    assert len(want) == 26
    missing = want - seen
    print(f"{fmt}: {cus} CUs, {len(want)} instantiations required, {len(seen)} reached by {len(std_cases())} cases")
    assert not missing, f"with {cus} CUs the case list does not reach {sorted(missing)}"


# --------------------------------------------------------------------------- fused epilogues
UTT = [(2, 33), (3, 97), (2, 203)]
# (form, split, B, L, N, wide): wide = which operand carries the non-zero lo half in the exact class
FUSED = ([(TRANS, 1, B, L, N, None) for (B, L), N in zip(UTT, (48, 64, 48))] +
         [(TRANS, 2, 3, 97, 64, "W"), (TRANS, 3, 2, 33, 48, "W"), (TRANS, 3, 3, 97, 64, "A")] +
         [(NA, 1, B, L, N, None) for (B, L), N in zip(UTT, (144, 1152, 144))] +
         [(NA, 3, 2, 33, 144, "W"), (NA, 3, 3, 97, 144, "A")] +
         [(GLU, 1, B, L, 1024, None) for B, L in UTT] +
         [(GLU, 3, 2, 33, 1024, "W"), (GLU, 3, 3, 97, 1024, "A")])


@pytest.mark.parametrize("klass", ["exact", "general"])
@pytest.mark.parametrize("case", FUSED,
                         ids=lambda c: f"{FORM_NAME[c[0]]}-s{c[1]}-B{c[2]}xL{c[3]}-N{c[4]}-wide{c[5]}")
def test_fused_epilogues(lib, case, klass):
    """TRANS / NA / GLU against the reference model's semantics (chunk(3): s, x, y with x * tanh(s);
    chunk(2): x * sigmoid(s), zero on masked rows), utterances of L rows so that tiles are cut at
    utterance boundaries; K = 512.  Split 3: the lo outputs are compared too, and the exact class
    runs with the non-zero lo half on either operand."""
    fmt, Lb = lib
    form, split, B, L, N, wide = case
    M, K = B * L, 512
    rng = np.random.default_rng(zlib.crc32(repr((case, klass)).encode()))
    if klass == "exact":
        A, W = exact_inputs(rng, M, N, K, fmt, wide)
        bias = rng.integers(-16, 17, N) / 8.0
    else:
        A, W, e = general_inputs(rng, M, N, K, fmt, split, 1)
        bias = e["bias"]
    mask = None
    if form == GLU:                                    # padded rows: the tail of every utterance but the first
        mask = (np.arange(M) % L >= L - 5) & (np.arange(M) >= L)
    out, rec, cus = run_linear(Lb, fmt, form, split, A, W, bias, rpb=L, rowmask=mask)
    As, Ws = kr.operands(A, W, split, fmt)
    if klass == "exact":
        assert np.array_equal(sum(As), A) and np.array_equal(sum(Ws), W)
        if wide:
            assert (As[1] if wide == "A" else Ws[1]).any()
        pre = kr.assert_fp32_exact(kr.assert_exact_dot(As, Ws) + bias)
        tp = np.zeros_like(pre)
    else:
        pre = A @ W.T + bias
        tp = kr.dot_tol(A, W, split) + kr.U32 * (np.abs(A) @ np.abs(W).T + np.abs(bias))
    tag = f"{fmt} {FORM_NAME[form]} split {split} B={B} L={L} N={N} wide={wide} {klass}"
    ratios = []

    def check(got, ref, tol, what, got_lo=None):
        assert (got_lo is not None) == (split == 3), f"{tag} {what}: lo output"
        if klass == "exact" and not np.any(tol):
            assert np.array_equal(got, kr.round16(ref, fmt)), f"{tag} {what}: not round16 of the exact value"
            if got_lo is not None:
                assert np.array_equal(got_lo, exact_lo(ref, fmt)), f"{tag} {what}: lo half"
            ratios.append(0.0)
            return
        if klass == "exact":
            bad, amb, r, _ = kr.check16(got, ref, tol, fmt)
            assert not bad.any(), f"{tag} {what}: {int(bad.sum())} values off ({int(amb.sum())} ambiguous)"
            ratios.append(r)
        else:
            ratios.append(check_16(got, ref, tol, fmt, f"{tag} {what}"))
        if got_lo is not None:
            check_pair(got, got_lo, ref, tol, fmt, f"{tag} {what} hi + lo")

    def untranspose(name, width):
        if name not in out:
            return None
        buf, ldct = out[name]
        vals = kr.decode16(buf.reshape(-1), fmt).reshape(B, width, ldct)
        assert (buf[:, :, L:] == CAN16).all(), f"{tag}: {name} written past the utterance's frames"
        return vals[:, :, :L].transpose(0, 2, 1).reshape(M, width)

    if form == TRANS:
        check(untranspose("Cth", N), pre, tp, "Cth", untranspose("Ctl", N))
    elif form == NA:
        hid = N // 3
        xs, y = kr.na_ref(pre, hid)
        s, x = pre[:, :hid], pre[:, hid:2 * hid]
        # d(x tanh s) <= |tanh s| dx + |x| (ds + the tanh formula's error) + the product's rounding
        txs = (np.abs(np.tanh(s)) * tp[:, hid:2 * hid] + np.abs(x) * (tp[:, :hid] + kr.TRANS_FACTOR * kr.ERR_TANH) +
               kr.U32 * np.abs(xs))
        check(untranspose("Cth", hid), xs, txs, "x * tanh(s)", untranspose("Ctl", hid))
        check(out["Ch"], y, tp[:, 2 * hid:], "y", out.get("Cl"))
    else:
        C = N // 2
        g = kr.glu_ref(pre, C, mask)
        x, s = pre[:, :C], pre[:, C:]
        tg = (kr.sigmoid(s) * tp[:, :C] + np.abs(x) * (0.25 * tp[:, C:] + kr.TRANS_FACTOR * kr.ERR_SIGMOID) +
              kr.U32 * np.abs(g))
        tg = np.where(mask[:, None], 0.0, tg)
        check(out["Ch"], g, tg, "x * sigmoid(s)", out.get("Cl"))
        assert (out["Ch"][mask] == 0).all(), f"{tag}: masked rows are not zero"
        if "Cl" in out:
            assert (out["Cl"][mask] == 0).all(), f"{tag}: masked rows' lo half is not zero"
    print(f"{tag}: launch {rec}, max |err| / allowed = {max(ratios):.3f}")


# --------------------------------------------------------------------------- activation sweep
@pytest.mark.parametrize("N", [64, 128])
def test_swoosh_l_sweep(lib, N):
    """SwooshL through the production plain form (N = 128: the counted epilogue; 64: the general
    one): K = 64 with two non-zero columns a0 (integers) and a1 (multiples of 1/64) against unit
    weights, so the pre-activation covers [-120, 120] in steps of 1/64 exactly."""
    fmt, L = lib
    u = np.arange(-120 * 64, 120 * 64 + 1)
    A = np.zeros((u.size, 64))
    A[:, 0], A[:, 1] = np.floor(u / 64.0), (u % 64) / 64.0
    W = np.zeros((N, 64))
    W[:, :2] = 1.0
    out, rec, _ = run_linear(L, fmt, PLAIN, 1, A, W, np.zeros(N), act=1)
    pre = kr.assert_fp32_exact(kr.assert_exact_dot(kr.round16(A, fmt), W))
    assert np.array_equal(pre[:, 0], u / 64.0)
    ref = kr.swoosh_l(pre)
    assert np.isfinite(out["Ch"]).all()
    bad, amb, r, multi = kr.check16(out["Ch"], ref, kr.tol_swoosh_l(pre), fmt)
    worst = pre[bad][:5]
    print(f"{fmt} SwooshL sweep N={N}: launch {rec}, {int(amb.sum())} ambiguous of {amb.size} "
          f"({multi} of them multi-ulp, next to SwooshL's zero), max |err| / allowed = {r:.3f}")
    assert not bad.any(), f"{int(bad.sum())} values outside 4x the fp32 formula's error, first at x = {worst}"
