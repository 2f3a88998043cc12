"""The ConvolutionModule's depthwise conv + SwooshR against a float64 reference of the same operation
(tests/kernel_ref.py dwconv_ref: plain loops over taps, zero padding per utterance), in both operand
libraries: the four kernels behind launch_dwconv (csrc/zv_elem.inc: generic, register-window, LDS,
pipelined LDS) through zv_dwconv_check, and the fused GLU + conv launch (csrc/zv_gemm256.inc
g256_epi_glu_dw) through zv_linear_check's ZV_LIN_GLU_DW.  tests/test_gpu_conv_fused.py compares the
fused launch with the unfused pair, which share the tap order, the padding convention and the zeroing
at utterance edges; here each is compared with the reference.

exact class    g in {-3..3}, w in {-4..4}/16, bias in {-8..8}/4: the pre-activation u is exact in fp32
               in any order (asserted by the reference), the only error is SwooshR's:
               tol_y = TRANS_FACTOR * err_swoosh_r(u).
general class  Gaussian g (rounded to the operand format), w, bias:
               tol_u = (ks + 2) 2^-23 (sum_t |g||w| + |bias|), tol_y = 0.92 tol_u + TRANS_FACTOR *
               err_swoosh_r_any(u) (kernel_ref.dwconv_inputs says how the inputs are placed so that the
               reference meets the ambiguity cap).
fused launch   the GLU value's tolerance as tests/test_gpu_linear_ref.py derives it, h = round16(g), an
               ambiguous h may be one ulp off: tol_u += sum_t |w_t| ulp16(h_t) over those.

Every 16-bit output that is not ambiguous under kernel_ref.check16 equals round16(reference) exactly;
an ambiguous one lies in check16's interval.  tests/test_kernel_ref.py asserts from the reference alone
that at most one output in ten of any case is ambiguous.  With more than one utterance the first and
last frame of each hold +-1000: a halo row taken from the neighbouring utterance, or an edge frame
repeated by a clamp, is off by hundreds.  Every output has guard rows and a row stride larger than
its width, canary-filled, which must come back intact."""
import ctypes
import os

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

CAN16, CAN8 = np.uint16(0x7FA5), np.uint8(0xA5)
GUARD = 2
GLU_DW = 9


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=request.param)


def _interior(buf, rows, width, can, what):
    """The (rows, width) output of a canary-guarded buffer; everything else must be untouched."""
    mask = np.ones(buf.shape, bool)
    mask[GUARD:GUARD + rows, :width] = False
    touched = int((buf[mask] != can).sum())
    assert touched == 0, f"{what}: {touched} elements outside the output were written"
    return buf[GUARD:GUARD + rows, :width]


def check_pair(hi, lo, ref, tol, fmt, what):
    """hi + lo is the kernel's fp32 value up to the lo half's own rounding (half an ulp of lo,
    |lo| <= half an ulp of hi), as tests/test_gpu_linear_ref.py judges Ch / Cl pairs."""
    lo_max = 0.5 * kr.ulp16(np.abs(ref) + tol, fmt)
    err = np.abs(hi + lo - ref)
    lim = tol + 0.5 * kr.ulp16(lo_max, fmt)
    assert (err <= lim).all(), f"{what}: max |hi + lo - ref| / allowed = {(err / lim).max():.3f}"


def run_dwconv(lib, fmt, env, g, w, bias, B, L, ks, split, ldin, q8):
    from zipvoice_amd.engine import ZvDwconvCheckArgs
    M, C = g.shape
    keep = [np.ascontiguousarray(x, np.float32) for x in (g, w, bias)]
    for k, src in zip(keep, (g, w, bias)):
        assert np.array_equal(k.astype(np.float64), src), "inputs must be fp32 values"
    a = ZvDwconvCheckArgs()
    a.B, a.L, a.C, a.ks, a.split, a.guard = B, L, C, ks, split, GUARD
    a.g, a.w, a.bias = (k.ctypes.data for k in keep)
    a.ldin = ldin
    a.ldout = C + 2 if C % 2 == 0 else C + 1                 # (an odd row stride with the odd width)
    Oh = np.full((M + 2 * GUARD, a.ldout), CAN16, np.uint16)
    Ol = np.full_like(Oh, CAN16) if split == 3 else None
    a.Oh, a.Ol = Oh.ctypes.data, None if Ol is None else Ol.ctypes.data
    q = qs = None
    if q8:
        a.ldq = C + 128
        q = np.full((M + 2 * GUARD, a.ldq), CAN8, np.uint8)
        qs = np.full((M + 2 * GUARD, a.ldq // 32), CAN8, np.uint8)
        a.q, a.qs = q.ctypes.data, qs.ctypes.data
    old = {k: os.environ.get(k) for k in ("ZV_DWCONV_PIPE", "ZV_DWCONV_LDS")}
    try:
        for k in old:
            os.environ.pop(k, None)
        os.environ.update(env)
        rc = lib.zv_dwconv_check(ctypes.byref(a))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert rc == 0, lib.zv_last_error().decode()
    out = {"Oh": kr.decode16(_interior(Oh, M, C, CAN16, "Oh"), fmt)}
    if Ol is not None:
        out["Ol"] = kr.decode16(_interior(Ol, M, C, CAN16, "Ol"), fmt)
    if q8:
        out["q"] = _interior(q, M, C, CAN8, "q")
        out["qs"] = _interior(qs, M, C // 32, CAN8, "qs")
    return out, list(a.launch), a.num_cus


def judge(got, y, tol_y, u, fmt, tag, got_lo=None, extra_amb=None):
    """check16 on the 16-bit output (tolerance 0 outside the ambiguous elements), the ambiguity cap,
    and the hi + lo pair where there is one.  Returns a line of figures."""
    assert np.isfinite(got).all(), tag
    bad, amb, r, multi = kr.check16(got, y, tol_y, fmt)
    if extra_amb is not None:
        amb = amb | extra_amb
    _, m = kr.amb16(y, tol_y, fmt)
    share = kr.assert_amb_cap(amb, m, u, tol_y, fmt, tag)
    off = np.abs(got - kr.round16(y, fmt))[bad]
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} values outside check16's interval " \
        f"(max |got - round16(ref)| = {off.max():.4g}, first at {np.argwhere(bad)[:4].tolist()})"
    exact = ~amb
    assert np.array_equal(got[exact], kr.round16(y, fmt)[exact]), f"{tag}: a non-ambiguous output is not round16(ref)"
    if got_lo is not None:
        check_pair(got, got_lo, y, tol_y, fmt, tag + " hi + lo")
    return f"{100 * share:.2f} % ambiguous ({multi} multi-ulp), max |err| / interval = {r:.3f}"


@pytest.mark.parametrize("case", kr.dwconv_cases(), ids=kr.dwconv_case_id)
def test_dwconv(lib, case):
    fmt, Lb = lib
    arm, ks, B, L, C, pad, split, q8 = case
    lines = []
    for klass in ("exact", "general"):
        g, w, bias = kr.dwconv_inputs(B, L, C, ks, fmt, klass, split)
        y, u, mag = kr.dwconv_ref(g, w, bias, B, L)
        if klass == "exact":
            kr.dwconv_exact_u(g, w, bias, u, mag)
        _, tol_y = kr.dwconv_tol(u, mag, ks, klass)
        out, rec, cus = run_dwconv(Lb, fmt, kr.DW_ENV[arm], g, w, bias, B, L, ks, split, C + pad, q8)
        assert rec == kr.dwconv_predict(case, cus), (rec, kr.dwconv_predict(case, cus), cus)
        tag = f"{fmt} {kr.dwconv_case_id(case)} {klass}"
        lines.append(judge(out["Oh"], y, tol_y, u, fmt, tag, out.get("Ol")))
        if q8:                                          # the fp8 copy == packing the returned 16-bit output
            from oracle import mx8_np
            rq, rs = mx8_np.quantize(out["Oh"].astype(np.float32), C)
            assert np.array_equal(out["qs"], rs), f"{tag}: fp8 scales"
            assert np.array_equal(out["q"], rq), f"{tag}: fp8 codes"
    print(f"{fmt} {kr.dwconv_case_id(case)}: launch {rec}; " + "; ".join(lines))


def test_dwconv_dispatch_coverage(lib):
    """The case list reaches every kernel and kernel-size instantiation launch_dwconv can choose, and
    the pipe kernel with whole, partial and single-tile chunks (each case asserts that the launch
    record equals this prediction)."""
    fmt, Lb = lib
    g, w, bias = kr.dwconv_inputs(1, 1, 6, 5, fmt, "exact")
    _, _, cus = run_dwconv(Lb, fmt, {}, g, w, bias, 1, 1, 5, 1, 6, False)
    seen = {tuple(kr.dwconv_predict(c, cus)[:4]) for c in kr.dwconv_cases()}
    want = {(3, k, 1, 0) for k in (7, 9, 15, 31)} | {(2, k, 1, 0) for k in (7, 9, 15)}
    want |= {(1, k, s, q) for k in (7, 9, 15, 31) for s, q in ((1, 0), (3, 0), (1, 1))}
    want |= {(0, 5, 1, 0), (0, 5, 3, 0), (0, 63, 1, 0), (0, 63, 3, 0), (0, 7, 1, 0)}
    assert len(want) == 24
    assert want <= seen, f"not reached: {sorted(want - seen)}"
    chunks = {(c[1], tuple(kr.dwconv_predict(c, cus)[4:])) for c in kr.dwconv_cases() if c[3] == 327 and c[0].startswith("pipe")
              and c[1] != 5 and c[1] != 63}
    for ks in (7, 9, 15, 31):                           # 6 tiles: 3 x 2, 2 x 3, 5 + 1, and the automatic chunk
        assert {(ks, (2, 3, 3, 2)), (ks, (2, 2, 3, 3)), (ks, (2, 2, 3, 5))} <= chunks, (ks, sorted(chunks))
    print(f"{fmt}: {cus} CUs, {len(want)} instantiations reached by {len(kr.dwconv_cases())} cases")


# --------------------------------------------------------------------------- fused GLU + conv
def run_glu_dw(lib, fmt, A, W, bias, mask, w, b, B, L):
    from zipvoice_amd.engine import ZvLinearCheckArgs
    M, K = A.shape
    N, C, ks = W.shape[0], w.shape[0], w.shape[1]
    keep = [np.ascontiguousarray(x, np.float32) for x in (A, W, bias, w, b)] + [np.ascontiguousarray(mask, np.uint8)]
    for k, src in zip(keep[:5], (A, W, bias, w, b)):
        assert np.array_equal(k.astype(np.float64), src), "inputs must be fp32 values"
    a = ZvLinearCheckArgs()
    a.M, a.N, a.K, a.split, a.form, a.act = M, N, K, 1, GLU_DW, 0
    a.rows_per_group, a.rpb, a.guard = 1, L, GUARD
    for name, arr in zip(("A", "W", "bias", "dw_w", "dw_b", "rowmask"), keep):
        setattr(a, name, arr.ctypes.data)
    a.dw_ks, a.dw_L = ks, L
    a.ldc, a.ldch = N + 4, C + 8
    Ch = np.full((M + 2 * GUARD, a.ldch), CAN16, np.uint16)
    a.Ch = Ch.ctypes.data
    rc = lib.zv_linear_check(ctypes.byref(a))
    assert rc == 0, lib.zv_last_error().decode()
    return kr.decode16(_interior(Ch, M, C, CAN16, "Ch"), fmt), list(a.launch)


@pytest.mark.parametrize("ks", [7, 15, 31])
@pytest.mark.parametrize("shape", kr.GLU_DW_SHAPES, ids=lambda s: f"B{s[0]}xL{s[1]}")
def test_glu_dwconv_fused(lib, shape, ks):
    """(1, 1); utterances shorter than the halo; a 16-frame chunk spanning several utterances; a tile
    boundary inside an utterance and an utterance boundary inside a tile; M = MSTEP and MSTEP + 1 for
    the three kernel sizes (226 / 242 / 250 rows per tile); two tiles with the tail of the second
    utterance masked: masked rows are zero before the conv and still give SwooshR(bias + their
    neighbours' taps) outputs."""
    fmt, Lb = lib
    B, L = shape
    masked = shape == kr.GLU_DW_MASKED
    lines = []
    for klass in ("exact", "general"):
        A, W, bias, mask, w, b = kr.glu_dw_inputs(B, L, ks, fmt, klass, masked)
        y, tol_y, u, amb, _ = kr.glu_dw_ref(A, W, bias, mask, w, b, B, L, fmt, klass)
        got, rec = run_glu_dw(Lb, fmt, A, W, bias, mask, w, b, B, L)
        assert rec[:6] == [256, 256, 1, 3, 3, 1], rec                   # the 256x256 kernel, GLU, counted
        tiles = 4 * -(-B * L // (256 - 2 * (ks // 2)))
        assert rec[6] == max(8, -(-tiles // 8) * 8), (rec, tiles)
        tag = f"{fmt} fused k{ks} B{B} L{L} {klass}"
        lines.append(judge(got, y, tol_y, u, fmt, tag, extra_amb=amb))
        if masked:                                                      # rows past the halo of the last kept frame
            far = np.arange(B * L) >= B * L - 37 + ks // 2
            ref = kr.swoosh_r(np.broadcast_to(b, (int(far.sum()), b.size)))
            bad = kr.check16(got[far], ref, kr.TRANS_FACTOR * kr.err_swoosh_r_any(ref * 0 + b), fmt)[0]
            assert not bad.any(), f"{tag}: masked rows are not SwooshR(bias)"
    print(f"{fmt} fused k{ks} B{B} L{L}: launch {rec}; " + "; ".join(lines))


def test_glu_dwconv_fused_rejects_what_the_engine_would_not_fuse(lib):
    """The check launches the fused kernel only under the engine's own conditions: a kernel size
    without an instantiation, or rows that are no whole utterances, are errors with a message, not
    a quiet unfused pair."""
    fmt, Lb = lib
    A, W, bias, mask, w, b = kr.glu_dw_inputs(2, 5, 7, fmt, "exact", False)
    for ks, L, reason in ((9, 5, "kernel size 7, 15 or 31"), (7, 3, "whole utterances")):
        with pytest.raises(AssertionError, match=reason):
            run_glu_dw(Lb, fmt, A, W, bias, mask, np.zeros((512, ks)), b, 2, L)
