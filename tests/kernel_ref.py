"""Float64 references for the engine's linear and fused FeedForward kernels (csrc/zv_gemm.inc,
zv_gemm256.inc, zv_ffn.inc); a helper, not a test.  numpy only.

Number formats: the 16-bit operand format of a library is "bf16" (8 significant bits) or "f16"
(IEEE half, 11); round16 is round-to-nearest-even from float64, split16 the engine's hi / lo pair.

Two input classes (tests/test_gpu_linear_ref.py, test_gpu_ffn_ref.py):

exact    operands are small dyadic rationals, chosen so that every product, every partial sum in
         any order and every epilogue step without a transcendental is exactly representable in
         fp32.  assert_exact_dot proves it for a product: with qa, qw the operands' common lsbs,
         every partial sum is an integer multiple of qa qw of magnitude at most
         sum_k |a_k||w_k|, so it is exact in fp32 when that sum is below 2^24 qa qw.  The fp32 kernel
         output must then equal the float64 result bit for bit (tolerance 0), whatever the MFMA's
         internal order.
general  Gaussian operands; per element |err| <= (K + 8) 2^-23 sum_k |a_k||w_k|: fp32 accumulation
         of K products in any order is within K u sum|a||w| of the exact sum (u = 2^-24), and the
         bound carries a factor 2 over u for the MFMA's internal accumulation (whose intermediate
         rounding is not specified) and 8 further terms for the bias and the K padding.  The split
         products (hi hi + hi lo + lo hi) add 2^-16 sum|a||w|: the dropped lo lo term and the lo
         halves' own rounding are each at most 2^-18 relative per product in bf16, less in fp16.
"""
import numpy as np

PREC = {"bf16": 8, "f16": 11}
# frexp exponent of the smallest normal number (x = m 2^e, 0.5 <= |m| < 1)
EMIN = {"bf16": -125, "f16": -13}
U32 = 2.0 ** -24          # fp32 unit roundoff


def ulp16(x, fmt):
    """Spacing of the format's numbers at |x| (float64)."""
    _, e = np.frexp(np.asarray(x, np.float64))
    return np.exp2(np.maximum(e, EMIN[fmt]).astype(np.float64) - PREC[fmt])


def round16(x, fmt):
    """Round-to-nearest-even to bf16 / fp16, as float64 values (fp16 overflows to inf)."""
    x = np.asarray(x, np.float64)
    q = ulp16(x, fmt)
    r = np.rint(x / q) * q                     # np.rint rounds half to even
    if fmt == "f16":
        r = np.where(np.abs(r) > 65504.0, np.copysign(np.inf, r), r)
    return r


def split16(x, fmt):
    """The engine's operand pair: hi = round16(x), lo = round16(fp32(x - hi))."""
    x = np.asarray(x, np.float64)
    hi = round16(x, fmt)
    lo = round16((x - hi).astype(np.float32).astype(np.float64), fmt)
    return hi, lo


def decode16(u, fmt):
    """uint16 bit patterns of the format -> float64."""
    u = np.ascontiguousarray(u, np.uint16)
    if fmt == "f16":
        return u.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):            # (canary NaN patterns decode quietly)
        return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def assert_fp32_exact(x, what=""):
    """Every value survives a round trip through fp32."""
    x = np.asarray(x, np.float64)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x), f"{what}: not exact in fp32"
    return x


def _lsb(x):
    """Largest power of two q with x / q integral for every element (x dyadic)."""
    x = np.asarray(x, np.float64)
    nz = x[x != 0]
    if nz.size == 0:
        return 1.0
    m, e = np.frexp(nz)
    # trailing zero bits of the 53-bit significand
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    tz = np.zeros(mi.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        z = (mi & ((1 << s) - 1)) == 0
        tz += np.where(z, s, 0)
        mi = np.where(z, mi >> s, mi)
    return float(np.exp2((e - 53 + tz).min()))


def assert_exact_dot(A, W):
    """A (M, K) . W (N, K)^T is exact in fp32 in any summation order (see the module docstring).
    A, W: arrays or lists of arrays (the hi / lo halves of a split operand, which are summed as
    separate products).  Returns the float64 product."""
    As = A if isinstance(A, (list, tuple)) else [A]
    Ws = W if isinstance(W, (list, tuple)) else [W]
    qa = min(_lsb(a) for a in As)
    qw = min(_lsb(w) for w in Ws)
    absA = sum(np.abs(a) for a in As)
    absW = sum(np.abs(w) for w in Ws)
    units = (absA @ absW.T) / (qa * qw)
    assert units.max() < 2.0 ** 24, f"sum |products| = {units.max():.0f} lsb units >= 2^24"
    return sum(As) @ sum(Ws).T


# --------------------------------------------------------------------------- activations
def swoosh_l(x):
    """scaling.py SwooshL: log(1 + exp(x - 4)) - 0.08 x - 0.035."""
    x = np.asarray(x, np.float64)
    return np.logaddexp(0.0, x - 4.0) - 0.08 * x - 0.035


def swoosh_r(x):
    x = np.asarray(x, np.float64)
    return np.logaddexp(0.0, x - 1.0) - 0.08 * x - 0.313261687


def sigmoid(x):
    x = np.asarray(x, np.float64)
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


# The same formulas as the kernels write them (zv_common.h), evaluated in fp32 numpy: their error
# against float64 is the yardstick of the transcendental tolerances.
_F = np.float32
_LOG2E, _LN2 = _F(1.44269504088896341), _F(0.693147180559945309)


def swoosh_l_f32(x):
    x = np.asarray(x, _F)
    t = x * _LOG2E + _F(-5.77078016355585362)
    with np.errstate(over="ignore"):
        l = np.maximum(np.log2(_F(1) + np.exp2(np.minimum(t, _F(126)))), t)
    return l * _LN2 + (x * _F(-0.08) + _F(-0.035))


def swoosh_r_f32(x):
    x = np.asarray(x, _F)
    xo = x - _F(1)
    with np.errstate(over="ignore"):
        ls = np.log2(_F(1) + np.exp2(xo * _LOG2E)) * _LN2
    ls = np.where(xo > _F(80), xo, ls)
    return ls - _F(0.08) * x - _F(0.313261687)


def sigmoid_f32(x):
    x = np.asarray(x, _F)
    with np.errstate(over="ignore"):
        return _F(1) / (_F(1) + np.exp2(-x * _LOG2E))


def tanh_f32(x):
    x = np.asarray(x, _F)
    with np.errstate(over="ignore"):
        t = _F(1) - _F(2) / (np.exp2(_F(2) * x * _LOG2E) + _F(1))
    return np.where(np.abs(x) > _F(15), np.copysign(_F(1), x), t)


# Error of the fp32 formulas against float64 (measured; tests/test_kernel_ref.py recomputes them).
# The kernels' v_exp_f32 / v_log_f32 / v_rcp_f32 are 1-ulp instructions, not correctly rounded as
# numpy's: a kernel value may be TRANS_FACTOR times as far off.
TRANS_FACTOR = 4.0


def err_swoosh_l(x):
    return 2.2 * U32 * (np.abs(x) + 6.0)


def err_swoosh_r(x):
    return 1.9 * U32 * (np.abs(x) + 6.0)


ERR_TANH = 3.0 * U32
ERR_SIGMOID = 1.5 * U32


def tol_swoosh_l(x):
    return TRANS_FACTOR * err_swoosh_l(x)


def check16(got, ref, tol, fmt):
    """The 16-bit ambiguity rule: an element is ambiguous when round16(ref - tol) !=
    round16(ref + tol).  Every other element must equal round16(ref) exactly; an ambiguous one
    may differ from it by one 16-bit ulp, and must lie in [round16(ref - tol), round16(ref + tol)]
    (rounding is monotone).  Only where the tolerance is not below the format's ulp at the
    reference value -- next to a zero of the function, where the ulps are tiny and the tolerance
    is absolute -- the one-ulp limit cannot hold and the interval alone is required; those
    elements are counted separately.
    Returns (bad mask, ambiguous mask, max |got - round16(ref)| / (hi - lo) over the ambiguous,
    number of multi-ulp elements)."""
    ref = np.asarray(ref, np.float64)
    lo, hi = round16(ref - tol, fmt), round16(ref + tol, fmt)
    amb = lo != hi
    r = round16(ref, fmt)
    diff = np.abs(got - r)
    inside = (got >= lo) & (got <= hi)
    narrow = tol < ulp16(ref, fmt)
    one = np.where(amb, ulp16(np.maximum(np.abs(lo), np.abs(hi)), fmt), 0.0)
    bad = ~inside | (narrow & ~(diff <= one)) | ~np.isfinite(got)
    ratio = np.where(diff == 0, 0.0, diff / np.maximum(hi - lo, 1e-300))
    return bad, amb, float(ratio.max()) if ratio.size else 0.0, int((~narrow & amb).sum())


# --------------------------------------------------------------------------- linear
def operands(A, W, split, fmt):
    """The operand values the kernel multiplies: lists of float64 arrays per side.
    split 1: round16 of both; 3: hi / lo pairs of both (the lo lo product is dropped);
    2: round16(A) against the weight's hi / lo pair."""
    if split == 1:
        return [round16(A, fmt)], [round16(W, fmt)]
    wh, wl = split16(W, fmt)
    if split == 2:
        return [round16(A, fmt)], [wh, wl]
    ah, al = split16(A, fmt)
    return [ah, al], [wh, wl]


def dot_kernel(As, Ws):
    """What the split kernels sum, in float64: all pairs except lo lo."""
    acc = As[0] @ Ws[0].T
    if len(Ws) > 1:
        acc = acc + As[0] @ Ws[1].T
    if len(As) > 1:
        acc = acc + As[1] @ Ws[0].T
    return acc


def dot_tol(A, W, split):
    """General-class accumulation bound per element (module docstring)."""
    K = A.shape[1]
    s = np.abs(A) @ np.abs(W).T
    return ((K + 8) * 2.0 ** -23 + (2.0 ** -16 if split != 1 else 0.0)) * s


def std_epilogue(acc, bias, act=0, resid=None, rowvec=None, rows_per_group=1, orig=None, byp=None,
                 exact=False):
    """The STD epilogue in the reference's op order (zv_gemm.inc header):
    v = acc + bias; act(v); v = resid + v; v += rowvec[row group]; v = orig + (v - orig) * byp.
    exact: assert every intermediate is exact in fp32 (exact class; no activation).
    Returns (v, mag, nops): mag bounds every intermediate's magnitude, nops counts the fp32
    operations, so a general-class value carries at most nops * 2^-24 * mag of epilogue roundoff
    (each operation rounds once, relative 2^-24 of a result no larger than mag, and no later
    step amplifies an earlier error: additions, and a product with 0 <= byp <= 1)."""
    chk = (lambda x, w: assert_fp32_exact(x, w)) if exact else (lambda x, w: x)
    assert not (exact and act)
    v = chk(acc + bias, "acc + bias")
    mag, nops = np.abs(acc) + np.abs(bias), 1
    if act == 1:
        v = swoosh_l(v)
        mag = np.maximum(mag, np.abs(v))
    if resid is not None:
        v = chk(resid + v, "resid + v")
        mag, nops = mag + np.abs(resid), nops + 1
    if rowvec is not None:
        rvv = rowvec[np.arange(acc.shape[0]) // rows_per_group]
        v = chk(v + rvv, "v + rowvec")
        mag, nops = mag + np.abs(rvv), nops + 1
    if orig is not None:
        d = chk(v - orig, "v - orig")
        d = chk(d * byp, "(v - orig) * byp")
        v = chk(orig + d, "orig + ...")
        mag, nops = mag + 2 * np.abs(orig), nops + 3
    return v, mag, nops


def glu_ref(pre, C, rowmask=None):
    """ConvolutionModule GLU from the reference: x, s = chunk(2); x * sigmoid(s), 0 on masked rows."""
    x, s = pre[:, :C], pre[:, C:]
    g = x * sigmoid(s)
    if rowmask is not None:
        g = np.where(rowmask[:, None] != 0, 0.0, g)
    return g


def na_ref(pre, hid):
    """NonlinAttention gate from the reference: s, x, y = chunk(3); (x * tanh(s), y)."""
    s, x, y = pre[:, :hid], pre[:, hid:2 * hid], pre[:, 2 * hid:]
    return x * np.tanh(s), y


def transpose_ref(v, rpb, ldct):
    """(M, N) -> (B, N, ldct) with [b][n][l] = v[b * rpb + l][n]; NaN where nothing is written."""
    M, N = v.shape
    B = -(-M // rpb)
    out = np.full((B, N, ldct), np.nan)
    for b in range(B):
        rows = v[b * rpb:min((b + 1) * rpb, M)]
        out[b, :, :rows.shape[0]] = rows.T
    return out


# --------------------------------------------------------------------------- fused FeedForward
FFN_D = 512


def ffn_inputs(M, H, fmt, seed):
    """The FeedForward test inputs: x in {-3..3}, W1 in {-4..4}/64, b1 in {-16..16}/8 (the hidden
    pre-activation u is exact in fp32: lsb 1/64, sum |products| <= 512 * 12 lsb), W2 ~ N(0, 1/H)
    rounded to the operand format, b2 and resid Gaussian."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (M, FFN_D)).astype(np.float64)
    W1 = rng.integers(-4, 5, (H, FFN_D)) / 64.0
    b1 = rng.integers(-16, 17, H) / 8.0
    W2 = round16(rng.standard_normal((FFN_D, H)) / np.sqrt(H), fmt)
    b2 = rng.standard_normal(FFN_D).astype(np.float32).astype(np.float64) * 0.1
    resid = (2.0 * rng.standard_normal((M, FFN_D))).astype(np.float32).astype(np.float64)
    return x, W1, b1, W2, b2, resid


def ffn_ref(x, W1, b1, W2, b2, fmt):
    """ff = W2 . round16(SwooshL(W1 . x + b1)) + b2 in float64 with its tolerance.
    u is exact (asserted).  h = round16(SwooshL(u)); a hidden value is ambiguous when the
    transcendental tolerance straddles a 16-bit rounding boundary, and may then be one 16-bit ulp
    off.  Per output: sum over ambiguous k of |w2_nk| ulp16(h_k), plus the fp32 accumulation bound
    (H + 8) 2^-23 sum_k |w2_nk||h_k|, plus one fp32 ulp for the + b2.
    Returns (ff, tol_ff, mag) (mag = sum |w2||h| + |b2|)."""
    u = assert_fp32_exact(assert_exact_dot(x, W1) + b1, "u")
    s = swoosh_l(u)
    tol = tol_swoosh_l(u)
    h = round16(s, fmt)
    amb = round16(s - tol, fmt) != round16(s + tol, fmt)
    H = W1.shape[0]
    aw2 = np.abs(W2)
    sabs = np.abs(h) @ aw2.T
    ff = h @ W2.T + b2
    mag = sabs + np.abs(b2)
    tol_ff = (np.where(amb, ulp16(h, fmt), 0.0) @ aw2.T) + (H + 8) * 2.0 ** -23 * sabs + 2 * U32 * mag
    return ff, tol_ff, mag


def ffn_epilogue(ff, tol_ff, mag, resid, rowvec=None, rows_per_group=1, orig=None, byp=None):
    """C = resid + ff [+ rowvec]; [C = orig + (C - orig) * byp].  One fp32 ulp per operation."""
    v, tol = resid + ff, tol_ff.copy()
    mag = mag + np.abs(resid)
    tol += 2 * U32 * mag
    if rowvec is not None:
        rvv = rowvec[np.arange(ff.shape[0]) // rows_per_group]
        v, mag = v + rvv, mag + np.abs(rvv)
        tol += 2 * U32 * mag
    if orig is not None:
        v = orig + (v - orig) * byp
        mag = mag + 2 * np.abs(orig)
        tol = tol * byp + 3 * 2 * U32 * mag
    return v, tol, mag


def biasnorm_bypass(x, tol_x, nb, log_scale, orig, byp):
    """The NORM epilogue: y = x * rsqrt(mean((x - nb)^2)) * e^log_scale; out = orig + (y - orig) * byp.
    Tolerance: with r = rsqrt(ms), ms = mean((x - nb)^2) = ||x - nb||^2 / 512,
      |dy| <= scale * (r |dx| + |x| |dr|),   |dr| / r = |d ms| / (2 ms),
      |d ms| <= (2 / 512) sum |x - nb||dx| <= (2 / 512) ||x - nb|| ||dx||   (Cauchy-Schwarz),
    so |dr| / r <= ||dx||_2 / ||x - nb||_2; the kernel's own fp32 evaluation of the mean (512 terms),
    the rsqrt and the products adds (512 + 16) 2^-23 relative.  For r <= 1 (asserted: the tests'
    rows have rms(x - nb) >= 1) this gives
      tol_out = byp * scale * (tol_x + |x| * (||tol_x||_2 / ||x - nb||_2 + (512 + 16) * 2^-23)),
    plus one fp32 ulp per bypass operation.  Returns (out, tol_out)."""
    scale = np.exp(log_scale)
    d = x - nb
    nrm = np.sqrt((d * d).sum(1, keepdims=True))
    r = np.sqrt(x.shape[1]) / nrm
    assert r.max() <= 1.0, "rows must have rms(x - nb) >= 1"
    y = x * r * scale
    out = orig + (y - orig) * byp
    tnorm = np.sqrt((tol_x * tol_x).sum(1, keepdims=True))
    tol = byp * scale * (tol_x + np.abs(x) * (tnorm / nrm + (512 + 16) * 2.0 ** -23))
    tol = tol + 3 * 2 * U32 * (np.abs(y) + 2 * np.abs(orig))
    return out, tol
