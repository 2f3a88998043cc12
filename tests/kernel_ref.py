"""Float64 references for the engine's linear and fused FeedForward kernels (csrc/zv_gemm.inc,
zv_gemm256.inc, zv_ffn.inc), the ConvolutionModule's depthwise conv (zv_elem.inc's four kernels and
the fused GLU + conv launch) and the kernels at the stack boundaries (the sections at the end, with
their case lists, which the CPU and the GPU tests share); a helper, not a test.  numpy only.

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


# --------------------------------------------------------------------------- depthwise conv
# (ConvolutionModule: depthwise_conv -> SwooshR, zipformer.py:1672, scaling.py:1185-1191; the kernels
# are csrc/zv_elem.inc's four behind launch_dwconv and csrc/zv_gemm256.inc's g256_epi_glu_dw)
#
# exact    g in {-3..3}, w in {-4..4}/16, bias in {-8..8}/4 (and the +-1000 edge frames below): every
#          product is a multiple of 1/16 and sum_t |g||w| + |bias| stays far below 2^24 / 16, so u is
#          exact in fp32 in any order (assert_exact_dot's argument, asserted by dwconv_exact_u); the only
#          error is SwooshR's: tol_y = TRANS_FACTOR * err_swoosh_r(u).
# general  Gaussian g (rounded to the operand format), w and bias:
#          tol_u = (ks + 2) 2^-23 (sum_t |g||w| + |bias|): an fp32 FMA chain of ks terms and the bias
#          add are within (ks + 1) u of the exact sum, with dot_tol's factor 2 over u = 2^-24;
#          tol_y = 0.92 tol_u + TRANS_FACTOR * err_swoosh_r(u) (SwooshR's slope lies in [-0.08, 0.92]).
# In every case with more than one utterance the first and the last frame of each utterance hold
# +-1000 (exact in bf16 and fp16): a halo row read from the neighbouring utterance, or an edge frame
# repeated by a clamp, is then off by hundreds.
EDGE = 1000.0
AMB_CAP = 0.1          # at most one output in ten may be ambiguous (a condition on the reference)
# the zeros of SwooshR: next to them the 16-bit ulps are tiny against the absolute tolerance, and an
# output may be several ulps off (check16's multi-ulp count); |slope| > 0.05 at both
SWOOSH_R_ZEROS = (-3.81482, 0.0)


def dwconv_taps(x, w, B, L):
    """sum_t x[b, l - ks // 2 + t, c] * w[c, t], zero outside the utterance's own [0, L): plain
    loops over taps and frames' source positions.  x (B * L, C), w (C, ks) -> (B * L, C)."""
    x = np.asarray(x, np.float64)
    C, ks = w.shape
    x3 = x.reshape(B, L, C)
    out = np.zeros((B, L, C))
    for t in range(ks):
        s = t - ks // 2                          # source frame = l + s
        lo, hi = max(0, -s), min(L, L - s)
        if lo < hi:
            out[:, lo:hi] += x3[:, lo + s:hi + s] * w[:, t]
    return out.reshape(B * L, C)


def dwconv_ref(g, w, bias, B, L):
    """(y, u, sum_t |g||w| + |bias|): u = conv + bias, y = SwooshR(u), float64."""
    u = dwconv_taps(g, w, B, L) + bias
    mag = dwconv_taps(np.abs(g), np.abs(w), B, L) + np.abs(bias)
    return swoosh_r(u), u, mag


def dwconv_exact_u(g, w, bias, u, mag):
    """The exact class's claim: every partial sum is a multiple of the operands' lsb product, of
    magnitude at most mag < 2^24 lsb, hence exact in fp32 in any order."""
    q = _lsb(g) * _lsb(w)
    q = min(q, _lsb(bias))
    assert mag.max() / q < 2.0 ** 24, f"sum |products| = {mag.max() / q:.0f} lsb units >= 2^24"
    return assert_fp32_exact(u, "u")


def err_swoosh_r_any(x):
    """err_swoosh_r's 1.9 was measured on multiples of 1/64 (it holds on them up to |x| = 1100, the
    exact class's range); over arbitrary fp32 arguments the fp32 formula reaches 2.26 2^-24 (|x| + 6)
    (dense sweep of |x| <= 9000, worst at x = 45.4; tests/test_kernel_ref.py measures it again over
    that sweep and over the general class's own pre-activations)."""
    return 2.4 * U32 * (np.abs(x) + 6.0)


def dwconv_tol(u, mag, ks, klass, extra_u=0.0):
    """(tol_u, tol_y) of the two classes (header comment); extra_u: further uncertainty of u."""
    if klass == "exact":
        return np.zeros_like(u), TRANS_FACTOR * err_swoosh_r(u)
    tol_u = (ks + 2) * 2.0 ** -23 * mag + extra_u
    return tol_u, 0.92 * tol_u + TRANS_FACTOR * err_swoosh_r_any(np.abs(u) + tol_u)


def put_edges(x, B, L, rng, sign=None):
    """+-1000 in the first and last frame of every utterance (more than one utterance only);
    sign (C): the channels' signs, random per utterance edge and channel where not given."""
    if B > 1:
        x3 = x.reshape(B, L, -1)
        for e in (0, -1):
            x3[:, e] = EDGE * (rng.choice([-1.0, 1.0], x3[:, e].shape) if sign is None else sign)
    return x


def dwconv_weights(rng, C, ks, klass, sign=None, shift=0.0):
    """Taps and bias of a class.  sign (C): every tap of channel c carries sign[c]; shift: added to
    the bias (see dwconv_inputs)."""
    if klass == "exact":
        w, b = rng.integers(-4, 5, (C, ks)) / 16.0, rng.integers(-8, 9, C) / 4.0
    else:
        f = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
        w, b = f(C, ks) / np.float32(np.sqrt(ks)).astype(np.float64), f(C)
    if sign is not None:
        w = np.abs(w) * sign[:, None]
    return w.astype(np.float32).astype(np.float64), (b + shift).astype(np.float32).astype(np.float64)


def dwconv_inputs(B, L, C, ks, fmt, klass, split=1):
    """The stand-alone conv's test inputs (seeded by the case itself).  split 3: g is an fp32 value
    whose hi / lo pair the kernel sums (exact class: exact in hi alone).
    General class: the issue's tol_y = 0.92 tol_u is SwooshR's steepest slope; where u is large and
    negative the slope is -0.08 and the bound is 11 times the ulp-relative size it has for u > 0, and
    around u = 0, SwooshR's zero, every output is ambiguous.  So the bias is N(4, 1), and with more
    than one utterance a channel's taps share one sign, which its +-1000 edge frames carry too: the
    pre-activations next to the edges are then large and positive, and the reference meets the
    ambiguity cap (tests/test_kernel_ref.py).  The exact class needs neither."""
    for salt in range(16):
        g, w, bias = _dwconv_inputs(B, L, C, ks, fmt, klass, split, salt)
        y, u, mag = dwconv_ref(g, w, bias, B, L)
        if amb16(y, dwconv_tol(u, mag, ks, klass)[1], fmt)[0].mean() <= AMB_CAP:
            break                       # (a case of 15 outputs needs a draw without two ambiguous ones)
    return g, w, bias


def _dwconv_inputs(B, L, C, ks, fmt, klass, split, salt):
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr((B, L, C, ks, fmt, klass, split, salt)).encode()))
    sign = None
    if klass == "exact":
        g = rng.integers(-3, 4, (B * L, C)).astype(np.float64)
    else:
        g = rng.standard_normal((B * L, C)).astype(np.float32).astype(np.float64)
        g = sum(split16(g, fmt)) if split == 3 else round16(g, fmt)
        sign = rng.choice([-1.0, 1.0], C) if B > 1 else None
    g = put_edges(g, B, L, rng, sign)
    w, bias = dwconv_weights(rng, C, ks, klass, sign, 0.0 if klass == "exact" else 4.0)
    return g, w, bias


def amb16(ref, tol, fmt):
    """(ambiguous, multi-ulp) masks of check16's rule, from the reference alone."""
    amb = round16(ref - tol, fmt) != round16(ref + tol, fmt)
    return amb, amb & ~(tol < ulp16(ref, fmt))


def near_swoosh_r_zero(u, tol_y, fmt):
    """|u - zero| within what a multi-ulp element needs: |y| < 2^(p + 1) tol_y there, and SwooshR's
    slope is steeper than 0.05 at both zeros."""
    d = np.min([np.abs(u - z) for z in SWOOSH_R_ZEROS], axis=0)
    return d <= 2.0 ** (PREC[fmt] + 1) * tol_y / 0.05 + 1e-3


def assert_amb_cap(amb, multi, u, tol_y, fmt, what):
    """The ambiguity condition on the reference: at most one output in ten ambiguous, multi-ulp ones
    only next to a zero of SwooshR."""
    share = float(amb.mean())
    assert share <= AMB_CAP, f"{what}: {100 * share:.1f} % of the outputs are ambiguous"
    assert near_swoosh_r_zero(u, tol_y, fmt)[multi].all(), f"{what}: multi-ulp away from SwooshR's zeros"
    return share


# the stand-alone conv's case list: (arm, ks, B, L, C, ldin - C, split, fp8 copy); arm = the
# environment that selects the kernel: "pipe" (default), "pipe2" / "pipe3" / "pipe5" (fixed chunks),
# "lds" (ZV_DWCONV_PIPE=0), "win" (both knobs 0, or a width / operand the LDS forms do not take)
DW_LENGTHS = (1, 3, 14, 8, 9, 63, 64, 65, 130, 327)
DW_ENV = {"pipe": {}, "pipe2": {"ZV_DWCONV_PIPE": "2"}, "pipe3": {"ZV_DWCONV_PIPE": "3"},
          "pipe5": {"ZV_DWCONV_PIPE": "5"}, "lds": {"ZV_DWCONV_PIPE": "0"},
          "win": {"ZV_DWCONV_PIPE": "0", "ZV_DWCONV_LDS": "0"}}


def dwconv_cases():
    cases = []
    for ks in (7, 9, 15, 31):
        for i, L in enumerate(DW_LENGTHS):
            C = (256, 128)[i % 2]
            cases.append(("pipe", ks, 3, L, C, 0, 1, False))
            if ks <= 15:
                cases.append(("lds", ks, 3, L, C, 8, 1, False))
            cases.append(("win", ks, 3, L, 192, 8, 1, False))       # C % 128 != 0: no knob needed
            cases.append(("win", ks, 3, L, 192, 8, 3, False))       # lo halves
        for L in (1, 9, 65, 327):
            cases.append(("win", ks, 3, L, 128, 0, 1, False))       # both knobs off at an LDS width
            cases.append(("win", ks, 3, L, 128, 0, 1, True))        # fp8 copy
        for arm in ("pipe2", "pipe3", "pipe5"):
            cases.append((arm, ks, 3, 327, 256, 0, 1, False))
        cases.append(("pipe", ks, 1, 327, 128, 0, 1, False))        # one utterance
    for ks in (5, 63):
        for L in DW_LENGTHS:
            cases.append(("pipe", ks, 3, L, 6, 2, 1, False))        # generic kernel: no model size
            cases.append(("pipe", ks, 3, L, 5, 0, 1 if L % 2 else 3, False))   # odd C, odd stride
    cases.append(("pipe", 7, 3, 65, 70, 1, 1, False))               # generic (odd stride): a second channel tile
    return cases


def dwconv_case_id(c):
    arm, ks, B, L, C, pad, split, q8 = c
    return f"{arm}-k{ks}-B{B}xL{L}-C{C}+{pad}-s{split}{'-q8' if q8 else ''}"


def dwconv_predict(case, cus):
    """launch_dwconv's choice for a case: [kernel, ks, 3 / 1, fp8, grid x, y, z, nft]."""
    arm, ks, B, L, C, pad, split, q8 = case
    ldin = C + pad
    model = ks in (7, 9, 15, 31)
    wide = split == 1 and not q8 and C % 128 == 0 and ldin % 8 == 0
    pipe = {"pipe": 1, "pipe2": 2, "pipe3": 3, "pipe5": 5}.get(arm, 0)
    ntile = -(-L // 64)
    if pipe and wide and model:
        nft = max(2, min(ntile, ntile * (C // 128) * B // (2 * cus)))
        if pipe > 1:
            nft = pipe
        return [3, ks, 1, 0, C // 128, -(-ntile // nft), B, nft]
    if arm != "win" and wide and ks in (7, 9, 15):
        return [2, ks, 1, 0, C // 128, ntile, B, 0]
    if model and C % 2 == 0 and ldin % 2 == 0:
        return [1, ks, split, int(q8), -(-(C // 2) // 64), -(-(-(-L // 8)) // 4), B, 0]
    return [0, ks, split, 0, -(-L // 64), -(-C // 64), B, 0]


# --------------------------------------------------------------------------- fused GLU + conv
# The ConvolutionModule's fused launch: in_proj (K = 512, N = 1024) -> GLU -> masked_fill ->
# round16 -> depthwise conv -> SwooshR.  The GEMM operands are exact-class ones in both classes
# (A in {-3..3}, W in {-4..4}/64, bias multiples of 1/8: the pre-activation is exact in fp32), so a
# GLU value's only error is the sigmoid's; the classes differ in the conv's taps and bias (dyadic /
# Gaussian).  Gaussian GEMM operands cannot meet the ambiguity cap: dot_tol's (K + 8) 2^-23 relative
# bound against a 2^-8 ulp makes about one bf16 GLU value in twenty ambiguous, and an output counts
# as ambiguous when any of its ks window entries is.  For the same reason the gate's bias is 4 +-
# 2: sigmoid(s) near 1 keeps |x| ERR_SIGMOID small against ulp16(x sigmoid(s)) (the fp16 library's
# 2^-11 ulps need it at ks = 31).  Column 511 of A is 0 except on the utterances' edge frames (1),
# against +-256 in the value half of W: the edge frames' GLU values are near +-250, with the sign
# of the channel's taps, and the conv's bias is shifted by 8 (dwconv_inputs explains both).
GLU_DW_SHAPES = [(1, 1), (2, 5), (40, 8), (3, 97), (1, 226), (1, 227), (1, 242), (1, 243), (1, 250),
                 (1, 251), (2, 300)]
GLU_DW_MASKED = (2, 300)                              # the tail of its second utterance is masked


def glu_dw_inputs(B, L, ks, fmt, klass, masked):
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr(("glu_dw", B, L, ks, fmt, klass)).encode()))
    M, K, C = B * L, 512, 512
    A = rng.integers(-3, 4, (M, K)).astype(np.float64)
    W = rng.integers(-4, 5, (2 * C, K)) / 64.0
    A[:, K - 1], W[:, K - 1] = 0.0, 0.0
    sign = rng.choice([-1.0, 1.0], C)
    if B > 1:
        A3 = A.reshape(B, L, K)
        A3[:, 0, K - 1] = A3[:, -1, K - 1] = 1.0
        W[:C, K - 1] = 256.0 * sign
    # (a small value bias: with taps of one sign a channel's mean is amplified by sum_t |w_t|)
    bias = np.concatenate([rng.integers(-4, 5, C) / 8.0, 4.0 + rng.integers(-16, 17, C) / 8.0])
    mask = np.zeros(M, bool)
    if masked:
        mask[M - 37:] = True
    w, b = dwconv_weights(rng, C, ks, klass, sign if B > 1 else None, 8.0)
    return A, W, bias, mask, w, b


def glu_dw_ref(A, W, bias, mask, w, b, B, L, fmt, klass):
    """Returns (y, tol_y, u, ambiguous-for-the-cap mask, multi-ulp mask)."""
    C, ks = w.shape
    pre = assert_fp32_exact(assert_exact_dot(round16(A, fmt), round16(W, fmt)) + bias, "pre")
    assert np.array_equal(round16(A, fmt), A) and np.array_equal(round16(W, fmt), W)
    g = glu_ref(pre, C, mask)
    x = pre[:, :C]
    tg = np.where(mask[:, None], 0.0, np.abs(x) * TRANS_FACTOR * ERR_SIGMOID + U32 * np.abs(g))
    h = round16(g, fmt)
    amb_h = round16(g - tg, fmt) != round16(g + tg, fmt)
    y, u, mag = dwconv_ref(h, w, b, B, L)
    extra = dwconv_taps(np.where(amb_h, ulp16(h, fmt), 0.0), np.abs(w), B, L)
    tol_u, tol_y = dwconv_tol(u, mag, ks, "general", extra)     # h is no dyadic rational: the FMA chain rounds
    amb, multi = amb16(y, tol_y, fmt)
    window = dwconv_taps(amb_h.astype(np.float64), np.ones((C, ks)), B, L) > 0
    return y, tol_y, u, amb | window, multi


# --------------------------------------------------------------------------- stack boundaries
def ds_weights(ds):
    """Dyadic downsampling weights that sum to 1 and differ per position: 1/2, 1/4, ..., the last twice."""
    w = [2.0 ** -(k + 1) for k in range(ds - 1)]
    return np.array(w + [2.0 ** -(ds - 1)] if ds > 1 else [1.0])


def downsample_ref(x, w, B, L, ds, exact=False):
    """SimpleDownsample (zipformer.py:887-913): right-pad each utterance by repeating its last frame,
    then the weighted sum of ds frames.  x (B * L, C) -> (B * dL, C)."""
    C = x.shape[1]
    dL = -(-L // ds)
    x3 = x.reshape(B, L, C)
    pad = dL * ds - L
    if pad:
        x3 = np.concatenate([x3, np.repeat(x3[:, -1:], pad, axis=1)], axis=1)
    x4 = x3.reshape(B, dL, ds, C)
    acc = np.zeros((B, dL, C))
    for k in range(ds):
        acc = acc + x4[:, :, k] * w[k]
        if exact:
            assert_fp32_exact(x4[:, :, k] * w[k], "x w"), assert_fp32_exact(acc, "partial sum")
    return acc.reshape(B * dL, C)


def upsample_combine_ref(orig, d, sc, B, L, ds, exact=False):
    """SimpleUpsample + BypassModule (zipformer.py:925-935): orig + (repeat(d, ds)[:L] - orig) * sc."""
    C = orig.shape[1]
    dL = -(-L // ds)
    up = np.repeat(d.reshape(B, dL, C), ds, axis=1)[:, :L].reshape(B * L, C)
    diff = up - orig
    out = orig + diff * sc
    if exact:
        assert_fp32_exact(diff, "u - o"), assert_fp32_exact(diff * sc, "(u - o) sc"), assert_fp32_exact(out, "out")
    return out


def mask_downsample_ref(mask, B, L, ds):
    """mask[..., ::ds] (zipformer.py:857-858)."""
    return mask.reshape(B, L)[:, ::ds].reshape(-1)
