"""Float64 references for the engine's linear and fused FeedForward kernels (csrc/zv_gemm.inc,
zv_gemm256.inc, zv_ffn.inc), the ConvolutionModule's depthwise conv (zv_elem.inc's four kernels and
the fused GLU + conv launch) and the kernels at the stack boundaries (with their case lists, which the CPU and the GPU tests share),
the BigVGAN kernels with the implicit-conv GEMM (its case lists are in tests/bigvgan_cases.py), and
the kernels around the decoder (the last section, "solve boundary"; case lists in tests/solve_cases.py);
a helper, not a test.  numpy only.

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


# --------------------------------------------------------------------------- BigVGAN
# (csrc/zv_bigvgan.inc's kernels, the implicit-conv GEMM and conv_pre's im2col, one launch at a time
# through zv_bigvgan_check; tests/test_gpu_bigvgan_ref.py.)  Every reference handles each utterance
# on its own: raggedness is "decode this utterance alone".  A stage stream holds utterance b in rows
# b * Lp + [0, Lmax), Lp = round_up(Lmax + halo, 8); its length is min(lens[b] * scale, Lmax).
#
# Classes and bounds (u = 2^-24; "2 u" carries dot_tol's factor 2 for an FMA chain in any order):
#  ACT   exact: small-integer x, the dyadic taps BV_TAPS_EXACT, ibeta = 0 (the sine is evaluated and
#        multiplied by 0): every partial sum is an fp32 value (asserted), tolerance 0; the 16-bit
#        copies equal split16 of it.
#        general: y = 2x upsample, 6-term FMA chain: dy = 6 * 2u * sum|f||x| (+ the input's own
#        uncertainty through sum|f|); t = sin^2(a y): dt = 2 |s| a dy + (a dy)^2 + E_TERM, where
#        E_TERM = BV_ETERM[class] is the measured error of the kernel's sin^2(a y) at an exact y
#        (the fp32 product, the hardware sine behind __sinf and the square), 2x the measured maximum
#        over the class's argument range; v = y + ib t: dv = dy + ib dt + 2u (ib t) + 2u |v|;
#        z = 12-term chain: dz = sum|d| dv + 12 * 2u * sum|d||v|.
#  CONV  exact: dyadic operands, assert_exact_dot; general: dot_tol with K = ks * Cp plus the
#        epilogue's roundings (std_epilogue's count).
#  CONVT gather alone: small integers, exact.  With the GEMM: per gathered term dot_tol of P plus one
#        rounding of the running sum, one more for the bias.
#  POST  clamp: (7 C + 2) u (sum|w||a| + |bias|); tanh: that bound through tanh's slope (<= 1) plus
#        TRANS_FACTOR * ERR_TANH.
#  AVG / IM2COL: fp32 numpy in the kernel's operation order, one rounding (u) per operation allowed.
# The sine term's allowance was measured on an MI355X through ZV_BV_ACT with a one-tap filter
# (z[t] = 2 x[t] + ib sin^2(2 a x[t]), a single evaluation per output; profiles/bigvgan_ref_pin.txt).
BV_TAPS_EXACT = np.array([1, -2, 3, -4, 5, 6, 7, -3, 2, -1, 4, -5]) / 16.0
BV_ARG_GENERAL = 16.0                  # |alpha y| of the general class, radians
BV_ARG_WIDE = 64 * 2 * np.pi           # ... of the wide class: 64 turns
# |error| of the kernel's sin^2(alpha y) for an exact y, measured: 1.30e-6 up to 16 rad, 3.50e-5 up to
# 64 turns (it grows with the argument: the fp32 product alpha y and its conversion to turns each
# round at 2^-24 |arg|); the allowance is twice that
BV_ETERM = {"general": 2 * 1.30e-6, "wide": 2 * 3.50e-5}


def encode16(x, fmt):
    """float64 values that are numbers of the format -> uint16 bit patterns (decode16's inverse)."""
    x = np.asarray(x, np.float64)
    assert np.array_equal(round16(x, fmt), x), "not values of the format"
    if fmt == "f16":
        return x.astype(np.float16).view(np.uint16)
    return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bv_rows(Lmax, halo):
    return -(-(Lmax + halo) // 8) * 8


def bv_lens(lens, scale, Lmax, B):
    return [Lmax if lens is None else min(int(lens[b]) * scale, Lmax) for b in range(B)]


def bv_upsample(x, f, absf=False):
    """UpSample1d(2) of one utterance x (T, C): replicate pad 5, 2 * conv_transpose1d(stride 2) with
    the 12 taps, crop 15 at both ends -> (2 T, C).  Plain loops over the taps."""
    T = x.shape[0]
    xp = np.concatenate([np.repeat(x[:1], 5, 0), x, np.repeat(x[-1:], 5, 0)], 0)
    full = np.zeros((2 * (T + 10 - 1) + 12, x.shape[1]))
    for j in range(12):                                 # frame i lands on sample 2 i + j
        full[j:j + 2 * (T + 10):2] += xp * (abs(f[j]) if absf else f[j])
    return 2.0 * full[15:full.shape[0] - 15]


def bv_downsample(y, f, absf=False):
    """DownSample1d(2) of one utterance y (2 T, C): replicate pad (5, 6), stride-2 correlation."""
    T = y.shape[0] // 2
    yp = np.concatenate([np.repeat(y[:1], 5, 0), y, np.repeat(y[-1:], 6, 0)], 0)
    z = np.zeros((T, y.shape[1]))
    for j in range(12):
        z += yp[j:j + 2 * T:2] * (abs(f[j]) if absf else f[j])
    return z


def bv_filter_ref(f):
    """The kernel's polyphase arguments, derived from the transposed convolution itself: the
    response of bv_upsample to a unit impulse at frame p gives the coefficient of x[p] in every
    y[s].  up_even[m] multiplies x[t + m - 3] in y[2 t], up_odd[m] multiplies x[t + m - 2] in
    y[2 t + 1]; down = the taps."""
    f = np.asarray(f, np.float64)
    p, T = 8, 17
    imp = np.zeros((T, 1))
    imp[p] = 1.0
    y = bv_upsample(imp, f)[:, 0]
    even = [y[2 * (p - (m - 3))] for m in range(6)]
    odd = [y[2 * (p - (m - 2)) + 1] for m in range(6)]
    # every other coefficient of the response is covered by the 6 + 6: nothing is left out
    assert np.isclose(sum(even) + sum(odd), y.sum())
    return np.array(even + odd + list(f))


def bv_act_ref(x, lens, scale, B, Lmax, Lp, alpha, ibeta, f, klass="general", tol_x=None, bug=None):
    """Activation1d(SnakeBeta) over a stage stream x (B * Lp, C) -> (z, tol) (B * Lp, C), zero
    outside each utterance's [0, len).  alpha = e^log_alpha, ibeta = 1 / (e^log_beta + 1e-9) as the
    kernel takes them.  klass "exact": asserts every partial result is an fp32 value, tol 0.
    bug: a deliberate off-by-one for the visibility tests ("clamp": the replicate clamp reaches
    frame len instead of len - 1; "neighbour": utterance b reads utterance b - 1's last frame in
    place of its own first)."""
    C = x.shape[1]
    z, tol = np.zeros((B * Lp, C)), np.zeros((B * Lp, C))
    ls = bv_lens(lens, scale, Lmax, B)
    u2 = 2.0 ** -23
    for b in range(B):
        n = ls[b]
        if n == 0:
            continue
        xs = x[b * Lp:b * Lp + n].copy()
        tx = np.zeros_like(xs) if tol_x is None else tol_x[b * Lp:b * Lp + n]
        if bug == "clamp":
            xs = x[b * Lp:b * Lp + n + 1].copy()      # the clamp's last frame is row len
        if bug == "neighbour" and b > 0:
            xs[0] = x[b * Lp - 1]
        y = bv_upsample(xs, f)
        if bug == "clamp":
            y = y[:2 * n]
            xs = xs[:n]
        ymag = bv_upsample(np.abs(xs), f, True)
        if klass == "exact":
            assert_fp32_exact(y, "upsampled y")
            assert ymag.max() / (_lsb(xs) * _lsb(2 * f)) < 2.0 ** 24
        dy = 6 * u2 * ymag + bv_upsample(tx, f, True)
        arg = y * alpha
        s = np.sin(arg)
        v = y + ibeta * s * s
        if klass == "exact":
            assert np.all(ibeta == 0)
            dv = np.zeros_like(v)
        else:
            ds = alpha * dy
            ds2 = 2 * np.abs(s) * ds + ds * ds + BV_ETERM[klass]
            dv = dy + ibeta * ds2 + u2 * ibeta * s * s + u2 * np.abs(v)
        zz = bv_downsample(v, f)
        zmag = bv_downsample(np.abs(v), f, True)
        if klass == "exact":
            assert_fp32_exact(zz, "z")
            assert zmag.max() / (_lsb(v) * _lsb(f)) < 2.0 ** 24
            dz = np.zeros_like(zz)
        else:
            dz = bv_downsample(dv, f, True) + 12 * u2 * zmag
        z[b * Lp:b * Lp + n], tol[b * Lp:b * Lp + n] = zz, dz
    return z, tol


def bv_conv_cols(a, n, ks, d, Cp):
    """The im2col matrix of one utterance's n valid frames a (n, C): (n, ks * Cp), zeros outside
    [0, n) and in the padded channels; tap-major like the GEMM's K."""
    C = a.shape[1]
    pad = d * (ks - 1) // 2
    cols = np.zeros((n, ks * Cp))
    for tap in range(ks):
        for t in range(n):
            s = t + tap * d - pad
            if 0 <= s < n:
                cols[t, tap * Cp:tap * Cp + C] = a[s]
    return cols


def bv_conv_wmat(w, Cp):
    """(Cout, Cin, ks) -> (Cout, ks * Cp), [o][tap * Cp + c]: what the reference's conv multiplies
    against bv_conv_cols (written from the definition, not from the engine's relayout)."""
    Cout, Cin, ks = w.shape
    m = np.zeros((Cout, ks * Cp))
    for tap in range(ks):
        m[:, tap * Cp:tap * Cp + Cin] = w[:, :, tap]
    return m


def bv_conv_ref(a, w, bias, d, lens, scale, B, Lmax, Lp, split, fmt, resid=None, klass="general", tol_a=None,
                bug=None):
    """Conv1d (dilation d, "same" zero padding inside each utterance) of the stream a (B * Lp, C)
    as the split kernel multiplies it (operands / dot_kernel) -> (out, tol, valid mask) with
    out (B * Lp, Cout); rows outside [0, len) are left 0 and are not part of the contract.
    tol_a: uncertainty of the operand's value (STEP), carried through sum |w|.
    bug "neighbour": the zero padding replaced by the stream's own rows beyond the utterance."""
    Cout, C, ks = w.shape
    Cp = -(-C // 32) * 32
    out, tol = np.zeros((B * Lp, Cout)), np.zeros((B * Lp, Cout))
    valid = np.zeros(B * Lp, bool)
    wm = bv_conv_wmat(w, Cp)
    ls = bv_lens(lens, scale, Lmax, B)
    for b in range(B):
        n = ls[b]
        if n == 0:
            continue
        r0 = b * Lp
        cols = bv_conv_cols(a[r0:r0 + n], n, ks, d, Cp)
        if bug == "neighbour":
            pad = d * (ks - 1) // 2
            ext = np.zeros((n + 2 * pad, C))
            lo, hi = max(r0 - pad, 0), min(r0 + n + pad, a.shape[0])
            ext[lo - (r0 - pad):hi - (r0 - pad)] = a[lo:hi]
            cols = bv_conv_cols(ext, n + 2 * pad, ks, d, Cp)[pad:pad + n]
        As, Ws = operands(cols, wm, split, fmt)
        acc = assert_exact_dot(As, Ws) if klass == "exact" else dot_kernel(As, Ws)
        rs = None if resid is None else resid[r0:r0 + n]
        v, mag, nops = std_epilogue(acc, bias, resid=rs, exact=klass == "exact")
        out[r0:r0 + n] = v
        valid[r0:r0 + n] = True
        if klass != "exact":
            t = dot_tol(cols, wm, split) + 2 * nops * U32 * mag
            if tol_a is not None:
                t = t + bv_conv_cols(tol_a[r0:r0 + n], n, ks, d, Cp) @ np.abs(wm).T
            tol[r0:r0 + n] = t
    return out, tol, valid


def bv_convt_ref(x, w, bias, u, lens, scale, B, Lin, Lin_s, Lo_s, split=None, fmt=None, klass="general",
                 bug=None):
    """ConvTranspose1d (Cin, Cout, k), stride u, padding (k - u) / 2, of each utterance's len_in
    frames alone: out[t] = bias + sum over (s, j) with s u + j - pad = t of x[s] . w[:, :, j], for
    t < len_in u; 0 beyond -> (out, tol) (B * Lo_s, Cout).  split None: x and w as they are (the
    gather's exact class feeds products P); else the operands' roundings.
    bug "le": frame len_in (the next row of the stream) is gathered too."""
    Cin, Cout, k = w.shape
    pad = (k - u) // 2
    out, tol = np.zeros((B * Lo_s, Cout)), np.zeros((B * Lo_s, Cout))
    ls = bv_lens(lens, scale, Lin, B)
    for b in range(B):
        n = ls[b]
        nsrc = n + 1 if (bug == "le" and b * Lin_s + n < x.shape[0]) else n
        xs = x[b * Lin_s:b * Lin_s + nsrc]
        acc, mag, cnt = np.zeros((n * u, Cout)), np.zeros((n * u, Cout)), np.zeros((n * u, 1))
        terr = np.zeros((n * u, Cout))
        for j in range(k):
            wj = w[:, :, j].T                                  # (Cout, Cin)
            if split is None:
                p = xs @ wj.T
                pt = np.zeros_like(p)
            else:
                As, Ws = operands(xs, wj, split, fmt)
                p = assert_exact_dot(As, Ws) if klass == "exact" else dot_kernel(As, Ws)
                pt = np.zeros_like(p) if klass == "exact" else dot_tol(xs, wj, split)
            for s in range(nsrc):
                t = s * u + j - pad
                if 0 <= t < n * u:
                    acc[t] += p[s]
                    mag[t] += np.abs(p[s])
                    terr[t] += pt[s]
                    cnt[t] += 1
        v = acc + bias
        if klass == "exact":
            assert_fp32_exact(v, "convt"), assert_fp32_exact(mag + np.abs(bias), "convt partial sums")
        out[b * Lo_s:b * Lo_s + n * u] = v
        tol[b * Lo_s:b * Lo_s + n * u] = 0 if klass == "exact" else terr + (cnt + 1) * 2 * U32 * (mag + np.abs(bias))
    return out, tol


def bv_post_ref(a, w, bias, lens, scale, B, Lmax, Ls, use_tanh, klass="general", bug=None):
    """conv_post (C -> 1, 7 taps, zero padding inside [0, len)) + clamp(-1, 1) / tanh -> (wav, tol)
    (B * Lmax,); 0 for t >= len.  w (C, 7).  bug "short": the window ends one frame early."""
    C = a.shape[1]
    wav, tol = np.zeros(B * Lmax), np.zeros(B * Lmax)
    ls = bv_lens(lens, scale, Lmax, B)
    for b in range(B):
        n = ls[b]
        for t in range(n):
            acc = mag = 0.0
            for tap in range(7):
                s = t + tap - 3
                if 0 <= s < (n - 1 if bug == "short" else n):
                    acc += float(a[b * Ls + s] @ w[:, tap])
                    mag += float(np.abs(a[b * Ls + s]) @ np.abs(w[:, tap]))
            pre = acc + bias
            if klass == "exact":
                assert_fp32_exact(np.array([pre, mag + abs(bias)]), "post")
            tp = 0.0 if klass == "exact" else (7 * C + 2) * U32 * (mag + abs(bias))
            if use_tanh:
                wav[b * Lmax + t], tol[b * Lmax + t] = np.tanh(pre), tp + TRANS_FACTOR * ERR_TANH
            else:
                wav[b * Lmax + t], tol[b * Lmax + t] = min(max(pre, -1.0), 1.0), tp
    return wav, tol


def bv_avg_ref(ys):
    """(y0 + y1 + y2) / n in the kernel's order -> (value, tol): one rounding per operation."""
    s, mag = ys[0].copy(), np.abs(ys[0])
    for y in ys[1:]:
        s, mag = s + y, mag + np.abs(y)
    n = len(ys)
    return s / n, n * U32 * mag


def im2col_ref(x, layout, div, sub, lens, B, T, C, ks):
    """zv_voc_im2col_kernel: v = x / div - sub; A[b T + t][tap C + c] = v[b, c, t + tap - ks // 2],
    0 where the source frame is outside [0, len_b) -> (A (B * T, ks * C), tol, zero mask)."""
    x3 = np.asarray(x, np.float64).reshape((B, C, T) if layout == 0 else (B, T, C))
    if layout == 0:
        x3 = x3.transpose(0, 2, 1)
    A, tol = np.zeros((B * T, ks * C)), np.zeros((B * T, ks * C))
    zero = np.ones((B * T, ks * C), bool)
    for b in range(B):
        n = T if lens is None else int(lens[b])
        for t in range(T):
            for tap in range(ks):
                ts = t + tap - ks // 2
                if 0 <= ts < n:
                    A[b * T + t, tap * C:(tap + 1) * C] = x3[b, ts] / div - sub
                    tol[b * T + t, tap * C:(tap + 1) * C] = 2 * U32 * (np.abs(x3[b, ts] / div) + abs(sub))
                    zero[b * T + t, tap * C:(tap + 1) * C] = False
    return A, tol, zero


def bv_operand_tol(z, tol, split, fmt):
    """How far the value a 16-bit operand holds may be from the value the reference's operand holds,
    when the fp32 value behind it is within tol of z.  split 1: nothing unless tol straddles a
    rounding boundary, then one 16-bit ulp; split 3: tol plus the pair's own resolution, 2^-(2 p)
    relative (|x - hi| <= 2^-p |x|, and lo rounds that remainder to p bits)."""
    if split == 1:
        amb = round16(z - tol, fmt) != round16(z + tol, fmt)
        return np.where(amb, ulp16(np.abs(z) + tol, fmt), 0.0)
    return tol + 2.0 ** (-2 * PREC[fmt]) * np.abs(z)


def bv_step_ref(c, split, fmt):
    """One AMP step, the references composed: out = x + conv2(act2(conv1_d(act1(x)))) -> (out, tol,
    valid rows).  The bounds add up: each activation's own bound, its operand's rounding, carried
    through the conv's sum |w|, the conv's dot_tol, and so on through the second pair."""
    B, Lmax, Lp, d, lens = c["B"], c["Lmax"], c["Lp"], c["d"], c["lens"]
    z1, t1 = bv_act_ref(c["x"], lens, 1, B, Lmax, Lp, c["alpha"], c["ibeta"], c["f"])
    h1, th1 = bv_conv_ref(z1, c["w"], c["bias"], d, lens, 1, B, Lmax, Lp, split, fmt,
                          tol_a=bv_operand_tol(z1, t1, split, fmt))[:2]
    z2, t2 = bv_act_ref(h1, lens, 1, B, Lmax, Lp, c["alpha2"], c["ibeta2"], c["f"], tol_x=th1)
    return bv_conv_ref(z2, c["w2"], c["bias2"], 1, lens, 1, B, Lmax, Lp, split, fmt, resid=c["x"],
                       tol_a=bv_operand_tol(z2, t2, split, fmt))


# --------------------------------------------------------------------------- solve boundary
# (csrc/zv_elem.inc's kernels around the decoder, one launch at a time through zv_solve_check;
# tests/test_gpu_solve_ref.py, case lists in tests/solve_cases.py.)  Every reference is written from the
# model's definition (solver.py, zipvoice.py, zipformer.py as oracle/zipvoice_np.py restates them), in
# float64; bug= selects a deliberate mistake for the visibility checks of tests/test_kernel_ref.py
# (host only).
ONE_PLUS = 1.0 + 2.0 ** -20            # absorbs the second-order terms of a first-order rounding bound


def build_input_ref(x, tc, sc, B, T, copies, zero_speech, bug=None):
    """DiffusionModel.forward's batch (solver.py:83-98) fed to forward_fm_decoder's cat (zipvoice.py:163):
    rows [0, B T) the unconditional copy (text zeroed; speech zeroed iff zero_speech), rows [B T, 2 B T)
    the conditional one; one copy: the conditional one.  x (B T, Fx), tc (B T, Ft), sc (B T, Fs) ->
    (copies B T, Fx + Ft + Fs).
    bug: "swap" the copies swapped; "text_kept" text not zeroed in the unconditional copy;
    "speech_flip" zero_speech inverted; "boundary" the first segment one column longer (column Fx
    continues x's flat array); "no_lo" is the caller's (the lo half left zero)."""
    cond = np.concatenate([x, tc, sc], axis=1)
    if bug == "boundary":
        flat = np.concatenate([x.reshape(-1), [0.0]])
        cond[:, x.shape[1]] = flat[np.arange(1, x.shape[0] + 1) * x.shape[1]]
    if copies == 1:
        return cond
    zs = bool(zero_speech) != (bug == "speech_flip")
    unc = np.concatenate([x, tc if bug == "text_kept" else np.zeros_like(tc), np.zeros_like(sc) if zs else sc], axis=1)
    if bug == "boundary":
        unc[:, x.shape[1]] = cond[:, x.shape[1]]
    return np.concatenate([cond, unc] if bug == "swap" else [unc, cond], axis=0)


def euler_ref(x, v, cfg, g, dt, grows=None, gmul=1.0, per_row=None, exact=False, bug=None):
    """One Euler step with the guidance combine (solver.py:100-110, :239): vv = (1 + g) v_cond - g v_uncond
    (v = [uncond | cond], 2 n values; cfg 0: vv = v), x + vv dt; g per row b = i // per_row as grows[b] gmul
    where grows is given.  x None: the combine alone.  Returns (value, tol).
    exact: every fp32 step is asserted exact (dyadic g, gmul, dt; small-integer x, v), tol 0.
    general: one fp32 rounding (relative 2^-24) per operation, weighted by the float64 magnitude of that
    operation's result, propagated to the output (contraction into FMA only removes roundings):
      gi = grows gmul          -> |gi| (|vc| + |vu|)        1 + gi -> |1 + gi| |vc|
      (1 + gi) vc, gi vu, their difference -> |(1 + gi) vc| + |gi vu| + |vv|
      vv dt -> |vv dt| (and everything above times |dt|)    x + vv dt -> |x + vv dt|
    bug: "swap" v_cond and v_uncond swapped; "gmul" ignored; "prev_row" the first element of row k >= 1
    takes row k - 1's scale; "dt_sign"."""
    chk = (lambda a, w: assert_fp32_exact(a, w)) if exact else (lambda a, w: a)
    n = v.shape[0] // 2 if cfg else v.shape[0]
    if cfg:
        vu, vc = (v[n:], v[:n]) if bug == "swap" else (v[:n], v[n:])
        if grows is not None:
            row = np.arange(n) // per_row
            if bug == "prev_row":
                row = np.where((np.arange(n) % per_row == 0) & (row > 0), row - 1, row)
            gi = chk(np.asarray(grows, np.float64)[row] * (1.0 if bug == "gmul" else gmul), "grows gmul")
        else:
            gi = np.full(n, float(g))
        a, b = chk(chk(1.0 + gi, "1 + g") * vc, "(1 + g) vc"), chk(gi * vu, "g vu")
        vv = chk(a - b, "vv")
        tol_vv = U32 * (np.abs(gi) * (np.abs(vc) + np.abs(vu)) + np.abs(1.0 + gi) * np.abs(vc) + np.abs(a) + np.abs(b) + np.abs(vv))
    else:
        vv, tol_vv = v, np.zeros(n)
    if x is None:
        return vv, (np.zeros(n) if exact else ONE_PLUS * tol_vv)
    dtt = -dt if bug == "dt_sign" else dt
    step = chk(vv * dtt, "vv dt")
    out = chk(x + step, "x + vv dt")
    tol = abs(dt) * tol_vv + U32 * (np.abs(step) + np.abs(out))
    return out, (np.zeros(n) if exact else ONE_PLUS * tol)


# the kernels' libm forms (cosf, sinf, atanf, logf, log1pf, expf) in fp32 numpy against float64, over the
# arguments the tests use (tests/test_kernel_ref.py recomputes each): |error| of cos / sin for |arg| <= 60
# (absolute: |value| <= 1), and of SwooshR in the logaddexp form the small linear applies
ERR_SINCOS = 1.2 * U32


def swoosh_r_lae_f32(x):
    """zv_common.h swoosh_r_lae: max(y, 0) + log1p(exp(-|y|)) - 0.08 x - 0.313261687, y = x - 1, in fp32."""
    x = np.asarray(x, _F)
    y = x - _F(1)
    return np.maximum(y, _F(0)) + np.log1p(np.exp(-np.abs(y))) - _F(0.08) * x - _F(0.313261687)


def err_swoosh_r_lae(x):
    return 1.7 * U32 * (np.abs(x) + 2.0)


def temb_freqs(dim, n=None):
    """timestep_embedding's frequencies as the engine computes them on the host (fp32):
    exp(-ln(10000) k / half), k < n (n = half: what the kernel is given)."""
    half = dim // 2
    k = np.arange(half if n is None else n, dtype=np.float32)
    return np.exp(np.float32(-np.log(10000.0)) * k / np.float32(half)).astype(np.float32).astype(np.float64)


def temb_ref(t, freqs, dim, bug=None):
    """timestep_embedding (zipformer.py:47-69): [cos(t f_k) | sin(t f_k) | 0 for an odd dim], of the fp32
    product t f_k (exact to form in float64) -> (value (M, dim), tol).  tol = TRANS_FACTOR * ERR_SINCOS.
    bug: "halves" sin first; "freq_index" the sine half reads freqs[k] instead of freqs[k - half] (freqs
    must then hold 2 half entries)."""
    half = dim // 2
    t = np.asarray(t, np.float64)[:, None]
    arg = (t.astype(np.float32) * freqs[None, :half].astype(np.float32)).astype(np.float64)
    arg_s = arg
    if bug == "freq_index":
        arg_s = (t.astype(np.float32) * freqs[None, half:2 * half].astype(np.float32)).astype(np.float64)
    out = np.zeros((t.shape[0], dim))
    c, s = np.cos(arg), np.sin(arg_s)
    out[:, :half], out[:, half:2 * half] = (s, c) if bug == "halves" else (c, s)
    return out, np.full(out.shape, TRANS_FACTOR * ERR_SINCOS)


def small_linear_ref(x, W, b, add, pre, exact=False, bug=None):
    """The time / guidance MLPs' linear (zipformer.py:267-278, :726-729): out = act(x) W^T + b + add, act
    the identity or SwooshR (pre 1).  x (M, K), W (N, K), b (N) or None, add (M, N) or None -> (value, tol).
    exact (pre 0): dyadic operands, every partial sum in any order an fp32 value (assert_exact_dot), as are
    the bias and add steps; tol 0.
    general: the kernels sum lane-strided partial sums of ceil(K / 64) FMAs, then a 6-level tree, then the
    bias and add: at most ceil(K / 64) + 6 + 2 roundings on any path, each relative 2^-24 of a partial
    result no larger than S = sum_k |act(x_k) w_k| + |b| + |add|; pre 1 adds sum_k |w_k| tol_act(x_k), tol_act =
    TRANS_FACTOR * err_swoosh_r_lae.
    bug: "no_add", "no_bias"; "tail": every output of the last partial block of 32 takes row N - 1's
    weight and bias."""
    M, K = x.shape
    N = W.shape[0]
    a = swoosh_r(x) if pre else x
    Wk, bk = W, b
    if bug == "tail" and N % 32:
        Wk = W.copy()
        Wk[N - N % 32:] = W[N - 1]
        if b is not None:
            bk = b.copy()
            bk[N - N % 32:] = b[N - 1]
    acc = assert_exact_dot(a, Wk) if exact else a @ Wk.T
    S = np.abs(a) @ np.abs(Wk).T
    chk = (lambda v, w: assert_fp32_exact(v, w)) if exact else (lambda v, w: v)
    if b is not None and bug != "no_bias":
        acc, S = chk(acc + bk, "+ bias"), S + np.abs(bk)
    if add is not None and bug != "no_add":
        acc, S = chk(acc + add, "+ add"), S + np.abs(add)
    if exact:
        assert not pre
        return acc, np.zeros_like(acc)
    tol = (-(-K // 64) + 8) * U32 * S * ONE_PLUS
    if pre:
        tol = tol + (TRANS_FACTOR * err_swoosh_r_lae(x)) @ np.abs(Wk).T
    return acc, tol


def posp_angle(L, D):
    """extend_pe's angle per row (zipformer.py:983-1032) in float64: row n encodes the offset x = n - (L - 1);
    x_c = c sgn(x) (ln(|x| + c) - ln c), c = sqrt(D); xa = atan(x_c / (D / 2 pi)).  -> (x, xa), (2 L - 1,)."""
    x = np.arange(-(L - 1), L, dtype=np.float64)
    c = np.sqrt(float(D))
    xc = c * np.sign(x) * (np.log(np.abs(x) + c) - np.log(c))
    return x, np.arctan(xc / (D / (2.0 * np.pi)))


def posp_angle_f32(L, D):
    """The same chain as zv_posp_kernel writes it, in fp32 numpy."""
    x = np.arange(-(L - 1), L, dtype=np.float32)
    c = np.sqrt(_F(D))
    xc = c * np.sign(x) * (np.log(np.abs(x) + c) - np.log(c))
    return np.arctan(xc / _F(D / (2.0 * np.pi)))


def err_posp_angle(x, D):
    """|error| of the fp32 angle chain: the two logarithms' roundings (each 2^-24 ln(|x| + c)) scaled by c
    and the length scale, through atan's slope, plus the roundings of x_c, the quotient and atan itself
    (relative to |xa| <= pi / 2); measured constant, recomputed by tests/test_kernel_ref.py."""
    c, ls = np.sqrt(float(D)), D / (2.0 * np.pi)
    xc = c * (np.log(np.abs(x) + c) - np.log(c))
    return 1.5 * U32 * (c * 2.0 * np.log(np.abs(x) + c) / ls / (1.0 + (xc / ls) ** 2) + np.pi / 2)


def posp_table(L, D, bug=None):
    """CompactRelPositionalEncoding.extend_pe in float64 -> (pe (2 L - 1, D), tol_pe): pe[2 k] =
    cos(xa (k + 1)), pe[2 k + 1] = sin(xa (k + 1)), pe[D - 1] = 1.
    tol_pe: a = xa (k + 1) carries (k + 1) TRANS_FACTOR err_posp_angle plus the product's rounding; cos / sin
    have slope <= 1 and their own TRANS_FACTOR ERR_SINCOS; the constant column is exact.
    bug: "offset" x = n - L; "mirror" rows reversed; "interleave" cos / sin swapped; "no_one" pe[D - 1]
    left as the sine; "one_at_D-2"."""
    x, xa = posp_angle(L, D)
    if bug == "offset":
        _, xa2 = posp_angle(L + 1, D)
        xa = xa2[:2 * L - 1]                       # offsets -L .. L - 2
    k1 = np.arange(1, D // 2 + 1, dtype=np.float64)
    ang = xa[:, None] * k1[None]
    pe, tol = np.zeros((2 * L - 1, D)), np.zeros((2 * L - 1, D))
    pe[:, 0::2], pe[:, 1::2] = (np.sin(ang), np.cos(ang)) if bug == "interleave" else (np.cos(ang), np.sin(ang))
    ta = k1[None] * TRANS_FACTOR * err_posp_angle(x, D)[:, None] + U32 * np.abs(ang) + TRANS_FACTOR * ERR_SINCOS
    tol[:, 0::2] = tol[:, 1::2] = ta
    if bug == "one_at_D-2":
        pe[:, D - 2] = 1.0
    elif bug != "no_one":
        pe[:, D - 1], tol[:, D - 1] = 1.0, 0.0
    if bug == "mirror":
        pe = pe[::-1].copy()
    return pe, tol


def posp_ref(W, L, nl, HPD, D, bug=None):
    """linear_pos (no bias, zipformer.py:1239) of every layer of a stack on the table: out[l, n, c] =
    sum_k pe[n, k] W[l HPD + c, k] -> (value (nl (2 L - 1), HPD), tol).  tol = sum_k |W_k| tol_pe_k +
    (D + 1) 2^-24 sum_k |pe_k W_k| (an FMA chain of D terms).
    bug: posp_table's, and "prev_layer": layer l >= 1 reads layer l - 1's weight."""
    pe, tp = posp_table(L, D, None if bug == "prev_layer" else bug)
    W3 = W.reshape(nl, HPD, D)
    if bug == "prev_layer":
        W3 = W3[[0] + list(range(nl - 1))]
    out = np.einsum("nk,lck->lnc", pe, W3).reshape(nl * (2 * L - 1), HPD)
    tol = np.einsum("nk,lck->lnc", tp, np.abs(W3)) + (D + 1) * U32 * ONE_PLUS * np.einsum("nk,lck->lnc", np.abs(pe), np.abs(W3))
    return out, tol.reshape(out.shape)


def embed_ref(tok, table):
    """nn.Embedding (zipvoice.py:205)."""
    return table[np.asarray(tok, np.int64)]


def spk_add_ref(emb, spk, table):
    """ZipVoiceDialog's speaker-turn embeddings (zipvoice_dialog.py:153-158): + table[0] where the code is
    0, + table[1] where it is 1, nothing at -1 (padding).  Asserted exact in fp32."""
    spk = np.asarray(spk)
    return assert_fp32_exact(emb + (spk == 0)[:, None] * table[0] + (spk == 1)[:, None] * table[1], "emb + spk")


def tokens_index(feat_lens, tok_lens, T, bug=None):
    """prepare_avg_tokens_durations + get_tokens_index (common.py:246-295): every token of utterance b lasts
    d = feat_lens[b] // tok_lens[b] frames, placed cumulatively; the frames left over take the next index,
    tok_lens[b], the pad slot.  (bug None equals oracle.zipvoice_np.get_tokens_index: tests/test_kernel_ref.py.)
    bug: "no_clamp" the left-over frames go on counting tokens every d frames; "clamp_low" they take
    tok_lens[b] - 1; "d_from_T" d = T // tok_lens[b]; "d0_token0" d = 0 sends every frame to token 0."""
    idx = np.zeros((len(feat_lens), T), np.int64)
    for b, (fl, S) in enumerate(zip(feat_lens, tok_lens)):
        d = (T if bug == "d_from_T" else int(fl)) // int(S)
        durs = [d] * int(S)
        cur = 0
        for i, dd in enumerate(durs):
            idx[b, cur:min(cur + dd, T)] = i
            cur = min(cur + dd, T)
        rest = int(S) - 1 if bug == "clamp_low" else int(S)
        if bug == "d0_token0" and d == 0:
            rest = 0
        idx[b, cur:] = rest
        if bug == "no_clamp" and d > 0:
            idx[b, cur:] = np.arange(cur, T) // d
    return idx


def text_cond_ref(emb, tok_lens, feat_lens, T, bug=None):
    """forward_text_condition (zipvoice.py:234-250): emb (B, S, C) gathered per frame -> (B T, C).
    A mistaken index past the embedding reads on into the next utterance's rows, as flat memory would."""
    B, S, C = emb.shape
    idx = tokens_index(feat_lens, tok_lens, T, bug)
    flat = np.concatenate([emb.reshape(B * S, C), np.full((T, C), -7.0)])
    rows = (np.arange(B)[:, None] * S + idx).reshape(-1)
    return flat[np.minimum(rows, flat.shape[0] - 1)]


def speech_cond_ref(pf, plen, T, bug=None):
    """ZipVoice.sample's speech condition (zipvoice.py:441-451): the prompt features (B, Tp, F) padded with
    zeros to T frames (or cut), zero from prompt_len on -> (B T, F).
    bug: "le" frame prompt_len kept; "no_tp" the t < Tp term missing (frames past the prompt read on in
    flat memory)."""
    B, Tp, F = pf.shape
    flat = np.concatenate([pf.reshape(B * Tp, F), np.full((T + 1, F), -7.0)])
    out = np.zeros((B, T, F))
    for b in range(B):
        for t in range(T):
            keep = (t <= plen[b]) if bug == "le" else (t < plen[b])
            if keep and (t < Tp or bug in ("no_tp", "le")):
                out[b, t] = flat[b * Tp + t] if (t < Tp or bug == "no_tp") else 0.0
    return out.reshape(B * T, F)


# --------------------------------------------------------------------------- attention
# (csrc/zv_flash.inc's first-generation kernels and zv_attn.inc's materialising softmax, one launch at a
# time through zv_attn_check; zv_flash2.inc's second generation through zv_attn2_check_stale;
# tests/test_gpu_attn_ref.py, case lists and input classes in tests/attn_cases.py.)
#
# Definition (RelPositionMultiheadAttentionWeights, zipformer.py:1149-1306): per utterance and head
#   s[i, j] = q_i . k_j + p_i . P[L-1-i+j];  s[i, j] = -1000 where key j is padded (masked_fill: the
#   score is REPLACED);  W = softmax_j(s).
# SelfAttention (:1359-1396): out[i] = sum_j W[i, j] v_j per head; NonlinAttention (:1499-1544):
# out[i] = y_i * sum_j W0[i, j] v_j with head 0's weights.  base "2": the scores arrive in base-2 units
# (the second generation, whose engine folds log2(e) into the k / p weights; the softmax kernel's b2):
# the masked value is -1000 log2(e) and the exponential is 2^s.
#
# Operands are taken as the kernel multiplies them: q, k, p, v, y rounded to the operand format, or their
# hi / lo pairs (split 3: hi hi + hi lo + lo hi for the MFMA products, hi + lo where the kernel adds the
# halves in fp32, as ld_split does for p and y).
#
# What the engine guarantees about V^T columns [L, Lpad) (Lpad = L rounded up to 64): every workspace
# buffer is zeroed when it is allocated (zv_engine.hip DBuf::get) and grows only; the transposed stores of
# the value / NonlinAttention projections (zv_gemm.inc gemm_epilogue_trans*, store_trans8) write frames
# below L only.  So those columns hold zero, or what an earlier pass of another length or batch wrote
# there: a finite 16-bit activation as long as the model's activations are finite, never an uninitialised
# pattern.  Every kernel reads them (a key step is 32 or 64 keys) and multiplies them by a weight that is
# exactly zero (2^-inf), so finite stale data is harmless and a NaN or Inf would not be; nothing in the
# engine can put one there without the activations themselves being non-finite.  The checks fill the
# columns with +-1000.
#
# Tolerance of a consumer's output, per element (derived, nothing fitted).  Let the computed weights be
# w_j (1 + e_j).  Where numerator and denominator are summed from the same computed p_j (SelfAttention:
# the ones row of the value tile), out' - out = sum_j w_j e_j (v_j - out) / (1 + sum_j w_j e_j), so with
# |e_j| <= E:  |out' - out| <= E / (1 - E) dev,  dev = sum_j w_j |v_j - out|, which vanishes on one-hot
# rows and on constant v.  Where the denominator comes from elsewhere (first-generation NonlinAttention:
# the statistics kernel, which scores with another instruction sequence; second-generation
# NonlinAttention: the fp32 sum of p before p is rounded), the part of e_j that the denominator does not
# share leaves  out' - out = (sum_j w_j a_j v_j - out sum_j w_j b_j) / (1 + sum_j w_j b_j), bounded by
# (A + B) / (1 - B) mag with mag = sum_j w_j |v_j| >= |out|: such terms go against mag, not dev.
# [Found while deriving, before any GPU run: a NonlinAttention row of equal weights 1/n has dev != 0 but
# every p = 1/n takes the same 16-bit rounding error, which the fp32 denominator does not share --
# zv_attn_na_kernel: ph[r] = (bf16)pr after cst = -m + log2(r) from the statistics; zv_attn_na2_kernel:
# psum += pr before ph[r] = (bf16)pr.]
# E is the sum of
#   2 ds            numerator and denominator; ds = ((36 + 8) 2^-23 [+ 2^-16 split]) (sum|q||k| + sum|p||P|),
#                   dot_tol's form with K = 32 + 4, maximum over the row's keys; in base 2 times ln 2
#   p rounding      half an ulp of the rounded p.  Where the denominator is summed from the rounded p too:
#                   2^-9 / 2^-12 (16-bit forms) or 2^-16 (hi / lo pair), once for the numerator and once
#                   more for the denominator.  Where only the numerator has it (NonlinAttention): the
#                   format's unit roundoff, 2^-8 / 2^-11 -- round-to-nearest to 8 (11) significant bits
#                   moves a value just above a power of two, 2^e (1 + 2^-8), by 2^(e-8).  [After the first
#                   GPU run: with 2^-9 the bf16 first-generation NonlinAttention exceeded the bound by up
#                   to 1.47 x on elements that one +-1000 key dominates; the error there is that key's
#                   p rounding alone, zv_attn_na_kernel "ph[r] = (bf16)pr".  The SelfAttention figure
#                   2 * 2^-9 is the same number.]
#   exponentials    TRANS_FACTOR ERR_EXP2, numerator and denominator
# The Toeplitz forms (stage_tp) round the positional table to the operand format before the MFMA
# ("hv[d] = (bf16)a[i][d]": natural units in the first generation, where log2(e) multiplies the fp32 score;
# the second generation's table arrives log2(e)-scaled).  The reference takes the table as those kernels
# multiply it, round16(P), like every other operand, so no term stands for that rounding.  [After the first
# GPU run: a bound term of half an ulp of 2^-9 sum|p||P| in its place was exceeded by up to 1.33 x by
# zv_attn_stats_kernel<1, 1>, for the same reason as above: the unit roundoff is 2^-8.]
# plus, absolute, fp16 only: p below the smallest normal 2^-14 is rounded to a multiple of 2^-24 (error at
# most 2^-25, and never more than p itself).  The largest p of a row is at least 1/2 in every form (first
# generation: the running maximum's own p is 1; second generation, FA2_OFS: the offset is the integer
# ceiling of a maximum over some of the row's keys, so the row maximum's p is above 1/2; it stays finite
# while no score rises 16 above the offset, else the exact path with the maximum subtracted), so the
# denominator is at least 1/2 and a weight is off by at most min(2^-24, w_j): sub = sum_j min(2^-24, w_j)
# (|v_j| + |out|) (and the same sum without v on the shared denominator).
# plus (L + 8) 2^-23 mag for the fp32 accumulation of L products (the online rescales included) and
# 4 2^-24 |out| for the final reciprocal and multiplies (NonlinAttention's y among them).
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
ATT_QD, ATT_PD = 32, 4
ATT_SUB = 2.0 ** -24                   # fp16: absolute error of a weight from p's subnormal range
# relative error of numpy's fp32 exp2 against float64 (measured; tests/test_kernel_ref.py recomputes it)
ERR_EXP2 = 1.8 * U32

# form -> what its bound needs: split; tp: the positional table rounded to the operand format; den: where
# the denominator comes from ("ones": summed from the rounded p; "stats": another pass; "psum": the fp32 p)
ATTN_FORMS = {
    # first generation (natural units)
    "stats1": dict(kind="stats", split=1, tp=False, base="e"),
    "stats1_tp": dict(kind="stats", split=1, tp=True, base="e"),
    "stats3": dict(kind="stats", split=3, tp=False, base="e"),
    "na1": dict(kind="na", split=1, tp=False, den="stats", base="e"),
    "na1_tp": dict(kind="na", split=1, tp=True, den="stats", base="e"),
    "na3": dict(kind="na", split=3, tp=False, den="stats", base="e"),
    "sa1": dict(kind="sa", split=1, tp=False, den="ones", base="e"),
    "sa3": dict(kind="sa", split=3, tp=False, den="ones", base="e"),
    "sa_tp2": dict(kind="sa", split=1, tp=True, den="ones", base="e"),
    "sa_tp1": dict(kind="sa", split=1, tp=True, den="ones", base="e"),
    "softmax1": dict(kind="softmax", split=1, tp=False, base="e"),
    "softmax3": dict(kind="softmax", split=3, tp=False, base="e"),
    "softmax1_b2": dict(kind="softmax", split=1, tp=False, base="2"),
    "softmax3_b2": dict(kind="softmax", split=3, tp=False, base="2"),
    # second generation (base 2)
    "sa2": dict(kind="sa", split=1, tp=True, den="ones", base="2"),
    "na2": dict(kind="na", split=1, tp=True, den="psum", base="2"),
}


def attn_parts(x, split, fmt):
    """The operand halves the kernel holds: [round16(x)] or the hi / lo pair."""
    return [round16(x, fmt)] if split == 1 else list(split16(x, fmt))


def attn_table(P, f, fmt):
    """The positional table as the form multiplies it: fp32, or rounded to the operand format (stage_tp)."""
    return round16(P, fmt) if f["tp"] else P


def attn_heads(qkp, H):
    """(L, 2 * 32 H + 4 H) rows [q | k | p] -> q (H, L, 32), k (H, L, 32), p (H, L, 4)."""
    L = qkp.shape[0]
    q = qkp[:, :H * ATT_QD].reshape(L, H, ATT_QD).transpose(1, 0, 2)
    k = qkp[:, H * ATT_QD:2 * H * ATT_QD].reshape(L, H, ATT_QD).transpose(1, 0, 2)
    p = qkp[:, 2 * H * ATT_QD:].reshape(L, H, ATT_PD).transpose(1, 0, 2)
    return q, k, p


def attn_weights_ref(q, k, p, P, pad, base, bug=None):
    """One utterance, one head.  q, k: lists of operand halves (L, 32) ([hi] or [hi, lo]: hi hi + hi lo +
    lo hi); p (L, 4) the value the kernel multiplies; P (2L - 1, 4); pad (L,) 1 = padded, or None.
    Returns (w (L, L), qmass, pmass): the weights and, per score, sum|q||k| and sum|p||P|.
    bug: "n_off" n = L - i + j; "mask_kept" the first padded key not masked; "mask_added" -1000 added to a
    padded key's score instead of replacing it."""
    L = p.shape[0]
    i = np.arange(L)[:, None]
    j = np.arange(L)[None, :]
    n = L - 1 - i + j
    if bug == "n_off":
        n = np.minimum(n + 1, 2 * L - 2)
    s = dot_kernel(q, k) + (p @ P.T)[i, n]
    qmass = sum(np.abs(a) for a in q) @ sum(np.abs(a) for a in k).T
    pmass = (np.abs(p) @ np.abs(P).T)[i, n]
    mval = -1000.0 * (LOG2E if base == "2" else 1.0)
    if pad is not None and np.any(pad):
        m = np.asarray(pad).astype(bool).copy()
        if bug == "mask_kept":
            m[np.flatnonzero(m)[0]] = False
        s = np.where(m[None, :], s + mval if bug == "mask_added" else mval, s)
    s = s - s.max(1, keepdims=True)
    e = np.exp2(s) if base == "2" else np.exp(s)
    return e / e.sum(1, keepdims=True), qmass, pmass


def attn_score_ref(q, k, p, P, pad, base):
    """The masked scores themselves (for the statistics), in the units given."""
    L = p.shape[0]
    i = np.arange(L)[:, None]
    j = np.arange(L)[None, :]
    s = dot_kernel(q, k) + (p @ P.T)[i, L - 1 - i + j]
    if pad is not None:
        s = np.where(np.asarray(pad).astype(bool)[None, :], -1000.0 * (LOG2E if base == "2" else 1.0), s)
    return s


def attn_E(form, fmt, qmass, pmass, L):
    """Per query row: (Es, En, Esm): the relative weight error that numerator and denominator share, the
    part only the numerator has, and the weights' own (for the softmax kernel)."""
    f = ATTN_FORMS[form]
    unit = LN2 if f["base"] == "2" else 1.0
    ds = ((36 + 8) * 2.0 ** -23 + (2.0 ** -16 if f["split"] == 3 else 0.0)) * (qmass + pmass)
    ds = ds.max(1) * unit
    prnd = 2.0 ** -(PREC[fmt] + 1) if f["split"] == 1 else 2.0 ** -16          # half an ulp at the top of a binade
    pone = 2.0 ** -PREC[fmt] if f["split"] == 1 else 2.0 ** -16                # ... at its bottom: the unit roundoff
    ex = TRANS_FACTOR * ERR_EXP2
    acc = (L + 8) * 2.0 ** -23
    den = f.get("den")
    if den == "ones":
        return 2 * ds + 2 * prnd + 2 * ex, np.zeros_like(ds), None
    if den == "psum":
        return 2 * ds + 2 * ex + acc, pone + np.zeros_like(ds), None
    if den == "stats":
        return np.zeros_like(ds), 2 * ds + pone + 2 * ex + acc, None
    return None, None, 2 * ds + 2 * ex + acc


def attn_dev(w, v, out):
    """dev = sum_j w_j |v_j - out| per (query, channel), in channel blocks."""
    dev = np.zeros_like(out)
    for c0 in range(0, v.shape[1], 16):
        d = np.abs(v[None, :, c0:c0 + 16] - out[:, None, c0:c0 + 16])        # (i, j, c)
        dev[:, c0:c0 + 16] = np.einsum("ij,ijc->ic", w, d)
    return dev


def attn_out_tol(form, fmt, w, v, out, qmass, pmass):
    """The consumer bound of the section comment for one utterance and head: (L, C).  NonlinAttention
    (hundreds of channels) takes dev <= mag + |out| instead of the sum itself: its shared part Es is the
    fp32-level part of E only (the p rounding goes against mag there anyway), so nothing visible is lost;
    sub is bounded the same way in every form, sum_j min(2^-24, w_j) (|v_j| + |out|)."""
    L = w.shape[0]
    f = ATTN_FORMS[form]
    Es, En, _ = attn_E(form, fmt, qmass, pmass, L)
    mag = w @ np.abs(v)
    dev = attn_dev(w, v, out) if f["kind"] == "sa" else mag + np.abs(out)
    sb = 0.0
    if fmt == "f16":
        ws = np.minimum(w, ATT_SUB)
        sb = ws @ np.abs(v) + ws.sum(1)[:, None] * np.abs(out)
        if f["den"] == "ones":
            Es = Es + ws.sum(1)
    Es = Es[:, None]
    assert Es.max() < 0.5
    return (Es * dev + En[:, None] * mag) / (1.0 - Es) + sb + (L + 8) * 2.0 ** -23 * mag + 4 * U32 * np.abs(out)


def attn_consumer_ref(form, fmt, qkp, P, pad, v, y, H, nv, bug=None, tol=True):
    """SelfAttention / NonlinAttention of a batch.  qkp (B, L, .), P (2L - 1, 4 H), pad (B, L) or None,
    v (B, L, H nv) / (B, L, nv), y (B, L, nv) or None: fp32 values (float64 arrays), rounded / split here.
    Returns (ref, tol) of shape v's.
    bug: attn_weights_ref's, or "past_L" a key L (zero k, no table row: score 0) whose value is +1000
    included; "utt_prev" utterance b reads utterance b - 1's values; "head_next" head h reads head h + 1's
    positional slice."""
    f = ATTN_FORMS[form]
    sa = f["kind"] == "sa"
    B, L, _ = qkp.shape
    ref = np.zeros(v.shape)
    tl = np.zeros(v.shape)
    vs = sum(attn_parts(v, f["split"], fmt))
    for b in range(B):
        q, k, p = attn_heads(qkp[b], H)
        vb = vs[b - 1 if bug == "utt_prev" else b]
        for h in (range(H) if sa else [0]):
            hp = (h + 1) % H if bug == "head_next" else h
            qq, kk = attn_parts(q[h], f["split"], fmt), attn_parts(k[h], f["split"], fmt)
            pp = sum(attn_parts(p[h], f["split"], fmt))
            Ph = attn_table(P[:, hp * ATT_PD:(hp + 1) * ATT_PD], f, fmt)
            w, qm, pm = attn_weights_ref(qq, kk, pp, Ph, None if pad is None else pad[b], f["base"], bug)
            vh = vb[:, h * nv:(h + 1) * nv] if sa else vb
            if bug == "past_L":
                s0 = attn_score_ref(qq, kk, pp, Ph, None if pad is None else pad[b], f["base"]).max(1)
                e = (np.exp2(-s0) if f["base"] == "2" else np.exp(-s0))[:, None]      # the extra key's weight
                o = (w @ vh + e * 1000.0) / (1.0 + e)
            else:
                o = w @ vh
            t = attn_out_tol(form, fmt, w, vh, o, qm, pm) if tol else 0.0
            if sa:
                ref[b, :, h * nv:(h + 1) * nv] = o
                tl[b, :, h * nv:(h + 1) * nv] = t
            else:
                yy = sum(attn_parts(y[b], f["split"], fmt))
                ref[b] = o * yy
                tl[b] = t * np.abs(yy) + U32 * np.abs(ref[b])
    return ref, tl


def attn_stats_ref(form, fmt, qkp, P, pad, H):
    """Head 0's row statistics in base 2: (lse2, mx2, tol) each (B, L): log2 sum_j 2^u_j and max_j u_j with
    u = log2(e) s.  tol: ds log2(e) for the scores, the accumulation and the exponentials of the sum, and
    fp32 roundings of m, log2 r and their difference."""
    f = ATTN_FORMS[form]
    B, L, _ = qkp.shape
    lse = np.zeros((B, L))
    mx = np.zeros((B, L))
    tl = np.zeros((B, L))
    for b in range(B):
        q, k, p = attn_heads(qkp[b], H)
        qq, kk = attn_parts(q[0], f["split"], fmt), attn_parts(k[0], f["split"], fmt)
        pp = sum(attn_parts(p[0], f["split"], fmt))
        pb = None if pad is None else pad[b]
        P0 = attn_table(P[:, :ATT_PD], f, fmt)
        u = attn_score_ref(qq, kk, pp, P0, pb, "e") * LOG2E
        _, qm, pm = attn_weights_ref(qq, kk, pp, P0, pb, "e")
        mx[b] = u.max(1)
        lse[b] = mx[b] + np.log2(np.exp2(u - mx[b][:, None]).sum(1))
        # (the bound of the scores as attn_E forms it, without the factor 2 and in base 2)
        ds = ((36 + 8) * 2.0 ** -23 + (2.0 ** -16 if f["split"] == 3 else 0.0)) * (qm + pm)
        tl[b] = ds.max(1) * LOG2E + ((L + 8) * 2.0 ** -23 + 2 * TRANS_FACTOR * ERR_EXP2 + 2.0 ** -22) / LN2 \
            + 2.0 ** -22 * (np.abs(mx[b]) + np.abs(lse[b]) + 1.0)
    return lse, mx, tl


def attn_softmax_ref(form, fmt, qkp, P, pad, H, bug=None):
    """The materialised weights (H, B, L, L) and their relative tolerance (H, B, L)."""
    f = ATTN_FORMS[form]
    B, L, _ = qkp.shape
    W = np.zeros((H, B, L, L))
    E = np.zeros((H, B, L))
    for b in range(B):
        q, k, p = attn_heads(qkp[b], H)
        for h in range(H):
            qq, kk = attn_parts(q[h], f["split"], fmt), attn_parts(k[h], f["split"], fmt)
            pp = sum(attn_parts(p[h], f["split"], fmt))
            W[h, b], qm, pm = attn_weights_ref(qq, kk, pp, P[:, h * ATT_PD:(h + 1) * ATT_PD],
                                               None if pad is None else pad[b], f["base"], bug)
            E[h, b] = attn_E(form, fmt, qm, pm, L)[2]
    return W, E


def attn_accept(got, ref, tol, fmt, split=1):
    """The interval rule: round16(ref - tol) <= got <= round16(ref + tol) per element; split 3: got = hi +
    lo within tol + 2^-16 |ref| (+ the pair's underflow).  Returns (bad mask, max |got - ref| / (tol + the format's half ulp))."""
    ref = np.asarray(ref, np.float64)
    if split == 3:
        # (+ what the pair cannot hold: half the format's smallest spacing, and fp32's smallest normal)
        t = tol + 2.0 ** -16 * np.abs(ref) + 0.5 * ulp16(0.0, fmt) + 2.0 ** -126
        lo, hi = ref - t, ref + t
        allow = t
    else:
        lo, hi = round16(ref - tol, fmt), round16(ref + tol, fmt)
        allow = tol + 0.5 * ulp16(ref, fmt)
    with np.errstate(invalid="ignore"):
        bad = ~((got >= lo) & (got <= hi)) | ~np.isfinite(got)
        err = np.where(got == ref, 0.0, np.abs(got - ref) / np.maximum(allow, 1e-300))
    return bad, float(np.nanmax(err)) if err.size else 0.0
