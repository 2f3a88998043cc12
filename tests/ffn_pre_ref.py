"""Float64 reference for the fused FeedForward's pre-projection form (csrc/zv_ffn.inc, PRE):

    cur1 = resid + (A . Wp^T + bp) [+ rowvec]      the conv + SelfAttention out-projection
    x    = round16(cur1)                            formed in registers, the module's input
    v    = cur1 + W2 . swoosh_l(W1 . x + b1) + b2   then the bypass / BiasNorm + bypass epilogue

Inputs (exact classes, asymmetric): A in {-2..3}, Wp in {-3..4}/8, bp and rowvec in {-8..9}/8, and
resid = x - (A . Wp^T + bp + rowvec) with x the class kernel_ref.ffn_inputs uses ({-3..3}).  Every
term is a multiple of 1/8 and sum |terms| <= 3 * 0.5 * K + |resid| + 3 stays below 2^12, so every
partial sum in any order is exact in fp32 (asserted: pre_inputs) and cur1 = x exactly, in both
16-bit formats.  kernel_ref.ffn_ref / ffn_epilogue / biasnorm_bypass then apply unchanged with cur1
as the residual.  Tolerance: theirs plus one fp32 ulp (at the result's magnitude) for each of the
three added operations (+ bp, + resid, + rowvec).

A wrong K order is far outside: pre_perturbed() drops or rotates one 32-wide K chunk of Wp, which
moves cur1 by whole units of its class (tests/test_ffn_pre_ref.py)."""
import numpy as np

import kernel_ref as kr

D = kr.FFN_D
PRE_OPS = 3


def pre_inputs(M, H, K, fmt, rpg, seed):
    """(x, W1, b1, W2, b2), (A, Wp, bp, resid, rowvec): rowvec None when rpg == 0."""
    x, W1, b1, W2, b2, _ = kr.ffn_inputs(M, H, fmt, seed)
    rng = np.random.default_rng(seed + 77)
    A = rng.integers(-2, 4, (M, K)).astype(np.float64)
    Wp = rng.integers(-3, 5, (D, K)) / 8.0
    bp = rng.integers(-8, 10, D) / 8.0
    rv = rng.integers(-8, 10, (-(-M // rpg), D)) / 8.0 if rpg else None
    pre = kr.assert_exact_dot(A, Wp) + bp
    if rv is not None:
        pre = pre + rv[np.arange(M) // rpg]
    resid = x - pre
    # every partial sum is a multiple of 1/8 bounded by the sum of magnitudes: exact in fp32
    bound = np.abs(A) @ np.abs(Wp).T + np.abs(bp) + np.abs(resid) + (0 if rv is None else np.abs(rv).max())
    assert bound.max() * 8 < 2.0 ** 24
    kr.assert_fp32_exact(resid, "resid")
    for v in (A, Wp):
        assert np.array_equal(kr.round16(v, fmt), v)
    return (x, W1, b1, W2, b2), (A, Wp, bp, resid, rv)


def cur1_of(A, Wp, bp, resid, rv, rpg):
    c = resid + (A @ Wp.T + bp)
    if rv is not None:
        c = c + rv[np.arange(A.shape[0]) // rpg]
    return c


def pre_ref(x, W1, b1, W2, b2, fmt):
    """(ff, tol_ff, mag) of kernel_ref.ffn_ref for the module on x = cur1, and the added tolerance."""
    ff, tol_ff, mag = kr.ffn_ref(x, W1, b1, W2, b2, fmt)
    return ff, tol_ff + PRE_OPS * 2 * kr.U32 * (np.abs(x) + np.abs(ff)), mag


def pre_perturbed(A, Wp, kind, chunk):
    """Wp with one 32-wide K chunk dropped ("drop") or its columns rotated by 4 ("perm")."""
    W = Wp.copy()
    k0, k1 = 32 * chunk, min(32 * chunk + 32, Wp.shape[1])
    if kind == "drop":
        W[:, k0:k1] = 0.0
    else:
        W[:, k0:k1] = np.roll(Wp[:, k0:k1], 4, axis=1)
    return W
