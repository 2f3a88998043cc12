"""Case lists and inputs of the solve-boundary kernel tests (tests/test_gpu_solve_ref.py), shared with
the host-side visibility checks of tests/test_kernel_ref.py; a helper, not a test.  numpy only.
Every input is an fp32 value held in float64, seeded by the case itself."""
import zlib

import numpy as np


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def gauss(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


# ---- build input: (Fx, Ft, ld): scalar form, quad form, stereo shape, the model's shape, and quad widths
# on a row stride that is no multiple of 4 (the policy's other way into the scalar form)
BUILD_SHAPES = [(10, 10, 33), (12, 12, 40), (24, 12, 64), (100, 100, 320), (12, 12, 37)]
BUILD_T = (1, 5)
BUILD_B = 2


def build_quad(Fx, Ft, ld):
    return Fx % 4 == 0 and Ft % 4 == 0 and ld % 4 == 0


def build_inputs(Fx, Ft, T, B=BUILD_B):
    """The three sources from disjoint ranges: x ~ N(0, 1), text 300 + N(0, 1), speech -300 + N(0, 1)."""
    rng = rng_for("build", Fx, Ft, T, B)
    f = lambda w, off: (off + rng.standard_normal((B * T, w))).astype(np.float32).astype(np.float64)
    return f(Fx, 0.0), f(Ft, 300.0), f(Fx, -300.0)


# ---- Euler / combine: B = 3 rows of per_row = T * 10 values (70: one block; 370: row boundaries inside
# blocks, a partial last block); guidance modes
EULER_B, EULER_FX = 3, 10
EULER_T = (7, 37)
EULER_GROWS = (0.0, 3.0, -0.5)
EULER_MODES = [("nocfg", None, 1.0), ("scalar", None, 1.0), ("rows", EULER_GROWS, 1.0), ("rows", EULER_GROWS, 2.0)]


def euler_inputs(T, klass, n=None):
    """(x, v (2 n), g, dt): exact: integers in [-8, 8], g = 1.5, dt = 1/8; general: Gaussian."""
    n = EULER_B * T * EULER_FX if n is None else n
    rng = rng_for("euler", T, klass, n)
    if klass == "exact":
        return (rng.integers(-8, 9, n).astype(np.float64), rng.integers(-8, 9, 2 * n).astype(np.float64), 1.5, 0.125)
    return gauss(rng, n), gauss(rng, 2 * n), float(np.float32(0.7)), float(np.float32(0.0371))


# ---- timestep embedding
TEMB_DIMS = (192, 6, 7)
TEMB_T = {1: [0.5], 3: [0.0, 2.0 ** -20, 1.0]}          # M -> t; plus the guidance-sized row below
TEMB_G = [0.3, 1.7, 3.0]


def temb_t(M, which):
    t = TEMB_T[M] if which == "t" else TEMB_G[:M]
    return np.asarray(t, np.float32).astype(np.float64)


# ---- small linear: (M, N, K, pre, bias, add): every K and N edge of the issue; add "out": add == out
SMALL_LINEAR = [
    (1, 1, 1, 0, True, None), (3, 31, 63, 0, True, "sep"), (1, 32, 64, 0, False, "sep"), (3, 33, 65, 0, True, None),
    (1, 512, 192, 0, True, "out"), (3, 512, 384, 0, False, None), (3, 33, 8192, 0, True, "sep"), (1, 31, 8193, 0, True, "sep"),
    (3, 1, 192, 0, False, "sep"), (1, 33, 1, 0, True, "out"), (3, 32, 63, 0, False, None),
    (1, 1, 1, 1, True, None), (3, 31, 63, 1, True, "sep"), (1, 32, 64, 1, False, None), (3, 33, 65, 1, True, "sep"),
    (3, 512, 192, 1, True, None), (1, 512, 384, 1, True, "sep"), (1, 33, 8192, 1, True, None), (3, 31, 8193, 1, False, "sep"),
    (3, 1, 384, 1, True, "out"), (1, 31, 65, 1, False, "out"),
]


def small_linear_inputs(M, N, K, pre, bias, add, klass):
    """exact (pre 0): x in {-3..3}, W in {-4..4}/16, bias and add multiples of 1/16: sum |x w| <= 12 K / 16,
    below 2^24 / 16 for every K here.  general: Gaussian x (scaled by 2 under SwooshR), W ~ N(0, 1 / K)."""
    rng = rng_for("small_linear", M, N, K, pre, bias, add, klass)
    if klass == "exact":
        x, W = rng.integers(-3, 4, (M, K)).astype(np.float64), rng.integers(-4, 5, (N, K)) / 16.0
        b = rng.integers(-64, 65, N) / 16.0 if bias else None
        a = rng.integers(-64, 65, (M, N)) / 16.0 if add else None
    else:
        x = gauss(rng, M, K) * (2.0 if pre else 1.0)
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32).astype(np.float64)
        b = gauss(rng, N) if bias else None
        a = gauss(rng, M, N) if add else None
    return x, W, b, a


# ---- posP: (L, nl, HPD, D); every L of the issue with both nl, HPD and the D list spread over them
POSP = [(1, 1, 16, 2), (1, 3, 5, 48), (2, 3, 16, 6), (2, 1, 5, 64), (3, 1, 16, 48), (3, 3, 5, 2), (64, 3, 16, 64),
        (64, 1, 5, 6), (65, 1, 16, 6), (65, 3, 5, 64), (1219, 3, 16, 48), (1219, 1, 5, 2), (1219, 1, 16, 64)]


def posp_shifts(nl, HPD, D):
    """The one-hot class's weight sets: together their rows hit every column of the table."""
    return range(0, D, nl * HPD)


def posp_weights(L, nl, HPD, D, klass, shift=0):
    """one-hot: row r = l HPD + c is the unit vector of column (r + shift) mod D; general: Gaussian."""
    if klass == "onehot":
        W = np.zeros((nl * HPD, D))
        r = np.arange(nl * HPD)
        W[r, (r + shift) % D] = 1.0
        return W
    return gauss(rng_for("posp", L, nl, HPD, D), nl * HPD, D)


# ---- the text side: tables with unique fp32-exact values 1000 b + 10 s + c / 16
TEXT_C = (5, 100)


def table(B, S, C):
    b, s, c = np.meshgrid(np.arange(B), np.arange(S), np.arange(C), indexing="ij")
    return 1000.0 * b + 10.0 * s + c / 16.0


# (T, tok_lens, feat_lens, S): the issue's batch (no remainder, remainder, d = 0, S_b = 1 in a row shorter
# than T), and a row so short that its left-over frames outlast another whole duration (the clamp's case)
TEXT_COND = [(23, (7, 3, 6, 1), (21, 23, 4, 20), 8), (23, (2, 3), (6, 23), 8)]
# (T, Tp, prompt_lens): Tp below and above T; prompt_len 0, Tp and beyond T
SPEECH_COND = [(9, 5, (0, 5, 12, 3)), (5, 9, (0, 9, 12, 3))]
