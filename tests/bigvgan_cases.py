"""The case lists and inputs of tests/test_gpu_bigvgan_ref.py, shared with the CPU tests of the
references (tests/test_kernel_ref.py); a helper, not a test.  numpy only.

Every stream holds utterance b in rows b * Lp + [0, Lmax); rows [len, Lp) hold junk of the size of
the edge frames, so a frame read past an utterance's end (a clamp to len instead of len - 1, a
window one frame long, s <= len_in, the neighbouring utterance) changes the result by far more than
any tolerance.  Edge frames: +-EDGE in the exact classes (exact in bf16 and fp16), +-ACT_EDGE where
the values pass through the sine (|alpha y| must stay inside the general class's range)."""
import zlib

import numpy as np

import kernel_ref as kr

ACT_C = (16, 24, 96)
ACT_LMAX = [1, 2, 5, 6, 7, 8, 9, 13, 16, 17, 40]
ACT_EDGE = 6.0
CONV_C = (16, 24, 48, 64, 96, 160, 192)
CONV_KD = ((3, 1), (3, 5), (7, 3), (11, 5), (11, 1))
CONVT_UK = ((4, 8), (2, 4), (3, 7), (2, 2), (1, 3))
POST_LMAX = (1, 3, 255, 256, 257, 260)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def g32(rng, *shape):
    return r32(rng.standard_normal(shape))


def fill_stream(rng, B, Lp, C, ls, body, edge, junk):
    """(B * Lp, C): body() values in each utterance's [0, len), +-edge in its first and last frame,
    +-junk (never 0) in rows [len, Lp)."""
    x = np.zeros((B * Lp, C))
    for b in range(B):
        r0, n = b * Lp, ls[b]
        x[r0:r0 + n] = body((n, C))
        x[r0 + n:r0 + Lp] = junk * rng.choice([-1.0, 1.0], (Lp - n, C))
        if n:
            x[r0] = edge * rng.choice([-1.0, 1.0], C)
            x[r0 + n - 1] = edge * rng.choice([-1.0, 1.0], C)
    return x


# --------------------------------------------------------------------------- ACT
def act_lens(Lmax):
    """Three utterances: full, one frame, and the longest with len % 8 in {1, 7}."""
    third = max(n for n in range(1, Lmax + 1) if n % 8 in (1, 7))
    return [Lmax, 1, third]


def act_case(Lmax, C, halo, klass):
    """Lmax "scaled": lens in units of 4 frames, one of them past Lmax (the kernel's min)."""
    from oracle.bigvgan_np import anti_alias_filter
    rng = rng_for("act", Lmax, C, halo, klass)
    if Lmax == "scaled":
        Lmax, scale, lens = 13, 4, [4, 1, 2]
    else:
        scale, lens = 1, act_lens(Lmax)
    B = 3
    Lp = kr.bv_rows(Lmax, halo)
    ls = kr.bv_lens(lens, scale, Lmax, B)
    if klass == "exact":
        x = fill_stream(rng, B, Lp, C, ls, lambda s: rng.integers(-8, 9, s).astype(np.float64), kr.EDGE, 777.0)
        alpha, ibeta = np.exp(g32(rng, C) * 0.2).astype(np.float32).astype(np.float64), np.zeros(C)
        taps, f = kr.BV_TAPS_EXACT, kr.BV_TAPS_EXACT
    else:
        # away from 0 (a channel keeps one sign): next to a zero the 16-bit ulps shrink below the
        # absolute allowance of the sine term and more than one fp16 output in ten would be ambiguous
        sign = rng.choice([-1.0, 1.0], C)
        x = fill_stream(rng, B, Lp, C, ls, lambda s: r32(sign * (2.0 + 0.5 * g32(rng, *s))), ACT_EDGE, 5.0)
        la, lb = rng.uniform(-0.3, 0.3, C), rng.uniform(-0.3, 0.3, C)
        alpha = np.exp(la).astype(np.float32).astype(np.float64)
        ibeta = (1.0 / (np.exp(lb) + 1e-9)).astype(np.float32).astype(np.float64)
        taps, f = None, anti_alias_filter(2).astype(np.float32).astype(np.float64)
        if klass == "wide":      # alpha spreads max |alpha y| over the channels up to 64 turns
            ymax = kr.bv_upsample(np.abs(x), f, True).max(0)
            alpha = r32(np.geomspace(kr.BV_ARG_GENERAL, 0.999 * kr.BV_ARG_WIDE, C) / ymax)
    return dict(x=x, lens=lens, scale=scale, B=B, Lmax=Lmax, Lp=Lp, alpha=alpha, ibeta=ibeta, taps=taps, f=f)


# --------------------------------------------------------------------------- CONV
def conv_predict(C, split):
    """BvHost::gemm<SPLIT, 1>'s choice for N = C: [BM, BN, SPLIT, BK]."""
    Cp = -(-C // 32) * 32
    if Cp % 64 == 0:
        bm, bn = (256, 48) if C <= 48 else (64, 64) if C <= 64 else (128, 128)
        return [bm, bn, split, 64]
    bm, bn = (256, 32) if C <= 32 else (128, 96) if C <= 96 else (128, 128)
    return [bm, bn, split, 32]


def conv_cases(C):
    """(C, ks, d, Lmax, with residual): every (ks, d) with two of the four lengths -- M = B * Lp one
    row group below, at, and one past two tiles, and Lmax <= pad -- so that each length meets each
    parity of the list."""
    bm = conv_predict(C, 1)[0]
    cases = []
    for i, (ks, d) in enumerate(CONV_KD):
        pad = d * (ks - 1) // 2
        halo = max(8, -(-pad // 8) * 8)
        lengths = (bm - 8 - halo, bm - halo, bm + 8 - halo, max(1, min(pad, 3)))
        for v, Lmax in enumerate(lengths):
            if (i + v) % 2 == 0:
                cases.append((C, ks, d, Lmax, (i + v) % 4 < 2))
    return cases


def conv_inputs(case, klass, split, fmt):
    C, ks, d, Lmax, with_resid = case
    rng = rng_for("conv", case, klass, split, fmt)
    B = 2
    pad = d * (ks - 1) // 2
    halo = max(8, -(-pad // 8) * 8)
    Lp, Cp = kr.bv_rows(Lmax, halo), -(-C // 32) * 32
    lens = [Lmax, max(1, Lmax - 3)]
    if klass == "exact":
        a = fill_stream(rng, B, Lp, C, lens, lambda s: rng.integers(-3, 4, s).astype(np.float64), kr.EDGE, 777.0)
        w = rng.integers(-4, 5, (C, C, ks)) / 16.0
        bias = rng.integers(-8, 9, C) / 4.0
        resid = rng.integers(-64, 65, (B * Lp, C)) / 4.0
        operand = [a, np.zeros_like(a)]
    else:
        a = fill_stream(rng, B, Lp, C, lens, lambda s: g32(rng, *s), 30.0, 20.0)
        w = r32(g32(rng, C, C, ks) / np.sqrt(C * ks))
        bias, resid = g32(rng, C), g32(rng, B * Lp, C)
        operand = list(kr.split16(a, fmt)) if split == 3 else [kr.round16(a, fmt)]
        a = sum(operand)                     # the value the kernel's operand holds
    return dict(a=a, w=w, bias=bias, resid=resid if with_resid else None, operand=operand, lens=lens, B=B,
                Lmax=Lmax, Lp=Lp, Cp=Cp, C=C, ks=ks, d=d, halo=halo, M=B * Lp, pad=pad)


def needed_rows(c):
    """Rows of the (halo + M + halo)-row operand that a valid output row reads: they hold the
    activation inside an utterance and zeros outside; every other row may hold anything finite."""
    need = np.zeros(c["M"] + 2 * c["halo"], bool)
    for b in range(c["B"]):
        r0 = c["halo"] + b * c["Lp"]
        need[r0 - c["pad"]:r0 + c["lens"][b] + c["pad"]] = True
    return need


# --------------------------------------------------------------------------- CONVT
def convt_inputs(u, k, Lin, Cout, stage0):
    """stage0: input rows b * Lin (Lin_s = Lin, lens in frames); else rows b * Lp of a later stage
    (Lin_s = Lp = round_up(Lin + halo, 8), lens in units of `scale` frames with one past Lin)."""
    rng = rng_for("convt", u, k, Lin, Cout, stage0)
    B, halo, Cin = 3, 8, 40
    if stage0:
        Ls, scale, lens = Lin, 1, [Lin, 1, max(1, Lin - 1)]
    else:
        Ls, scale = kr.bv_rows(Lin, halo), 2
        lens = [Lin, 1, max(1, Lin // 2)]            # * 2: past Lin, 2, about Lin
    ls = kr.bv_lens(lens, scale, Lin, B)
    Lo = kr.bv_rows(Lin * u, halo)
    # the gather's exact class: P (B * Ls, k * Cout) of small integers, as the products of an identity
    # "weight" (k * Cout input channels, Cout outputs: eye[j * Cout + o, o, j] = 1)
    P = fill_stream(rng, B, Ls, k * Cout, ls, lambda s: rng.integers(-64, 65, s).astype(np.float64), kr.EDGE, 777.0) \
        if Ls > 0 else None
    eye = np.zeros((k * Cout, Cout, k))
    for j in range(k):
        for o in range(Cout):
            eye[j * Cout + o, o, j] = 1.0
    x = {"exact": fill_stream(rng, B, Ls, Cin, ls, lambda s: rng.integers(-3, 4, s).astype(np.float64), kr.EDGE, 777.0),
         "general": fill_stream(rng, B, Ls, Cin, ls, lambda s: g32(rng, *s), 30.0, 20.0)}
    w = {"exact": rng.integers(-4, 5, (Cin, Cout, k)) / 16.0,
         "general": r32(g32(rng, Cin, Cout, k) / np.sqrt(Cin))}
    bias = rng.integers(-8, 9, Cout) / 4.0
    return dict(B=B, halo=halo, Cin=Cin, Ls=Ls, Lo=Lo, scale=scale, lens=lens, P=P, eye=eye, x=x, w=w, bias=bias)


# --------------------------------------------------------------------------- POST
def post_inputs(Lmax, C, klass):
    rng = rng_for("post", Lmax, C, klass)
    B, Ls, scale = 3, kr.bv_rows(Lmax, 8), 1
    lens = [Lmax, 1, max(1, Lmax - 2)]
    if klass == "exact":        # pre-activations are multiples of 1/8 of magnitude up to ~ 7 C: well past +-1
        a = fill_stream(rng, B, Ls, C, lens, lambda s: rng.integers(-2, 3, s).astype(np.float64), 16.0, 777.0)
        w, bias0 = rng.integers(-2, 3, (C, 7)) / 8.0, 0.375
    else:
        a = fill_stream(rng, B, Ls, C, lens, lambda s: g32(rng, *s), 6.0, 5.0)
        w = r32(g32(rng, C, 7) / np.sqrt(7 * C))
        bias0 = float(np.float32(0.3))
    return dict(a=a, w=w, bias0=bias0, lens=lens, scale=scale, B=B, Ls=Ls)


# --------------------------------------------------------------------------- STEP
def step_inputs(C, ks, d):
    from oracle.bigvgan_np import anti_alias_filter
    rng = rng_for("step", C, ks, d)
    B, Lmax = 3, 21
    pad = d * (ks - 1) // 2
    halo = max(8, -(-pad // 8) * 8)
    Lp = kr.bv_rows(Lmax, halo)
    lens = [Lmax, 1, 15]
    x = fill_stream(rng, B, Lp, C, lens, lambda s: g32(rng, *s), 3.0, 5.0)
    c = dict(x=x, lens=lens, B=B, Lmax=Lmax, Lp=Lp, halo=halo, M=B * Lp, C=C, ks=ks, d=d,
             f=anti_alias_filter(2).astype(np.float32).astype(np.float64))
    for s in ("", "2"):
        c["alpha" + s] = np.exp(rng.uniform(-0.3, 0.3, C)).astype(np.float32).astype(np.float64)
        c["ibeta" + s] = (1.0 / (np.exp(rng.uniform(-0.3, 0.3, C)) + 1e-9)).astype(np.float32).astype(np.float64)
        c["w" + s] = r32(g32(rng, C, C, ks) / np.sqrt(C * ks))
        c["bias" + s] = r32(0.1 * g32(rng, C))
    return c
