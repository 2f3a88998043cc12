"""Case lists and input classes of the attention kernel tests (tests/test_gpu_attn_ref.py), shared with
the host-side checks of tests/test_kernel_ref.py; a helper, not a test.  numpy only.  Every input is an
fp32 value held in float64, seeded by the case itself.

Lengths: 1 and 2; then each side of every size at which a kernel changes path: 16-query tiles, 32- and
64-key steps, 64 / 128 / 192 / 256-query blocks; 321 = six 64-key steps (one wrap of the second
generation's 3-slot ring) and two blocks of the widest form plus a ragged third.

Input classes (attn_inputs):
  onehot   indexing.  k_j = the +-1 binary code of j in dims 0..30, k_j[31] = 1; q_i = 32 code(pi(i)) in
           dims 0..30, q_i[31] = -992; p = 0.  Then s[i, j] = -64 hamming(pi(i), j): 0 at the match,
           <= -64 elsewhere (the match's weight is 1 to within 2^-55), and every operand is a value of both
           16-bit formats.  pi maps the queries into the kept keys with a stride near 0.38 of their
           number, so neighbouring queries land in different tiles, steps and blocks.  v and y are
           non-zero dyadics {+-1..+-8} / 4.  The output is exactly v[pi(i)] (NonlinAttention: y v, a
           7-bit product, exact in both formats): tolerance 0.  Why the kernels are exact on such a row:
           the match's p is 2^0 = 1, every other p is at most 2^-92 (natural units; 2^-64 in base 2), so the
           fp32 sums v + sum of (p_j v_j) and 1 + sum of p_j round to v and 1 whatever the order of the
           additions, and 1 / 1, v * 1 and the 7-bit y v are exact.
           hot_masked (first generation only): the padded keys carry k_j[31] = -1, which puts their
           unmasked scores at 1984 - 64 hamming: a kernel that adds -1000 to a padded key's score instead
           of replacing it gives those keys the whole weight.  The second generation's masks are
           additive by design (zv_flash2.inc: the MFMA chain starts from the key's bias), which equals
           the definition only while padded keys' raw scores stay far below 1000; it is not given this
           twist.
  shift    positional index.  q = k = 0, p_i = (1, 0, 0, 0), P[n, h, 0] = 0 at n = L - 1 + d_h and -64
           elsewhere, one offset d_h per head out of {0, +1, -1, +17, -(L - 1)}: s[i, j] = 0 iff
           j = i + d_h.  Rows whose target exists and is kept are one-hot; the others are uniform over the
           kept keys; both fall under the general bound (dev vanishes on the one-hot rows).
  general  Gaussian q, k, p, P at std 0.5, Gaussian v and y, rounded to the operand format (split 1).
Masks: B = 3 utterances per launch: full, len = 1 (every query returns v[0]) and a middle length (33 / 64 /
65 where L allows, else L - 1); padded keys carry v = +-1000 in every class, and in the general class the
first and last kept key of each utterance do too.  mask = False: the same inputs with key_pad = NULL."""
import zlib

import numpy as np

import kernel_ref as kr

H, QD, PD = 4, 32, 4
LDQ = 2 * H * QD + H * PD
B = 3
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 321)
GENERAL_LENGTHS = (1, 2, 17, 33, 64, 65, 129, 192, 257, 321)      # thinned (the general class only)
SHIFTS = ("0", "+1", "-1", "+17", "-(L-1)")
NA_HIDS = (384, 144, 128, 40)                                     # DTW 3, 2, 1 and a ragged last tile
SA_NV = 12
SA_NV_ODD = 5
STALE = 1000.0


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def utt_lens(L):
    """Kept keys of the three utterances: full, one, and the middle length."""
    c = [m for m in (33, 64, 65) if m < L]
    mid = c[L % len(c)] if c else max(L - 1, 1)
    return (L, 1, mid)


def key_pad(L):
    return (np.arange(L)[None, :] >= np.array(utt_lens(L))[:, None]).astype(np.uint8)


def shift_of(L, h):
    """Head h's offset d_h at length L (rotating through SHIFTS with the position of L in LENGTHS, so
    that head 0 -- the NonlinAttention head -- meets every offset)."""
    idx = LENGTHS.index(L) if L in LENGTHS else L
    return (0, 1, -1, 17, -(L - 1))[(idx + h) % 5]


def onehot_map(L, nkept, rng):
    """pi: query i -> a kept key; stride near 0.38 nkept and coprime to it, seeded start."""
    if nkept == 1:
        return np.zeros(L, np.int64)
    st = max(1, int(round(0.381966 * nkept)))
    while np.gcd(st, nkept) != 1:
        st += 1
    return (int(rng.integers(nkept)) + st * np.arange(L)) % nkept


def dyadic(rng, *shape):
    """Non-zero dyadics {+-1..+-8} / 4."""
    return rng.integers(1, 9, shape) * rng.choice([-1.0, 1.0], shape) / 4.0


def code(j):
    """The +-1 binary code of the integers j in dims 0..30."""
    return np.where((np.asarray(j)[..., None] >> np.arange(31)) & 1, 1.0, -1.0)


def attn_inputs(klass, L, kernel, nv, fmt, split=1, mask=True, hot_masked=False):
    """-> dict(qkp (B, L, LDQ), P (2L - 1, 4 H), pad (B, L) uint8 or None, v, y or None, pi or None).
    kernel "sa": v (B, L, H nv); "na": v, y (B, L, nv).  The padded keys and their +-1000 values are
    there with mask = False too (the keys then simply count)."""
    rng = rng_for("attn", klass, L, kernel, nv, fmt if klass == "general" and split == 1 else "", mask)
    lens = utt_lens(L)
    pad = key_pad(L)
    kept = lens if mask else (L,) * B
    C = H * nv if kernel == "sa" else nv
    q = np.zeros((B, L, H, QD))
    k = np.zeros((B, L, H, QD))
    p = np.zeros((B, L, H, PD))
    pi = None
    if klass == "onehot":
        P = 0.5 * rng.standard_normal((2 * L - 1, H * PD))
        pi = np.zeros((B, H, L), np.int64)
        k[..., :31] = code(np.arange(L))[None, :, None, :]
        k[..., 31] = 1.0
        if hot_masked and mask:
            k[..., 31] = np.where(pad != 0, -1.0, 1.0)[:, :, None]
        for b in range(B):
            for h in range(H):
                pi[b, h] = onehot_map(L, kept[b], rng)
                q[b, :, h, :31] = 32.0 * code(pi[b, h])
        q[..., 31] = -992.0
        v = dyadic(rng, B, L, C)
        y = dyadic(rng, B, L, C) if kernel == "na" else None
    elif klass == "shift":
        p[..., 0] = 1.0
        P = rng.choice([-1.0, 1.0], (2 * L - 1, H, PD))
        P[:, :, 0] = -64.0
        for h in range(H):
            n = L - 1 + shift_of(L, h)
            if 0 <= n <= 2 * L - 2:
                P[n, h, 0] = 0.0
        P = P.reshape(2 * L - 1, H * PD)
        v = dyadic(rng, B, L, C)
        y = dyadic(rng, B, L, C) if kernel == "na" else None
    elif klass == "general":
        q = 0.5 * rng.standard_normal(q.shape)
        k = 0.5 * rng.standard_normal(k.shape)
        p = 0.5 * rng.standard_normal(p.shape)
        P = 0.5 * rng.standard_normal((2 * L - 1, H * PD))
        v = rng.standard_normal((B, L, C))
        y = rng.standard_normal((B, L, C)) if kernel == "na" else None
        for b in range(B):
            v[b, 0] = 1000.0 * rng.choice([-1.0, 1.0], C)
            v[b, lens[b] - 1] = 1000.0 * rng.choice([-1.0, 1.0], C)
    else:
        raise ValueError(klass)
    big = 1000.0 * rng.choice([-1.0, 1.0], (B, L, C))
    v = np.where(pad[:, :, None] != 0, big, v)
    qkp = np.concatenate([q.reshape(B, L, H * QD), k.reshape(B, L, H * QD), p.reshape(B, L, H * PD)], -1)
    f32 = lambda a: None if a is None else np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    if klass == "general" and split == 1:
        r16 = lambda a: None if a is None else kr.round16(a, fmt)  # noqa: E731
        qkp, P, v, y = r16(qkp), f32(P), r16(v), r16(y)
    return dict(qkp=f32(qkp), P=f32(P), pad=pad if mask else None, v=f32(v), y=f32(y), pi=pi, lens=lens)


def onehot_expected(inp, kernel, nv):
    """The one-hot class's exact output: v[pi(i)] (times y)."""
    v, pi = inp["v"], inp["pi"]
    out = np.zeros(v.shape)
    for b in range(B):
        if kernel == "sa":
            for h in range(H):
                out[b, :, h * nv:(h + 1) * nv] = v[b, pi[b, h], h * nv:(h + 1) * nv]
        else:
            out[b] = v[b, pi[b, 0]] * inp["y"][b]
    return out


# (bug, class, length, kernel): the smallest case at which each deliberate mistake of the reference must
# fall outside the right reference's tolerance (tests/test_kernel_ref.py)
BUG_CASES = [
    ("n_off", "shift", 2, "sa"),
    ("mask_kept", "general", 2, "sa"),
    ("past_L", "general", 1, "sa"),
    ("mask_added", "onehot", 2, "sa"),
    ("utt_prev", "onehot", 1, "sa"),
    ("head_next", "shift", 2, "sa"),
    ("n_off", "shift", 2, "na"),
    ("mask_kept", "general", 2, "na"),
    ("past_L", "general", 1, "na"),
    ("mask_added", "onehot", 2, "na"),
    ("utt_prev", "onehot", 1, "na"),
    ("head_next", "shift", 2, "na"),
]
