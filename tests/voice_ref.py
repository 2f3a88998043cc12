"""numpy restatement of the voice store's kernels as include/zipvoice_hip.h defines them
(zv_prompt_rms, zv_prompt_scale, zv_voice_gather).  Written from the header, not from the kernels."""
import numpy as np

LANES = 256


def prompt_rms(x) -> np.float32:
    """rms of one row in the header's order: lane j adds the float64 squares of elements
    j, j + 256, ... in rising order from 0, the 256 partial sums are folded at widths 128, 64, ..., 1
    (p[j] += p[j + w] for j < w), then sqrt(p[0] / len) in float64, rounded once to fp32."""
    x = np.asarray(x, np.float32)
    n = x.size
    assert n >= 1
    sq = np.zeros(-(-n // LANES) * LANES, np.float64)
    sq[:n] = x.astype(np.float64) ** 2              # (exact: a 24-bit significand squared)
    p = np.zeros(LANES, np.float64)
    for row in sq.reshape(-1, LANES):               # element i = k * 256 + j reaches lane j at turn k
        p = p + row
    w = LANES // 2
    while w:
        p[:w] = p[:w] + p[w:2 * w]
        w //= 2
    return np.float32(np.sqrt(p[0] / np.float64(n)))


def gains(rms, target):
    """(gain_in, gain_out) of fp32 rms values against fp32(target), IEEE fp32 divisions."""
    rms = np.asarray(rms, np.float32)
    t = np.float32(target)
    quiet = rms < t
    one = np.ones_like(rms)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.where(quiet, t / rms, one).astype(np.float32),
                np.where(quiet, rms / t, one).astype(np.float32))


def prompt_scale(x, rms, target, ld):
    """One row: (x * fp32(target)) / rms in fp32 below the target, a copy otherwise, zeros up to ld."""
    x = np.asarray(x, np.float32)
    t, r = np.float32(target), np.float32(rms)
    out = np.zeros(ld, np.float32)
    out[:x.size] = (x * t) / r if r < t else x
    return out


def voice_gather(pool, table, T, gains_pool=None):
    """out (n, T, F): row r the pool rows [offset, offset + frames), then zeros; gains[r] =
    gains_pool[offset]."""
    pool = np.asarray(pool, np.float32)
    out = np.zeros((len(table), T, pool.shape[1]), np.float32)
    for r, (off, fr) in enumerate(table):
        out[r, :fr] = pool[off:off + fr]
    g = None if gains_pool is None else np.asarray(gains_pool, np.float32)[[off for off, _ in table]]
    return out, g
