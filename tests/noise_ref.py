"""Numpy restatement of the seeded-noise function of include/zipvoice_hip.h (zv_noise_normal):
Philox4x32-10 in uint64 arithmetic (the uint32 words are the bit-exact layer), u in fp32 as the
definition rounds it, the radius and the trigonometric functions in float64 (the reference the
device's fp32 normals are held to, within 16 * 2^-24 * (1 + r))."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TOL = 16 * 2.0 ** -24          # |z - z_ref| <= TOL * (1 + r)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> (..., 4) uint32."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                  # 32 x 32 -> 64 bit products
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_blocks(counter, key, nblocks):
    """`nblocks` consecutive blocks from a start counter of four uint32: the 64-bit number
    (counter[0] low, counter[1] high) counts up, words 2 and 3 stay -> (nblocks, 4) uint32."""
    lo = (int(counter[0]) | (int(counter[1]) << 32)) + np.arange(nblocks, dtype=np.uint64)
    return philox4x32_10((lo & MASK, lo >> S32, np.uint64(counter[2]), np.uint64(counter[3])), key)


def unit(x):
    """u(x) = fl32(fl32(x) * 2^-32 + 2^-33), in (0, 1]."""
    return np.asarray(x, np.uint32).astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)


def box_muller(words):
    """(..., 4) uint32 -> ((..., 4) float64 normals z0..z3, (..., 4) float64 radius of each)."""
    w = np.asarray(words, np.uint32)
    u = unit(w).astype(np.float64)
    assert u.min() > 0.0 and u.max() <= 1.0
    r = np.sqrt(-2.0 * np.log(u[..., 0::2]))           # r(u(x0)), r(u(x2))
    a = 2.0 * np.pi * u[..., 1::2]
    z = np.stack([r[..., 0] * np.sin(a[..., 0]), r[..., 0] * np.cos(a[..., 0]),
                  r[..., 1] * np.sin(a[..., 1]), r[..., 1] * np.cos(a[..., 1])], axis=-1)
    return z, np.repeat(r, 2, axis=-1)


def normal(seed, stream, n, with_radius=False):
    """Elements 0 .. n-1 of the row keyed (seed, stream), float64."""
    seed, nblk = int(seed), (int(n) + 3) // 4
    w = philox_blocks((0, 0, int(stream) & 0xFFFFFFFF, 0), (seed & 0xFFFFFFFF, seed >> 32), nblk)
    z, r = box_muller(w)
    z, r = z.reshape(-1)[:n], r.reshape(-1)[:n]
    return (z, r) if with_radius else z
