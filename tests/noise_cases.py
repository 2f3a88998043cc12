"""Cases and helpers the seeded-noise tests share (tests/test_noise_spec.py without a GPU,
tests/test_gpu_noise.py on one): the Random123 known answers, the counter-carry case, the edge
words of the Box-Muller step, and zv_noise_check through ctypes (where 0: the library's host
functions, where 1: the same source on the device)."""
import ctypes

import numpy as np

import noise_ref

# Random123 kat_vectors, philox4x32-10: (counter, key, words)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
CARRY = ((0xffffffff, 0, 7, 0), (0x12345678, 0x9abcdef0), 3)      # counter, key, blocks
X1_EDGES = (0, 0x3fffffff, 0x40000000, 0x7fffffff, 0x80000000, 0xffffffff)


def lib_bits(counter, key, nblocks, where=0):
    from zipvoice_amd import engine
    lib = engine.load_library()
    out = np.zeros((nblocks, 4), np.uint32)
    a = engine.ZvNoiseCheckArgs(mode=0, where=where, count=nblocks, bits=out.ctypes.data)
    a.counter[:] = counter
    a.key[:] = key
    assert lib.zv_noise_check(ctypes.byref(a)) == 0, lib.zv_last_error().decode()
    return out


def lib_normals(words, where=0):
    from zipvoice_amd import engine
    lib = engine.load_library()
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, 4)
    out = np.full(w.shape, np.nan, np.float32)
    a = engine.ZvNoiseCheckArgs(mode=1, where=where, count=len(w), words=w.ctypes.data,
                                normals=out.ctypes.data)
    assert lib.zv_noise_check(ctypes.byref(a)) == 0, lib.zv_last_error().decode()
    return out


def edge_words():
    """Quadruples that put every edge word in both pair positions: x0 in {0, 0xffffffff, a
    generic word} against every quadrant edge of x1."""
    quads = []
    for x0 in (0, 0xffffffff, 0x12345678):
        for x1 in X1_EDGES:
            quads.append((x0, x1, 0x9abcdef0, 0x0badcafe))
            quads.append((0x9abcdef0, 0x0badcafe, x0, x1))
    return np.array(quads, np.uint32)


def check_normals(got, words):
    """got (m, 4) fp32 against the float64 reference within 16 * 2^-24 * (1 + r); returns the
    largest fraction of the bound reached."""
    z, r = noise_ref.box_muller(words)
    frac = np.abs(got.astype(np.float64) - z) / (noise_ref.TOL * (1.0 + r))
    assert np.isfinite(got).all() and frac.max() <= 1.0, (frac.max(), words[frac.max(1).argmax()])
    # u = 1 (x = 0xffffffff in the radius position): the radius is 0 and z exactly 0
    for p in (0, 2):
        dead = words[:, p] == 0xffffffff
        assert dead.any() and (got[dead][:, p:p + 2] == 0.0).all()
    return float(frac.max())
