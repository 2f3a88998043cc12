"""zv_noise_normal on the GPU (zipvoice_amd/csrc/zv_noise.inc; definition in
include/zipvoice_hip.h) against the numpy restatement tests/noise_ref.py.

* The uint32 layer on the device is bit-exact: the Random123 known answers and the counter carry.
* The normals agree with the float64 reference within 16 * 2^-24 * (1 + r) per element, r that
  element's float64 radius.  The bound is derived, not measured: log, sqrt, the trigonometric
  function, the two products and the argument 2 pi u each contribute a few fp32 units in the last
  place, and the argument error enters scaled by r.  Every case prints the largest fraction of the
  bound it reaches.  Shapes: B = 3, n in {1, 3, 4, 5, 1023, 37 * 100}, ld in {n, n + 1, n + 7},
  the base 0 and 1 float off a 16-byte boundary, streams NULL and (0, 1, 2^31 - 1), seeds 0, 1,
  2^63 and 2^64 - 1: the 16-byte store path, the row tail, rows whose base is unaligned because of
  the stride or of the base, and more than one workgroup per row.  Everything outside [0, n) of
  each row is pre-filled with a pattern and must keep it, bit for bit.
* Invariance, bitwise: a row's values do not depend on B, the row's position, the stride, the
  alignment, the row's length, the call, or the operand build of the library.
* A warm call makes no host-blocking runtime call.
Indices are 64-bit in the kernel; an element index past 2^31 needs an 8 GiB row and is not run
here (the carry into the counter's second word is reached through the bits mode instead)."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import noise_ref  # noqa: E402
from noise_cases import CARRY, KAT, check_normals, edge_words, lib_bits, lib_normals  # noqa: E402
from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.noise import seeded_normal, seeded_normal_into  # noqa: E402

PATTERN = 0x7fc0beef                     # a NaN payload no draw produces
PAD = 16                                 # floats kept around the rows
SEED_SETS = ((0, 1, 1 << 63), ((1 << 64) - 1, 1234, 1 << 63))
STREAMS = (None, (0, 1, (1 << 31) - 1))
NS = (1, 3, 4, 5, 1023, 37 * 100)


def twos(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


@functools.lru_cache(maxsize=None)
def ref_row(seed, stream):
    """(z, r) float64 of the longest row the tests draw; shorter rows are its prefixes."""
    return noise_ref.normal(seed, stream, max(NS), with_radius=True)


def fill(seeds, streams, n, ld=None, off=0, lib=None):
    """One zv_noise_normal call into a pattern-filled buffer whose first row starts `off` floats
    past a 16-byte boundary -> (rows (B, n) fp32, untouched: everything else kept the pattern)."""
    lib = lib or engine.load_library()
    B, ld = len(seeds), n if ld is None else ld
    buf = torch.full((PAD + off + B * ld + PAD,), PATTERN, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    base = PAD + off
    sd = torch.tensor([twos(s, 64) for s in seeds], dtype=torch.int64, device="cuda")
    st = None if streams is None else torch.tensor([twos(s, 32) for s in streams],
                                                   dtype=torch.int32, device="cuda")
    rc = lib.zv_noise_normal(engine._ptr(sd), engine._ptr(st), B, n, ld,
                             ctypes.c_void_p(buf.data_ptr() + 4 * base), engine._stream())
    assert rc == 0, lib.zv_last_error().decode()
    host = buf.cpu().numpy()
    written = np.zeros(host.shape, bool)
    for b in range(B):
        written[base + b * ld:base + b * ld + n] = True
    rows = np.stack([host[base + b * ld:base + b * ld + n] for b in range(B)]).view(np.float32)
    return rows, bool((host[~written] == PATTERN).all())


def test_bits_on_device():
    for counter, key, want in KAT:
        assert lib_bits(counter, key, 1, where=1)[0].tolist() == list(want)
    counter, key, nb = CARRY
    assert np.array_equal(lib_bits(counter, key, nb, where=1), noise_ref.philox_blocks(counter, key, nb))
    # more blocks than one workgroup, across the carry: the host functions are the same source
    assert np.array_equal(lib_bits((0xfffffe00, 5, 7, 9), key, 1000, where=1),
                          lib_bits((0xfffffe00, 5, 7, 9), key, 1000, where=0))


def test_normals_on_device_edge_words():
    words = edge_words()
    frac = check_normals(lib_normals(words, where=1), words)
    print(f"device normals, edge words: largest fraction of the bound {frac:.3f}")


@pytest.mark.parametrize("n", NS)
def test_normals_against_float64(n):
    worst = 0.0
    for seeds in SEED_SETS:
        for streams in STREAMS:
            refs = [ref_row(s, 0 if streams is None else streams[b]) for b, s in enumerate(seeds)]
            z = np.stack([r[0][:n] for r in refs])
            rad = np.stack([r[1][:n] for r in refs])
            for ld in (n, n + 1, n + 7):
                for off in (0, 1):
                    got, untouched = fill(seeds, streams, n, ld, off)
                    assert untouched, (n, ld, off)
                    assert np.isfinite(got).all()
                    frac = np.abs(got.astype(np.float64) - z) / (noise_ref.TOL * (1.0 + rad))
                    worst = max(worst, float(frac.max()))
                    assert frac.max() <= 1.0, (n, ld, off, seeds, streams, float(frac.max()))
    print(f"n = {n}: largest fraction of the bound 16 * 2^-24 * (1 + r) reached: {worst:.3f}")


def test_invariance_bitwise():
    n, key = 37 * 100, ((1 << 63) + 5, 77)
    alone, ok = fill([key[0]], [key[1]], n)
    assert ok
    alone = alone[0].view(np.int32)
    # row 2 of B = 3, and row 0
    assert np.array_equal(fill([3, 4, key[0]], [0, 1, key[1]], n)[0][2].view(np.int32), alone)
    assert np.array_equal(fill([key[0], 3, 4], [key[1], 0, 1], n)[0][0].view(np.int32), alone)
    # stride and alignment (row 2 at ld = n + 7 and at ld = n + 1 is unaligned by its stride)
    for ld, off in ((n + 7, 0), (n + 1, 0), (n, 1), (n + 7, 1)):
        got, ok = fill([3, 4, key[0]], [0, 1, key[1]], n, ld, off)
        assert ok and np.array_equal(got[2].view(np.int32), alone), (ld, off)
    # a (20, 100) draw is the first 20 * 100 elements of the (37, 100) draw, tail path included
    for m in (20 * 100, 20 * 100 + 3):
        assert np.array_equal(fill([key[0]], [key[1]], m)[0][0].view(np.int32), alone[:m])
    # the same call twice
    assert np.array_equal(fill([key[0]], [key[1]], n)[0][0].view(np.int32), alone)
    # the fp16-operand build of the library
    f16 = engine.load_library(operand="f16")
    assert f16 is not engine.load_library()
    for off in (0, 1):
        assert np.array_equal(fill([key[0]], [key[1]], n, off=off, lib=f16)[0][0].view(np.int32), alone)
    # streams NULL is stream 0
    assert np.array_equal(fill([key[0]], None, n)[0], fill([key[0]], [0], n)[0])
    # other keys give other noise
    assert not np.array_equal(fill([key[0] + 1], [key[1]], n)[0][0].view(np.int32), alone)
    assert not np.array_equal(fill([key[0]], [key[1] + 1], n)[0][0].view(np.int32), alone)


def test_python_layer_matches_the_entry():
    seeds, streams = [0, (1 << 64) - 1, 1 << 63], [5, 0, (1 << 31) - 1]
    want, _ = fill(seeds, streams, 37 * 100)
    x = seeded_normal(seeds, (37, 100), streams)
    assert x.shape == (3, 37, 100) and x.dtype == torch.float32 and x.is_cuda
    assert np.array_equal(x.cpu().numpy().reshape(3, -1).view(np.int32), want.view(np.int32))
    assert torch.equal(seeded_normal(seeds[:1], (37, 100)), seeded_normal(seeds[:1], 3700, [0]).view(1, 37, 100))
    # rows of an existing tensor, strided: the columns beside them stay
    buf = torch.full((3, 40, 100), 7.0, device="cuda")
    out = seeded_normal_into(buf[:, :37], seeds, streams)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf[:, :37], x) and (buf[:, 37:] == 7.0).all()
    with pytest.raises(ValueError):
        seeded_normal_into(buf[:, :, :50], seeds)                 # rows are not contiguous
    assert seeded_normal([1], (0, 100)).shape == (1, 0, 100)


def test_no_host_block():
    lib = engine.load_library()
    B, T, F = 4, 300, 100
    sd = torch.arange(B, dtype=torch.int64, device="cuda")
    out = torch.empty((B, T, F), device="cuda")
    args = (engine._ptr(sd), None, B, T * F, T * F, engine._ptr(out), engine._stream())
    assert lib.zv_noise_normal(*args) == 0                        # warm
    torch.cuda.synchronize()
    before = engine.host_block_count()
    assert lib.zv_noise_normal(*args) == 0
    assert engine.host_block_count() == before
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
