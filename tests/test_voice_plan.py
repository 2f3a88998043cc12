"""The voice store's host side (zipvoice_amd/voices.py FrameAllocator), the numpy restatement of its
kernels (tests/voice_ref.py) and its C ABI.  No GPU.

* Allocator: first fit, neighbours merged on free, a capacity error that names the largest free range.
* voice_ref.prompt_rms follows the header's lane order in float64; against the plain float64 mean it is
  held to 1 fp32 ulp: either float64 sum of n <= 33000 exact squares is within n * 2^-53 relative of the
  true sum, far below half an fp32 ulp (2^-24), so both roots round to the same or to neighbouring
  fp32 values.
* The header declares the zv_prompt_* / zv_voice_* entries, the library exports them and the ctypes
  table lists them."""
import os
import re

import numpy as np
import pytest

import voice_ref
from zipvoice_amd.voices import FrameAllocator

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("zv_prompt_rms", "zv_prompt_scale", "zv_voice_create", "zv_voice_destroy", "zv_voice_device_bytes",
           "zv_voice_gather")


def test_allocator_fragments_and_coalesces():
    a = FrameAllocator(100)
    o = [a.alloc(n) for n in (10, 20, 30, 40)]
    assert o == [0, 10, 30, 60] and a.free_ranges() == [] and a.largest() == 0
    a.free(10)
    a.free(60)
    assert a.free_ranges() == [(10, 20), (60, 40)]             # two holes, not neighbours
    a.free(30)                                                   # joins both
    assert a.free_ranges() == [(10, 90)]
    a.free(0)
    assert a.free_ranges() == [(0, 100)] and a.largest() == 100


def test_allocator_first_fit_exact_fit_and_reuse():
    a = FrameAllocator(64)
    x, y, z = a.alloc(16), a.alloc(8), a.alloc(40)
    assert (x, y, z) == (0, 16, 24) and a.free_ranges() == []    # 64 frames: an exact fit of the rest
    a.free(y)
    assert a.alloc(8) == 16                                     # the freed range, at the same offset
    a.free(x)
    assert a.alloc(4) == 0 and a.free_ranges() == [(4, 12)]      # first fit: the lowest hole that holds it
    assert a.alloc(12) == 4


def test_allocator_capacity_error_names_the_largest_free_range():
    a = FrameAllocator(50)
    a.alloc(10), a.alloc(15), a.alloc(25)
    a.free(0)
    a.free(25)                                                   # 35 frames free, in ranges of 10 and 25
    with pytest.raises(ValueError, match=r"30 frames asked for, the largest free range has 25"):
        a.alloc(30)
    assert a.free_ranges() == [(0, 10), (25, 25)]                # a refusal changes nothing
    with pytest.raises(ValueError):
        a.free(5)                                                # no range starts there
    with pytest.raises(ValueError):
        a.alloc(0)
    with pytest.raises(ValueError):
        FrameAllocator(0)


def ulp_apart(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 33000])
def test_prompt_rms_spec_against_the_plain_mean(n):
    rng = np.random.default_rng(n)
    for amp in (0.03, 0.1, 0.3):
        x = (amp * rng.standard_normal(n)).astype(np.float32)
        got = voice_ref.prompt_rms(x)
        plain = np.float32(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
        assert got.dtype == np.float32 and ulp_apart(got, plain) <= 1, (n, amp, got, plain)
    # the order is the header's: one element per lane and turn, so a row of 256 * k equal values sums exactly
    assert voice_ref.prompt_rms(np.full(512, 0.5, np.float32)) == np.float32(0.5)


def test_gain_and_scale_spec():
    t = np.float32(0.1)
    rms = np.array([0.03, np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1)), 0.3], np.float32)
    gin, gout = voice_ref.gains(rms, 0.1)
    assert gin.dtype == gout.dtype == np.float32
    assert (gin[2:] == 1).all() and (gout[2:] == 1).all()        # at or above the target: untouched
    assert gin[0] == t / rms[0] and gout[1] == rms[1] / t and gin[1] > 1 > gout[1]
    x = np.array([0.01, -0.02, 0.03], np.float32)
    y = voice_ref.prompt_scale(x, rms[0], 0.1, 8)
    assert np.array_equal(y[:3], (x * t) / rms[0]) and (y[3:] == 0).all()
    assert np.array_equal(voice_ref.prompt_scale(x, rms[4], 0.1, 4)[:3], x)
    pool = np.arange(40, dtype=np.float32).reshape(10, 4)
    out, g = voice_ref.voice_gather(pool, [(7, 3), (0, 2), (7, 3)], 4, np.arange(10, dtype=np.float32))
    assert np.array_equal(out[0, :3], pool[7:]) and (out[0, 3] == 0).all() and np.array_equal(out[0], out[2])
    assert np.array_equal(g, [7, 0, 7])


def test_header_declares_and_library_exports_the_voice_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "zipvoice_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(zv_[a-z0-9_]+)\s*\(", src))
    from zipvoice_amd.csrc.build import build
    build(verbose=False)
    from zipvoice_amd import engine
    lib = engine.load_library()
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    # a bad call is refused on the host, before any launch: no GPU is needed to see it
    assert lib.zv_voice_gather(None, None, 1, 4, None, 1, 4, None, None, None, None) != 0
    assert "null voice handle" in lib.zv_last_error().decode()
    lens = np.array([0], np.int32)
    one = np.zeros(4, np.float32).ctypes.data
    assert lib.zv_prompt_rms(one, 4, one, lens.ctypes.data, 1, 0.1, one, one, one, None) != 0
    assert "length" in lib.zv_last_error().decode()              # a row of length 0
