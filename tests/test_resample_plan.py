"""Host side of the prompt resampler (zipvoice_amd/feature.py resample_plan): the compact
polyphase table against torchaudio's dense formula (tests/resample_ref.py), and the formula
itself against an analytic sine.  CPU only."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import resample_ref as ref  # noqa: E402
from zipvoice_amd.feature import resample_plan  # noqa: E402

RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000)
S_TABLE = {8000: 15, 11025: 15, 16000: 15, 22050: 15, 32000: 19, 44100: 25, 48000: 27, 96000: 51}
NEW = 24000


@pytest.mark.parametrize("sr", RATES)
def test_dense_and_direct_references_agree(sr):
    rng = np.random.default_rng(sr)
    for L in (1, 5, 300, 301, 1013):
        x = rng.uniform(-1, 1, L)
        a, b = ref.resample_dense(x, sr, NEW), ref.resample_direct(x, sr, NEW)
        assert a.shape == b.shape == (ref.out_len(sr, NEW, L),)
        assert np.abs(a - b).max() < 1e-12, (sr, L)


@pytest.mark.parametrize("sr", RATES + (36000,))
def test_plan_expands_to_the_dense_table(sr):
    """Scattered back to [n, 2 width + o], the plan equals torchaudio's float32 table
    wherever |t| < lw and is 0 elsewhere; every such tap lies inside the plan's window."""
    orig, new = (sr, NEW) if sr != 36000 else (NEW, 16000)
    p = resample_plan(orig, new)
    o, n, base, width = ref.reduced(orig, new)
    assert (p.o, p.n, p.width) == (o, n, width)
    assert p.start.dtype == np.int32 and p.start.shape == (n,)
    assert p.table.dtype == np.float32 and p.table.shape == (n, p.S)
    dense = ref.dense_kernel(orig, new).numpy()
    inside = (ref.dense_t(orig, new).abs() < ref.LW).numpy()
    K = dense.shape[1]
    exp = np.zeros_like(dense)
    covered = np.zeros_like(inside)
    for j in range(n):
        k = p.start[j] + width + np.arange(p.S)       # dense column of each compact tap
        ok = (k >= 0) & (k < K)
        assert not p.table[j][~ok].any()              # nothing outside torchaudio's support
        exp[j, k[ok]] = p.table[j][ok]
        covered[j, k[ok]] = True
    assert (covered | ~inside).all()
    assert np.array_equal(exp[inside], dense[inside])
    assert not exp[~inside].any()


@pytest.mark.parametrize("sr", RATES)
def test_taps_per_output(sr):
    assert resample_plan(sr, NEW).S == S_TABLE[sr]


@pytest.mark.parametrize("orig,new", [(sr, NEW) for sr in RATES] + [(NEW, 16000), (48001, NEW)])
def test_out_len_is_the_integer_ceiling(orig, new):
    p = resample_plan(orig, new)
    o, n = p.o, p.n
    for L in (1, o - 1, o, o + 1, 7 * o, 7 * o + 1):
        if L < 1:
            continue
        assert p.out_len(L) == -((-n * L) // o) == ref.out_len(orig, new, L), (orig, new, L)
    assert p.out_len(2 ** 40 + 1) == -((-n * (2 ** 40 + 1)) // o)     # no float division


def test_near_coprime_plan_is_compact():
    p = resample_plan(48001, NEW)
    assert (p.o, p.n, p.S) == (48001, 24000, 27)
    assert p.table.nbytes + p.start.nbytes < 4 << 20
    assert (np.diff(p.start) >= 0).all() and p.start[-1] - p.start[0] <= p.o


def test_create_rejects_bad_arguments_without_gpu():
    import ctypes
    from zipvoice_amd import engine
    lib = engine.load_library()
    p = resample_plan(16000, NEW)
    args = (p.start.ctypes.data_as(ctypes.c_void_p), p.table.ctypes.data_as(ctypes.c_void_p))
    assert not lib.zv_resample_create(3, 3, p.S, *args)
    assert "o == n" in lib.zv_last_error().decode()
    assert not lib.zv_resample_create(p.o, p.n, 513, *args)
    assert "S must" in lib.zv_last_error().decode()
    assert not lib.zv_resample_create(p.o, p.n, p.S, None, None)
    assert "host_start" in lib.zv_last_error().decode()
    bad = np.ascontiguousarray(p.start[::-1])
    assert not lib.zv_resample_create(p.o, p.n, p.S, bad.ctypes.data_as(ctypes.c_void_p), args[1])
    assert "non-decreasing" in lib.zv_last_error().decode()
    assert lib.zv_resample_device_bytes(None) == 0


def test_no_cpu_fallback():
    from zipvoice_amd.feature import Resample
    x = np.zeros(100, np.float32)
    assert Resample(24000, 24000)(x) is x                 # equal rates: nothing to run
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Resample(16000, NEW)(x)


@pytest.mark.parametrize("sr", RATES)
def test_reference_resamples_a_sine(sr):
    """The formula itself: a sine at 0.31 of the lower Nyquist frequency, resampled by the
    reference, is the same sine sampled at 24 kHz (within 2e-3 away from the edges)."""
    f = 0.31 * min(sr, NEW) / 2
    L = int(round(0.1 * sr))
    x = np.sin(2 * math.pi * f * np.arange(L) / sr)
    y = ref.resample_direct(x, sr, NEW)
    want = np.sin(2 * math.pi * f * np.arange(len(y)) / NEW)
    assert len(y) > 600
    assert np.abs(y - want)[200:-200].max() < 2e-3
