"""The row padding mode's kernels (csrc/zv_elem.inc zv_row_len_kernel, zv_downsample_row_kernel), launched
as zv_engine launches them (zv_padrow_check), against the float64 restatement tests/padrow_ref.py, in both
operand libraries.

Input classes and bounds are those of tests/test_gpu_stackedge_ref.py's downsample: "exact" (small
integers, dyadic weights, +-1000 in every utterance's edge frames: every product and partial sum is an
fp32 value, asserted by the restatement) compares bit for bit; "general" (Gaussian) allows one rounding
per product and per addition, 2 ds u sum_k |w[k] x|.  In the exact class the frames past a row's end hold
+-4096, so a group that read past the end is off by hundreds.

The lengths are exact: masks cover n = 1, L, L - 1, a length of the form k ds + 1, and a mask with a hole
before its last unmasked frame; a fully masked row gives L.  With every length L the output is bit for bit
zv_stackedge_check(ZV_SE_DOWNSAMPLE)'s on the same input.  The length table and the output lie between
canary-filled guards, which must come back intact."""
import ctypes
import zlib

import numpy as np
import pytest

import kernel_ref as kr
import padrow_ref as pr

pytestmark = pytest.mark.gpu

CAN32 = np.uint32(0x7FC5A5A5)
GUARD = 2
B = 3


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return request.param, engine.load_library(operand=request.param)


def run(lib, mask, x, w, L, C, ds):
    """One zv_padrow_check call: (lengths (B) int32, out (B * dL, C) as float64, launch record)."""
    from zipvoice_amd.engine import ZvPadrowCheckArgs
    dL = -(-L // ds)
    a = ZvPadrowCheckArgs()
    a.B, a.L, a.C, a.ds, a.guard = B, L, C, ds, GUARD
    m = np.ascontiguousarray(mask, np.uint8)
    xf, wf = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32)
    assert np.array_equal(xf.astype(np.float64), x) and np.array_equal(wf.astype(np.float64), w)
    lens = np.full(B + 2 * GUARD, CAN32, np.uint32)
    out = np.full((B * dL + 2 * GUARD, C), CAN32, np.uint32)
    a.mask, a.x, a.w, a.lens, a.out = m.ctypes.data, xf.ctypes.data, wf.ctypes.data, lens.ctypes.data, out.ctypes.data
    rc = lib.zv_padrow_check(ctypes.byref(a))
    assert rc == 0, lib.zv_last_error().decode()
    assert (lens[:GUARD] == CAN32).all() and (lens[GUARD + B:] == CAN32).all(), "length table: guards written"
    assert (out[:GUARD] == CAN32).all() and (out[GUARD + B * dL:] == CAN32).all(), "output: guard rows written"
    return (lens[GUARD:GUARD + B].view(np.int32).copy(),
            out[GUARD:GUARD + B * dL].view(np.float32).astype(np.float64), list(a.launch))


def stackedge_downsample(lib, x, w, L, C, ds):
    from zipvoice_amd.engine import ZvStackedgeCheckArgs
    dL = -(-L // ds)
    a = ZvStackedgeCheckArgs()
    a.kind, a.B, a.L, a.C, a.ds, a.guard, a.rows_per_group = 0, B, L, C, ds, GUARD, 1
    xf, wf = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32)
    out = np.full((B * dL + 2 * GUARD, C), CAN32, np.uint32)
    a.x, a.w, a.out = xf.ctypes.data, wf.ctypes.data, out.ctypes.data
    assert lib.zv_stackedge_check(ctypes.byref(a)) == 0, lib.zv_last_error().decode()
    return out[GUARD:GUARD + B * dL].copy()


def masks(L, ds):
    """[(name, mask (B, L), lengths)]: between them n = 1, L, L - 1, k ds + 1, a hole and a fully masked row."""
    def prefix(lens):
        return (np.arange(L)[None, :] >= np.array(lens)[:, None]).astype(np.uint8)
    kds1 = ((L - 1) // ds) * ds + 1                # the largest k ds + 1 <= L ...
    if kds1 == L and L > ds:
        kds1 -= ds                                 # ... below L where L allows (the clamp then acts inside the row)
    sets = [("prefix", prefix([L, max(L - 1, 1), 1]), [L, max(L - 1, 1), 1]),
            ("kds1", prefix([kds1, L, min(2, L)]), [kds1, L, min(2, L)])]
    hole = prefix([L, max(L - 1, 1), L])
    hole[0, : max(L - 1, 0)] = 1                   # row 0: only its last frame is free -> L
    if L > 2:
        hole[1, 0] = 1                             # row 1: a hole at the front, length still L - 1
    hole[2, :] = 1                                 # row 2: fully masked -> L
    sets.append(("hole", hole, [L, max(L - 1, 1), L]))
    return sets


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


CASES = [(ds, L, C) for ds in (2, 4) for L in (1, 2, 5, 9, 64, 65) for C in (512, 384)]


@pytest.mark.parametrize("ds,L,C", CASES)
def test_row_lengths_and_downsample(lib, ds, L, C):
    fmt, Lb = lib
    dL = -(-L // ds)
    figs = []
    for name, mask, want_lens in masks(L, ds):
        assert pr.row_lengths(mask.reshape(-1), B, L).tolist() == want_lens, "the test's own masks"
        for klass in ("exact", "general"):
            rng = rng_for("padrow", ds, L, C, name, klass)
            if klass == "exact":
                x = kr.put_edges(rng.integers(-64, 65, (B * L, C)).astype(np.float64), B, L, rng)
                x3 = x.reshape(B, L, C)
                for b, n in enumerate(want_lens):  # the row's own edge frame at its end, +-4096 past it
                    x3[b, n - 1] = 1000.0 * rng.choice([-1.0, 1.0], C)
                    x3[b, n:] = 4096.0 * rng.choice([-1.0, 1.0], (L - n, C))
                w = kr.ds_weights(ds)
            else:
                x = rng.standard_normal((B * L, C)).astype(np.float32).astype(np.float64)
                w = np.exp(rng.standard_normal(ds).astype(np.float32).astype(np.float64))
                w = (w / w.sum()).astype(np.float32).astype(np.float64)
            lens, out, rec = run(Lb, mask, x, w, L, C, ds)
            assert lens.tolist() == want_lens, (name, lens.tolist(), want_lens)
            assert rec[1:3] == [B, 64] and rec[4] == 256, rec
            ref = pr.downsample_row_ref(x, w, want_lens, B, L, ds, exact=klass == "exact")
            err = np.abs(out - ref)
            if klass == "exact":
                assert np.array_equal(out, ref), f"{name}: {int((out != ref).sum())} values differ, max {err.max()}"
            else:                                  # ds products and ds additions, one rounding each
                mag = pr.downsample_row_ref(np.abs(x), np.abs(w), want_lens, B, L, ds)
                assert (err <= 2 * ds * kr.U32 * mag).all(), f"{name}: max |err| {err.max()}"
            figs.append(float(err.max()))
    print(f"{fmt} ds={ds} L={L} C={C}: max |err| per (mask, class) = {figs}")


@pytest.mark.parametrize("ds,L,C", CASES)
def test_full_lengths_are_the_batch_kernel(lib, ds, L, C):
    """Every n_b = L (nothing masked, and a fully masked batch): bit for bit zv_downsample_kernel."""
    fmt, Lb = lib
    rng = rng_for("padrow-full", ds, L, C)
    x = rng.standard_normal((B * L, C)).astype(np.float32).astype(np.float64)
    w = np.exp(rng.standard_normal(ds).astype(np.float32).astype(np.float64))
    w = (w / w.sum()).astype(np.float32).astype(np.float64)
    want = stackedge_downsample(Lb, x, w, L, C, ds)
    for fill in (0, 1):
        lens, out, _ = run(Lb, np.full((B, L), fill, np.uint8), x, w, L, C, ds)
        assert lens.tolist() == [L] * B
        assert np.array_equal(out.astype(np.float32).view(np.uint32), want), f"mask of {fill}s"
