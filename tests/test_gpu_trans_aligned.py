"""Utterance-aligned tiles with 16-byte transposed stores (csrc/zv_gemm.inc UTT tiling, store_trans8:
the counted NonlinAttention in-projection and the value projection) against the row tiles with
per-element stores they replace, ZV_TRANS_ALIGNED=1 against =0.  Same MFMA sequence per accumulator
and the same epilogue operations, so every output buffer is compared bit for bit and whole: the
canaries past the utterance's frames in [L, ldct), the guard rows, the row padding.  The launch goes
through the engine's dispatch (zv_linear_check) in both operand libraries; the launch record tells
which tiling ran (aux bit 256) and on how many blocks (one tile per block, rounded up to 8).
tests/test_gpu_linear_ref.py::test_fused_epilogues pins the same launches against float64."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRANS, NA = 6, 7
CAN16 = np.uint16(0x7FA5)
GUARD = 2
BM = 64
BN = {TRANS: 64, NA: 96}
# every residue of L mod 8, no full 8-frame group (1, 7), exactly one (8), a tile that ends at L (64),
# one row past a tile (65), two tiles and a part (203)
LENGTHS = (1, 7, 8, 9, 34, 61, 63, 64, 65, 70, 100, 203)


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    return engine.load_library(operand=request.param)


def run_linear(lib, form, split, M, L, N, K, seed):
    """One zv_linear_check call on Gaussian operands.  Returns ({name: whole raw buffer}, record)."""
    from zipvoice_amd.engine import ZvLinearCheckArgs
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K), dtype=np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N, dtype=np.float32)
    a = ZvLinearCheckArgs()
    a.M, a.N, a.K, a.split, a.form, a.act = M, N, K, split, form, 0
    a.rows_per_group, a.rpb, a.guard = 1, L, GUARD
    a.A, a.W, a.bias = A.ctypes.data, W.ctypes.data, bias.ctypes.data
    rows_t = N // 3 if form == NA else N
    a.ldc, a.ldch, a.ldct = 4, cdiv(rows_t, 8) * 8 + 8, cdiv(L, 8) * 8 + 8
    buf = lambda rows, ld: np.full((rows + 2 * GUARD, ld), CAN16, np.uint16)
    out = {"Cth": buf(rows_t * cdiv(M, L), a.ldct)}
    if split == 3:
        out["Ctl"] = buf(rows_t * cdiv(M, L), a.ldct)
    if form == NA:
        out["Ch"] = buf(M, a.ldch)
        if split == 3:
            out["Cl"] = buf(M, a.ldch)
    for name, arr in out.items():
        setattr(a, name, arr.ctypes.data)
    rc = lib.zv_linear_check(ctypes.byref(a))
    assert rc == 0, lib.zv_last_error().decode()
    return out, tuple(a.launch)


def blocks(tiles):
    return max(8, cdiv(tiles, 8) * 8)


def both_arms(lib, monkeypatch, form, split, B, L, N, K, extra_rows=0):
    """The =0 and =1 runs of one shape: whole buffers bitwise equal, each on the tiling it should use
    (extra_rows > 0: M is not whole utterances, so =1 must fall back to the row tiles)."""
    M = B * L + extra_rows
    what = f"form {form} split {split} B={B} L={L} N={N} K={K} M={M}"
    got = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("ZV_TRANS_ALIGNED", flag)
        got[flag] = run_linear(lib, form, split, M, L, N, K, seed=1000 * L + 10 * N + B)
    (ref, rec0), (out, rec1) = got["0"], got["1"]
    row_tiles = cdiv(M, BM) * cdiv(N, BN[form])
    utt_tiles = B * cdiv(L, BM) * cdiv(N, BN[form])
    aligned = extra_rows == 0 and (form == TRANS or split == 1)   # the split NA product is not counted
    assert rec0[:2] == rec1[:2] and (form == NA and split == 3 or rec0[:2] == (BM, BN[form])), (what, rec0, rec1)
    assert not rec0[7] & 256 and (form == NA and split == 3 or rec0[6] == blocks(row_tiles)), (what, rec0)
    if aligned:
        assert rec1[7] & 256 and rec1[6] == blocks(utt_tiles), (what, rec1, utt_tiles)
    else:
        assert rec1 == rec0, (what, rec0, rec1)
    for name in ref:
        assert (ref[name][GUARD:-GUARD] != CAN16).any(), f"{what}: {name} was not written at all"
        diff = int((ref[name] != out[name]).sum())
        assert diff == 0, f"{what}: {name} differs in {diff} of {ref[name].size} elements (canaries and guards included)"


@pytest.mark.parametrize("N", [16, 48, 64])
def test_value_projection_lengths(lib, monkeypatch, N):
    for L in LENGTHS:
        for B in (1, 3):
            both_arms(lib, monkeypatch, TRANS, 1, B, L, N, 64)


@pytest.mark.parametrize("N", [48, 144])
def test_na_in_projection_lengths(lib, monkeypatch, N):
    """N = 144: a half-filled second tile column (the sink for columns >= N)."""
    for L in LENGTHS:
        for B in (1, 3):
            both_arms(lib, monkeypatch, NA, 1, B, L, N, 64)


@pytest.mark.parametrize("form,split,N", [(TRANS, 2, 64), (TRANS, 3, 64), (NA, 1, 1152), (NA, 3, 144)])
def test_deep_k_and_split_products(lib, monkeypatch, form, split, N):
    """K = 512 (8 K steps), L = 97: the weight-split and the hi/lo split value projection (lo output
    too), the NonlinAttention in-projection at its real width, and the split NA product, which stays
    on the general epilogue under either setting."""
    both_arms(lib, monkeypatch, form, split, 3, 97, N, 512)


@pytest.mark.parametrize("form,N", [(TRANS, 64), (NA, 144)])
def test_partial_utterance_falls_back(lib, monkeypatch, form, N):
    """M = 2 L + 5 breaks M % rpb == 0: the row tiles run under either setting."""
    both_arms(lib, monkeypatch, form, 1, 2, 70, N, 64, extra_rows=5)


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_decoder_velocity_bitwise(monkeypatch, precision):
    """A guided velocity for three utterances of different lengths (T = 70: stacks of 70, 35 and 18
    frames) from engines built under ZV_TRANS_ALIGNED=0 and =1; bf16 and fp32 run the bf16-operand
    library, fp16 the fp16-operand one with its weight-split value projection."""
    torch = pytest.importorskip("torch")
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    from zipvoice_amd.weights import synthetic_state_dict
    cfg = default_config("zipvoice")
    sd = synthetic_state_dict(cfg, 0)
    rng = np.random.default_rng(5)
    B, T = 3, 70
    dev = "cuda:0"
    f = lambda: torch.from_numpy(rng.standard_normal((B, T, 100), dtype=np.float32)).to(dev)
    x, tc, sc = f(), f(), f()
    pm = torch.from_numpy(np.arange(T)[None] >= np.array([T, 63, 41])[:, None]).to(dev)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("ZV_TRANS_ALIGNED", flag)
        m = build_model(cfg, precision=precision)
        m.load_state_dict(sd)
        m = m.to(dev)
        outs.append(m.engine.velocity(0.4, 1.0, x, tc, sc, pm).cpu())
        del m
    assert torch.isfinite(outs[0]).all()
    d = (outs[0] - outs[1]).abs().max().item()
    print(f"{precision} decoder velocity ZV_TRANS_ALIGNED=0 vs 1: max |diff| = {d:.3e}")
    assert torch.equal(outs[0], outs[1])
