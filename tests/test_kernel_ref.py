"""CPU checks of the float64 kernel references (tests/kernel_ref.py) that the GPU tests
test_gpu_linear_ref.py / test_gpu_ffn_ref.py rely on: the 16-bit rounding helpers against torch,
the exact class's exactness argument, the fp32-formula error table the transcendental tolerances
come from, and the FeedForward tolerance's 2 % cap."""
import numpy as np
import pytest

import kernel_ref as kr

torch = pytest.importorskip("torch")

TDT = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_round16_matches_torch(fmt):
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-12, 12, 200000))).astype(np.float32)
    # exact ties (odd multiples of half an ulp) and values around the fp16 subnormal range
    p = kr.PREC[fmt]
    ties = (2 * rng.integers(2 ** p, 2 ** (p + 1), 4096) + 1) * 2.0 ** -(p + 1)
    small = rng.standard_normal(4096) * 2.0 ** -15
    x = np.concatenate([x, ties.astype(np.float32), -ties.astype(np.float32), small.astype(np.float32),
                        np.float32([0.0, 1.0, -1.0, 65504.0, 3.0e4])])
    want = torch.from_numpy(x).to(TDT[fmt]).to(torch.float64).numpy()
    got = kr.round16(x.astype(np.float64), fmt)
    assert np.array_equal(got, want)
    # the bit decoder inverts torch's encoding
    bits = torch.from_numpy(x).to(TDT[fmt]).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(kr.decode16(bits, fmt), want)
    # hi / lo pair as the engine forms it: fp32 subtraction, then a second rounding
    hi, lo = kr.split16(x.astype(np.float64), fmt)
    th = torch.from_numpy(x).to(TDT[fmt])
    tl = (torch.from_numpy(x) - th.float()).to(TDT[fmt])
    assert np.array_equal(hi, th.to(torch.float64).numpy())
    assert np.array_equal(lo, tl.to(torch.float64).numpy())


def test_exact_class_is_exact_in_fp32_blas_order():
    """A 300 x 200 x 1920 integer-operand fp32 matmul (BLAS's own summation order) equals the
    float64 product exactly, as assert_exact_dot promises for any order."""
    rng = np.random.default_rng(1)
    A = rng.integers(-3, 4, (300, 1920)).astype(np.float64)
    W = rng.integers(-4, 5, (200, 1920)) / 64.0
    ref = kr.assert_exact_dot(A, W)
    got = A.astype(np.float32) @ W.astype(np.float32).T
    assert np.array_equal(got.astype(np.float64), ref)
    kr.assert_fp32_exact(ref + rng.integers(-16, 17, 200) / 8.0)


def test_exactness_assertions_bite():
    rng = np.random.default_rng(2)
    A = rng.integers(-2047, 2048, (8, 1920)).astype(np.float64)
    W = rng.integers(-64, 65, (8, 1920)).astype(np.float64)
    with pytest.raises(AssertionError):
        kr.assert_exact_dot(A, W)                      # sum |products| past 2^24
    with pytest.raises(AssertionError):
        kr.assert_fp32_exact(np.array([1.0 + 2.0 ** -30]))
    with pytest.raises(AssertionError):                # an epilogue step that is not exact
        kr.std_epilogue(np.array([[2.0 ** 20]]), np.array([2.0 ** -10]), exact=True)
    assert kr._lsb(np.array([0.75, 3.0, 0.0])) == 0.25


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_split_operand_lo_is_exact(fmt):
    """An operand of p + 3 significant bits has a non-zero lo half and hi + lo == the value, so
    against an operand that is exact in hi alone the dropped lo lo term is zero."""
    p = kr.PREC[fmt]
    rng = np.random.default_rng(3)
    m = 2 * rng.integers(2 ** (p + 1), 2 ** (p + 2), 4096) + 1       # odd, p + 3 bits
    x = m * 2.0 ** -(p + 2)
    hi, lo = kr.split16(x, fmt)
    assert np.array_equal(hi + lo, x) and (lo != 0).all()
    n = rng.integers(-3, 4, 4096).astype(np.float64)
    _, lo = kr.split16(n, fmt)
    assert (lo == 0).all()


def test_fp32_formula_error_table():
    """The measured error of the kernels' formulas in fp32 numpy against float64 (the table the
    transcendental tolerances are 4x of)."""
    x = np.arange(-120 * 64, 120 * 64 + 1) / 64.0
    e = np.abs(kr.swoosh_l_f32(x).astype(np.float64) - kr.swoosh_l(x))
    r = (e / (kr.U32 * (np.abs(x) + 6.0))).max()
    print(f"SwooshL: {r:.2f} * 2^-24 * (|x| + 6)")
    assert r <= 2.2
    e = np.abs(kr.swoosh_r_f32(x).astype(np.float64) - kr.swoosh_r(x))
    r = (e / (kr.U32 * (np.abs(x) + 6.0))).max()
    print(f"SwooshR: {r:.2f} * 2^-24 * (|x| + 6)")
    assert r <= 1.9
    xs = np.arange(-40 * 256, 40 * 256 + 1) / 256.0
    r = np.abs(kr.tanh_f32(xs).astype(np.float64) - np.tanh(xs)).max() / kr.U32
    print(f"tanh: {r:.2f} * 2^-24")
    assert r <= 3.0
    r = np.abs(kr.sigmoid_f32(xs).astype(np.float64) - kr.sigmoid(xs)).max() / kr.U32
    print(f"sigmoid: {r:.2f} * 2^-24")
    assert r <= 1.5
    assert np.isfinite(kr.swoosh_l_f32(x)).all()


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("H", [64, 192, 1536])
def test_ffn_tolerance_cap(fmt, H):
    """Every output's FeedForward tolerance stays below 2 % of the RMS of the FeedForward
    contribution (a condition on the reference, not a measurement of the kernel), and a dropped
    32-wide hidden chunk is far outside it."""
    x, W1, b1, W2, b2, resid = kr.ffn_inputs(129, H, fmt, seed=H)
    ff, tol, mag = kr.ffn_ref(x, W1, b1, W2, b2, fmt)
    _, tol, _ = kr.ffn_epilogue(ff, tol, mag, resid)
    rms = np.sqrt((ff * ff).mean())
    worst = tol.max() / rms
    u = x @ W1.T + b1
    h = kr.round16(kr.swoosh_l(u), fmt)
    drop = np.abs(h[:, :32] @ W2[:, :32].T)
    print(f"{fmt} H={H}: max tol / rms(ff) = {100 * worst:.2f} %, dropped chunk / tol: median "
          f"{np.median(drop / tol):.0f}x")
    assert worst < 0.02
    assert np.median(drop / tol) > 10
