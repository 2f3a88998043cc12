"""CPU checks of the float64 kernel references (tests/kernel_ref.py) that the GPU tests
test_gpu_linear_ref.py / test_gpu_ffn_ref.py rely on: the 16-bit rounding helpers against torch,
the exact class's exactness argument, the fp32-formula error table the transcendental tolerances
come from, the FeedForward tolerance's 2 % cap, and for test_gpu_dwconv_ref.py / test_gpu_stackedge_ref.py
the conv reference against independent formulations, the exact class's exactness, SwooshR's error over
the conv's range and the ambiguity cap of every case's inputs; for test_gpu_bigvgan_ref.py the BigVGAN
references against oracle/bigvgan_np.py and torch in float64, the exact classes' exactness, the
visibility of an off-by-one at an utterance edge in every case, and the ambiguity cap."""
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


# --------------------------------------------------------------------------- depthwise conv
@pytest.mark.parametrize("B,L,C,ks", [(1, 1, 4, 7), (3, 3, 6, 7), (2, 14, 5, 31), (3, 65, 8, 15), (2, 40, 3, 63),
                                      (2, 9, 6, 5), (1, 130, 4, 9)])
def test_dwconv_ref_matches_conv1d(B, L, C, ks):
    """dwconv_ref (loops over taps) against torch's grouped conv1d in float64, one utterance at a time."""
    rng = np.random.default_rng(ks * 1000 + L)
    g, w, bias = rng.standard_normal((B * L, C)), rng.standard_normal((C, ks)), rng.standard_normal(C)
    y, u, mag = kr.dwconv_ref(g, w, bias, B, L)
    for b in range(B):
        x = torch.from_numpy(g[b * L:(b + 1) * L].T.copy())[None]            # (1, C, L)
        ref = torch.nn.functional.conv1d(x, torch.from_numpy(w)[:, None, :], torch.from_numpy(bias),
                                         padding=ks // 2, groups=C)[0].T.numpy()
        assert np.abs(u[b * L:(b + 1) * L] - ref).max() < 1e-12
        m = torch.nn.functional.conv1d(x.abs(), torch.from_numpy(np.abs(w))[:, None, :], torch.from_numpy(np.abs(bias)),
                                       padding=ks // 2, groups=C)[0].T.numpy()
        assert np.abs(mag[b * L:(b + 1) * L] - m).max() < 1e-12
    assert np.array_equal(y, kr.swoosh_r(u))


def test_dwconv_ref_matches_oracle_conv_module():
    """dwconv_ref against the oracle's ConvolutionModule conv (oracle/zipvoice_np.py, fp32) on the
    depthwise weights the golden fixtures were made with (the synthetic state dict, seed 0)."""
    from oracle.zipvoice_np import depthwise_conv1d, swoosh_r_fwd
    from zipvoice_amd.config import default_config
    from zipvoice_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(default_config("zipvoice"), 0)
    keys = sorted(k for k in sd if k.startswith("fm_decoder") and k.endswith("conv_module1.depthwise_conv.weight"))
    sizes = set()
    for k in keys:
        w3 = np.asarray(sd[k], np.float32)
        bias = np.asarray(sd[k[:-6] + "bias"], np.float32)
        C, _, ks = w3.shape
        if ks in sizes:
            continue
        sizes.add(ks)
        B, L = 2, 41
        x = np.random.default_rng(ks).standard_normal((B, L, C)).astype(np.float32)
        want = depthwise_conv1d(x, w3, bias).astype(np.float64).reshape(B * L, C)
        y, u, mag = kr.dwconv_ref(x.reshape(B * L, C).astype(np.float64), w3[:, 0].astype(np.float64),
                                  bias.astype(np.float64), B, L)
        assert (np.abs(u - want) <= (ks + 2) * 2.0 ** -23 * mag).all(), ks
        yo = swoosh_r_fwd(want.astype(np.float32)).astype(np.float64)
        assert (np.abs(y - yo) <= 0.92 * (ks + 2) * 2.0 ** -23 * mag + 2 * kr.err_swoosh_r(u)).all(), ks
    assert {7, 15, 31} <= sizes, sizes


def _dw_ref(case, fmt, klass):
    arm, ks, B, L, C, pad, split, q8 = case
    g, w, bias = kr.dwconv_inputs(B, L, C, ks, fmt, klass, split)
    y, u, mag = kr.dwconv_ref(g, w, bias, B, L)
    return g, w, bias, y, u, mag


_DW_SHAPES = sorted({c[1:5] + c[6:7] for c in kr.dwconv_cases()})     # (ks, B, L, C, split)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_dwconv_exact_class_is_exact(fmt):
    """Exact class: the operands are exact 16-bit values (in hi alone), u is exact in fp32 in any
    order (the lsb argument), and an fp32 evaluation in the reverse tap order gives the same bits."""
    for ks, B, L, C, split in _DW_SHAPES:
        g, w, bias, y, u, mag = _dw_ref(("", ks, B, L, C, 0, split, False), fmt, "exact")
        assert np.array_equal(kr.round16(g, fmt), g) and np.array_equal(w.astype(np.float32), w)
        kr.dwconv_exact_u(g, w, bias, u, mag)
        if L in (9, 65):
            acc = np.zeros((B, L, C), np.float32)
            g3 = g.reshape(B, L, C).astype(np.float32)
            for t in reversed(range(ks)):
                s = t - ks // 2
                lo, hi = max(0, -s), min(L, L - s)
                if lo < hi:
                    acc[:, lo:hi] += g3[:, lo + s:hi + s] * w[:, t].astype(np.float32)
            assert np.array_equal((acc + bias.astype(np.float32)).reshape(B * L, C).astype(np.float64), u)
    with pytest.raises(AssertionError):
        kr.dwconv_exact_u(np.array([[3.0]]), np.array([[1 / 16.0]]), np.zeros(1), np.array([[2.0 ** 18]]),
                          np.array([[2.0 ** 21]]))                # 2^25 lsb units


@pytest.mark.parametrize("klass", ["exact", "general"])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_dwconv_ambiguity_cap(fmt, klass):
    """Every stand-alone conv case's inputs, from the reference alone: at most one output in ten is
    ambiguous under check16's rule, multi-ulp ones only next to SwooshR's zeros; and the fp32 SwooshR
    formula's error over these very pre-activations stays within err_swoosh_r (exact class: multiples
    of 1/16) / err_swoosh_r_any (general class), of which the tolerance is TRANS_FACTOR times.  Measured worst ambiguous share: bf16 4.8 % (exact) /
    1.9 % (general), fp16 9.8 % (exact, ks = 31 at L = 327) / 8.5 % (general); the fp32 formula at most
    0.87 of err_swoosh_r over the exact class's |u| <= 504, 0.94 of err_swoosh_r_any over the general
    class's |u| <= 2.0e3."""
    worst, werr, umax = 0.0, 0.0, 0.0
    for ks, B, L, C, split in _DW_SHAPES:
        g, w, bias, y, u, mag = _dw_ref(("", ks, B, L, C, 0, split, False), fmt, klass)
        _, tol_y = kr.dwconv_tol(u, mag, ks, klass)
        amb, multi = kr.amb16(y, tol_y, fmt)
        worst = max(worst, kr.assert_amb_cap(amb, multi, u, tol_y, fmt, f"{fmt} {klass} k{ks} B{B} L{L} C{C}"))
        e = np.abs(kr.swoosh_r_f32(u).astype(np.float64) - kr.swoosh_r(u.astype(np.float32).astype(np.float64)))
        werr = max(werr, float((e / (kr.err_swoosh_r(u) if klass == "exact" else kr.err_swoosh_r_any(u))).max()))
        umax = max(umax, float(np.abs(u).max()))
        assert np.isfinite(kr.round16(y, fmt)).all()
    print(f"{fmt} {klass}: worst ambiguous share {100 * worst:.2f} %, fp32 SwooshR error / bound <= "
          f"{werr:.2f} over |u| <= {umax:.3g}")
    assert werr <= 1.0


def test_swoosh_r_error_over_the_conv_range():
    """err_swoosh_r on the exact class's grid out to its edge frames' range, err_swoosh_r_any on a
    dense sweep of arbitrary fp32 arguments.  Measured: 1.86 and 2.21 here (2.26 on a sweep twice as
    dense), in units of 2^-24 (|x| + 6)."""
    x = np.arange(-1100 * 64, 1100 * 64 + 1) / 64.0
    r = (np.abs(kr.swoosh_r_f32(x).astype(np.float64) - kr.swoosh_r(x)) / (kr.U32 * (np.abs(x) + 6.0))).max()
    print(f"SwooshR on multiples of 1/64, |x| <= 1100: {r:.2f}")
    assert r <= 1.9
    x = np.linspace(-9000.0, 9000.0, 4000001).astype(np.float32).astype(np.float64)
    r = (np.abs(kr.swoosh_r_f32(x).astype(np.float64) - kr.swoosh_r(x)) / (kr.U32 * (np.abs(x) + 6.0))).max()
    print(f"SwooshR on a dense sweep, |x| <= 9000: {r:.2f}")
    assert r <= 2.4


@pytest.mark.parametrize("ks", [7, 15, 31])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_glu_dw_ambiguity_cap(fmt, ks):
    """The fused launch's cases: outputs whose window holds an ambiguous GLU value count as ambiguous;
    still at most one in ten.  Measured worst share: bf16 0.5 / 0.9 / 2.2 % at ks = 7 / 15 / 31,
    fp16 2.3 / 4.3 / 8.1 %."""
    worst = 0.0
    for B, L in kr.GLU_DW_SHAPES:
        for klass in ("exact", "general"):
            ins = kr.glu_dw_inputs(B, L, ks, fmt, klass, (B, L) == kr.GLU_DW_MASKED)
            y, tol_y, u, amb, multi = kr.glu_dw_ref(*ins, B, L, fmt, klass)
            worst = max(worst, kr.assert_amb_cap(amb, multi, u, tol_y, fmt, f"{fmt} {klass} k{ks} B{B} L{L}"))
            assert np.isfinite(kr.round16(y, fmt)).all()
    print(f"{fmt} ks={ks}: worst ambiguous share {100 * worst:.2f} %")


# --------------------------------------------------------------------------- stack boundaries
def test_stackedge_refs():
    """downsample_ref / upsample_combine_ref / mask_downsample_ref against the oracle's formulation
    (pad by repeating the last frame, reshape, weighted sum; repeat and cut; [:, ::ds]), and the
    exactness of the dyadic inputs."""
    rng = np.random.default_rng(5)
    for ds in (2, 4):
        w = kr.ds_weights(ds)
        assert w.sum() == 1.0 and len(w) == ds
        for L in (1, 2, 5, 9, 64, 65):
            B, C = 2, 8
            x = rng.integers(-64, 65, (B * L, C)).astype(np.float64)
            d = kr.downsample_ref(x, w, B, L, ds, exact=True)
            dL = -(-L // ds)
            for b in range(B):
                for i in range(dL):
                    rows = [x[b * L + min(i * ds + k, L - 1)] * w[k] for k in range(ds)]
                    assert np.array_equal(d[b * dL + i], np.sum(rows, axis=0))
            sc = rng.choice([0.0, 0.25, 0.5, 1.0], C)
            out = kr.upsample_combine_ref(x, d * 4, sc, B, L, ds, exact=True)
            for b in range(B):
                for l in range(L):
                    o, u = x[b * L + l], 4 * d[b * dL + l // ds]
                    assert np.array_equal(out[b * L + l], o + (u - o) * sc)
            m = rng.integers(0, 2, B * L).astype(np.uint8)
            md = kr.mask_downsample_ref(m, B, L, ds)
            assert md.shape == (B * dL,) and all(md[b * dL + i] == m[b * L + i * ds] for b in range(B) for i in range(dL))


# --------------------------------------------------------------------------- BigVGAN references
# (tests/test_gpu_bigvgan_ref.py; case lists in tests/bigvgan_cases.py)
import bigvgan_cases as bc  # noqa: E402
from oracle import bigvgan_np as bvo  # noqa: E402

BV_F = bvo.anti_alias_filter(2).astype(np.float32).astype(np.float64)


def _torch_act(x, la, lb, f):
    """Activation1d with torch's own ops in float64: F.pad(replicate), conv_transpose1d, conv1d."""
    F = torch.nn.functional
    xt = torch.from_numpy(x.T.copy())[None]                         # (1, C, T)
    C = xt.shape[1]
    ft = torch.from_numpy(f)[None, None].expand(C, 1, 12)
    y = 2 * F.conv_transpose1d(F.pad(xt, (5, 5), mode="replicate"), ft, stride=2, groups=C)[..., 15:-15]
    y = y + (1.0 / (torch.exp(torch.from_numpy(lb)) + 1e-9))[:, None] * torch.sin(y * torch.exp(torch.from_numpy(la))[:, None]) ** 2
    z = F.conv1d(F.pad(y, (5, 6), mode="replicate"), ft, stride=2, groups=C)
    return z[0].numpy().T


@pytest.mark.parametrize("T", [1, 2, 3, 5, 6, 7, 20])
def test_bv_act_ref_matches_oracle_and_torch(T):
    rng = np.random.default_rng(T)
    C = 5
    x, la, lb = rng.standard_normal((T, C)), rng.uniform(-0.3, 0.3, C), rng.uniform(-0.3, 0.3, C)
    z, _ = kr.bv_act_ref(x, None, 1, 1, T, T, np.exp(la), 1.0 / (np.exp(lb) + 1e-9), BV_F)
    assert np.abs(z - bvo.activation1d_snakebeta(x.T, la, lb, BV_F).T).max() < 1e-13
    assert np.abs(z - _torch_act(x, la, lb, BV_F)).max() < 1e-13


def test_bv_filter_ref_is_the_polyphase_form_of_the_upsampler():
    """The 6 + 6 coefficients, derived from impulse responses, reproduce the transposed convolution
    inside a signal; the fp32 taps are anti_alias_filter(2) rounded once."""
    rng = np.random.default_rng(3)
    for f in (BV_F, kr.BV_TAPS_EXACT):
        r = kr.bv_filter_ref(f)
        x = rng.standard_normal((30, 1))
        y = kr.bv_upsample(x, f)[:, 0]
        for t in range(3, 26):
            assert np.isclose(y[2 * t], sum(r[m] * x[t + m - 3, 0] for m in range(6)), atol=1e-13)
            assert np.isclose(y[2 * t + 1], sum(r[6 + m] * x[t + m - 2, 0] for m in range(6)), atol=1e-13)
        assert np.array_equal(r[12:], f)
    assert np.abs(BV_F - bvo.anti_alias_filter(2)).max() <= 2.0 ** -25 * np.abs(BV_F).max() * 2


@pytest.mark.parametrize("ks,d", bc.CONV_KD)
def test_bv_conv_ref_matches_oracle_and_torch(ks, d):
    rng = np.random.default_rng(ks * 10 + d)
    C, Co = 6, 4
    for n in (1, 2, 9):
        a = kr.round16(rng.standard_normal((n, C)), "bf16")
        w = kr.round16(rng.standard_normal((Co, C, ks)), "bf16")
        bias = rng.standard_normal(Co)
        pad = d * (ks - 1) // 2
        got = kr.bv_conv_ref(a, w, bias, d, None, 1, 1, n, n, 1, "bf16")[0]
        assert np.abs(got - bvo.conv1d(a.T, w, bias, d, pad).T).max() < 1e-12
        t = torch.nn.functional.conv1d(torch.from_numpy(a.T.copy())[None], torch.from_numpy(w),
                                       torch.from_numpy(bias), dilation=d, padding=pad)[0].numpy().T
        assert np.abs(got - t).max() < 1e-12


@pytest.mark.parametrize("u,k", bc.CONVT_UK)
def test_bv_convt_ref_matches_oracle_and_torch(u, k):
    rng = np.random.default_rng(u * 10 + k)
    Cin, Co = 5, 3
    for n in (1, 2, 5):
        x, w, bias = rng.standard_normal((n, Cin)), rng.standard_normal((Cin, Co, k)), rng.standard_normal(Co)
        Lo = kr.bv_rows(n * u, 8)
        got = kr.bv_convt_ref(x, w, bias, u, None, 1, 1, n, n, Lo)[0]
        assert (got[n * u:] == 0).all()
        assert np.abs(got[:n * u] - bvo.conv_transpose1d(x.T, w, bias, u, (k - u) // 2).T).max() < 1e-12
        t = torch.nn.functional.conv_transpose1d(torch.from_numpy(x.T.copy())[None], torch.from_numpy(w),
                                                 torch.from_numpy(bias), stride=u, padding=(k - u) // 2)[0].numpy().T
        assert np.abs(got[:n * u] - t).max() < 1e-12


def test_bv_post_and_im2col_refs_match_torch():
    rng = np.random.default_rng(9)
    C = 4
    for n in (1, 3, 10):
        a, w = rng.standard_normal((n, C)), rng.standard_normal((C, 7))
        got = kr.bv_post_ref(a, w, 0.25, None, 1, 1, n, n, 0)[0]
        t = torch.nn.functional.conv1d(torch.from_numpy(a.T.copy())[None], torch.from_numpy(w)[None], padding=3)[0, 0]
        assert np.abs(got - np.clip(t.numpy() + 0.25, -1, 1)).max() < 1e-13
        assert np.abs(kr.bv_post_ref(a, w, 0.25, None, 1, 1, n, n, 1)[0] - np.tanh(t.numpy() + 0.25)).max() < 1e-13
        # im2col . W == conv1d, in both layouts
        for layout in (0, 1):
            x = rng.standard_normal((1, C, n) if layout == 0 else (1, n, C))
            A = kr.im2col_ref(x, layout, 0.5, -1.0, None, 1, n, C, 7)[0]
            wc = rng.standard_normal((3, C, 7))
            v = (x[0] if layout == 0 else x[0].T) / 0.5 + 1.0
            want = bvo.conv1d(v, wc, None, 1, 3).T
            assert np.abs(A @ np.concatenate([wc[:, :, t] for t in range(7)], 1).T - want).max() < 1e-12


def _visible(true, bugged, tol, valid, what):
    """A deliberate off-by-one differs from the reference by >= 1000 tolerances (>= 1 where the
    class is exact) on some valid output."""
    diff = np.abs(true - bugged)[valid]
    lim = np.maximum(1000 * tol[valid], 1e-30)
    assert (diff >= np.where(tol[valid] > 0, lim, 1.0)).any(), f"{what}: the edge mistake is invisible"


@pytest.mark.parametrize("C", bc.ACT_C)
@pytest.mark.parametrize("Lmax", bc.ACT_LMAX + ["scaled"])
def test_bv_act_cases(Lmax, C):
    """Exactness of the exact class (asserted inside the reference), visibility of a clamp to len and
    of the neighbouring utterance's frame, and the ambiguity cap of the 16-bit operand."""
    for halo in (8, 32):
        for klass in ("exact", "general"):
            c = bc.act_case(Lmax, C, halo, klass)
            a = (c["x"], c["lens"], c["scale"], c["B"], c["Lmax"], c["Lp"], c["alpha"], c["ibeta"], c["f"], klass)
            z, tol = kr.bv_act_ref(*a)
            valid = np.zeros(z.shape, bool)
            for b, n in enumerate(kr.bv_lens(c["lens"], c["scale"], c["Lmax"], c["B"])):
                valid[b * c["Lp"]:b * c["Lp"] + n] = True
            assert (z[~valid] == 0).all() and valid.any()
            for bug in ("clamp", "neighbour"):
                _visible(z, kr.bv_act_ref(*a, bug=bug)[0], tol, valid, f"ACT {klass} {bug} Lmax={Lmax} halo={halo}")
            if klass == "general":
                assert np.abs(c["alpha"] * kr.bv_upsample(np.abs(c["x"]), c["f"], True)).max() <= kr.BV_ARG_GENERAL
                w = bc.act_case(Lmax, C, halo, "wide")
                top = np.abs(w["alpha"] * kr.bv_upsample(np.abs(w["x"]), w["f"], True)).max()
                assert 0.9 * kr.BV_ARG_WIDE <= top <= kr.BV_ARG_WIDE
                for fmt in ("bf16", "f16"):
                    assert kr.amb16(z[valid], tol[valid], fmt)[0].mean() <= kr.AMB_CAP


@pytest.mark.parametrize("C", bc.CONV_C)
def test_bv_conv_cases(C):
    seen = set()
    for case in bc.conv_cases(C):
        for klass in ("exact", "general"):
            c = bc.conv_inputs(case, klass, 1, "bf16")
            a = (c["a"], c["w"], c["bias"], c["d"], c["lens"], 1, c["B"], c["Lmax"], c["Lp"], 1, "bf16", c["resid"], klass)
            ref, tol, valid = kr.bv_conv_ref(*a)           # (the exact class asserts its exactness)
            bug = kr.bv_conv_ref(*a[:-1], "general", bug="neighbour")[0]
            _visible(ref, bug, tol, np.repeat(valid[:, None], C, 1), f"CONV {klass} {case}")
        seen.add((case[1], case[2]))
        M = 2 * kr.bv_rows(case[3], c["halo"])
        seen.add(("M", np.sign(M - 2 * bc.conv_predict(C, 1)[0]) if case[3] > 3 else "short"))
    assert seen >= set(bc.CONV_KD) | {("M", -1), ("M", 0), ("M", 1), ("M", "short")}


@pytest.mark.parametrize("u,k", bc.CONVT_UK)
def test_bv_convt_cases(u, k):
    for Lin in (1, 2, 5):
        for stage0 in (True, False):
            c = bc.convt_inputs(u, k, Lin, 8, stage0)
            a = (c["bias"], u, c["lens"], c["scale"], c["B"], Lin, c["Ls"], c["Lo"])
            ref, _ = kr.bv_convt_ref(c["P"], c["eye"], *a, klass="exact")
            bug, _ = kr.bv_convt_ref(c["P"], c["eye"], *a, bug="le")
            # (k = u: frame len_in lands on outputs t >= len_in * u only, which the kernel zeroes anyway)
            edge = k > u and c["Ls"] > min(kr.bv_lens(c["lens"], c["scale"], Lin, c["B"]))
            if edge:
                assert np.abs(ref - bug).max() >= 1.0, f"CONVT u={u} k={k} Lin={Lin}: s <= len_in is invisible"
            for klass in ("exact", "general"):
                r, t = kr.bv_convt_ref(c["x"][klass], c["w"][klass], *a, 1, "bf16", klass)
                b = kr.bv_convt_ref(c["x"][klass], c["w"][klass], *a, 1, "bf16", "general", bug="le")[0]
                if edge:
                    _visible(r, b, t, t >= 0, f"CONVT {klass} u={u} k={k} Lin={Lin} stage0={stage0}")


@pytest.mark.parametrize("Lmax", bc.POST_LMAX)
def test_bv_post_cases(Lmax):
    for klass in ("exact", "general"):
        c = bc.post_inputs(Lmax, 16, klass)
        a = (c["a"], c["w"], c["bias0"], c["lens"], c["scale"], c["B"], Lmax, c["Ls"])
        for use_tanh in (0, 1):
            ref, tol = kr.bv_post_ref(*a, use_tanh, klass)
            bug = kr.bv_post_ref(*a, use_tanh, "general", bug="short")[0]
            if Lmax > 1 and use_tanh:              # (the clamp can hide a difference past +-1)
                _visible(ref, bug, tol, np.ones(ref.shape, bool), f"POST {klass} Lmax={Lmax}")


def test_bv_step_reference_composes():
    c = bc.step_inputs(24, 3, 1)
    ref, tol, valid = kr.bv_step_ref(c, 3, "bf16")
    # against the oracle's own composition on the first utterance, in float64 without operand rounding
    n = c["Lmax"]
    x = c["x"][:n].T
    la, lb = np.log(c["alpha"]), np.log(1.0 / c["ibeta"] - 1e-9)
    t = bvo.activation1d_snakebeta(x, la, lb, c["f"])
    t = bvo.conv1d(t, c["w"], c["bias"], 1, 1)
    t = bvo.activation1d_snakebeta(t, np.log(c["alpha2"]), np.log(1.0 / c["ibeta2"] - 1e-9), c["f"])
    want = (bvo.conv1d(t, c["w2"], c["bias2"], 1, 1) + x).T
    assert np.abs(ref[:n] - want).max() < 1e-3 and (np.abs(ref[:n] - want) <= 50 * tol[:n] + 1e-4).all()
    assert valid.sum() == sum(c["lens"]) and (tol[valid] > 0).all()


# --------------------------------------------------------------------------- solve-boundary references
# (tests/test_gpu_solve_ref.py; inputs and case lists in tests/solve_cases.py)
import solve_cases as sc  # noqa: E402
from oracle import zipvoice_np as zvo  # noqa: E402


def _differs(true, bugged, tol, what):
    """A mutant differs from the true reference by more than the tolerance (exact class: at all) on the
    GPU test's own inputs."""
    d = np.abs(np.asarray(true, np.float64) - np.asarray(bugged, np.float64))
    assert (d > np.asarray(tol) * np.ones_like(d)).any(), f"{what}: the mistake is invisible"


def test_solve_fp32_formula_errors():
    """The measured constants of the solve-boundary tolerances: cos / sin up to 60 rad, SwooshR in the
    logaddexp form over the small linear's inputs, the positional angle chain over every test's L and D."""
    a = np.linspace(-60.0, 60.0, 400001).astype(np.float32)
    e = max(np.abs(np.cos(a).astype(np.float64) - np.cos(a.astype(np.float64))).max(),
            np.abs(np.sin(a).astype(np.float64) - np.sin(a.astype(np.float64))).max())
    print(f"cos / sin: {e / kr.U32:.2f} * 2^-24")
    assert e <= kr.ERR_SINCOS
    x = np.concatenate([np.linspace(-40.0, 40.0, 200001), 2.0 * np.random.default_rng(0).standard_normal(100000)])
    x = x.astype(np.float32).astype(np.float64)
    r = (np.abs(kr.swoosh_r_lae_f32(x).astype(np.float64) - kr.swoosh_r(x)) / kr.err_swoosh_r_lae(x)).max()
    print(f"SwooshR (logaddexp form): {1.7 * r:.2f} * 2^-24 * (|x| + 2)")
    assert r <= 1.0
    worst = 0.0
    for L, D in sorted({(c[0], c[3]) for c in sc.POSP}):
        xs, xa = kr.posp_angle(L, D)
        worst = max(worst, (np.abs(kr.posp_angle_f32(L, D).astype(np.float64) - xa) / kr.err_posp_angle(xs, D)).max())
    print(f"posP angle: {1.5 * worst:.2f} * err_posp_angle's unit")
    assert worst <= 1.0


def test_solve_refs_match_the_oracle():
    """The references against oracle/zipvoice_np.py's restatement of the model (fp32) and its index rule."""
    for T, tl, fl, S in sc.TEXT_COND:
        assert np.array_equal(kr.tokens_index(fl, tl, T), zvo.get_tokens_index(np.asarray(fl), np.asarray(tl), T))
    for L, D in ((1, 2), (5, 48), (65, 64)):
        assert np.abs(kr.posp_table(L, D)[0] - zvo.rel_pos_table(L, D)).max() < 1e-5
    for dim in sc.TEMB_DIMS:
        t = np.array([0.0, 0.5, 1.0, 3.0])
        ref, _ = kr.temb_ref(t, kr.temb_freqs(dim), dim)
        assert np.abs(ref - zvo.timestep_embedding(t.astype(np.float32), dim)).max() < 1e-6
    # the doubled batch as the oracle's velocity() builds it
    x, tc, s = sc.build_inputs(10, 10, 5)
    B, T = sc.BUILD_B, 5
    for zs in (0, 1):
        want = np.concatenate([np.concatenate([x, np.zeros_like(tc), np.zeros_like(s) if zs else s], 1),
                               np.concatenate([x, tc, s], 1)], 0)
        assert np.array_equal(kr.build_input_ref(x, tc, s, B, T, 2, zs), want)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_solve_build_input_mutants_visible(fmt):
    for Fx, Ft, ld in sc.BUILD_SHAPES:
        for T in sc.BUILD_T:
            x, tc, s = sc.build_inputs(Fx, Ft, T)
            for zs in (0, 1):
                ref = kr.build_input_ref(x, tc, s, sc.BUILD_B, T, 2, zs)
                hi, lo = kr.split16(ref, fmt)
                for bug in ("swap", "text_kept", "speech_flip", "boundary"):
                    _differs(hi, kr.split16(kr.build_input_ref(x, tc, s, sc.BUILD_B, T, 2, zs, bug=bug), fmt)[0], 0.0,
                             f"build {bug} ({Fx}, {Ft}) T={T} zs={zs}")
                _differs(lo, np.zeros_like(lo), 0.0, "build: the lo half dropped")
            ref1 = kr.build_input_ref(x, tc, s, sc.BUILD_B, T, 1, 0)
            _differs(ref1, kr.build_input_ref(x, tc, s, sc.BUILD_B, T, 1, 0, bug="boundary"), 0.0, "build boundary, one copy")


@pytest.mark.parametrize("klass", ["exact", "general"])
@pytest.mark.parametrize("T", sc.EULER_T)
def test_solve_euler_mutants_visible(T, klass):
    per_row = T * sc.EULER_FX
    x, v, g, dt = sc.euler_inputs(T, klass)
    ex = klass == "exact"
    for mode, grows, gmul in sc.EULER_MODES:
        cfg = int(mode != "nocfg")
        vk = v if cfg else v[:x.shape[0]]
        for xin in (x, None) if cfg else (x,):
            ref, tol = kr.euler_ref(xin, vk, cfg, g, dt, grows, gmul, per_row, exact=ex)
            bugs = (["dt_sign"] if xin is not None else []) + (["swap"] if cfg else [])
            bugs += ["prev_row"] if grows is not None else []
            bugs += ["gmul"] if grows is not None and gmul != 1.0 else []
            for bug in bugs:
                _differs(ref, kr.euler_ref(xin, vk, cfg, g, dt, grows, gmul, per_row, bug=bug)[0], tol, f"euler {mode} {bug}")


def test_solve_temb_mutants_visible():
    for dim in sc.TEMB_DIMS:
        for M in (1, 3):
            for which in ("t", "g"):
                t = sc.temb_t(M, which)
                if not t.any():
                    continue
                ref, tol = kr.temb_ref(t, kr.temb_freqs(dim), dim)
                _differs(ref, kr.temb_ref(t, kr.temb_freqs(dim), dim, bug="halves")[0], tol, f"temb halves dim={dim}")
                if dim >= 6:
                    _differs(ref, kr.temb_ref(t, kr.temb_freqs(dim, 2 * (dim // 2)), dim, bug="freq_index")[0], tol,
                             f"temb freq_index dim={dim}")


@pytest.mark.parametrize("M,N,K,pre,bias,add", sc.SMALL_LINEAR)
def test_solve_small_linear_mutants_visible(M, N, K, pre, bias, add):
    for klass in (("exact", "general") if not pre else ("general",)):
        x, W, b, a = sc.small_linear_inputs(M, N, K, pre, bias, add, klass)
        ref, tol = kr.small_linear_ref(x, W, b, a, pre, exact=klass == "exact")
        bugs = (["no_bias"] if bias else []) + (["no_add"] if add else []) + (["tail"] if N % 32 > 1 else [])
        for bug in bugs:
            _differs(ref, kr.small_linear_ref(x, W, b, a, pre, bug=bug)[0], tol, f"small linear {bug} {klass}")
        # a condition on the reference: the tolerance stays far below the outputs' scale
        if klass == "general":
            assert np.median(tol) <= 1e-3 * max(np.abs(ref).mean(), 1e-3) * (8 if K > 4096 else 1)


@pytest.mark.parametrize("L,nl,HPD,D", sc.POSP)
def test_solve_posp_mutants_visible(L, nl, HPD, D):
    for klass, shifts in (("onehot", sc.posp_shifts(nl, HPD, D)), ("general", (0,))):
        seen = set()
        for sh in shifts:
            W = sc.posp_weights(L, nl, HPD, D, klass, sh)
            ref, tol = kr.posp_ref(W, L, nl, HPD, D)
            bugs = ["offset", "interleave", "no_one", "one_at_D-2"] + (["mirror"] if L > 1 and D > 2 else [])   # D = 2: cos alone, even in x
            bugs += ["prev_layer"] if nl > 1 and (klass == "general" or HPD % D) else []
            for bug in bugs:
                d = np.abs(ref - kr.posp_ref(W, L, nl, HPD, D, bug=bug)[0])
                if (d > tol).any():
                    seen.add(bug)
            want = set(bugs)
        assert seen == want, f"posP {klass} L={L} D={D}: invisible {want - seen}"


def test_solve_text_side_mutants_visible():
    for C in sc.TEXT_C:
        vis = set()
        for T, tl, fl, S in sc.TEXT_COND:
            emb = sc.table(len(tl), S, C)
            ref = kr.text_cond_ref(emb, tl, fl, T)
            for bug in ("no_clamp", "clamp_low", "d_from_T", "d0_token0"):
                if (ref != kr.text_cond_ref(emb, tl, fl, T, bug=bug)).any():
                    vis.add(bug)
        assert vis == {"no_clamp", "clamp_low", "d_from_T", "d0_token0"}, vis
        for T, Tp, plen in sc.SPEECH_COND:
            pf = sc.table(len(plen), Tp, C) + 1.0
            ref = kr.speech_cond_ref(pf, plen, T)
            _differs(ref, kr.speech_cond_ref(pf, plen, T, bug="le"), 0.0, "speech t <= plen")
            if T > Tp:
                _differs(ref, kr.speech_cond_ref(pf, plen, T, bug="no_tp"), 0.0, "speech t < Tp missing")


# ---------------------------------------------------------------------------------------------
# attention (kernel_ref's section "attention", tests/attn_cases.py, tests/test_gpu_attn_ref.py)
# ---------------------------------------------------------------------------------------------
import attn_cases as ac  # noqa: E402


def test_attn_exp2_error_table():
    """numpy's fp32 exp2 against float64 over the softmax's range (the yardstick ERR_EXP2 that the
    attention tolerances take TRANS_FACTOR times)."""
    x = np.linspace(-140.0, 24.0, 400001).astype(np.float32)
    got = np.exp2(x).astype(np.float64)
    ref = np.exp2(x.astype(np.float64))
    ok = ref >= 2.0 ** -126
    r = (np.abs(got - ref)[ok] / ref[ok]).max() / kr.U32
    print(f"exp2: {r:.2f} * 2^-24 relative")
    assert r <= kr.ERR_EXP2 / kr.U32


def _sa_weights(inp, fmt, base="e"):
    for b in range(ac.B):
        q, k, p = kr.attn_heads(inp["qkp"][b], ac.H)
        for h in range(ac.H):
            w, _, _ = kr.attn_weights_ref([kr.round16(q[h], fmt)], [kr.round16(k[h], fmt)], kr.round16(p[h], fmt),
                                          inp["P"][:, h * ac.PD:(h + 1) * ac.PD],
                                          None if inp["pad"] is None else inp["pad"][b], base)
            yield b, h, w


@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("L", ac.LENGTHS)
def test_attn_onehot_construction(L, mask):
    """Every case of the list: the match's weight is at least 1 - 2^-50 (in both units, with and without
    the padded keys' raised scores), pi stays inside the kept keys, and every operand of the one-hot and
    shift classes is a value of both 16-bit formats."""
    for hot in (False, True):
        inp = ac.attn_inputs("onehot", L, "sa", ac.SA_NV, "bf16", mask=mask, hot_masked=hot)
        for fmt in ("bf16", "f16"):
            for name in ("qkp", "v"):
                assert np.array_equal(kr.round16(inp[name], fmt), inp[name]), (name, fmt)
        for base in ("e", "2"):
            for b, h, w in _sa_weights(inp, "bf16", base):
                pi = inp["pi"][b, h]
                assert pi.max() < (inp["lens"][b] if mask else L)
                assert w[np.arange(L), pi].min() >= 1.0 - 2.0 ** -50, (b, h)
    na = ac.attn_inputs("onehot", L, "na", 40, "bf16", mask=mask)
    prod = na["v"] * na["y"]
    sh = ac.attn_inputs("shift", L, "sa", ac.SA_NV, "bf16", mask=mask)
    kr.assert_fp32_exact(prod)       # NonlinAttention's y v is one exact fp32 product, then rounded once
    for fmt in ("bf16", "f16"):
        for name in ("qkp", "P", "v"):
            assert np.array_equal(kr.round16(sh[name], fmt), sh[name]), (name, fmt)
    # the shift class's rows: one-hot on j = i + d where that key exists and is kept, else uniform
    for b, h, w in _sa_weights(sh, "bf16"):
        d = ac.shift_of(L, h)
        nk = sh["lens"][b] if mask else L
        for i in range(L):
            if 0 <= i + d < nk:
                assert w[i, i + d] >= 1.0 - 2.0 ** -50
            else:
                assert np.allclose(w[i, :nk], 1.0 / nk, rtol=1e-12)


def test_attn_dev_bound_against_perturbation():
    """The bounds of the section comment against brute force: weights perturbed by relative errors up to
    E, at random and at the worst signs; a shared denominator is bounded through dev, a denominator with
    errors of its own through mag."""
    rng = np.random.default_rng(5)
    worst = [0.0, 0.0]
    for trial in range(200):
        n, E = int(rng.integers(1, 40)), float(rng.choice([1e-6, 2.0 ** -9, 0.05, 0.3]))
        w = rng.random(n) ** 4
        w /= w.sum()
        v = rng.standard_normal(n) * rng.choice([1.0, 1000.0], n)
        out = w @ v
        dev, mag = w @ np.abs(v - out), w @ np.abs(v)
        for k in range(6):
            e = E * (np.sign(v - out) * (1 if k == 0 else -1) if k < 2 else rng.uniform(-1, 1, n))
            got = (w * (1 + e)) @ v / (w * (1 + e)).sum()
            bound = E / (1 - E) * dev
            assert abs(got - out) <= bound + 1e-13 * mag       # (+ this test's own float64 noise)
            if bound > 1e-9 * mag:
                worst[0] = max(worst[0], abs(got - out) / bound)
            e2 = E * (np.sign(v) * np.sign(out) * -1 if k == 0 else rng.uniform(-1, 1, n))
            got = (w * (1 + e)) @ v / (w * (1 + e2)).sum()
            bound = 2 * E / (1 - E) * mag
            assert abs(got - out) <= bound + 1e-13 * mag       # (+ this test's own float64 noise)
            if bound > 1e-9 * mag:
                worst[1] = max(worst[1], abs(got - out) / bound)
    print(f"worst |out' - out| / bound: shared {worst[0]:.3f}, separate {worst[1]:.3f}")
    assert worst[0] > 0.9            # the dev bound is attained (not slack the kernels could hide in)


@pytest.mark.parametrize("case", ac.BUG_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_attn_classes_see_each_bug(case):
    """Each deliberate mistake of the reference falls outside the right reference's tolerance on at least
    one element of its smallest case, in both operand formats (first-generation 16-bit forms; the one-hot
    class at tolerance 0)."""
    bug, klass, L, kernel = case
    nv = ac.SA_NV if kernel == "sa" else 40
    form = "sa1" if kernel == "sa" else "na1"
    for fmt in ("bf16", "f16"):
        inp = ac.attn_inputs(klass, L, kernel, nv, fmt, hot_masked=True)
        args = (form, fmt, inp["qkp"], inp["P"], inp["pad"], inp["v"], inp["y"], ac.H, nv)
        ref, tol = kr.attn_consumer_ref(*args)
        if klass == "onehot":
            assert np.array_equal(ref, ac.onehot_expected(inp, kernel, nv))
            tol = np.zeros_like(tol)
        wrong, _ = kr.attn_consumer_ref(*args, bug=bug, tol=False)
        bad, worst = kr.attn_accept(kr.round16(wrong, fmt), ref, tol, fmt)
        print(f"{case} [{fmt}]: {int(bad.sum())} of {bad.size} elements outside, worst {worst:.3g} x the allowance")
        assert bad.any()
        ok, _ = kr.attn_accept(kr.round16(ref, fmt), ref, tol, fmt)
        assert not ok.any()
