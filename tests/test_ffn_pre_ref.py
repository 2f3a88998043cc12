"""Conditions on the pre-projection reference itself (tests/ffn_pre_ref.py), on the CPU: the
inputs land where they must, and a dropped or permuted 32-wide K chunk of the pre-projection is
far outside the tolerance the GPU test allows (tests/test_gpu_ffn_pre_ref.py)."""
import numpy as np
import pytest

import ffn_pre_ref as pr
import kernel_ref as kr


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("K", [48, 560, 656])
def test_pre_inputs_and_wrong_k_order(fmt, K):
    M, H, rpg = 129, 192, 7
    (x, W1, b1, W2, b2), (A, Wp, bp, resid, rv) = pr.pre_inputs(M, H, K, fmt, rpg, seed=K)
    cur1 = pr.cur1_of(A, Wp, bp, resid, rv, rpg)
    assert np.array_equal(cur1, x) and np.abs(x).max() <= 3 and np.array_equal(x, np.rint(x))
    assert np.array_equal(kr.round16(cur1, fmt), cur1)
    ff, tol_ff, mag = pr.pre_ref(x, W1, b1, W2, b2, fmt)
    ref, tol, _ = kr.ffn_epilogue(ff, tol_ff, mag, cur1)
    for kind in ("drop", "perm"):
        for chunk in (0, (K - 1) // 32):
            Wb = pr.pre_perturbed(A, Wp, kind, chunk)
            c_bad = pr.cur1_of(A, Wb, bp, resid, rv, rpg)
            assert (c_bad != cur1).mean() > 0.5
            # what a kernel with that K order would give: the module on round16 of the wrong cur1
            h = kr.round16(kr.swoosh_l(kr.round16(c_bad, fmt) @ W1.T + b1), fmt)
            bad = c_bad + (h @ W2.T + b2)
            ratio = np.abs(bad - ref) / tol
            print(f"{fmt} K={K} {kind} chunk {chunk}: median |err| / tol = {np.median(ratio):.0f}")
            assert np.median(ratio) > 10
