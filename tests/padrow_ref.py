"""Float64 restatement of the row padding mode (ZV_PAD_ROW, include/zipvoice_hip.h): the rows'
lengths from the key padding mask (csrc/zv_elem.inc zv_row_len_kernel) and the downsample that pads
every row with its own last frame (zv_downsample_row_kernel).  No reference counterpart as a batch
operation: the definition is "what SimpleDownsample (zipformer.py:887-913) gives for the row alone",
which tests/test_padrow_ref.py checks against kernel_ref.downsample_ref row by row."""
import numpy as np

import kernel_ref as kr


def row_lengths(mask, B, L):
    """n[b] = 1 + the last l with mask[b, l] == 0; L for a row without one.  mask (B * L) bytes."""
    m = np.asarray(mask).reshape(B, L)
    n = np.full(B, L, np.int32)
    for b in range(B):
        free = np.flatnonzero(m[b] == 0)
        if free.size:
            n[b] = free[-1] + 1
    return n


def downsample_row_ref(x, w, lens, B, L, ds, exact=False):
    """out[b, i] = sum_k w[k] x[b, min(i ds + k, lens[b] - 1)] for every i < dL = ceil(L / ds), summed
    in the order k = 0 .. ds - 1.  x (B * L, C) -> (B * dL, C).  exact: assert that every product and
    partial sum is an fp32 value, as kernel_ref.downsample_ref does."""
    C = x.shape[1]
    dL = -(-L // ds)
    x3 = x.reshape(B, L, C)
    out = np.zeros((B, dL, C))
    for b in range(B):
        assert 1 <= lens[b] <= L, "a row's length lies in [1, L]"
        idx = np.minimum(np.arange(dL * ds), lens[b] - 1).reshape(dL, ds)
        for k in range(ds):
            term = x3[b, idx[:, k]] * w[k]
            out[b] = out[b] + term
            if exact:
                kr.assert_fp32_exact(term, "x w"), kr.assert_fp32_exact(out[b], "partial sum")
    return out.reshape(B * dL, C)
