"""The row padding mode's float64 restatement (tests/padrow_ref.py) against its definition: every
row of a padded batch is downsampled as kernel_ref.downsample_ref (SimpleDownsample,
zipformer.py:887-913) downsamples that row alone at its own length.  No GPU."""
import os
import re

import numpy as np
import pytest

import kernel_ref as kr
import padrow_ref as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lengths_of_prefix_masks():
    B, L = 4, 13
    lens = [13, 6, 1, 12]
    m = (np.arange(L)[None, :] >= np.array(lens)[:, None]).astype(np.uint8)
    assert pr.row_lengths(m.reshape(-1), B, L).tolist() == lens


def test_lengths_of_masks_with_holes():
    L = 9
    m = np.ones((5, L), np.uint8)
    m[0, [0, 4]] = 0            # the last unmasked frame counts, the hole before it does not
    m[1, 8] = 0                 # only the last frame is free
    m[2, 0] = 0                 # only the first
    m[3, :] = 0                 # nothing masked
    m[3, 3] = 1                 # ... but a hole inside
    #  row 4: fully masked -> L
    assert pr.row_lengths(m.reshape(-1), 5, L).tolist() == [5, 9, 1, 9, 9]
    assert pr.row_lengths(m.reshape(-1), 5, L).dtype == np.int32


@pytest.mark.parametrize("ds", [2, 4])
def test_batch_rows_equal_rows_alone(ds):
    """B = 3, L = 13, lens (13, 6, 1): on the groups that hold a valid frame, i < ceil(n_b / ds), the
    row-clamped downsample of the batch is downsample_ref of the row alone, exactly; the groups past
    them repeat the row's last frame (weights summing to one), whatever lies past the row's end."""
    B, L, C = 3, 13, 8
    lens = [13, 6, 1]
    rng = np.random.default_rng(ds)
    x = rng.integers(-64, 65, (B * L, C)).astype(np.float64)
    w = kr.ds_weights(ds)
    for b, n in enumerate(lens):                                 # what must not be read: huge frames
        x.reshape(B, L, C)[b, n:] = 1e6 * (b + 1)
    got = pr.downsample_row_ref(x, w, lens, B, L, ds, exact=False).reshape(B, -1, C)
    for b, n in enumerate(lens):
        alone = kr.downsample_ref(x.reshape(B, L, C)[b, :n].copy(), w, 1, n, ds)
        g = -(-n // ds)
        assert alone.shape[0] == g
        assert np.array_equal(got[b, :g], alone), f"row {b}"
        assert np.array_equal(got[b, g:], np.broadcast_to(x.reshape(B, L, C)[b, n - 1], got[b, g:].shape))
    # n_b = L for every row: the batch kernel's rule
    full = pr.downsample_row_ref(x, w, [L] * B, B, L, ds)
    assert np.array_equal(full, kr.downsample_ref(x, w, B, L, ds))


def test_new_symbols_in_header_and_signatures():
    from zipvoice_amd import engine
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "zipvoice_hip.h")).read(), flags=re.S)
    for name in ("zv_set_padding", "zv_get_padding", "zv_padrow_check"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in engine.SIGNATURES, name
    assert re.search(r"enum\s+zv_padding\s*\{\s*ZV_PAD_BATCH\s*=\s*0\s*,\s*ZV_PAD_ROW\s*=\s*1\s*\}", src)
    assert "padding" not in [f[0] for f in engine.ZvConfig._fields_]      # zv_config's layout is unchanged
    assert engine.PADDING_MODES == ("batch", "row")
    for bad in ("rows", "", None, 1):
        with pytest.raises(ValueError):
            engine.padding_id(bad)


def test_model_remembers_the_mode_without_an_engine():
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    m = build_model(default_config("zipvoice"))
    assert m.padding == "batch"
    m.padding = "row"
    assert m.padding == "row"
    assert build_model(default_config("zipvoice_distill"), padding="row").padding == "row"
    with pytest.raises(ValueError):
        build_model(default_config("zipvoice"), padding="utterance")
    with pytest.raises(ValueError):
        m.padding = "none"
    assert m.padding == "row"
