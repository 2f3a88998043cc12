"""Pin tests/golden/sample_intermediate.npz (the reference's ``ZipVoice.sample_intermediate``,
written by tests/golden/make_golden_edit.py) with the CPU oracle: ``forward_text_embed`` +
``forward_text_condition`` over the rows' own lengths, ``speech_c = where(mask, 0, features)``
and ``euler``, to the bar tests/test_oracle_golden.py holds its samples to.  The oracle's solver
takes one guidance scale per call, so the fixture's (B, 1, 1) tensor is run row by row: rows of
a batch do not see each other."""
import numpy as np

from golden_io import load, tokens_list
from oracle.zipvoice_np import ZipVoiceOracle
from zipvoice_amd.config import default_config
from zipvoice_amd.weights import synthetic_state_dict


def test_fixture_is_what_it_says():
    d = load("sample_intermediate.npz")
    assert d["features"].shape == d["noise"].shape == d["x"].shape == (2, 37, 100)
    assert d["features_lens"].tolist() == [37, 29] and d["x_lens"].tolist() == [37, 29]
    assert d["guidance_scale"].shape == (2, 1, 1) and int(d["num_step"]) == 2
    assert float(d["t_start"]) == 0.0 and float(d["t_end"]) == 1.0
    m = d["speech_condition_mask"]
    for b, L in enumerate(d["features_lens"]):
        on = np.flatnonzero(m[b])
        assert on.size and (np.diff(on) == 1).all()          # one span ...
        assert 0 < on[0] and on[-1] + 1 < L                  # ... inside the row


def test_oracle_matches_reference_sample_intermediate():
    d = load("sample_intermediate.npz")
    cfg = default_config(str(d["variant"]))
    o = ZipVoiceOracle(cfg, synthetic_state_dict(cfg, int(d["seed"])))
    embed, tokens_lens = o.forward_text_embed(tokens_list(d["tokens"]))
    tc, pm = o.forward_text_condition(embed, tokens_lens, d["features_lens"])
    sc = np.where(d["speech_condition_mask"][..., None], np.float32(0), d["features"]).astype(np.float32)
    x = np.concatenate([
        o.euler(d["noise"][b:b + 1], tc[b:b + 1], sc[b:b + 1], pm[b:b + 1], int(d["num_step"]),
                float(d["guidance_scale"][b, 0, 0]), t_start=float(d["t_start"]),
                t_end=float(d["t_end"]))
        for b in range(2)])
    assert x.shape == d["x"].shape
    assert np.abs(x - d["x"]).mean() < 1e-5
    assert np.abs(x - d["x"]).max() < 5e-5
