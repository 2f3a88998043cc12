"""ZipVoice.sample_edit / sample_intermediate on the GPU (synthetic weights, default config).

(a) An edit that replaces the padding after a prompt by G generated frames is the prefix-prompt
    case: its generated part is sample(duration="real")'s, bit for bit, from the same x0.
(b) sample_intermediate against the reference's (tests/golden/sample_intermediate.npz), at the
    tolerances tests/test_gpu_parity.py holds its sample fixtures to.
(c) With seeds the noise follows the row, not the batch (compared as
    tests/test_gpu_seeded_sampling.py compares its rows: the bits the solver receives over the
    row's own frames).
(d) An interior edit: generated frames differ from the original, kept frames come back bitwise
    with keep_original, and the mask counts the generated frames."""
import numpy as np
import pytest

import edit_ref
from golden_io import load, tokens_list

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = {"fp32": (1e-3, 3e-2), "fp16": (1e-3, 2e-2), "bf16": (5e-2, 0.25)}   # tests/test_gpu_parity.py
_models = {}


def model(precision):
    if precision not in _models:
        from zipvoice_amd.config import default_config
        from zipvoice_amd.models import build_model
        cfg = default_config("zipvoice")
        _models[precision] = build_model(cfg, precision=precision).load_synthetic(0).to("cuda:0")
    return _models[precision]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def prefix_case():
    rng = np.random.default_rng(31)
    P, L, G = [33, 20], [40, 27], [30, 41]
    feat = (0.3 * rng.standard_normal((2, 40, 100)) - 0.5).astype(np.float32)   # frames past P_b: junk
    ptoks = [[int(v) for v in rng.integers(1, 360, n)] for n in (5, 4)]
    toks = [[int(v) for v in rng.integers(1, 360, n)] for n in (4, 6)]
    x0 = rng.standard_normal((2, 63, 100)).astype(np.float32)
    return P, L, G, feat, ptoks, toks, x0


@pytest.mark.parametrize("num_step", [2, [2, 3]], ids=["scalar", "per-row-steps"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_prefix_edit_is_sample_real_duration(precision, num_step):
    m = model(precision)
    P, L, G, feat, ptoks, toks, x0 = prefix_case()
    kw = dict(num_step=num_step, guidance_scale=0.7, t_shift=0.5)
    gen, gl, prm, pl = m.sample(tokens=toks, prompt_tokens=ptoks, prompt_features=cuda(feat[:, :33]),
                                prompt_features_lens=torch.tensor(P), features_lens=torch.tensor(G),
                                duration="real", x0=cuda(x0), **kw)
    spans = [[(P[b], L[b], G[b])] for b in range(2)]
    x1, lens, mask = m.sample_edit(tokens=[p + t for p, t in zip(ptoks, toks)], features=cuda(feat),
                                   features_lens=torch.tensor(L), spans=spans, x0=cuda(x0), **kw)
    assert x1.shape == (2, 63, 100) and lens.tolist() == [63, 61] and gl.tolist() == G
    assert torch.isfinite(x1).all()
    for b in range(2):
        assert np.array_equal(bits(x1[b, P[b]:P[b] + G[b]]), bits(gen[b, :G[b]]))
        assert np.array_equal(bits(x1[b, :P[b]]), bits(cuda(feat)[b, :P[b]]))       # keep_original
        assert mask[b].tolist() == [False] * P[b] + [True] * G[b] + [False] * (63 - P[b] - G[b])
        assert not x1[b, P[b] + G[b]:].any()
    assert float(gen[0, :G[0]].abs().max()) > 0


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_sample_intermediate_golden(precision):
    d = load("sample_intermediate.npz")
    x, lens = model(precision).sample_intermediate(
        tokens=tokens_list(d["tokens"]), features=cuda(d["features"]),
        features_lens=cuda(d["features_lens"]), noise=cuda(d["noise"]),
        speech_condition_mask=cuda(d["speech_condition_mask"]), t_start=float(d["t_start"]),
        t_end=float(d["t_end"]), num_step=int(d["num_step"]), guidance_scale=cuda(d["guidance_scale"]))
    assert lens.tolist() == d["x_lens"].tolist()
    out = x.cpu().numpy()
    assert out.shape == d["x"].shape and np.isfinite(out).all()
    err = np.abs(out - d["x"])
    print(f"sample_intermediate [{precision}] mean={err.mean():.3e} max={err.max():.3e}")
    assert err.mean() < TOL[precision][0]
    assert err.max() < TOL[precision][1]


def interior_case():
    rng = np.random.default_rng(32)
    L = [50, 37, 44]
    feat = (0.3 * rng.standard_normal((3, 50, 100)) - 0.5).astype(np.float32)
    toks = [[int(v) for v in rng.integers(1, 360, n)] for n in (11, 8, 9)]
    spans = [[(12, 20, 11), (33, 33, 4)], [(5, 18, 13)], [(0, 6, 6), (20, 26, 0), (40, 44, 7)]]
    return L, feat, toks, spans


def test_noise_follows_the_row(monkeypatch):
    m = model("bf16")
    L, feat, toks, spans = interior_case()
    calls = []
    inner = m.solver.sample

    def sample(*args, **kw):
        calls.append((kw["x"].clone(), (~kw["padding_mask"]).sum(-1).tolist()))
        return inner(*args, **kw)
    monkeypatch.setattr(m.solver, "sample", sample)
    seeds = [5, (1 << 64) - 3, 1 << 63]
    kw = dict(num_step=2, guidance_scale=1.0, t_shift=0.5)
    x3, l3, m3 = m.sample_edit(tokens=toks, features=cuda(feat), features_lens=torch.tensor(L), spans=spans,
                               seeds=seeds, **kw)
    x1, l1, m1 = m.sample_edit(tokens=toks[1:2], features=cuda(feat[1:2, :37]), features_lens=torch.tensor(L[1:2]),
                               spans=spans[1:2], seeds=seeds[1:2], **kw)
    (n3, len3), (n1, len1) = calls
    T1 = L[1]                                          # row 1 replaces 13 frames by 13
    assert len1 == [T1] == [len3[1]] == l1.tolist() and l3.tolist() == len3 and len(set(len3)) == 3
    assert n3.shape[1] == max(len3) and n1.shape[1] == T1
    assert np.array_equal(bits(n1[0, :T1]), bits(n3[1, :T1]))
    assert not np.array_equal(bits(n3[0, :T1]), bits(n3[1, :T1]))
    assert torch.equal(m1[0, :T1], m3[1, :T1])
    # the kept frames of the row are the recording's, in a batch or alone
    keep = ~m1[0, :T1]
    assert np.array_equal(bits(x1[0, :T1][keep]), bits(x3[1, :T1][keep]))
    with pytest.raises(ValueError):
        m.sample_edit(tokens=toks, features=cuda(feat), features_lens=torch.tensor(L), spans=spans,
                      seeds=seeds, x0=n3, **kw)
    with pytest.raises(ValueError):
        m.sample_edit(tokens=toks, features=cuda(feat), features_lens=torch.tensor(L), spans=spans,
                      seeds=seeds[:2], **kw)


def test_interior_edit():
    m = model("fp32")
    L, feat, toks, spans = interior_case()
    tables = [edit_ref.plan(n, sp) for n, sp in zip(L, spans)]
    Tb = [int(t[-1, 0] + t[-1, 2]) for t in tables]
    T = max(Tb)
    x0 = cuda(np.random.default_rng(33).standard_normal((3, T, 100)).astype(np.float32))
    kw = dict(tokens=toks, features=cuda(feat), features_lens=torch.tensor(L), spans=spans, num_step=2,
              guidance_scale=1.0, t_shift=0.5, x0=x0)
    raw, lens, mask = m.sample_edit(keep_original=False, **kw)
    kept, lens2, mask2 = m.sample_edit(**kw)
    assert lens.tolist() == Tb == lens2.tolist() and torch.equal(mask, mask2)
    assert raw.shape == (3, T, 100) and torch.isfinite(raw).all()
    ref, rmask = edit_ref.gather(feat, None, tables, T)
    assert np.array_equal(mask.cpu().numpy(), rmask)
    for b in range(3):
        assert int(mask[b].sum()) == sum(n for _, _, n in spans[b])
        g = mask[b].cpu().numpy()
        assert np.abs(raw[b].cpu().numpy()[g]).mean() > 1e-2           # generated frames hold speech
        # without keep_original the kept frames are the solver's, close to the condition but not it
        assert not np.array_equal(bits(raw[b, :Tb[b]])[~g[:Tb[b]]], bits(cuda(ref)[b, :Tb[b]])[~g[:Tb[b]]])
    # row 1 replaces frames [5, 18) one for one: there the result differs from the original
    assert np.abs(raw[1, 5:18].cpu().numpy() - feat[1, 5:18]).mean() > 1e-2
    # with keep_original: the kept frames bitwise, the generated ones the solver's
    want, _ = edit_ref.gather(feat, raw.cpu().numpy(), tables, T)
    assert np.array_equal(bits(kept), want.view(np.int32))
    with pytest.raises(ValueError, match="row 1 span 0"):
        m.sample_edit(**{**kw, "spans": [spans[0], [(5, 38, 1)], spans[2]]})
    with pytest.raises(ValueError):
        m.sample_edit(**{**kw, "x0": x0[:, :-1]})
