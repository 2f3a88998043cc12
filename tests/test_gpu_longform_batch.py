"""Pooled long-form synthesis and the per-row pause trim end to end on the GPU
(zipvoice_amd/longform.py generate_long_batch, zipvoice_amd/infer.py generate_batch with
remove_long_sil), full-size synthetic model at num_step = 4.

The wiring is checked bit for bit against direct model.sample + decode_features calls on the
same groups, prompts and initial noise; the joins against tests/wavjoin_docs_ref.py (the
float64 reference once per document) under the conditions of tests/test_gpu_longform.py:
margin >= 1e-3 asserted on the reference first, spans and lengths exact, samples within
4 * 2^-23 * max |g x|, bit copies outside overlaps at gain 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import wavjoin_docs_ref as dref  # noqa: E402
from zipvoice_amd.common import predict_features_lens  # noqa: E402
from zipvoice_amd.feature import VocosFbank  # noqa: E402
from zipvoice_amd.infer import _prompt_rms_normalise, generate_batch  # noqa: E402
from zipvoice_amd.longform import (WavJoiner, generate_long, generate_long_batch,  # noqa: E402
                                   plan_long_batch)

BREAK, SOFT = (3, 4), (5,)
TARGET, HOP = 0.1, 256


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def stack():
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    from zipvoice_amd.vocoder import Vocos
    from zipvoice_amd.weights import synthetic_state_dict
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="bf16")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m = m.to("cuda:0")
    voc = Vocos().load_synthetic(0).to("cuda:0")
    return m, voc, VocosFbank()


@pytest.fixture(scope="module")
def requests():
    """Request 0: the text and prompt of test_gpu_longform.test_generate_long_end_to_end (1 s
    at amplitude 0.05: gain 0.5).  Request 1: 0.75 s at amplitude 0.2 (gain 1), 9 prompt
    tokens, 60 tokens with two sentence ends."""
    rng = np.random.default_rng(0)
    t0 = [int(t) for t in rng.integers(10, 90, 120)]
    for i in (17, 33, 41, 58, 79, 96, 110):
        t0[i] = BREAK[i % 2]
    for i in (8, 25, 50, 70, 101):
        t0[i] = SOFT[0]
    pw0 = (0.05 * rng.standard_normal(24000)).astype(np.float32)
    rng = np.random.default_rng(1)
    t1 = [int(t) for t in rng.integers(10, 90, 60)]
    t1[27], t1[59] = BREAK
    pw1 = (0.2 * rng.standard_normal(18000)).astype(np.float32)
    return [(t0, list(range(40, 52)), pw0), (t1, list(range(60, 69)), pw1)]


def prompt_features(fx, prompts):
    """Host RMS normalisation and one extract_batch, as generate_batch prepares 24 kHz
    prompts -> (features * 0.1 (R, T, 100), frame counts (R,) on the device, rms)."""
    ws, rms = zip(*[_prompt_rms_normalise(torch.from_numpy(p), TARGET) for p in prompts])
    wb = torch.zeros((len(ws), max(len(w) for w in ws)))
    for i, w in enumerate(ws):
        wb[i, :len(w)] = w
    feats, nfr = fx.extract_batch(wb.cuda(), torch.tensor([len(w) for w in ws]))
    return (feats + 0.0) * 0.1, nfr, list(rms)


def direct(m, voc, pf, nfr, tokens, prompt_tokens, rows, x0):
    """One model.sample + decode_features with rows' prompts -> the raw waveforms."""
    di = torch.tensor(rows, device="cuda")
    P = int(nfr[di].max())
    pred, pl, _, _ = m.sample(tokens=tokens, prompt_tokens=prompt_tokens,
                              prompt_features=pf[di][:, :P].contiguous(),
                              prompt_features_lens=nfr[di], speed=1.0, t_shift=0.5,
                              duration="predict", num_step=4, guidance_scale=1.0, x0=x0)
    wv = voc.decode_features(pred, pl, feat_scale=0.1, feat_bias=0.0, clamp=True)
    return [wv[i, :int(pl[i]) * HOP] for i in range(len(rows))]


def noise_for(groups, frames, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(len(g), max(frames[i] for i in g), 100, generator=gen).cuda()
            for g in groups]


def test_generate_long_batch_end_to_end(stack, requests):
    m, voc, fx = stack
    R = len(requests)
    plan = plan_long_batch([r[0] for r in requests], [12, 9], [24000, 18000], BREAK, SOFT,
                           max_seconds=5.0, batch_size=2)
    K = len(plan.chunks)
    assert plan.doc_sizes[0] >= 3 and plan.doc_sizes[1] >= 2 and len(plan.groups) == -(-K // 2)
    assert any(len({plan.doc_of[i] for i in g}) == 2 for g in plan.groups)   # a mixed batch
    x0 = noise_for(plan.groups, plan.frames, 0)

    pf, nfr, rms = prompt_features(fx, [r[2] for r in requests])
    assert nfr.tolist() == [94, 70] and rms[0] < TARGET <= rms[1]
    want = [None] * K
    for g, z in zip(plan.groups, x0):
        docs = [plan.doc_of[i] for i in g]
        for i, w in zip(g, direct(m, voc, pf, nfr, [plan.chunks[i] for i in g],
                                  [requests[d][1] for d in docs], docs, z)):
            want[i] = w

    wavs, met, cw, spans, got_plan = generate_long_batch(
        requests, m, voc, fx, BREAK, SOFT, max_seconds=5.0, batch_size=2, x0=x0,
        return_chunks=True, num_step=4)
    assert got_plan == plan
    assert met["num_chunks"] == K and met["num_batches"] == len(plan.groups)
    assert met["num_requests"] == R and met["t"] > 0 and met["rtf"] > 0
    # 1. the wiring: every chunk is what the direct calls give, in join order
    assert len(cw) == K
    for a, b in zip(cw, want):
        assert a.shape == b.shape and a.numel() > 0 and torch.equal(a, b)

    # 2. the join, per document, against the float64 reference of those chunk waveforms
    j = WavJoiner()
    xs = [c.cpu().numpy() for c in cw]
    gains = [rms[d] / TARGET if rms[d] < TARGET else 1.0 for d in plan.doc_of]
    assert gains[0] == pytest.approx(0.5, rel=0.05) and gains[-1] == 1.0
    doc_ptr = np.concatenate([[0], np.cumsum(plan.doc_sizes)]).tolist()
    r = dref.wavjoin_docs(xs, [len(c) for c in xs], gains, doc_ptr, j.frame, j.thr, j.keep_edge,
                          j.max_gap, j.fade)
    print(f"generate_long_batch: K={K} groups={plan.groups} lens={[len(c) for c in xs]} "
          f"m={r.m.tolist()} F={r.F.tolist()} N={r.N.tolist()} margin {r.margin:.3e}")
    assert r.margin >= 1e-3, r.margin
    assert np.array_equal(spans.cpu().numpy(), np.stack([r.m, r.off, r.F], 1))
    assert len(wavs) == R and (r.N > 0).all() and (r.F[1:plan.doc_sizes[0]] > 0).all()
    tol = 4 * 2.0 ** -23 * max(float(np.abs(gains[b] * xs[b]).max()) for b in range(K))
    for d, w in enumerate(wavs):
        assert w.is_cuda and w.shape == (1, int(r.N[d])) and torch.isfinite(w).all()
        err = float(np.abs(w.cpu().numpy() - r.outs[d]).max())
        print(f"  request {d}: N {int(r.N[d])} max err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (d, err, tol)
    assert abs(met["wav_seconds"] - int(r.N.sum()) / 24000) < 1e-9
    # request 1 has gain 1: outside the overlaps its samples are the chunks' bits
    o = wavs[1].cpu().numpy()
    live = [b for b in range(doc_ptr[1], doc_ptr[2]) if r.m[b]]
    for i, b in enumerate(live):
        lo = int(r.F[b])
        hi = int(r.m[b] - (r.F[live[i + 1]] if i + 1 < len(live) else 0))
        assert hi > lo
        assert np.array_equal(bits(o[0, r.off[b] + lo:r.off[b] + hi]),
                              bits(xs[b][r.kept[b][lo:hi]]))


def test_one_request_unsorted_equals_generate_long(stack, requests):
    m, voc, fx = stack
    tokens, prompt_tokens, pw = requests[0]
    plan = plan_long_batch([tokens], [12], [24000], BREAK, SOFT, max_seconds=5.0, batch_size=2,
                           sort_by_length=False)
    assert len(plan.groups) == 2
    fl = predict_features_lens(torch.tensor([94]), torch.tensor([12]),
                               torch.tensor([len(c) for c in plan.chunks]), 1.0).tolist()
    assert fl == plan.frames
    x0 = noise_for(plan.groups, plan.frames, 2)
    want, _ = generate_long(tokens, prompt_tokens, pw, m, voc, fx, BREAK, SOFT, max_seconds=5.0,
                            batch_size=2, x0=x0, num_step=4)
    got, met = generate_long_batch([(tokens, prompt_tokens, pw, 24000)], m, voc, fx, BREAK, SOFT,
                                   max_seconds=5.0, batch_size=2, x0=x0, sort_by_length=False,
                                   num_step=4)
    assert len(got) == 1 and met["num_requests"] == 1 and met["num_batches"] == 2
    assert got[0].shape == want.shape and want.shape[1] > 0 and torch.equal(got[0], want)


def test_generate_batch_remove_long_sil(stack, requests):
    m, voc, fx = stack
    rng = np.random.default_rng(3)
    prompts = [requests[0][2], requests[1][2],
               (0.15 * rng.standard_normal(20000)).astype(np.float32)]
    ptoks = [requests[0][1], requests[1][1], list(range(30, 40))]
    toks = [[int(t) for t in rng.integers(10, 90, n)] for n in (30, 22, 26)]
    items = list(zip(toks, ptoks, prompts))
    pf, nfr, rms = prompt_features(fx, prompts)
    fl = predict_features_lens(nfr.cpu(), torch.tensor([len(p) for p in ptoks]),
                               torch.tensor([len(t) for t in toks]), 1.0)
    x0 = torch.randn(3, int(fl.max()), 100, generator=torch.Generator().manual_seed(4)).cuda()
    raw = direct(m, voc, pf, nfr, toks, ptoks, [0, 1, 2], x0)
    gains = [r / TARGET if r < TARGET else 1.0 for r in rms]
    assert gains[0] < 1.0 and gains[1:] == [1.0, 1.0]

    # off: the results of the plain path, bit for bit
    plain, met0 = generate_batch(items, m, voc, fx, num_step=4, x0=x0)
    for i, w in enumerate(plain):
        want = raw[i] * rms[i] / TARGET if rms[i] < TARGET else raw[i]
        assert w.shape == (1, raw[i].numel()) and torch.equal(w[0], want)
    assert abs(met0["wav_seconds"] - sum(w.numel() for w in raw) / 24000) < 1e-9

    j = WavJoiner()
    xs = [w.cpu().numpy() for w in raw]
    r = dref.wavjoin_docs(xs, [len(x) for x in xs], gains, [0, 1, 2, 3], j.frame, j.thr,
                          j.keep_edge, j.max_gap, j.fade)
    print(f"remove_long_sil: lens={[len(x) for x in xs]} N={r.N.tolist()} margin {r.margin:.3e}")
    assert r.margin >= 1e-3, r.margin
    trimmed, met = generate_batch(items, m, voc, fx, num_step=4, x0=x0, remove_long_sil=True)
    assert len(trimmed) == 3 and (r.N > 0).all()
    for i, w in enumerate(trimmed):
        assert w.is_cuda and w.shape == (1, int(r.N[i]))
        tol = 4 * 2.0 ** -23 * float(np.abs(gains[i] * xs[i]).max())
        err = float(np.abs(w.cpu().numpy() - r.outs[i]).max())
        print(f"  item {i}: N {int(r.N[i])} of {len(xs[i])} max err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (i, err, tol)
        if gains[i] == 1.0:
            assert np.array_equal(bits(w.cpu().numpy()[0]), bits(xs[i][r.kept[i]]))
    assert abs(met["wav_seconds"] - int(r.N.sum()) / 24000) < 1e-9 and met["rtf"] > 0
    again, _ = generate_batch(items, m, voc, fx, num_step=4, x0=x0, remove_long_sil=True, joiner=j)
    assert all(torch.equal(a, b) for a, b in zip(again, trimmed))
