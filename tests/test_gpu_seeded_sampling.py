"""Per-request seeds through the public generation entries on the GPU: full-size synthetic model,
bf16, num_step = 2.

* model.sample(seeds=S) is model.sample(x0=seeded_normal(S, (num_frames, F))), bit for bit, so the
  seeded path inherits what the explicit-x0 path is already tested for.
* The noise follows the request, not the batch: the x that model.solver.sample receives is
  recorded, and over a request's own frames it is the same bits in generate_batch [a, b, c], in
  generate_batch [c, a] and in generate_sentence.
* Pooled equals sequential at the noise level: generate_long_batch (5 chunks of two requests,
  sorted and regrouped into 3 calls) and generate_long per request hand every (request, chunk) the
  same bits, those of seeded_normal([seed], ..., streams=[chunk]).
* Without a seed nothing changes: torch.randn draws the noise and zv_noise_normal is not called.
The token and prompt recipe is that of tests/test_gpu_longform_batch.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.common import predict_features_lens  # noqa: E402
from zipvoice_amd.feature import VocosFbank  # noqa: E402
from zipvoice_amd.infer import generate_batch, generate_sentence  # noqa: E402
from zipvoice_amd.longform import generate_long, generate_long_batch  # noqa: E402
from zipvoice_amd.noise import seeded_normal  # noqa: E402

BREAK, SOFT = (3, 4), (5,)
STEPS = 2


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
    """The two requests of tests/test_gpu_longform_batch.py: 120 tokens with a 1 s prompt of 12
    tokens (3 chunks at max_seconds = 5), 60 tokens with a 0.75 s prompt of 9 tokens (2 chunks)."""
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


@pytest.fixture(scope="module")
def items(requests):
    """Three short items (a few dozen tokens, prompts of about 1 s) with different lengths."""
    rng = np.random.default_rng(3)
    prompts = [requests[0][2], requests[1][2], (0.15 * rng.standard_normal(20000)).astype(np.float32)]
    ptoks = [requests[0][1], requests[1][1], list(range(30, 40))]
    toks = [[int(t) for t in rng.integers(10, 90, n)] for n in (30, 22, 26)]
    return list(zip(toks, ptoks, prompts))


class Recorder:
    """model.solver.sample wrapped: keeps every call's initial noise and row lengths, then calls
    through."""

    def __init__(self, monkeypatch, model):
        self.calls = []
        inner = model.solver.sample

        def sample(*args, **kw):
            lens = (~kw["padding_mask"]).sum(-1).tolist()
            self.calls.append((kw["x"].clone(), lens))
            return inner(*args, **kw)
        monkeypatch.setattr(model.solver, "sample", sample)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def own(x, row, length):
    """The bits of a recorded row over the request's own frames."""
    return x[row, :length].cpu().numpy().view(np.int32)


def test_seeds_are_the_explicit_x0_path(stack):
    m, _, _ = stack
    rng = np.random.default_rng(5)
    plens = torch.tensor([94, 70, 80])
    pf = torch.from_numpy(rng.standard_normal((3, 94, 100)).astype(np.float32)).cuda() * 0.3
    ptoks = [list(range(40, 52)), list(range(60, 69)), list(range(30, 40))]
    toks = [[int(t) for t in rng.integers(10, 90, n)] for n in (30, 22, 26)]
    fl = predict_features_lens(plens, torch.tensor([len(p) for p in ptoks]),
                               torch.tensor([len(t) for t in toks]), 1.0)
    assert len(set(fl.tolist())) == 3                                  # a ragged batch
    S, streams = [11, (1 << 64) - 1, 1 << 63], [0, 2, 1]
    kw = dict(tokens=toks, prompt_tokens=ptoks, prompt_features=pf, prompt_features_lens=plens,
              speed=1.0, t_shift=0.5, duration="predict", num_step=STEPS, guidance_scale=1.0)
    for st in (None, streams):
        a = m.sample(**kw, seeds=S, seed_streams=st)
        b = m.sample(**kw, x0=seeded_normal(S, (int(fl.max()), 100), st))
        assert a[0].numel() > 0 and torch.isfinite(a[0]).all()
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    c = m.sample(**kw, seeds=[12] + S[1:])
    assert not torch.equal(c[0][0], m.sample(**kw, seeds=S)[0][0])      # another seed, other speech
    with pytest.raises(ValueError):
        m.sample(**kw, seeds=S, x0=seeded_normal(S, (int(fl.max()), 100)))


def test_noise_follows_the_request(stack, items, monkeypatch):
    m, voc, fx = stack
    rec = Recorder(monkeypatch, m)
    a, b, c = items
    sa, sb, sc = 101, (1 << 64) - 2, 1 << 63
    generate_batch([a, b, c], m, voc, fx, num_step=STEPS, seeds=[sa, sb, sc])
    (x3, l3), = rec.take()
    generate_batch([c, a], m, voc, fx, num_step=STEPS, seeds=[sc, sa])
    (x2, l2), = rec.take()
    assert l3[0] == l2[1] and l3[2] == l2[0] and len(set(l3)) == 3
    assert x3.shape[1] == max(l3) and x2.shape[1] == max(l2)
    for i, j in ((0, 1), (2, 0)):
        assert np.array_equal(own(x3, i, l3[i]), own(x2, j, l2[j]))
    for i, (it, s) in enumerate(zip((a, b, c), (sa, sb, sc))):
        wav, _ = generate_sentence(it[0], it[1], it[2], m, voc, fx, num_step=STEPS, seed=s)
        (x1, l1), = rec.take()
        assert l1 == [l3[i]] and wav.numel() > 0
        assert np.array_equal(own(x1, 0, l1[0]), own(x3, i, l3[i]))
        direct = seeded_normal([s], (l1[0], 100))
        assert np.array_equal(own(direct, 0, l1[0]), own(x3, i, l3[i]))
    assert not np.array_equal(own(x3, 0, 100), own(x3, 1, 100))
    with pytest.raises(ValueError):
        generate_batch([a, b], m, voc, fx, num_step=STEPS, seeds=[1])
    with pytest.raises(ValueError):
        generate_batch([a], m, voc, fx, num_step=STEPS, seeds=[1], x0=x3[:1])


def test_pooled_equals_sequential_noise(stack, requests, monkeypatch):
    m, voc, fx = stack
    rec = Recorder(monkeypatch, m)
    seeds = [7, (1 << 63) + 9]
    kw = dict(max_seconds=5.0, batch_size=2, num_step=STEPS)
    outs, met, _, _, plan = generate_long_batch(requests, m, voc, fx, BREAK, SOFT, seeds=seeds,
                                                return_chunks=True, **kw)
    pooled = rec.take()
    assert plan.doc_sizes == [3, 2] and len(plan.groups) == 3 and len(pooled) == 3
    assert any(len({plan.doc_of[i] for i in g}) == 2 for g in plan.groups)   # a mixed batch
    assert sorted(i for g in plan.groups for i in g) != [i for g in plan.groups for i in g]
    got = {}
    for g, (x, lens) in zip(plan.groups, pooled):
        for row, i in enumerate(g):
            assert lens[row] == plan.frames[i]
            got[i] = own(x, row, lens[row])
    first = [0, plan.doc_sizes[0]]
    for d, (tokens, ptoks, pw) in enumerate(requests):
        wav, met1 = generate_long(tokens, ptoks, pw, m, voc, fx, BREAK, SOFT, seed=seeds[d], **kw)
        seq = rec.take()
        assert met1["num_chunks"] == plan.doc_sizes[d] and len(seq) == -(-plan.doc_sizes[d] // 2)
        for k in range(plan.doc_sizes[d]):
            i = first[d] + k
            x, lens = seq[k // 2]
            assert lens[k % 2] == plan.frames[i]
            assert np.array_equal(own(x, k % 2, lens[k % 2]), got[i]), (d, k)
            direct = seeded_normal([seeds[d]], (plan.frames[i], 100), streams=[k])
            assert np.array_equal(own(direct, 0, plan.frames[i]), got[i]), (d, k)
    # chunks of one request draw from different streams
    assert not np.array_equal(got[0][:50], got[1][:50])
    with pytest.raises(ValueError):
        generate_long_batch(requests, m, voc, fx, BREAK, SOFT, seeds=[1], **kw)
    with pytest.raises(ValueError):
        generate_long(*requests[0], m, voc, fx, BREAK, SOFT, seed=1, x0=[None, None], **kw)


def test_onnx_adapter_draws_the_same_noise(stack):
    from zipvoice_amd.onnx_compat import OnnxModel, sample
    om = OnnxModel.from_model(stack[0])
    rng = np.random.default_rng(2)
    toks = [[int(v) for v in rng.integers(1, 360, 12)]]
    ptoks = [[int(v) for v in rng.integers(1, 360, 8)]]
    pf = torch.from_numpy((0.3 * rng.standard_normal((1, 40, 100)) - 0.5).astype(np.float32))
    T = om.run_text_encoder(torch.tensor(toks), torch.tensor(ptoks), torch.tensor(40),
                            torch.tensor(1.0)).shape[1]
    s = (1 << 63) + 3
    a = sample(om, toks, ptoks, pf, num_step=STEPS, seeds=[s])
    b = sample(om, toks, ptoks, pf, num_step=STEPS, x0=seeded_normal([s], (T, 100)))
    assert a.shape == (1, T - 40, 100) and torch.isfinite(a).all() and torch.equal(a, b)
    with pytest.raises(ValueError):
        sample(om, toks, ptoks, pf, num_step=STEPS, seeds=[s], x0=torch.zeros(1, T, 100))
    with pytest.raises(ValueError):
        sample(om, toks, ptoks, pf, num_step=STEPS, seeds=[s, s])


def test_default_still_draws_with_torch_randn(stack, items, monkeypatch):
    m, _, _ = stack
    lib = engine.load_library()
    calls, inner = [], lib.zv_noise_normal

    def counted(*args):
        calls.append(args[2])
        return inner(*args)
    monkeypatch.setattr(lib, "zv_noise_normal", counted)
    rng = np.random.default_rng(6)
    pf = torch.from_numpy(rng.standard_normal((2, 80, 100)).astype(np.float32)).cuda() * 0.3
    kw = dict(tokens=[items[0][0], items[1][0]], prompt_tokens=[items[0][1], items[1][1]],
              prompt_features=pf, prompt_features_lens=torch.tensor([80, 64]), speed=1.0,
              t_shift=0.5, duration="predict", num_step=STEPS, guidance_scale=1.0)
    rec = Recorder(monkeypatch, m)
    torch.manual_seed(0)
    a = m.sample(**kw)
    torch.manual_seed(0)
    b = m.sample(**kw)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and calls == []
    (xa, _), (xb, _) = rec.take()
    torch.manual_seed(0)
    assert torch.equal(xa, torch.randn(xa.shape, device=xa.device)) and torch.equal(xa, xb)
    m.sample(**kw, seeds=[1, 2])                                     # the wrapper does see calls
    assert calls == [2]
