"""The scheduled solve (zv_euler_sample_sched: every row with its own step count, grid and guidance scale
in one call) on the default-size synthetic model, T <= 97.

* A uniform schedule is today's solve, bit for bit: against engine.euler_sample with the same scalars,
  and with per-row scales against the (B, 1, 1)-tensor path (zipvoice fp32 / bf16, distill fp32).
* A mixed pool against the CPU oracle run on each row alone with that row's scalars, on valid frames,
  held to the fp32 bound of tests/test_gpu_fullsize.py (mean < 1e-3, max < 3e-2).
* A finished row is left alone and skipped: its result does not depend on how long the others run, and
  zv_sched_stats reports the plan's sum of (copies + active) rows and its step count.
* A warm scheduled solve makes no host-blocking runtime call and no synchronising torch op; two
  different schedules queued back to back each equal their own synchronised run.
* The public entries: model.sample and generate_batch with per-row sequences."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_fullsize as fs  # noqa: E402
from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.solver import RowSchedule  # noqa: E402

T = 71
MIXED = [RowSchedule(3, 1.0, t_shift=0.5), RowSchedule(1, 0.0, t_shift=1.0),
         RowSchedule(2, 2.5, 0.25, 0.9, 0.7), RowSchedule(3, 0.0, t_shift=0.5)]
MIXED_DISTILL = [RowSchedule(3, 1.0, t_shift=0.5), RowSchedule(1, 3.0, t_shift=1.0),
                 RowSchedule(2, 2.5, 0.25, 0.9, 0.7), RowSchedule(3, 0.5, t_shift=0.5)]


def batch(B, lens, seed):
    x, tc, sc, pm = fs.inputs(B, T, 100, lens, seed=seed)
    return (x, tc, sc, pm), tuple(fs.cuda(a) for a in (x, tc, sc, pm))


def plan_totals(sched, distill):
    """(decoder rows, steps) of a schedule, from the rules: active rows plus guided active rows per step."""
    K = max(r.num_step for r in sched)
    rows = sum(sum(1 + int(not distill and r.guidance_scale != 0) for r in sched if k < r.num_step) for k in range(K))
    return rows, K


@pytest.mark.parametrize("variant,precision", [("zipvoice", "fp32"), ("zipvoice", "bf16"), ("zipvoice_distill", "fp32")])
def test_uniform_schedule_is_the_existing_solve(variant, precision):
    B, lens = 3, [71, 50, 33]
    _, (x, tc, sc, pm) = batch(B, lens, seed=31)
    eng = fs.model(variant, precision).engine
    ref = eng.euler_sample(x, tc, sc, pm, 3, 1.0, t_shift=0.5)
    got = eng.euler_sample_sched(x, tc, sc, pm, [RowSchedule(3, 1.0, t_shift=0.5)] * B)
    assert torch.isfinite(got).all() and not torch.equal(got, x)
    assert torch.equal(got, ref)
    assert eng.sched_stats() == plan_totals([RowSchedule(3, 1.0)] * B, variant == "zipvoice_distill")
    gs = [1.0, 2.5, 0.7]
    ref = eng.euler_sample(x, tc, sc, pm, 3, torch.tensor(gs).reshape(B, 1, 1), t_shift=0.5)
    got = eng.euler_sample_sched(x, tc, sc, pm, [RowSchedule(3, g, t_shift=0.5) for g in gs])
    assert torch.equal(got, ref)


@pytest.mark.parametrize("variant", ["zipvoice", "zipvoice_distill"])
def test_mixed_pool_vs_oracle_per_row(variant):
    B, lens = 4, [71, 50, 33, 64]
    sched = MIXED_DISTILL if variant == "zipvoice_distill" else MIXED
    (x, tc, sc, pm), dev = batch(B, lens, seed=32)
    eng = fs.model(variant, "fp32").engine
    got = eng.euler_sample_sched(*dev, sched)
    assert eng.sched_stats() == plan_totals(sched, variant == "zipvoice_distill")
    if variant == "zipvoice":
        assert eng.sched_stats() == (14, 3)          # against 2 * 4 * 3 = 24 at the most expensive setting
    o = fs.oracle(variant)
    ref = np.concatenate([o.euler(x[b:b + 1], tc[b:b + 1], sc[b:b + 1], pm[b:b + 1], r.num_step, r.guidance_scale,
                                  t_start=r.t_start, t_end=r.t_end, t_shift=r.t_shift)
                          for b, r in enumerate(sched)])
    fs.check(got, ref, "fp32", f"{variant} mixed pool vs the oracle per row", valid=~pm)


def test_finished_rows_are_left_alone_and_skipped():
    B, lens = 2, [71, 50]
    _, dev = batch(B, lens, seed=33)
    eng = fs.model("zipvoice", "fp32").engine
    short = eng.euler_sample_sched(*dev, [RowSchedule(1, 1.0, t_shift=0.5), RowSchedule(1, 1.0, t_shift=0.5)])
    assert eng.sched_stats() == (4, 1)
    # row 1 runs on: a step of 3 has another dt, so row 1 differs; row 0's only step saw the same decoder batch
    longer = eng.euler_sample_sched(*dev, [RowSchedule(1, 1.0, t_shift=0.5), RowSchedule(3, 1.0, t_shift=0.5)])
    assert eng.sched_stats() == (4 + 2 + 2, 3)
    assert torch.equal(short[0], longer[0])
    assert not torch.equal(short[1], longer[1])
    # the same with the finished row unguided: one decoder row for it
    eng.euler_sample_sched(*dev, [RowSchedule(1, 0.0), RowSchedule(3, 1.0, t_shift=0.5)])
    assert eng.sched_stats() == (3 + 2 + 2, 3)


def test_rejections_raise():
    _, dev = batch(2, [71, 50], seed=33)
    eng = fs.model("zipvoice", "fp32").engine
    with pytest.raises(ValueError):
        eng.euler_sample_sched(*dev, [RowSchedule(1)])
    with pytest.raises(ValueError):
        eng.euler_sample_sched(*dev, [RowSchedule(1), RowSchedule(0)])
    with pytest.raises(ValueError):
        eng.euler_sample_sched(*dev, [RowSchedule(1), RowSchedule(2, t_shift=0.0)])


def test_warm_scheduled_solve_has_no_host_block():
    B, lens = 4, [71, 50, 33, 64]
    _, dev = batch(B, lens, seed=34)
    eng = fs.model("zipvoice", "bf16").engine
    other = [RowSchedule(2, 0.7, t_shift=0.5), RowSchedule(3, 0.0), RowSchedule(1, 1.0), RowSchedule(2, 2.0, t_shift=0.7)]
    want_a = eng.euler_sample_sched(*dev, MIXED)
    want_b = eng.euler_sample_sched(*dev, other)
    torch.cuda.synchronize()

    torch.cuda.set_sync_debug_mode("error")          # the guard must really catch a synchronising op
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda:0").item()
        guarded = True
    except pytest.fail.Exception:
        guarded = False
    finally:
        torch.cuda.set_sync_debug_mode("default")

    gc.collect()
    torch.cuda.synchronize()
    gc.disable()
    try:
        c0 = engine.host_block_count()
        if guarded:
            torch.cuda.set_sync_debug_mode("error")
        # two different schedules queued back to back, no sync between: each sees its own tables
        got_a = eng.euler_sample_sched(*dev, MIXED)
        got_b = eng.euler_sample_sched(*dev, other)
        c1 = engine.host_block_count()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    torch.cuda.synchronize()
    print(f"host-blocking engine calls in two warm scheduled solves: {c1 - c0}; torch sync guard "
          f"{'on' if guarded else 'unavailable on this build'}")
    assert c1 - c0 == 0
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
    assert not torch.equal(want_a, want_b)


@pytest.fixture(scope="module")
def request_batch():
    rng = np.random.default_rng(35)
    plens = torch.tensor([40, 33, 38])
    pf = torch.from_numpy(rng.standard_normal((3, 40, 100)).astype(np.float32)).cuda() * 0.3
    ptoks = [list(range(40, 48)), list(range(60, 67)), list(range(30, 39))]
    toks = [[int(t) for t in rng.integers(10, 90, n)] for n in (9, 8, 10)]
    return toks, ptoks, pf, plens


def test_model_sample_with_per_row_settings(request_batch):
    from oracle.zipvoice_np import ZipVoiceOracle
    toks, ptoks, pf, plens = request_batch
    m = fs.model("zipvoice", "fp32")
    steps, gs, shifts, speeds = [3, 1, 2], [1.0, 0.0, 2.5], [0.5, 1.0, 0.7], [1.0, 1.3, 0.8]
    want_lens = [int(ZipVoiceOracle.predict_features_lens(plens[b:b + 1].numpy(), np.array([len(ptoks[b])]),
                                                          np.array([len(toks[b])]), speeds[b])[0]) for b in range(3)]
    Tn = max(want_lens)
    assert Tn <= 97 and len(set(want_lens)) == 3
    x0 = torch.from_numpy(np.random.default_rng(36).standard_normal((3, Tn, 100)).astype(np.float32)).cuda()
    kw = dict(tokens=toks, prompt_tokens=ptoks, prompt_features=pf, prompt_features_lens=plens, duration="predict")
    pred, pred_lens, prm, prm_lens = m.sample(**kw, num_step=steps, guidance_scale=gs, t_shift=shifts, speed=speeds, x0=x0)
    assert (pred_lens.cpu() + plens).tolist() == want_lens
    # by hand: the text path with the per-row speeds, then the scheduled solve
    from zipvoice_amd.models import split_prompt
    tc, pm = m.forward_text_inference_ratio_duration(tokens=toks, prompt_tokens=ptoks,
                                                     prompt_features_lens=plens.cuda(),
                                                     speed=torch.tensor(speeds, dtype=torch.float32, device="cuda:0"))
    assert tc.shape[1] == Tn and (~pm).sum(-1).tolist() == want_lens
    sc = m.engine.speech_condition(pf, plens.cuda(), Tn)
    x1 = m.solver.sample_rows(x=x0, text_condition=tc, speech_condition=sc, padding_mask=pm,
                              schedule=[RowSchedule(n, g, t_shift=s) for n, g, s in zip(steps, gs, shifts)])
    hand = split_prompt(x1, plens.cuda(), (~pm).sum(-1) - plens.cuda())
    assert torch.equal(pred, hand[0]) and torch.equal(pred_lens, hand[1]) and torch.equal(prm, hand[2])
    assert torch.isfinite(pred).all() and pred.abs().max() > 0
    # one sequence is enough to schedule; the scalars broadcast
    a = m.sample(**kw, num_step=[2, 2, 2], guidance_scale=1.0, t_shift=0.5, speed=1.0, x0=x0[:, :m_frames(m, kw)])
    b = m.sample(**kw, num_step=2, guidance_scale=1.0, t_shift=0.5, speed=1.0, x0=x0[:, :m_frames(m, kw)])
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    for bad in (dict(num_step=[2, 2]), dict(guidance_scale=[1.0] * 4), dict(t_shift=[0.5]), dict(speed=[1.0, 1.0])):
        with pytest.raises(ValueError):
            m.sample(**{**kw, **dict(num_step=2, guidance_scale=1.0, t_shift=0.5, speed=1.0), **bad})


def m_frames(m, kw):
    """The padded length of the batch at speed 1."""
    from zipvoice_amd.common import predict_features_lens
    fl = predict_features_lens(kw["prompt_features_lens"], torch.tensor([len(p) for p in kw["prompt_tokens"]]),
                               torch.tensor([len(t) for t in kw["tokens"]]), 1.0)
    return int(fl.max())


def test_generate_batch_with_per_item_settings():
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.infer import generate_batch
    from zipvoice_amd.vocoder import Vocos
    m = fs.model("zipvoice", "bf16")
    voc, fx = Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()
    rng = np.random.default_rng(37)
    items = [([int(t) for t in rng.integers(10, 90, n)], list(range(40, 40 + p)),
              (0.1 * rng.standard_normal(w)).astype(np.float32)) for n, p, w in ((8, 8, 9600), (7, 9, 8000))]
    seeds = [5, 6]
    # speed 2 is a power of two, so dividing by it as a tensor and as a scalar round alike
    a, _ = generate_batch(items, m, voc, fx, num_step=2, guidance_scale=1.0, speed=2.0, t_shift=0.5, seeds=seeds)
    b, _ = generate_batch(items, m, voc, fx, num_step=[2, 2], guidance_scale=[1.0, 1.0], speed=[2.0, 2.0],
                          t_shift=[0.5, 0.5], seeds=seeds)
    assert len(a) == len(b) == 2 and all(torch.equal(u, v) for u, v in zip(a, b))
    assert all(u.numel() > 0 and torch.isfinite(u).all() for u in a)
    c, _ = generate_batch(items, m, voc, fx, num_step=[2, 1], guidance_scale=[1.0, 0.0], speed=2.0, t_shift=0.5,
                          seeds=seeds)
    assert [u.shape for u in c] == [u.shape for u in a]            # the lengths follow the speed alone
    assert not torch.equal(c[1], a[1]) and torch.isfinite(c[1]).all()
    for bad in (dict(num_step=[2]), dict(guidance_scale=[1.0] * 3), dict(speed=[1.0]), dict(t_shift=[0.5] * 3)):
        with pytest.raises(ValueError):
            generate_batch(items, m, voc, fx, **{**dict(num_step=2, seeds=seeds), **bad})
