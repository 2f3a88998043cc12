"""The row padding mode (zv_set_padding(ZV_PAD_ROW), HipEngine.padding / model.padding = "row") on the
default-size synthetic models, T <= 97.

In "batch" mode (the default, the reference's behaviour on a padded batch) the decoder's downsampling lets
the frames past a row's end into the row's last valid frames; in "row" mode every row is downsampled as the
reference downsamples it alone.

1. Independence: lens [71, 50, 33] at T = 71 with noise past the rows' ends, and the same inputs zeroed
   past the ends: in "row" mode the valid frames of euler_sample, euler_sample_sched and fm_decoder are the
   same bits; in "batch" mode rows 1 and 2 differ (the inputs do exercise the leak).
2. Each row is the row alone: "row" mode on the noisy batch against the CPU oracle on each row alone at
   T = its length, within the fp32 bound of tests/test_gpu_fullsize.py (mean 1e-3, max 3e-2).
3. Session: the staggered admission of tests/test_gpu_session.py with a D of 62 frames and the oracle given
   every row alone at its own length; zv_set_padding is rejected while a slot is occupied; a warm admit,
   three ticks and a retire in "row" mode make no host-blocking call.
4. Graph: a solve captured in "batch" mode is not replayed in "row" mode, and the other way round.
5. Public surface: model.sample with seeds (batch against each item alone), ContinuousBatcher(padding="row")
   (a request alone against the same request beside two longer ones), bad mode strings.

The models of test_gpu_fullsize are shared with the other test modules: every test here leaves them in
"batch" mode."""
import contextlib
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_fullsize as fs  # noqa: E402
from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.solver import RowSchedule  # noqa: E402

LENS = [71, 50, 33]
MIXED = [RowSchedule(3, 1.0, t_shift=0.5), RowSchedule(1, 0.0, t_shift=1.0), RowSchedule(2, 2.5, 0.25, 0.9, 0.7)]
MIXED_DISTILL = [RowSchedule(3, 1.0, t_shift=0.5), RowSchedule(1, 3.0, t_shift=1.0), RowSchedule(2, 2.5, 0.25, 0.9, 0.7)]


@contextlib.contextmanager
def padding(target, mode):
    """target.padding = mode inside the block, "batch" after it (target: an engine or a model)."""
    target.padding = mode
    try:
        yield target
    finally:
        target.padding = "batch"


def noisy_and_zeroed(seed):
    """fs.inputs(3, 71, 100, LENS) as they come (noise past the rows' ends) and with x, text and speech zeroed
    there: (host noisy, device noisy, device zeroed)."""
    host = fs.inputs(3, 71, 100, LENS, seed=seed)
    zeroed = [a.copy() for a in host]
    for a in zeroed[:3]:
        a[host[3]] = 0
    return host, tuple(fs.cuda(a) for a in host), tuple(fs.cuda(a) for a in zeroed)


def ops(eng, distill):
    sched = MIXED_DISTILL if distill else MIXED
    t = torch.tensor([0.3, 0.6, 0.1], device="cuda:0")
    g = torch.tensor([1.0, 3.0, 2.0], device="cuda:0") if distill else None
    return {"euler_sample": lambda d: eng.euler_sample(*d, 2, 1.0, t_shift=0.5),
            "euler_sample_sched": lambda d: eng.euler_sample_sched(*d, sched),
            "fm_decoder": lambda d: eng.fm_decoder(t, *d, guidance=g)}


@pytest.mark.parametrize("variant,precision", [("zipvoice", "fp32"), ("zipvoice", "bf16"), ("zipvoice_distill", "fp32")])
def test_valid_frames_do_not_depend_on_what_lies_past_the_end(variant, precision):
    eng = fs.model(variant, precision).engine
    _, noisy, zeroed = noisy_and_zeroed(61)
    assert eng.padding == "batch"
    for name, f in ops(eng, variant == "zipvoice_distill").items():
        a, b = f(noisy), f(zeroed)                         # batch mode: the leak
        d = [(a[r, :n] - b[r, :n]).abs().max().item() for r, n in enumerate(LENS)]
        print(f"{variant} {precision} {name} batch mode: max |noisy - zeroed| per row = {d}")
        assert torch.equal(a[0, :71], b[0, :71]), name     # (the full row has nothing past its end)
        assert not torch.equal(a[1, :50], b[1, :50]) and not torch.equal(a[2, :33], b[2, :33]), name
        with padding(eng, "row"):
            assert eng.padding == "row"
            a, b = f(noisy), f(zeroed)
        assert torch.isfinite(a).all()
        for r, n in enumerate(LENS):
            assert torch.equal(a[r, :n], b[r, :n]), (variant, precision, name, r)
    assert eng.padding == "batch"


@pytest.mark.parametrize("variant", ["zipvoice", "zipvoice_distill"])
def test_each_row_is_the_row_alone(variant):
    """The same comparison in "batch" mode (the only behaviour before the mode existed) is printed, not
    asserted: rows 1 and 2 miss the bound by two orders of magnitude (zipvoice: mean 0.24 / 0.39, max 2.4 /
    4.6 against 1e-3 / 3e-2; row mode: mean 2e-5, max 9e-5 on every row)."""
    eng = fs.model(variant, "fp32").engine
    host, noisy, _ = noisy_and_zeroed(62)
    g = 3.0 if variant == "zipvoice_distill" else 1.0
    run = lambda: eng.euler_sample(*noisy, 3, g, t_shift=0.5)
    leak = run()
    with padding(eng, "row"):
        got = run()
    o = fs.oracle(variant)
    x, tc, sc, pm = host
    for r, n in enumerate(LENS):
        ref = o.euler(x[r:r + 1, :n], tc[r:r + 1, :n], sc[r:r + 1, :n], pm[r:r + 1, :n], 3, g, t_shift=0.5)
        e = np.abs(leak[r:r + 1, :n].cpu().numpy() - ref)
        print(f"{variant} row {r} (n = {n}) batch mode vs the oracle alone: mean={e.mean():.3e} max={e.max():.3e}")
        fs.check(got[r:r + 1, :n], ref, "fp32", f"{variant} row {r} (n = {n}) row mode vs the oracle alone")


def batch1(n, seed):
    """One row of n frames at T = n (host, device)."""
    host = fs.inputs(1, n, 100, [n], seed=seed)
    return host, tuple(fs.cuda(a) for a in host)


@pytest.mark.parametrize("variant", ["zipvoice", "zipvoice_distill"])
def test_staggered_admission_vs_oracle_alone(variant):
    distill = variant == "zipvoice_distill"
    lens = dict(A=71, B=50, C=33, D=62)
    sched = dict(A=RowSchedule(3, 1.0, t_shift=0.5), B=RowSchedule(2, 3.0 if distill else 0.0, t_shift=1.0),
                 C=RowSchedule(1, 2.5, 0.25, 0.9, 0.7), D=RowSchedule(2, 0.7, t_shift=0.5))
    host, dev = {}, {}
    for i, name in enumerate(lens):
        host[name], dev[name] = batch1(lens[name], 45 + i)
    eng = fs.model(variant, "fp32").engine
    with padding(eng, "row"):
        sess = eng.open_session(3, 97)
        try:
            admit = lambda slot, name: sess.admit([slot], *dev[name][:3], [lens[name]], [sched[name]])
            admit(0, "A")
            with pytest.raises(RuntimeError, match="occupied"):
                eng.padding = "batch"                      # a row is in flight
            assert eng.padding == "row"
            sess.step()                                    # tick 0: A
            admit(1, "B")
            admit(2, "C")
            sess.step()                                    # tick 1: A, B, C
            assert sess.steps_left() == [1, 1, 0]
            got = dict(C=sess.retire([2]))
            admit(2, "D")                                  # into C's slot
            sess.step()                                    # tick 2: A, B, D
            assert sess.steps_left() == [0, 0, 1] and sess.stats()[3] == 71
            sess.step()                                    # tick 3: D alone, at its own length
            assert sess.steps_left() == [0, 0, 0] and sess.stats()[0] == 4 and sess.stats()[3] == 62
            with pytest.raises(RuntimeError, match="occupied"):
                eng.padding = "batch"                      # finished, but not yet retired
            out = sess.retire([0, 1, 2])
            got.update(A=out[0:1], B=out[1:2], D=out[2:3])
            eng.padding = "batch"                          # every slot is free: the mode may change
            eng.padding = "row"
        finally:
            sess.close()
    o = fs.oracle(variant)
    for name, r in sched.items():
        x, tc, sc, pm = host[name]
        ref = o.euler(x, tc, sc, pm, r.num_step, r.guidance_scale, t_start=r.t_start, t_end=r.t_end, t_shift=r.t_shift)
        n = lens[name]
        fs.check(got[name][:, :n], ref, "fp32", f"{variant} row mode, staggered row {name} vs the oracle alone at T = {n}")


def test_warm_ticks_in_row_mode_do_not_block_the_host():
    host = fs.inputs(3, 71, 100, LENS, seed=49)
    x, tc, sc, _ = (fs.cuda(a) for a in host)
    eng = fs.model("zipvoice", "bf16").engine
    with padding(eng, "row"):
        sess = eng.open_session(4, 97)

        def round_trip():
            sess.admit([0, 1, 3], x, tc, sc, LENS, MIXED)
            for _ in range(3):
                sess.step()
            return sess.retire([0, 1, 3], 71)

        try:
            want = round_trip()
            torch.cuda.synchronize()
            again = round_trip()
            torch.cuda.synchronize()
            assert torch.equal(want, again)
            gc.collect()
            torch.cuda.synchronize()
            gc.disable()
            try:
                c0 = engine.host_block_count()
                got = round_trip()
                c1 = engine.host_block_count()
            finally:
                gc.enable()
            torch.cuda.synchronize()
            print(f"host-blocking engine calls in a warm admit, three ticks and a retire in row mode: {c1 - c0}")
            assert c1 - c0 == 0
            assert torch.equal(got, want)
        finally:
            sess.close()


def test_a_captured_solve_is_not_replayed_in_the_other_mode(monkeypatch):
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    from zipvoice_amd.weights import synthetic_state_dict
    _, noisy, _ = noisy_and_zeroed(63)
    eng = fs.model("zipvoice", "fp32").engine
    solve = lambda e: e.euler_sample(*noisy, 2, 1.0, t_shift=0.5)
    first = solve(eng)                                     # batch mode: the shape's uncaptured warm-up,
    assert torch.equal(solve(eng), first)                  # captured,
    assert torch.equal(solve(eng), first)                  # and replayed
    with padding(eng, "row"):
        row = [solve(eng) for _ in range(3)]               # warm-up, capture, replay in row mode
    again = solve(eng)
    assert torch.equal(again, first)
    assert torch.equal(row[0], row[1]) and torch.equal(row[0], row[2])
    assert not torch.equal(row[0][1, :50], first[1, :50])
    monkeypatch.setenv("ZV_GRAPH", "0")                    # an engine that never captures
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="fp32", padding="row")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    plain = m.to("cuda:0").engine
    assert plain.padding == "row"
    assert torch.equal(solve(plain), row[0])


def sample_inputs():
    rng = np.random.default_rng(5)
    plens = torch.tensor([30, 22, 26])
    pf = torch.from_numpy(rng.standard_normal((3, 30, 100)).astype(np.float32)).cuda() * 0.3
    for b, n in enumerate(plens.tolist()):
        pf[b, n:] = 0
    ptoks = [list(range(40, 52)), list(range(60, 69)), list(range(30, 40))]
    toks = [[int(t) for t in rng.integers(10, 90, n)] for n in (24, 21, 19)]
    return plens, pf, ptoks, toks


def test_model_sample_batch_is_each_item_alone():
    from zipvoice_amd.common import predict_features_lens
    m = fs.model("zipvoice", "fp32")
    plens, pf, ptoks, toks = sample_inputs()
    fl = predict_features_lens(plens, torch.tensor([len(p) for p in ptoks]), torch.tensor([len(t) for t in toks]), 1.0)
    assert max(fl.tolist()) <= 97 and any(v % 4 for v in fl.tolist()), fl.tolist()
    assert sum(v != max(fl.tolist()) and v % 4 != 0 for v in fl.tolist()) >= 1, "a shorter row must end inside a group"
    seeds = [11, 12, 13]
    kw = dict(speed=1.0, t_shift=0.5, duration="predict", num_step=2, guidance_scale=1.0)
    run = lambda idx: m.sample(tokens=[toks[i] for i in idx], prompt_tokens=[ptoks[i] for i in idx],
                               prompt_features=pf[idx, :int(plens[idx].max())], prompt_features_lens=plens[idx],
                               seeds=[seeds[i] for i in idx], **kw)
    batch_mode = run([0, 1, 2])
    with padding(m, "row"):
        assert m.engine.padding == "row"
        pred, pred_lens, _, _ = run([0, 1, 2])
        alone = [run([i]) for i in range(3)]
    assert m.padding == "batch" and m.engine.padding == "batch"
    for i in range(3):
        n = int(pred_lens[i])
        assert n == int(alone[i][1][0]) == int(fl[i] - plens[i])
        ref = alone[i][0][0, :n].cpu().numpy()
        e = np.abs(batch_mode[0][i, :n].cpu().numpy() - ref)
        print(f"item {i} ({int(fl[i])} frames) batch mode, batch vs alone: mean={e.mean():.3e} max={e.max():.3e}")
        fs.check(pred[i, :n], ref, "fp32", f"model.sample row mode, item {i} ({int(fl[i])} frames) in the batch vs alone")


def test_continuous_batcher_row_mode():
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.serving import ContinuousBatcher
    from zipvoice_amd.vocoder import Vocos
    m = fs.model("zipvoice", "fp32")
    voc, fx = Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()
    rng = np.random.default_rng(37)
    items = [([int(t) for t in rng.integers(10, 90, n)], list(range(40, 40 + p)),
              (0.1 * rng.standard_normal(w)).astype(np.float32)) for n, p, w in ((8, 9, 8000), (8, 8, 9600), (9, 8, 9600))]    # 45, 57 and 60 frames at speed 2
    kw = dict(num_step=2, guidance_scale=1.0, speed=2.0, t_shift=0.5)

    def mel_of(ticket, cb):
        mels = {}
        while sum(cb.pending()):
            cb.step()
            mels.update(dict(cb.last_mel))
        return mels[ticket]

    try:
        with pytest.raises(ValueError):
            ContinuousBatcher(m, voc, fx, max_rows=3, max_frames=97, padding="rows")
        assert m.padding == "batch"
        cb = ContinuousBatcher(m, voc, fx, max_rows=3, max_frames=97, padding="row")
        assert m.padding == "row" and m.engine.padding == "row"
        frames = [cb._frames(*it, None, 2.0)[1] for it in items]
        assert frames[0] < min(frames[1:]) and frames[0] % 4 != 0, frames
        alone = mel_of(cb.submit(*items[0], seed=5, **kw), cb).clone()
        for it, s in zip(items[1:], (6, 7)):               # two longer requests first, already in flight ...
            cb.submit(*it, seed=s, **dict(kw, num_step=3))
        cb.step()
        assert cb.pending() == (0, 2)
        beside = mel_of(cb.submit(*items[0], seed=5, **kw), cb)   # ... when the same request and seed come in
        cb.close()
        cb = ContinuousBatcher(m, voc, fx, max_rows=1, max_frames=97)       # None leaves the model's mode
        assert m.padding == "row" and m.engine.padding == "row"
        cb.close()
        print(f"request of {frames[0]} frames beside {frames[1:]}")
        fs.check(beside, alone.float().cpu().numpy(), "fp32", "ContinuousBatcher row mode, a request beside two longer vs alone (mel)")
    finally:
        gc.collect()                                       # (the batchers' sessions close with them)
        m.padding = "batch"


def test_bad_mode_strings_raise():
    m = fs.model("zipvoice", "fp32")
    for bad in ("rows", "", None, 1):
        with pytest.raises(ValueError):
            m.padding = bad
        with pytest.raises(ValueError):
            m.engine.padding = bad
    assert m.padding == "batch" and m.engine.padding == "batch"
    assert m.engine.lib.zv_set_padding(m.engine.h, 2) != 0 and m.engine.lib.zv_get_padding(m.engine.h) == 0
