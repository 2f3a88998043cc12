"""The solve session (zv_session_*: continuous batching) and serving.ContinuousBatcher on the default-size
synthetic models, T <= 97, at most 4 slots.

* Rows all admitted before the first tick run the scheduled solve's decoder batches: bit-identical to
  engine.euler_sample_sched at T = max len on valid frames (zipvoice fp32 / bf16, distill fp32).  Admit
  zero-fills a slot past the row's length, and the decoder's downsampling lets the frames just past a
  row's end into its last valid frames (SimpleDownsample groups ds frames, as the reference's), so the
  inputs of this comparison are zero past each row's length on both sides.
* A slot is reused: each row equals its own one-row scheduled solve at T = its length, and the second
  row does not depend on the first having been there.
* Rows admitted at different ticks each match the CPU oracle on that row alone with its own scalars, on
  valid frames, within the fp32 bound of tests/test_gpu_fullsize.py (the scheduled solve's bound).  The
  oracle sees what the session's decoder saw: rows A, B, C run every tick at T_k = 71 with zero padding,
  so their oracle input is that; row D outlives A (its last tick runs at T_k = 64, its own length) and
  has a length divisible by every downsampling factor, which makes its valid frames independent of the
  padded length.
* A warm admit, three ticks and a retire make no host-blocking runtime call and no synchronising torch op.
* Rejections raise ValueError and leave the session usable; a session whose engine is gone raises.
* ContinuousBatcher against infer.generate_batch."""
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


def batch(lens, seed, T=None):
    """fs.inputs with x, text and speech zero past each row's length (what admit leaves in a slot)."""
    T = max(lens) if T is None else T
    x, tc, sc, pm = fs.inputs(len(lens), T, 100, lens, seed=seed)
    for a in (x, tc, sc):
        a[pm] = 0
    return (x, tc, sc, pm), tuple(fs.cuda(a) for a in (x, tc, sc, pm))


def plan_rows(sched, distill, k):
    return sum(1 + int(not distill and r.guidance_scale != 0) for r in sched if k < r.num_step)


def run_all(sess, slots, dev, lens, sched):
    """Admit, tick until every row is done, retire: (rows (n, T, Fx), stats after the first tick, after the last)."""
    x, tc, sc, _ = dev
    sess.admit(slots, x, tc, sc, lens, sched)
    first = None
    while max(sess.steps_left()) > 0:
        sess.step()
        first = first or sess.stats()
    return sess.retire(slots), first, sess.stats()


@pytest.mark.parametrize("variant,precision", [("zipvoice", "fp32"), ("zipvoice", "bf16"), ("zipvoice_distill", "fp32")])
def test_all_at_once_is_the_scheduled_solve(variant, precision):
    distill = variant == "zipvoice_distill"
    sched = MIXED_DISTILL if distill else MIXED
    _, dev = batch(LENS, seed=41)
    eng = fs.model(variant, precision).engine
    ref = eng.euler_sample_sched(*dev, sched)
    sess = eng.open_session(4, 97)
    slots = [0, 2, 3]                                  # a free slot between them: the map does the compaction
    assert sess.steps_left() == [-1] * 4 and sess.stats() == (0, 0, 0, 0)
    got, first, last = run_all(sess, slots, dev, LENS, sched)
    assert first == (1, plan_rows(sched, distill, 0), plan_rows(sched, distill, 0) * 71, 71)
    assert last[:2] == (3, sum(plan_rows(sched, distill, k) for k in range(3))) and last[3] == 71
    assert last[:2] == tuple(reversed(eng.sched_stats()))
    assert got.shape == ref.shape and torch.isfinite(got).all()
    for b, n in enumerate(LENS):
        assert torch.equal(got[b, :n], ref[b, :n]), (variant, precision, b)
        assert not torch.equal(got[b, :n], dev[0][b, :n])
        assert (got[b, n:] == 0).all()
    assert sess.steps_left() == [-1] * 4
    sess.step()                                        # nothing active: nothing runs
    assert sess.stats() == last
    sess.close()


def test_tick_length_follows_the_active_rows():
    """The 71-frame row finishes first: the later ticks run at the longest remaining length."""
    sched = [RowSchedule(1, 1.0, t_shift=0.5), RowSchedule(3, 1.0, t_shift=0.5), RowSchedule(2, 0.0)]
    _, dev = batch(LENS, seed=42)
    eng = fs.model("zipvoice", "fp32").engine
    sess = eng.open_session(3, 97)
    got, first, last = run_all(sess, [0, 1, 2], dev, LENS, sched)
    assert first == (1, 5, 5 * 71, 71)
    assert last == (3, 5 + 3 + 2, 5 * 71 + 3 * 50 + 2 * 50, 50)
    assert torch.isfinite(got).all()
    sess.close()


def test_slot_reuse():
    eng = fs.model("zipvoice", "fp32").engine
    (_, _, _, _), a = batch([71], seed=43)
    (_, _, _, _), b = batch([50], seed=44)
    sa, sb = [RowSchedule(2, 1.0, t_shift=0.5)], [RowSchedule(3, 2.5, t_shift=0.7)]
    sess = eng.open_session(1, 97)
    got_a, _, _ = run_all(sess, [0], a, [71], sa)
    got_b, _, _ = run_all(sess, [0], b, [50], sb)      # into the slot row A has just left
    sess.close()
    fresh = eng.open_session(1, 97)
    alone_b, _, _ = run_all(fresh, [0], b, [50], sb)
    fresh.close()
    assert torch.equal(got_a, eng.euler_sample_sched(*a, sa))
    assert torch.equal(got_b, eng.euler_sample_sched(*b, sb))
    assert torch.equal(got_b, alone_b)
    assert got_a.shape == (1, 71, 100) and got_b.shape == (1, 50, 100)


def test_graph_replay_between_ticks_changes_nothing():
    """A captured scalar solve at another length replayed between the ticks: the replay writes the stacks'
    positional projections for its own length from the graph, without the host code that keeps their
    reuse key, so a tick must not trust what an earlier tick left there."""
    eng = fs.model("zipvoice", "fp32").engine
    _, row = batch([50], seed=52)
    _, other = batch([71], seed=53)
    sched = [RowSchedule(3, 1.0, t_shift=0.5)]
    solve = lambda: eng.euler_sample(*other, 2, 1.0, t_shift=0.5)
    first = solve()                                    # the shape's uncaptured warm-up
    assert torch.equal(solve(), first)                 # captured and replayed
    sess = eng.open_session(2, 97)                     # (moves the workspace: the next solve captures again)
    solve()
    want, _, _ = run_all(sess, [1], row, [50], sched)
    assert torch.equal(want, eng.euler_sample_sched(*row, sched))
    sess.admit([1], *row[:3], [50], sched)
    for _ in range(3):
        sess.step()
        assert torch.equal(solve(), first)             # a replay, at T = 71, between two ticks at T_k = 50
    got = sess.retire([1])
    sess.close()
    assert torch.equal(got, want)


@pytest.mark.parametrize("variant", ["zipvoice", "zipvoice_distill"])
def test_staggered_admission_vs_oracle_per_row(variant):
    distill = variant == "zipvoice_distill"
    lens = dict(A=71, B=50, C=33, D=64)
    sched = dict(A=RowSchedule(3, 1.0, t_shift=0.5), B=RowSchedule(2, 3.0 if distill else 0.0, t_shift=1.0),
                 C=RowSchedule(1, 2.5, 0.25, 0.9, 0.7), D=RowSchedule(2, 0.7, t_shift=0.5))
    host, dev = {}, {}
    for i, (name, T) in enumerate(dict(A=71, B=71, C=71, D=64).items()):
        host[name], dev[name] = batch([lens[name]], seed=45 + i, T=T)
    eng = fs.model(variant, "fp32").engine
    sess = eng.open_session(3, 97)
    admit = lambda slot, name: sess.admit([slot], *dev[name][:3], [lens[name]], [sched[name]])
    admit(0, "A")
    sess.step()                                        # tick 0: A
    bc = [torch.cat([dev["B"][i], dev["C"][i]]) for i in range(3)]
    sess.admit([1, 2], *bc, [lens["B"], lens["C"]], [sched["B"], sched["C"]])
    sess.step()                                        # tick 1: A, B, C
    assert sess.steps_left() == [1, 1, 0]
    got = dict(C=sess.retire([2]))
    admit(2, "D")                                      # into C's slot
    sess.step()                                        # tick 2: A, B, D
    assert sess.steps_left() == [0, 0, 1] and sess.stats()[3] == 71
    sess.step()                                        # tick 3: D alone, at its own length
    assert sess.steps_left() == [0, 0, 0] and sess.stats()[0] == 4 and sess.stats()[3] == 64
    out = sess.retire([0, 1, 2])
    got.update(A=out[0:1], B=out[1:2], D=out[2:3])
    sess.close()
    o = fs.oracle(variant)
    for name, r in sched.items():
        x, tc, sc, pm = host[name]
        ref = o.euler(x, tc, sc, pm, r.num_step, r.guidance_scale, t_start=r.t_start, t_end=r.t_end, t_shift=r.t_shift)
        n = lens[name]
        fs.check(got[name][:, :n], ref[:, :n], "fp32", f"{variant} staggered row {name} vs the oracle alone")


def test_warm_ticks_do_not_block_the_host():
    _, dev = batch(LENS, seed=49)
    eng = fs.model("zipvoice", "bf16").engine
    sess = eng.open_session(4, 97)
    x, tc, sc, _ = dev

    def round_trip():
        sess.admit([0, 1, 3], x, tc, sc, LENS, MIXED)
        for _ in range(3):
            sess.step()
        return sess.retire([0, 1, 3], 71)

    want = round_trip()
    torch.cuda.synchronize()
    again = round_trip()                               # (a second warm-up: the session is as it will be below)
    torch.cuda.synchronize()
    assert torch.equal(want, again)

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
        got = round_trip()
        left = sess.steps_left()
        c1 = engine.host_block_count()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    torch.cuda.synchronize()
    print(f"host-blocking engine calls in a warm admit, three ticks and a retire: {c1 - c0}; torch sync guard "
          f"{'on' if guarded else 'unavailable on this build'}")
    assert c1 - c0 == 0
    assert left == [-1] * 4
    assert torch.equal(got, want) and not torch.equal(got[:, :33], x[:, :33])
    sess.close()


def test_rejections_leave_the_session_usable():
    _, dev = batch(LENS, seed=50)
    x, tc, sc, _ = dev
    eng = fs.model("zipvoice", "fp32").engine
    want = eng.euler_sample_sched(*dev, MIXED)
    sess = eng.open_session(4, 97)
    one = lambda slot, n=33, r=MIXED[2]: sess.admit([slot], x[2:], tc[2:], sc[2:], [n], [r])
    one(1)
    bad = [lambda: sess.admit([], x[:0], tc[:0], sc[:0], [], []),
           lambda: one(4), lambda: one(-1),                                   # outside [0, slots)
           lambda: one(1),                                                    # not free
           lambda: sess.admit([0, 0], x[:2], tc[:2], sc[:2], [5, 5], MIXED[:2]),   # named twice
           lambda: one(0, 0), lambda: one(0, 72),                             # len < 1, len > T_in
           lambda: one(0, 33, RowSchedule(0)), lambda: one(0, 33, RowSchedule(2, t_shift=0.0)),
           lambda: one(0, 33, RowSchedule(2, float("nan"))),
           lambda: sess.retire([0]),                                          # free
           lambda: sess.retire([1]),                                          # steps left
           lambda: sess.retire([4])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    long = torch.zeros((1, 98, 100), device="cuda:0")
    with pytest.raises(ValueError):                                           # len > max_frames
        sess.admit([0], long, long, long, [98], [MIXED[0]])
    assert sess.steps_left() == [-1, 2, -1, -1]
    sess.step()
    sess.step()
    for f in (lambda: sess.retire([1, 1]), lambda: sess.retire([1], 32)):     # named twice, T_out < len
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError):
        eng.open_session(0, 97)
    with pytest.raises(ValueError):
        eng.open_session(2, 0)
    lone = sess.retire([1])
    assert torch.isfinite(lone).all() and sess.steps_left() == [-1] * 4
    # ... and the session still computes what it should
    got, _, _ = run_all(sess, [0, 1, 3], dev, LENS, MIXED)
    for b, n in enumerate(LENS):
        assert torch.equal(got[b, :n], want[b, :n])
    sess.close()
    with pytest.raises(RuntimeError):
        sess.step()


def test_session_outliving_its_engine_raises():
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    from zipvoice_amd.weights import synthetic_state_dict
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="bf16")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    eng = m.to("cuda:0").engine
    sess = eng.open_session(2, 40)
    _, dev = batch([33], seed=51)
    sess.admit([0], *dev[:3], [33], [RowSchedule(1, 1.0)])
    torch.cuda.synchronize()
    eng.__del__()                                      # the engine goes first (the session keeps the Python object)
    for f in (sess.step, sess.steps_left, lambda: sess.retire([0])):
        with pytest.raises(RuntimeError, match="engine"):
            f()
    sess.close()


@pytest.fixture(scope="module")
def serving():
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.vocoder import Vocos
    m = fs.model("zipvoice", "bf16")
    voc, fx = Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()
    rng = np.random.default_rng(37)                    # test_generate_batch_with_per_item_settings' items
    items = [([int(t) for t in rng.integers(10, 90, n)], list(range(40, 40 + p)),
              (0.1 * rng.standard_normal(w)).astype(np.float32)) for n, p, w in ((8, 8, 9600), (7, 9, 8000))]
    return m, voc, fx, items


def batcher_run(serving, max_rows):
    from zipvoice_amd.serving import ContinuousBatcher
    m, voc, fx, items = serving
    cb = ContinuousBatcher(m, voc, fx, max_rows=max_rows, max_frames=97)
    tickets = [cb.submit(*it, num_step=2, guidance_scale=1.0, speed=2.0, t_shift=0.5, seed=s) for it, s in zip(items, (5, 6))]
    assert tickets == [0, 1] and cb.pending() == (2, 0)
    wavs, mels, order = {}, {}, []
    while sum(cb.pending()):
        for ticket, w in cb.step():
            wavs[ticket] = w
            order.append((ticket, cb.session.stats()[0]))
            mels.update(dict(cb.last_mel))
    assert cb.pending() == (0, 0)
    cb.close()
    return wavs, mels, order


def test_continuous_batcher_frame_counts(serving, monkeypatch):
    """submit's host-side frame count is what admission finds, for a prompt at another rate too; and if it
    ever were short, the over-long request is dropped with an error and nothing else is lost."""
    from zipvoice_amd.serving import ContinuousBatcher
    m, voc, fx, items = serving
    toks, ptoks, _ = items[0]
    wav16 = (0.1 * np.random.default_rng(38).standard_normal(6401)).astype(np.float32)   # 16 kHz: resampled first
    cb = ContinuousBatcher(m, voc, fx, max_rows=2, max_frames=97)
    p, total = cb._frames(toks, ptoks, wav16, 16000, 2.0)
    first = cb.submit(toks, ptoks, wav16, 16000, num_step=1, speed=2.0, seed=7)
    assert cb.step() == [] and cb._rows[0][:3] == (first, total, p)
    monkeypatch.setattr(cb, "_frames", lambda *a: (1, 1))
    cb.submit(list(range(10, 90)) * 3, ptoks, items[0][2], num_step=1)          # far more than 97 frames
    monkeypatch.undo()
    good = cb.submit(*items[1], num_step=1, speed=2.0, seed=8)
    with pytest.raises(ValueError, match="dropped"):
        cb.step()                                      # retires the first, then meets the over-long request
    assert cb.pending() == (1, 0)
    out = cb.step()                                    # the retired row was kept; the good request goes in
    assert [t for t, _ in out] == [first] and cb.pending() == (0, 1)
    assert [t for t, _ in cb.drain()] == [good]
    cb.close()


def test_continuous_batcher(serving):
    from zipvoice_amd.infer import generate_batch
    from zipvoice_amd.serving import ContinuousBatcher
    m, voc, fx, items = serving
    ref, _ = generate_batch(items, m, voc, fx, num_step=[2, 2], guidance_scale=[1.0, 1.0], speed=[2.0, 2.0],
                            t_shift=[0.5, 0.5], seeds=[5, 6])
    wavs, mels, order = batcher_run(serving, 2)
    assert order == [(0, 2), (1, 2)]                   # both ran the same two ticks
    for i in range(2):
        d = (wavs[i] - ref[i]).abs().max().item() if wavs[i].shape == ref[i].shape else None
        print(f"ContinuousBatcher(max_rows=2) item {i}: shape {tuple(wavs[i].shape)} vs {tuple(ref[i].shape)}, max |diff| {d}")
    assert all(torch.equal(wavs[i], ref[i]) for i in range(2))
    # one slot: the second request starts when the first has been retired
    wavs1, mels1, order1 = batcher_run(serving, 1)
    assert order1 == [(0, 3), (1, 4)]                  # (the step that retires the first admits the second and ticks)
    for i in range(2):
        assert wavs1[i].shape == ref[i].shape and torch.isfinite(wavs1[i]).all()
        fs.check(mels1[i], mels[i].float().cpu().numpy(), "bf16", f"ContinuousBatcher one slot vs all at once, item {i} (mel)")
    cb = ContinuousBatcher(m, voc, fx, max_rows=1, max_frames=97)
    with pytest.raises(ValueError):
        cb.submit(list(range(10, 90)) * 3, items[0][1], items[0][2], num_step=2)
    assert cb.pending() == (0, 0)
    cb.close()
