"""The editing service end to end: recordings registered in a VoiceStore, edits through
ContinuousBatcher.submit_edit, and edit_batch over (tokens, Recording, spans) items.  The recordings and edits of
tests/test_gpu_edit_pipeline.py (about 60 frames; one at 16 kHz and quiet, one at 16 kHz without spans, a quiet
deletion), the synthetic bf16 zipvoice and Vocos, num_step = 2.

* Kept segments: outside the cross-fade windows every kept segment is the resampled recording's own samples,
  bitwise, and every generated segment is the store's gain times the vocoder's output, bitwise.
* The item without spans comes back bitwise (the store's waveform, which is the batched resample's) and causes
  no tick and no vocoder call.
* Against edit_batch on the wav items with the same seeds, both in padding = "row" mode: equal shapes, and the
  mels within fs.check(..., "bf16"), the project's bound for "one slot vs all at once"
  (tests/test_gpu_session.py); the waveform difference is printed.  Equality is not required: edit_batch takes
  the scalar solve path, and its host RMS is another reduction for the quiet recordings.
* In "row" mode the same edit and seed, alone and admitted at a later tick beside two generation requests: the
  mels within the same bound, the kept segments bitwise in both runs.
* edit_batch with Recording items: bitwise the wav items' result for a loud recording, within the bound on the
  mel for a quiet one."""
import numpy as np
import pytest

import edit_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import test_gpu_fullsize as fs  # noqa: E402
from test_gpu_edit_pipeline import FADE, HOP, bits, resampled  # noqa: E402
from zipvoice_amd.edit import edit_batch, plan_edit, sample_table, table_length  # noqa: E402

SEEDS = [1, 2, 3, 4]


def make_items():
    """tests/test_gpu_edit_pipeline.py's items (its fixture, restated: the same generator and order)."""
    rng = np.random.default_rng(40)
    toks = [[int(v) for v in rng.integers(1, 360, n)] for n in (14, 12, 9, 10)]
    loud = (0.2 * rng.standard_normal(15400)).astype(np.float32)          # 60 frames at 24 kHz
    quiet16 = (0.02 * rng.standard_normal(10000)).astype(np.float32)      # 15000 samples at 24 kHz
    plain16 = (0.05 * rng.standard_normal(9001)).astype(np.float32)
    quiet = (0.03 * rng.standard_normal(14500)).astype(np.float32)        # 57 frames
    return [(toks[0], loud, [(20, 30, 12)]), (toks[1], quiet16, [(10, 25, 15)], 16000),
            (toks[2], plain16, [], 16000), (toks[3], quiet, [(15, 25, 0)])]


class Spy:
    """Keeps what goes into and comes out of the vocoder."""

    def __init__(self, monkeypatch, voc):
        self.feats, self.gen = [], []
        decode = voc.decode_features

        def decode_features(x, *a, **kw):
            self.feats.append(x)
            self.gen.append(decode(x, *a, **kw))
            return self.gen[-1]
        monkeypatch.setattr(voc, "decode_features", decode_features)


@pytest.fixture(scope="module")
def service():
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.vocoder import Vocos
    from zipvoice_amd.voices import VoiceStore
    m, voc, fx = fs.model("zipvoice", "bf16"), Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()
    items = make_items()
    store = VoiceStore(fx, 512)
    recs = store.register_recording_batch([it[1] if len(it) < 4 else (it[1], it[3]) for it in items])
    before = m.padding
    yield m, voc, fx, items, store, recs
    m.padding = before                                                  # (the model is shared with other modules)


def run_batcher(service, requests, padding=None, max_rows=4, plan=None):
    """requests: indices of the items to edit.  ``plan(cb, submit)`` may drive the batcher itself.  Returns
    ({ticket: wav}, {ticket: mel}, the batcher's session stats)."""
    from zipvoice_amd.serving import ContinuousBatcher
    m, voc, fx, items, store, recs = service
    cb = ContinuousBatcher(m, voc, fx, max_rows=max_rows, max_frames=97, padding=padding, voices=store)
    submit = lambda i: cb.submit_edit(items[i][0], recs[i], items[i][2], num_step=2, seed=SEEDS[i], fade=FADE)
    wavs, mels = {}, {}

    def step():
        for ticket, w in cb.step():
            wavs[ticket] = w
            mels.update(dict(cb.last_mel))
    tickets = plan(cb, submit, step) if plan else [submit(i) for i in requests]
    while sum(cb.pending()) or cb._done:
        step()
    stats = cb.session.stats()
    cb.close()
    return tickets, wavs, mels, stats


def held_bitwise(out, w, gen_row, g, spans, what):
    """out (1, N'): every kept segment is w's samples and every generated one g * gen_row's, outside the windows."""
    N = len(w)
    L = (N + HOP // 2) // HOP
    tab = sample_table(plan_edit(L, spans), N, HOP)
    assert np.array_equal(tab, edit_ref.sample_table(edit_ref.plan(L, spans), N, HOP, L))
    T = L - sum(e - s for s, e, _ in spans) + sum(n for _, _, n in spans)
    assert out.shape == (1, table_length(tab)) and np.isfinite(out).all(), what
    hs = edit_ref.half_windows(tab, N, T * HOP, FADE)
    for k, (o, src, ln, kind) in enumerate(tab.tolist()):
        a, b = (hs[k - 1] if k else 0), ln - hs[k]
        assert b - a > 0
        got = out[0, o + a:o + b]
        if kind == 0:
            assert np.array_equal(bits(got), bits(w[src + a:src + b])), (what, k)
        elif gen_row is not None:
            assert np.array_equal(bits(got), bits(g * gen_row[src + a:src + b])), (what, k)
    return tab, T


def test_recordings_are_registered_as_the_voices_are(service):
    m, voc, fx, items, store, recs = service
    wavs = resampled(items)
    assert [r.samples for r in recs] == [len(w) for w in wavs] and recs[1].samples == 15000
    assert [r.frames for r in recs] == [(len(w) + HOP // 2) // HOP for w in wavs]
    for r, w in zip(recs, wavs):
        assert np.array_equal(bits(store.waveform(r).cpu()), bits(w))   # un-normalised, at the model's rate
    g = store.gains[torch.tensor([r.offset for r in recs])].cpu().numpy()
    assert g[0] == 1 and (g[1:] < 1).all() and (g[1:] > 0.1).all()
    # a voice of the same samples has the same arena rows and gain
    v = store.register(items[3][1], [1, 2, 3])
    assert v.frames == recs[3].frames
    assert torch.equal(store.arena[v.offset:v.offset + v.frames], store.arena[recs[3].offset:recs[3].offset + v.frames])
    assert torch.equal(store.gains[v.offset], store.gains[recs[3].offset])
    used = store.alloc.largest()
    store.drop(v)
    assert store.alloc.largest() > used
    with pytest.raises(ValueError, match="reflect padding"):
        store.register_recording(np.zeros(100, np.float32))
    with pytest.raises(ValueError, match="full"):
        store.register_recording(np.zeros(512 * HOP, np.float32) + 0.1)
    assert store.alloc.largest() > used                                 # a refusal registers nothing


def test_kept_and_generated_segments_are_bitwise(service, monkeypatch):
    m, voc, fx, items, store, recs = service
    spy = Spy(monkeypatch, voc)
    wavs = resampled(items)
    tickets, outs, mels, stats = run_batcher(service, [0, 1, 2, 3])
    assert tickets == [0, 1, 2, 3] and sorted(outs) == tickets
    assert len(spy.gen) == 1 and spy.gen[0].shape[0] == 3 and stats[0] == 2      # one group of three rows, two ticks
    gen = spy.gen[0].cpu().numpy()
    # the item without spans: its resampled input, bitwise
    assert outs[2].shape == (1, len(wavs[2])) and np.array_equal(bits(outs[2][0].cpu()), bits(wavs[2]))
    for r, i in enumerate((0, 1, 3)):
        g = store.gains[recs[i].offset].cpu().numpy()
        assert g.dtype == np.float32 and (g < 1) == (i != 0)
        tab, T = held_bitwise(outs[i].cpu().numpy(), wavs[i].numpy(), gen[r], g, items[i][2], f"item {i}")
        assert mels[i].shape == (T, 100) and len(tab) == (2 if i == 3 else 3)
        # inside the windows: a mix of the two sides, within the splice kernel's own bound
        N = len(wavs[i])
        ref, inside, amp = edit_ref.splice(wavs[i].numpy()[None, None], [N], gen[r][None, None, :T * HOP], [T * HOP], [tab],
                                           [g], FADE, outs[i].shape[1])
        assert inside.sum() == 2 * FADE * (len(tab) - 1)
        assert (np.abs(outs[i].cpu().numpy() - ref[0]) <= 4 * 2.0 ** -23 * amp[0]).all()
    assert outs[3].shape[1] == len(wavs[3]) - 10 * HOP                  # the deletion


def test_no_solve_without_spans(service, monkeypatch):
    m, voc, fx, items, store, recs = service
    spy = Spy(monkeypatch, voc)
    tickets, outs, mels, stats = run_batcher(service, [2])
    assert np.array_equal(bits(outs[tickets[0]][0].cpu()), bits(resampled(items)[2]))
    assert stats == (0, 0, 0, 0) and spy.gen == [] and mels == {}
    assert store.uses(recs[2]) == 0


def test_against_edit_batch_in_row_mode(service, monkeypatch):
    m, voc, fx, items, store, recs = service
    spy = Spy(monkeypatch, voc)
    m.padding = "row"
    ref, _ = edit_batch(items, m, voc, fx, num_step=2, fade=FADE, seeds=SEEDS)
    ref_feats = spy.feats[0].float().cpu().numpy()
    _, outs, mels, _ = run_batcher(service, [0, 1, 2, 3], padding="row")
    assert m.padding == "row"
    for r, i in enumerate((0, 1, 3)):
        assert outs[i].shape == ref[i].shape, i
        T = mels[i].shape[0]
        fs.check(mels[i], ref_feats[r, :T], "bf16", f"edit through the batcher vs edit_batch, item {i} (mel)")
        print(f"item {i}: max |wav(batcher) - wav(edit_batch)| = {(outs[i] - ref[i]).abs().max().item():.3e}, "
              f"max |wav| = {ref[i].abs().max().item():.3e}")
    assert torch.equal(outs[2], ref[2])


def test_an_edit_does_not_depend_on_its_company(service):
    m, voc, fx, items, store, recs = service
    wavs = resampled(items)
    _, alone, mel_alone, _ = run_batcher(service, [1], padding="row")
    rng = np.random.default_rng(37)                                      # test_gpu_session.py's generation requests
    gens = [([int(t) for t in rng.integers(10, 90, n)], list(range(40, 40 + p)),
             (0.1 * rng.standard_normal(w)).astype(np.float32)) for n, p, w in ((8, 8, 9600), (7, 9, 8000))]
    seen = {}

    def later(cb, submit, step):
        for g, s in zip(gens, (5, 6)):
            cb.submit(*g, num_step=3, guidance_scale=1.0, speed=2.0, t_shift=0.5, seed=s)
        step()                                                           # both generation rows admitted, tick 0
        t = submit(1)
        step()                                                           # the edit joins at tick 1
        seen["in flight"] = cb.pending()
        seen["ticks"] = cb.session.stats()[0]
        return [t]
    (t,), beside, mel_beside, _ = run_batcher(service, None, padding="row", max_rows=3, plan=later)
    assert seen == {"in flight": (0, 3), "ticks": 2}
    fs.check(mel_beside[t], mel_alone[0].float().cpu().numpy(), "bf16", "the same edit alone and beside two generation rows (mel)")
    print(f"max |wav(beside) - wav(alone)| = {(beside[t] - alone[0]).abs().max().item():.3e}")
    for out, what in ((alone[0], "alone"), (beside[t], "beside")):
        held_bitwise(out.cpu().numpy(), wavs[1].numpy(), None, None, items[1][2], what)


def test_edit_batch_with_recordings(service, monkeypatch):
    m, voc, fx, items, store, recs = service
    spy = Spy(monkeypatch, voc)
    m.padding = "batch"
    as_rec = lambda i: (items[i][0], recs[i], items[i][2])
    # a loud recording (RMS >= target): neither path scales; bitwise the wav item's result
    ref, _ = edit_batch([items[0], items[2]], m, voc, fx, num_step=2, fade=FADE, seeds=[1, 3])
    got, met = edit_batch([as_rec(0), as_rec(2)], m, voc, fx, num_step=2, fade=FADE, seeds=[1, 3])
    assert set(met) == {"t", "wav_seconds", "gen_seconds", "rtf"} and abs(met["gen_seconds"] - 12 * HOP / 24000) < 1e-9
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    whole, _ = edit_batch([as_rec(0)], m, voc, fx, num_step=2, fade=FADE, seeds=[1], keep_original_audio=False)
    whole_ref, _ = edit_batch([items[0]], m, voc, fx, num_step=2, fade=FADE, seeds=[1], keep_original_audio=False)
    assert torch.equal(whole[0], whole_ref[0]) and whole[0].shape == (1, 62 * HOP)
    # quiet ones: the stored RMS is another reduction than the host's
    del spy.feats[:]
    ref, _ = edit_batch([items[1], items[3]], m, voc, fx, num_step=2, fade=FADE, seeds=[2, 4])
    got, _ = edit_batch([as_rec(1), as_rec(3)], m, voc, fx, num_step=2, fade=FADE, seeds=[2, 4])
    want, have = spy.feats[0].float().cpu().numpy(), spy.feats[1]
    for r, i in enumerate((1, 3)):
        assert got[r].shape == ref[r].shape
        fs.check(have[r], want[r], "bf16", f"edit_batch on a quiet recording vs its wav item, item {i} (mel)")
        print(f"item {i}: max |wav(recording) - wav(wav item)| = {(got[r] - ref[r]).abs().max().item():.3e}")
    with pytest.raises(ValueError, match="mix"):
        edit_batch([as_rec(0), items[3]], m, voc, fx, num_step=2)
    with pytest.raises(ValueError, match="row 0 span 0"):
        edit_batch([(items[0][0], recs[0], [(20, 61, 3)])], m, voc, fx, num_step=2)
