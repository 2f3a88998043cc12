"""The voice store end to end (zipvoice_amd/voices.py) on test_gpu_session.py's serving setup: synthetic bf16
zipvoice, Vocos().load_synthetic(0), VocosFbank, prompts of 8000-9600 samples, T <= 97.

* Loud prompts (level 0.3: neither path scales, both gains are 1): generate_batch with (tokens, Voice) items
  and ContinuousBatcher with voice= are torch.equal to their wav forms with the same seeds and settings.
* A quiet prompt (0.03): the two paths may differ in the last bit of the rms.  The stored features are held to
  the fbank's own bound against the float64 oracle (tests/test_gpu_fbank.py compare), the final mel to the
  fs.check "bf16" bound test_continuous_batcher uses; the output is bitwise the unscaled output times gain_out.
* A 16 kHz prompt registers to the frame count the batcher's host rule predicts, and its arena rows are
  extract_batch of the device-resampled, device-normalised samples, bit for bit.
* A warm gather and the whole warm admission of a voice group run under torch's sync guard and add no
  host-blocking engine call beyond the text encoder's and text condition's own.  (Neither instrument sees a
  host-to-device copy from pageable memory that stalls inside the runtime; the voice path makes its uploads
  from pinned memory.)
* Lifecycle: drop refuses a queued voice, succeeds once the request is admitted, the row still finishes, the
  range is reused; mixed batches and foreign voices are ValueErrors."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_fbank as fb  # noqa: E402
import test_gpu_fullsize as fs  # noqa: E402
from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.common import to_device  # noqa: E402
from zipvoice_amd.voices import VoiceStore, prompt_rms, prompt_scale  # noqa: E402

SET = dict(num_step=2, guidance_scale=1.0, speed=2.0, t_shift=0.5)
SEEDS = (5, 6)


@pytest.fixture(scope="module")
def serving():
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.vocoder import Vocos
    return fs.model("zipvoice", "bf16"), Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()


def make_items(level, seed=37):
    rng = np.random.default_rng(seed)
    return [([int(t) for t in rng.integers(10, 90, n)], list(range(40, 40 + p)),
             (level * rng.standard_normal(w)).astype(np.float32)) for n, p, w in ((8, 8, 9600), (7, 9, 8000))]


def as_voices(store, items):
    vs = store.register_batch([(it[2], it[1]) for it in items])
    return vs, [(it[0], v) for it, v in zip(items, vs)]


def batch(serving, items, **kw):
    from zipvoice_amd.infer import generate_batch
    m, voc, fx = serving
    out, _ = generate_batch(items, m, voc, fx, **{k: [v] * len(items) for k, v in SET.items()}, seeds=list(SEEDS), **kw)
    return out


def batcher(serving, requests, store=None, max_rows=2, between=None):
    """requests: (tokens, prompt_tokens, wav) or (tokens, Voice).  Returns ({ticket: wav}, {ticket: mel})."""
    from zipvoice_amd.serving import ContinuousBatcher
    m, voc, fx = serving
    cb = ContinuousBatcher(m, voc, fx, max_rows=max_rows, max_frames=97, voices=store)
    for r, s in zip(requests, SEEDS):
        if len(r) == 2:
            cb.submit(r[0], voice=r[1], seed=s, **SET)
        else:
            cb.submit(*r, seed=s, **SET)
    wavs, mels = {}, {}
    while sum(cb.pending()):
        for ticket, w in cb.step():
            wavs[ticket] = w
            mels.update(dict(cb.last_mel))
        if between is not None:
            between(cb)
    cb.close()
    return wavs, mels


@pytest.fixture(scope="module")
def loud(serving):
    items = make_items(0.3)
    store = VoiceStore(serving[2], 256)
    vs, vitems = as_voices(store, items)
    return items, store, vs, vitems


def test_loud_generate_batch_is_the_wav_form(serving, loud):
    items, store, vs, vitems = loud
    assert [v.frames for v in vs] == [38, 31] and [v.samples for v in vs] == [9600, 8000]
    ref, got = batch(serving, items), batch(serving, vitems)
    for i in range(2):
        assert got[i].shape == ref[i].shape and torch.equal(got[i], ref[i]), i
    ref, got = batch(serving, items, remove_long_sil=True), batch(serving, vitems, remove_long_sil=True)
    for i in range(2):
        assert torch.equal(got[i], ref[i]), i
    _, g = store.gather(vs, 40)
    assert (g == 1).all()


def test_loud_batcher_is_the_wav_form(serving, loud):
    items, store, _, vitems = loud
    ref, _ = batcher(serving, items)
    got, _ = batcher(serving, vitems, store)
    assert sorted(got) == sorted(ref) == [0, 1]
    for i in range(2):
        assert torch.equal(got[i], ref[i]), i


def test_quiet_prompt(serving):
    from oracle.fbank_np import vocos_fbank
    m, voc, fx = serving
    items = make_items(0.03, seed=39)
    # the stored features, unscaled (feat_scale 1), against the float64 oracle on the normalised samples
    plain = VoiceStore(fx, 128, feat_scale=1.0)
    for (_, ptoks, wav), v in zip(items, plain.register_batch([(it[2], it[1]) for it in items])):
        rms = np.float32(np.sqrt(np.mean(wav.astype(np.float64) ** 2)))
        assert rms < 0.1
        ref = vocos_fbank((wav * np.float32(0.1)) / rms, fx.window.numpy(), fx.fb.numpy())
        assert v.frames == ref.shape[0]
        fb.compare(plain.arena[v.offset:v.offset + v.frames].cpu().numpy(), ref)
    store = VoiceStore(fx, 256)
    vs, vitems = as_voices(store, items)
    # the final mel against the wav path
    _, ref_mel = batcher(serving, items)
    got_wav, got_mel = batcher(serving, vitems, store)
    for i in range(2):
        fs.check(got_mel[i], ref_mel[i].float().cpu().numpy(), "bf16", f"quiet prompt, voice vs wav path, item {i} (mel)")
    ref = batch(serving, items)
    got = batch(serving, vitems)
    for i in range(2):
        d = (got[i] - ref[i]).abs().max().item()
        print(f"quiet prompt item {i}: max |wav(voice) - wav(wav path)| = {d:.3e}, max |wav| = {ref[i].abs().max().item():.3e}")
    # the output gain, on the device: the same run with every gain at 1 gives the unscaled output
    _, gain = store.gather(vs, 40)
    assert (gain < 1).all() and (gain > 0.2).all()
    saved = store.gains.clone()
    store.gains.fill_(1.0)
    unscaled = batch(serving, vitems)
    store.gains.copy_(saved)
    for i in range(2):
        assert torch.equal(got[i], unscaled[i] * gain[i]) and not torch.equal(got[i], unscaled[i]), i
        assert torch.equal(got_wav[i], got[i]), i                # the batcher applies the same device gain


def test_resampled_prompt(serving):
    from zipvoice_amd.infer import _resampler
    from zipvoice_amd.serving import ContinuousBatcher
    m, voc, fx = serving
    toks, ptoks, _ = make_items(0.3)[0]
    wav16 = (0.05 * np.random.default_rng(38).standard_normal(6401)).astype(np.float32)
    store = VoiceStore(fx, 128)
    v = store.register(wav16, ptoks, 16000)
    cb = ContinuousBatcher(m, voc, fx, max_rows=1, max_frames=97, voices=store)
    p, total = cb._frames(toks, ptoks, wav16, 16000, 2.0)
    assert v.frames == p and v.samples == 9602 and cb._frames(toks, v.prompt_tokens, None, None, 2.0, voice=v) == (p, total)
    cb.close()
    out, olens = _resampler(16000, 24000).resample_batch(fs.cuda(wav16[None]), [6401])
    assert olens.tolist() == [v.samples]
    rms, _, _, ln = prompt_rms(out.contiguous(), [v.samples], 0.1)
    feats, nfr = fx.extract_batch(prompt_scale(out.contiguous(), [v.samples], ln, rms, 0.1), torch.tensor([v.samples]))
    assert int(nfr[0]) == v.frames and rms.item() < 0.1
    assert torch.equal(store.arena[v.offset:v.offset + v.frames], ((feats + 0.0) * 0.1)[0, :v.frames])


def guard_works():
    """test_warm_ticks_do_not_block_the_host's proof that the guard catches a synchronising op."""
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda:0").item()
        return True
    except pytest.fail.Exception:
        return False
    finally:
        torch.cuda.set_sync_debug_mode("default")


def guarded(fn, on):
    """fn() under the sync guard with the collector off: (result, host-blocking engine calls it added)."""
    gc.collect()
    torch.cuda.synchronize()
    gc.disable()
    try:
        c0 = engine.host_block_count()
        if on:
            torch.cuda.set_sync_debug_mode("error")
        out = fn()
        c1 = engine.host_block_count()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gc.enable()
    torch.cuda.synchronize()
    return out, c1 - c0


def test_warm_gather_and_admission_do_not_block_the_host(serving, loud):
    from zipvoice_amd.serving import ContinuousBatcher
    m, voc, fx = serving
    _, store, vs, vitems = loud
    on = guard_works()
    want, wg = store.gather([vs[1], vs[0], vs[1]], 71)              # the warm-up round at these shapes
    torch.cuda.synchronize()
    (got, gg), added = guarded(lambda: store.gather([vs[1], vs[0], vs[1]], 71), on)
    print(f"host-blocking engine calls in a warm gather: {added}; torch sync guard {'on' if on else 'unavailable'}")
    assert added == 0 and torch.equal(got, want) and torch.equal(gg, wg)

    cb = ContinuousBatcher(m, voc, fx, max_rows=2, max_frames=97, voices=store)

    def submit():
        return [cb.submit(toks, voice=v, seed=s, **SET) for (toks, v), s in zip(vitems, SEEDS)]

    first = {}
    for _ in range(2):                                              # two warm-up rounds, as the session's test
        tickets = submit()
        first = dict(cb.drain())
        torch.cuda.synchronize()
    # what the text encoder and the text condition add by themselves when warm, on the same tokens
    tickets2 = submit()
    T_in = max(q[7] for q in cb._queue)
    text = lambda: m.forward_text_inference_ratio_duration(
        tokens=[t for t, _ in vitems], prompt_tokens=[list(v.prompt_tokens) for v in vs],
        prompt_features_lens=to_device(torch.tensor([v.frames for v in vs]), m.device),
        speed=to_device(torch.tensor([SET["speed"]] * 2, dtype=torch.float32), m.device), num_frames=T_in)
    text()
    _, base = guarded(text, on)
    _, added = guarded(cb._admit, on)
    print(f"host-blocking engine calls: warm text encoder + text condition alone {base}, the whole voice admission {added}")
    assert added <= base
    assert cb.pending() == (0, 2)
    second = dict(cb.drain())
    cb.close()
    for a, b in zip(tickets, tickets2):
        assert torch.equal(first[a], second[b])


def test_lifecycle(serving, loud):
    from zipvoice_amd.infer import generate_batch
    from zipvoice_amd.serving import ContinuousBatcher
    m, voc, fx = serving
    items, _, _, _ = loud
    store = VoiceStore(fx, 80)
    keep = store.register(items[1][2], items[1][1])                 # 31 frames at 0
    v = store.register(items[0][2], items[0][1])                    # 38 frames at 31
    assert (keep.offset, v.offset) == (0, 31)
    with pytest.raises(ValueError, match=r"38 frames asked for, the largest free range has 11"):
        store.register(items[0][2], items[0][1])
    want, _ = batcher(serving, [(items[0][0], v)], store, max_rows=1)

    dropped = []

    def drop_once_admitted(cb):
        if not dropped:
            assert cb.pending() == (0, 1)
            store.drop(v)
            dropped.append(store.register(items[1][2], items[1][1]))    # takes the freed range at once
    cb = ContinuousBatcher(m, voc, fx, max_rows=1, max_frames=97, voices=store)
    cb.submit(items[0][0], voice=v, seed=SEEDS[0], **SET)
    with pytest.raises(ValueError, match="queued"):
        store.drop(v)
    cb.close()                                                      # (gives its queued request up)
    got, _ = batcher(serving, [(items[0][0], v)], store, max_rows=1, between=drop_once_admitted)
    assert torch.equal(got[0], want[0])                             # the admitted row owned its condition
    assert dropped[0].offset == 31 and dropped[0].frames == 31
    with pytest.raises(ValueError, match="dropped"):
        store.gather([v], 40)
    with pytest.raises(ValueError, match="dropped"):
        store.drop(v)
    other = VoiceStore(fx, 64)
    foreign = other.register(items[0][2], items[0][1])
    kw = {k: [val] * 2 for k, val in SET.items()}
    with pytest.raises(ValueError, match="mix"):
        generate_batch([(items[0][0], keep), items[1]], m, voc, fx, **kw)
    with pytest.raises(ValueError, match="another store"):
        generate_batch([(items[0][0], keep), (items[1][0], foreign)], m, voc, fx, **kw)
    cb = ContinuousBatcher(m, voc, fx, max_rows=1, max_frames=97, voices=store)
    with pytest.raises(ValueError, match="another store"):
        cb.submit(items[0][0], voice=foreign, **SET)
    with pytest.raises(ValueError, match="not both"):
        cb.submit(items[0][0], items[0][1], items[0][2], voice=keep, **SET)
    assert cb.pending() == (0, 0)
    cb.close()
