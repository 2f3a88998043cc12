"""edit_batch / edit_sentence end to end on the GPU: synthetic ZipVoice (bf16) and Vocos weights,
recordings of about 60 frames.  One batch holds a 24 kHz replacement, a quiet 16 kHz replacement,
a 16 kHz item without spans and a quiet deletion; the vocoder's output is recorded, so every
output sample outside the cross-fade windows can be held bitwise to where it came from: the
resampled recording (kept segments) or gain * vocoder output (generated segments)."""
import numpy as np
import pytest

import edit_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from zipvoice_amd.edit import edit_batch, edit_sentence, plan_edit, sample_table, table_length  # noqa: E402
from zipvoice_amd.infer import _prompt_rms_normalise, _resampler  # noqa: E402

HOP, FADE, RMS = 256, 240, 0.1


@pytest.fixture(scope="module")
def stack():
    from zipvoice_amd.config import default_config
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.models import build_model
    from zipvoice_amd.vocoder import Vocos
    m = build_model(default_config("zipvoice"), precision="bf16").load_synthetic(0).to("cuda:0")
    return m, Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()


@pytest.fixture(scope="module")
def items():
    rng = np.random.default_rng(40)
    toks = [[int(v) for v in rng.integers(1, 360, n)] for n in (14, 12, 9, 10)]
    loud = (0.2 * rng.standard_normal(15400)).astype(np.float32)          # 60 frames at 24 kHz
    quiet16 = (0.02 * rng.standard_normal(10000)).astype(np.float32)      # 15000 samples at 24 kHz
    plain16 = (0.05 * rng.standard_normal(9001)).astype(np.float32)
    quiet = (0.03 * rng.standard_normal(14500)).astype(np.float32)        # 57 frames
    return [(toks[0], loud, [(20, 30, 12)]), (toks[1], quiet16, [(10, 25, 15)], 16000),
            (toks[2], plain16, [], 16000), (toks[3], quiet, [(15, 25, 0)])]


def resampled(items):
    """The items' recordings at 24 kHz, the 16 kHz ones through one batched resample as
    edit_batch runs it."""
    idx = [i for i, it in enumerate(items) if len(it) > 3]
    lens = [len(items[i][1]) for i in idx]
    rb = torch.zeros((len(idx), max(lens)))
    for r, i in enumerate(idx):
        rb[r, :lens[r]] = torch.from_numpy(items[i][1])
    out, olens = _resampler(16000, 24000).resample_batch(rb.cuda(), lens)
    wavs = [torch.from_numpy(it[1]) for it in items]
    for r, i in enumerate(idx):
        wavs[i] = out[r, :int(olens[r])].cpu()
    return wavs


class Spy:
    """Counts the rows the solver is asked for and keeps the vocoder's output."""

    def __init__(self, monkeypatch, m, voc):
        self.rows, self.gen = [], []
        solve, decode = m.solver.sample, voc.decode_features

        def sample(*a, **kw):
            self.rows.append(kw["x"].shape[0])
            return solve(*a, **kw)

        def decode_features(*a, **kw):
            self.gen.append(decode(*a, **kw))
            return self.gen[-1]
        monkeypatch.setattr(m.solver, "sample", sample)
        monkeypatch.setattr(voc, "decode_features", decode_features)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_edit_batch(stack, items, monkeypatch):
    m, voc, fx = stack
    spy = Spy(monkeypatch, m, voc)
    wavs = resampled(items)
    outs, met = edit_batch(items, m, voc, fx, num_step=2, fade=FADE, seeds=[1, 2, 3, 4])
    assert set(met) == {"t", "wav_seconds", "gen_seconds", "rtf"}
    assert spy.rows == [3] and len(spy.gen) == 1                   # the item without spans: no solve
    gen = spy.gen[0].cpu().numpy()
    assert len(wavs[1]) == 15000
    # the item without spans: its resampled input, bitwise
    assert outs[2].shape == (1, len(wavs[2])) and np.array_equal(bits(outs[2][0].cpu()), bits(wavs[2]))
    gen_frames = 0
    for r, i in enumerate((0, 1, 3)):
        w = wavs[i].numpy()
        N = len(w)
        L = (N + HOP // 2) // HOP
        tab = sample_table(plan_edit(L, items[i][2]), N, HOP)
        assert np.array_equal(tab, edit_ref.sample_table(edit_ref.plan(L, items[i][2]), N, HOP, L))
        out = outs[i].cpu().numpy()
        assert out.shape == (1, table_length(tab)) and np.isfinite(out).all()
        rms = _prompt_rms_normalise(wavs[i], RMS)[1]
        g = np.float32(rms / RMS if rms < RMS else 1.0)
        assert (g < 1) == (i != 0)
        T = L - sum(e - s for s, e, _ in items[i][2]) + sum(n for _, _, n in items[i][2])
        gen_frames += sum(n for _, _, n in items[i][2])
        hs = edit_ref.half_windows(tab, N, T * HOP, FADE)
        assert len(tab) == (2 if i == 3 else 3) and all(h == FADE for h in hs[:-1])
        for k, (o, src, ln, kind) in enumerate(tab.tolist()):
            a, b = (hs[k - 1] if k else 0), ln - hs[k]
            got = out[0, o + a:o + b]
            if kind == 0:      # the recording's own samples, whatever its level
                assert np.array_equal(bits(got), bits(w[src + a:src + b])), (i, k)
            else:              # the vocoder's rendering, at the recording's level
                assert np.array_equal(bits(got), bits(g * gen[r, src + a:src + b])), (i, k)
        # inside the windows: a mix of the two sides, within the kernel test's bound
        ref, inside, amp = edit_ref.splice(w[None, None], [N], gen[r][None, None, :T * HOP], [T * HOP], [tab], [g],
                                           FADE, out.shape[1])
        assert inside.sum() == 2 * FADE * (len(tab) - 1)
        assert (np.abs(out - ref[0]) <= 4 * 2.0 ** -23 * amp[0] + 0 * out).all()
    assert outs[3].shape[1] == len(wavs[3]) - 10 * HOP             # the deletion
    secs = sum(o.shape[1] for o in outs) / 24000
    assert abs(met["wav_seconds"] - secs) < 1e-9
    assert abs(met["gen_seconds"] - gen_frames * HOP / 24000) < 1e-9 and met["rtf"] > 0
    # only items without spans: nothing reaches the decoder or the vocoder
    outs2, met2 = edit_batch([items[2]], m, voc, fx, num_step=2)
    assert spy.rows == [3] and len(spy.gen) == 1
    assert np.array_equal(bits(outs2[0][0].cpu()), bits(wavs[2])) and met2["gen_seconds"] == 0


def test_whole_row_rendering_and_edit_sentence(stack, items, monkeypatch):
    m, voc, fx = stack
    spy = Spy(monkeypatch, m, voc)
    toks, wav, spans = items[3]
    out, met = edit_sentence(toks, wav, [(15, 25, 4)], m, voc, fx, seed=9, num_step=2, fade=FADE,
                             keep_original_audio=False)
    T = 57 - 10 + 4
    rms = _prompt_rms_normalise(torch.from_numpy(wav), RMS)[1]
    assert out.shape == (1, T * HOP) and spy.rows == [1]
    assert np.array_equal(bits(out[0].cpu()), bits(np.float32(rms / RMS) * spy.gen[0][0, :T * HOP].cpu().numpy()))
    assert abs(met["gen_seconds"] - T * HOP / 24000) < 1e-9
    with pytest.raises(ValueError, match="row 0 span 0"):
        edit_sentence(toks, wav, [(15, 58, 4)], m, voc, fx, num_step=2)
    assert spy.rows == [1]                                         # refused before any solve


def test_stereo_raises(stack):
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    _, voc, fx = stack
    stereo = build_model(default_config("zipvoice_dialog_stereo"))
    with pytest.raises(NotImplementedError):
        edit_batch([([1, 2], np.zeros(9000, np.float32), [(3, 5, 2)])], stereo, voc, fx)
