"""Prompt resampler on the GPU (zipvoice_amd/feature.py Resample, csrc/zv_resample.inc)
against the float64 direct reference of tests/resample_ref.py (torchaudio's formula with
its float32 taps), and the inference entry points that use it."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import resample_ref as ref  # noqa: E402
from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.common import predict_features_lens  # noqa: E402
from zipvoice_amd.feature import Resample, VocosFbank, compute_num_frames, resample_plan  # noqa: E402
from zipvoice_amd.infer import generate_batch, generate_sentence, prepare_prompt  # noqa: E402

PAIRS = [(8000, 24000), (16000, 24000), (22050, 24000), (32000, 24000), (44100, 24000),
         (48000, 24000), (11025, 24000), (48001, 24000), (24000, 16000)]


@functools.lru_cache(maxsize=None)
def resampler(orig, new):
    return Resample(orig, new)


@functools.lru_cache(maxsize=None)
def cases(orig, new):
    """[(x float32 (L,), reference float64, l1 gain of the filter)] for the lengths 1,
    width - 1, 7 o, 7 o + 1 and ~5000: rows shorter than the filter, both sides of the
    ceil boundary, several workgroups."""
    p = resample_plan(orig, new)
    rng = np.random.default_rng(orig + new)
    out = []
    for L in (1, p.width - 1, 7 * p.o, 7 * p.o + 1, 5003):
        x = rng.uniform(-1, 1, L).astype(np.float32)
        y, gain = ref.resample_direct(x, orig, new, return_abs_sum=True)
        out.append((x, y, gain))
    return out


@pytest.mark.parametrize("orig,new", PAIRS)
def test_matches_reference(orig, new):
    """Every output within the worst-case fp32 accumulation bound of an S-term sum:
    (S + 2) * 2^-24 * max_j sum_k |K[j, k]| * max |x|."""
    rs = resampler(orig, new)
    S = rs.plan.S
    for x, y, gain in cases(orig, new):
        got = rs(x)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        assert got.shape == y.shape == (rs.plan.out_len(len(x)),)
        err = float(np.abs(got - y).max())
        bound = (S + 2) * 2.0 ** -24 * gain * float(np.abs(x).max())
        print(f"resample {orig}->{new} L={len(x)} S={S}: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (orig, new, len(x), err, bound)


@pytest.mark.parametrize("orig,new", [(22050, 24000), (48000, 24000), (48001, 24000)])
def test_ragged_batch_is_bitwise_the_single_rows(orig, new):
    rs = resampler(orig, new)
    xs = [c[0] for c in cases(orig, new)][2:]           # 7 o, 7 o + 1, 5003
    lens = [len(x) for x in xs]
    N = max(lens) + 13                                   # wav_ld > N, garbage past each row
    wb = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (3, N)).astype(np.float32))
    for r, x in enumerate(xs):
        wb[r, :lens[r]] = torch.from_numpy(x)
    out, olens = rs.resample_batch(wb.cuda(), lens)
    assert out.is_cuda and out.shape == (3, max(rs.plan.out_len(v) for v in lens))
    assert olens.tolist() == [rs.plan.out_len(v) for v in lens]
    for r, x in enumerate(xs):
        single = rs(torch.from_numpy(x).cuda())
        assert torch.equal(out[r, :olens[r]], single), r
        assert not out[r, olens[r]:].any()


def test_two_channel_input():
    rs = resampler(44100, 24000)
    a, b = cases(44100, 24000)[4][0], cases(44100, 24000)[4][0][::-1].copy()
    got = rs(torch.from_numpy(np.stack([a, b])).cuda())
    assert got.is_cuda and got.shape == (2, rs.plan.out_len(len(a)))
    assert torch.equal(got[0], rs(torch.from_numpy(a).cuda()))
    assert torch.equal(got[1], rs(torch.from_numpy(b).cuda()))


def test_equal_rates_return_the_input():
    rs = Resample(24000, 24000)
    x = torch.zeros(2, 100)
    assert rs(x) is x
    xn = np.zeros(7, np.float32)
    assert rs(xn) is xn
    assert rs._h is None and rs.device_bytes() == 0     # no handle, nothing launched


def test_create_rejects_bad_arguments():
    lib = engine.load_library()
    st = np.zeros(4, np.int32)
    tb = np.zeros((4, 8), np.float32)
    args = (st.ctypes.data_as(ctypes.c_void_p), tb.ctypes.data_as(ctypes.c_void_p))
    assert not lib.zv_resample_create(4, 4, 8, *args)
    assert "o == n" in lib.zv_last_error().decode()
    assert not lib.zv_resample_create(0, 4, 8, *args)
    assert "positive" in lib.zv_last_error().decode()
    assert not lib.zv_resample_create(3, 4, 513, *args)
    assert "S must" in lib.zv_last_error().decode()


def test_near_coprime_rates_keep_the_compact_table():
    rs = resampler(48001, 24000)
    rs(np.zeros(10, np.float32))
    assert 0 < rs.device_bytes() < 16 << 20


# ---------------------------------------------------------------- inference entry points
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


def prompt(n, seed):
    rng = np.random.default_rng(seed)
    return (0.05 * rng.standard_normal(n)).astype(np.float32)


def test_generate_batch_mixed_rates_equals_preresampled(stack):
    m, voc, fx = stack
    toks = [(list(range(1, 20)), list(range(30, 40))), (list(range(5, 50)), list(range(60, 66)))]
    raw = [(prompt(16000, 1), 16000), (prompt(66150, 2), 44100)]
    pre = [Resample(sr, 24000)(w) for w, sr in raw]
    assert [len(p) for p in pre] == [24000, 36000]
    pfl = torch.tensor([compute_num_frames(len(p), 256) for p in pre])
    fl = predict_features_lens(pfl, torch.tensor([len(t[1]) for t in toks]),
                               torch.tensor([len(t[0]) for t in toks]), 1.0)
    x0 = torch.randn(2, int(fl.max()), 100, generator=torch.Generator().manual_seed(0)).cuda()
    a, _ = generate_batch([(t[0], t[1], w, sr) for t, (w, sr) in zip(toks, raw)], m, voc, fx,
                          num_step=4, x0=x0)
    b, _ = generate_batch([(t[0], t[1], p) for t, p in zip(toks, pre)], m, voc, fx,
                          num_step=4, x0=x0)
    for u, v in zip(a, b):
        assert u.shape == v.shape and u.shape[1] > 0 and torch.isfinite(u).all()
        assert torch.equal(u, v)


def test_generate_sentence_resamples_the_prompt(stack):
    m, voc, fx = stack
    wav, met = generate_sentence(list(range(1, 30)), list(range(40, 52)), prompt(16000, 0), m,
                                 voc, fx, num_step=4, prompt_sampling_rate=16000)
    assert wav.shape[0] == 1 and wav.shape[1] % 256 == 0 and wav.shape[1] > 0
    assert torch.isfinite(wav).all()
    for k in ("t", "t_no_vocoder", "t_vocoder", "wav_seconds", "rtf", "rtf_no_vocoder",
              "rtf_vocoder"):
        assert k in met


def test_prepare_prompt_layouts():
    rs = resampler(16000, 24000)
    a, b = prompt(1600, 3), prompt(800, 4)               # -> 2400 and 1200 samples
    ra, rb = rs(torch.from_numpy(a).cuda()), rs(torch.from_numpy(b).cuda())
    st = np.stack([a, a[::-1]])
    rst = rs(torch.from_numpy(st.copy()).cuda())
    # mono: channels kept, resampled one by one
    mono = prepare_prompt(st, 16000, "mono")
    assert mono.is_cuda and torch.equal(mono, rst)
    assert torch.equal(prepare_prompt(a, 16000, "mono"), ra[None])
    # dialog: each wav to one channel, then concatenated in time; rates may differ
    d = prepare_prompt([st, rb.cpu().numpy()[None]], [16000, 24000], "dialog")
    assert d.shape == (1, 3600)
    assert torch.equal(d[0, :2400], rst.mean(0)) and torch.equal(d[0, 2400:], rb)
    assert torch.equal(prepare_prompt([a], [16000], "dialog"), ra[None])
    # stereo, one two-channel wav
    assert torch.equal(prepare_prompt(st, 16000, "stereo"), rst)
    # stereo, two two-channel wavs: concatenated in time
    s2 = prepare_prompt([st, st[:, :800]], 16000, "stereo")
    assert s2.shape == (2, 3600) and torch.equal(s2[:, :2400], rst)
    assert torch.equal(s2[:, 2400:], rs(torch.from_numpy(st[:, :800].copy()).cuda()))
    # stereo, two mono wavs: speaker 1 on channel 0 first, speaker 2 on channel 1 after,
    # everything else the background
    bg = prompt(2 * 4000, 5).reshape(2, 4000)
    s3 = prepare_prompt([a, b], [16000, 16000], "stereo", silence=bg)
    bgd = torch.from_numpy(bg).cuda()
    assert s3.shape == (2, 3600)
    assert torch.equal(s3[0, :2400], ra) and torch.equal(s3[0, 2400:], bgd[0, 2400:3600])
    assert torch.equal(s3[1, :2400], bgd[1, :2400]) and torch.equal(s3[1, 2400:], rb)
    s4 = prepare_prompt([a, b], [16000, 16000], "stereo")
    assert not s4[1, :2400].any() and not s4[0, 2400:].any()
    assert torch.equal(s4[0, :2400], ra) and torch.equal(s4[1, 2400:], rb)
    with pytest.raises(AssertionError):
        prepare_prompt(a, 16000, "stereo")               # one wav must be two-channel
