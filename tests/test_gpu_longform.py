"""Long-form trim and join on the GPU (zipvoice_amd/longform.py WavJoiner, generate_long;
csrc/zv_wavjoin.inc) against the float64 restatement tests/wavjoin_ref.py.

Every comparison first asserts, on the reference, that no frame's energy lies within 1e-3
(relative) of the threshold: the fp32 frame sum is off by at most about 240 * 2^-24
relative, so at that margin no flag may differ and no case may be excused.  Output samples
are held to 4 * 2^-23 * max |g x| (two products, one add and the rounding of w); samples
outside the overlaps with gain 1 must be the input's bits."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import wavjoin_ref as ref  # noqa: E402
from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.common import predict_features_lens  # noqa: E402
from zipvoice_amd.feature import VocosFbank  # noqa: E402
from zipvoice_amd.infer import _prompt_rms_normalise  # noqa: E402
from zipvoice_amd.longform import WavJoiner, chunk_budget, chunk_tokens, generate_long  # noqa: E402

THR = 10.0 ** (-42.0 / 20.0)
P = dict(frame=240, thr=THR, keep_edge=2, max_gap=4, fade=480)
LOUD, QUIET = 0.1, 1e-4
CANARY = 7.0


@functools.lru_cache(maxsize=None)
def handle(frame, thr, keep_edge, max_gap, fade):
    h = engine.load_library().zv_wavjoin_create(frame, thr, keep_edge, max_gap, fade)
    assert h, engine.load_library().zv_last_error().decode()
    return h


def noise(rng, *segments):
    """segments: (amplitude, samples), ... -> one float32 chunk of Gaussian noise."""
    return np.concatenate([(a * rng.standard_normal(n)).astype(np.float32) for a, n in segments])


def batch(chunks, pad=13, seed=99):
    """Chunks ((n_b,) or (C, n_b)) -> ((B, C, longest + pad) with garbage past each length,
    lens)."""
    chunks = [c[None] if c.ndim == 1 else c for c in chunks]
    lens = [c.shape[1] for c in chunks]
    x = np.random.default_rng(seed).uniform(-1, 1, (len(chunks), chunks[0].shape[0],
                                                     max(lens) + pad)).astype(np.float32)
    for b, c in enumerate(chunks):
        x[b, :, :lens[b]] = c
    return x, lens


def apply(x, lens, gains=None, params=P, out_cap=None, out_ld=None):
    """One zv_wavjoin_apply on a canary-filled output -> (out (C, out_ld), N, spans (B, 3))."""
    lib = engine.load_library()
    h = handle(**params)
    B, C, n = x.shape
    xd = torch.from_numpy(x).cuda()
    ln = torch.tensor(lens, dtype=torch.int32).cuda()
    g = None if gains is None else torch.tensor(gains, dtype=torch.float32).cuda()
    cap = sum(lens) if out_cap is None else out_cap
    out = torch.full((C, max(cap, 1) if out_ld is None else out_ld), CANARY, device="cuda")
    out_len = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    spans = torch.full((max(B, 1), 3), -9, dtype=torch.int32, device="cuda")
    rc = lib.zv_wavjoin_apply(h, engine._ptr(xd), n, engine._ptr(ln), engine._ptr(g), B, C,
                              engine._ptr(out), out.shape[1], cap, engine._ptr(out_len),
                              engine._ptr(spans), engine._stream())
    assert rc == 0, lib.zv_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(out_len.item()), spans[:B].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check(x, lens, gains=None, params=P):
    """The engine against the reference on one batch; returns the reference result."""
    r = ref.wavjoin(x, lens, gains, **params)
    print(f"wavjoin B={len(lens)} C={x.shape[1]} lens={lens}: margin {r.margin:.3e} "
          f"m={r.m.tolist()} F={r.F.tolist()} N={r.out.shape[1]}")
    assert r.margin >= 1e-3, r.margin                    # a condition on the inputs
    out, N, spans = apply(x, lens, gains, params)
    cap = sum(lens)
    assert np.array_equal(spans, np.stack([r.m, r.off, r.F], 1))
    assert N == r.out.shape[1]
    g = np.ones(len(lens)) if gains is None else np.asarray(gains, np.float64)
    peak = max([float(np.abs(g[b] * x[b, :, :lens[b]]).max()) for b in range(len(lens)) if lens[b]],
               default=0.0)
    err = float(np.abs(out[:, :N] - r.out).max()) if N else 0.0
    tol = 4 * 2.0 ** -23 * peak
    print(f"  max err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)
    # outside the overlaps, with gain 1: the input's bits
    live = [b for b in range(len(lens)) if r.m[b]]
    for i, b in enumerate(live):
        if g[b] != 1.0:
            continue
        lo = int(r.F[b])
        hi = int(r.m[b] - (r.F[live[i + 1]] if i + 1 < len(live) else 0))
        src = x[b][:, r.kept[b][lo:hi]]
        assert np.array_equal(bits(out[:, r.off[b] + lo:r.off[b] + hi]), bits(src)), b
    assert not out[:, N:cap].any()                       # zero-filled up to the capacity
    return r, out[:, :N]


def test_trim_and_join_against_reference():
    rng = np.random.default_rng(0)
    x, lens = batch([
        noise(rng, (QUIET, 1000), (LOUD, 3001), (QUIET, 5003), (LOUD, 777), (QUIET, 2500)),
        noise(rng, (QUIET, 4000)),                       # an empty chunk in the middle
        noise(rng, (LOUD, 100)),                         # shorter than a frame
        noise(rng, (LOUD, 1203), (QUIET, 700), (LOUD, 1500)),   # a gap of <= max_gap frames
        noise(rng, (QUIET, 239), (LOUD, 2), (QUIET, 239)),
        noise(rng, (LOUD, 6000))])
    assert x.shape[2] == max(lens) + 13
    r, _ = check(x, lens, [1, 1, 0.5, 1, 1, 0.25])
    # chunk 0: loud frames 4..16 and 37..40, 2 + 2 of the 20 quiet frames between, 2 + 2 at
    # the edges; chunk 4's two loud samples (0.1 |z| each, one per frame) stay under the
    # frame threshold with this seed, so it is a second empty chunk
    assert r.m.tolist() == [240 * (2 + 13 + 4 + 4 + 2), 0, 100, 3403, 0, 6000]
    assert r.F.tolist() == [0, 0, 50, 50, 0, 480]


def test_single_chunk():
    rng = np.random.default_rng(1)
    x, lens = batch([noise(rng, (QUIET, 900), (LOUD, 1000), (QUIET, 1300))])
    r, _ = check(x, lens)
    assert r.off.tolist() == [0] and r.F.tolist() == [0] and 0 < r.m[0] < lens[0]


def test_first_and_last_chunk_empty():
    rng = np.random.default_rng(2)
    x, lens = batch([noise(rng, (QUIET, 500)), noise(rng, (LOUD, 700)), noise(rng, (LOUD, 300)),
                     noise(rng, (QUIET, 900))])
    r, _ = check(x, lens)
    assert r.off.tolist() == [-1, 0, 700 - 150, -1]


def test_zero_length_chunk_and_all_empty():
    rng = np.random.default_rng(3)
    x, lens = batch([noise(rng, (LOUD, 1000)), np.zeros(0, np.float32), noise(rng, (LOUD, 800))])
    assert lens[1] == 0
    r, _ = check(x, lens)
    assert r.m.tolist() == [1000, 0, 800]
    x, lens = batch([noise(rng, (QUIET, 1000)), np.zeros(0, np.float32)])
    r, out = check(x, lens)
    assert out.shape == (1, 0)


def test_fade_zero_is_plain_concatenation():
    rng = np.random.default_rng(4)
    x, lens = batch([noise(rng, (QUIET, 700), (LOUD, 1000)), noise(rng, (LOUD, 501), (QUIET, 900)),
                     noise(rng, (LOUD, 77))])
    r, out = check(x, lens, params=dict(P, fade=0))
    assert not r.F.any()
    want = np.concatenate([x[b][:, r.kept[b]] for b in range(3)], axis=1)
    assert np.array_equal(bits(out), bits(want))


def test_quiet_runs_at_the_gap_threshold():
    rng = np.random.default_rng(5)
    x, lens = batch([noise(rng, (LOUD, 480), (QUIET, 4 * 240), (LOUD, 480), (QUIET, 5 * 240),
                           (LOUD, 480))])
    r, _ = check(x, lens)
    assert r.m[0] == lens[0] - 240                       # only the longer run loses a frame
    r, _ = check(x, lens, params=dict(P, max_gap=3))     # odd: 2 frames in front, 1 behind
    assert r.m[0] == lens[0] - 240 - 2 * 240
    r, _ = check(x, lens, params=dict(P, max_gap=0))
    assert r.m[0] == 3 * 480


def test_keep_edge_beyond_the_chunk_edge():
    rng = np.random.default_rng(6)
    x, lens = batch([noise(rng, (QUIET, 300), (LOUD, 500), (QUIET, 400)),
                     noise(rng, (QUIET, 2400), (LOUD, 500), (QUIET, 250))])
    r, _ = check(x, lens, params=dict(P, keep_edge=5))
    assert r.m.tolist() == [1200, 5 * 240 + (3150 - 2400)]


def test_long_chunk_spans_many_workgroups():
    rng = np.random.default_rng(7)
    x, lens = batch([noise(rng, (LOUD, 30000), (QUIET, 10001), (LOUD, 30000)),
                     noise(rng, (LOUD, 1501))])
    assert lens[0] == 70001
    r, _ = check(x, lens, [0.7, 1.0])
    assert r.m[0] < 70001 - 8000 and r.F[1] == 480


@pytest.mark.parametrize("frame", [1, 7, 250])
def test_frame_sizes_off_the_vector_width(frame):
    """Frames that are no multiple of 4 samples: a thread's 4 samples straddle frames, kept
    and dropped ones included, so they move one by one."""
    rng = np.random.default_rng(13)
    n = 9 * frame
    x, lens = batch([noise(rng, (QUIET, 3 * frame), (LOUD, n), (QUIET, 7 * frame), (LOUD, n + 3),
                           (QUIET, 2 * frame + 1)),
                     noise(rng, (LOUD, 5 * frame + 2))])
    r, _ = check(x, lens, [1.0, 0.5], params=dict(P, frame=frame, keep_edge=1, fade=3 * frame + 1))
    assert 0 < r.m[0] < lens[0] and r.F[1] > 0


def test_two_channels_share_the_plan():
    rng = np.random.default_rng(8)
    seg = [1200, 1500, 2000, 900, 1003]
    ch0 = noise(rng, *zip([QUIET, LOUD, QUIET, QUIET, QUIET], seg))
    ch1 = noise(rng, *zip([QUIET, QUIET, QUIET, LOUD, QUIET], seg))   # loud where ch0 is quiet
    other = np.stack([noise(rng, (LOUD, 2000)), noise(rng, (QUIET, 2000))])
    x, lens = batch([np.stack([ch0, ch1]), other])
    assert x.shape[1] == 2
    r, out = check(x, lens, [1.0, 0.5])
    assert out.shape[0] == 2 and 0 < r.m[0] < lens[0] and r.m[1] == 2000


def test_same_call_twice_is_bitwise_equal():
    rng = np.random.default_rng(9)
    x, lens = batch([noise(rng, (QUIET, 1000), (LOUD, 3000), (QUIET, 3000), (LOUD, 500)),
                     noise(rng, (LOUD, 2500)), noise(rng, (LOUD, 900), (QUIET, 500))])
    a = apply(x, lens, [0.3, 1.0, 0.9])
    b = apply(x, lens, [0.3, 1.0, 0.9])
    assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[0]), bits(b[0]))


def test_small_out_cap_is_respected_and_reported():
    rng = np.random.default_rng(10)
    x, lens = batch([noise(rng, (LOUD, 3000)), noise(rng, (LOUD, 2001), (QUIET, 2000)),
                     noise(rng, (LOUD, 1500))])
    r = ref.wavjoin(x, lens, None, **P)
    assert r.margin >= 1e-3
    N = r.out.shape[1]
    for cap in (N - 1000, 1234, 1, 0):
        out, n, spans = apply(x, lens, out_cap=cap, out_ld=sum(lens))
        assert n == N                                    # the true length, so the caller sees it
        assert np.array_equal(spans, np.stack([r.m, r.off, r.F], 1))
        assert (out[:, cap:] == CANARY).all()            # nothing at or past out_cap
        tol = 4 * 2.0 ** -23 * float(np.abs(x).max())
        assert np.abs(out[:, :cap] - r.out[:, :cap]).max(initial=0.0) <= tol


def test_python_joiner():
    rng = np.random.default_rng(11)
    x, lens = batch([noise(rng, (QUIET, 1000), (LOUD, 3000)), noise(rng, (LOUD, 2000), (QUIET, 700))])
    j = WavJoiner(frame=240, threshold_db=-42.0, keep_edge=2, max_gap=4, fade=480)
    r = ref.wavjoin(x, lens, [1.0, 0.5], **P)
    out, spans = j(torch.from_numpy(x[:, 0]).cuda(), lens, [1.0, 0.5])
    assert out.is_cuda and out.shape == r.out.shape and spans.dtype == torch.int32
    assert np.array_equal(spans.cpu().numpy(), np.stack([r.m, r.off, r.F], 1))
    assert np.abs(out.cpu().numpy() - r.out).max() <= 4 * 2.0 ** -23
    out2, _ = j(torch.from_numpy(x).cuda(), torch.tensor(lens))       # (B, C, n), no gains
    assert out2.shape == r.out.shape and j.device_bytes() > 0
    with pytest.raises(ValueError):
        j(torch.from_numpy(x).cuda(), [lens[0], x.shape[2] + 1])


def test_rejections():
    lib = engine.load_library()
    err = lambda: lib.zv_last_error().decode()  # noqa: E731
    for args, word in (((0, THR, 2, 4, 480), "frame"), ((240, -1.0, 2, 4, 480), "thr"),
                       ((240, THR, -1, 4, 480), "keep_edge"), ((240, THR, 2, -1, 480), "max_gap"),
                       ((240, THR, 2, 4, -1), "fade")):
        assert not lib.zv_wavjoin_create(*args)
        assert word in err(), (args, err())
    assert lib.zv_wavjoin_device_bytes(None) == 0
    h = handle(**P)
    x = torch.zeros((2, 1, 512), device="cuda")
    ln = torch.tensor([512, 512], dtype=torch.int32, device="cuda")
    out = torch.zeros((3, 1024), device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call(B, C, out_ld, out_cap, hh=h):
        return lib.zv_wavjoin_apply(hh, engine._ptr(x), 512, engine._ptr(ln), None, B, C,
                                    engine._ptr(out), out_ld, out_cap, engine._ptr(n), None,
                                    engine._stream())
    for C in (0, 3):
        assert call(2, C, 1024, 1024) != 0 and "C must be 1 or 2" in err()
    assert call(-1, 1, 1024, 1024) != 0 and "B must be non-negative" in err()
    assert call(2, 1, 1000, 1001) != 0 and "out_cap exceeds out_ld" in err()
    assert call(2, 1, 1024, 1024, None) != 0 and "null" in err()
    assert call(2, 1, 1024, 1024) == 0 and call(0, 1, 1024, 1024) == 0
    torch.cuda.synchronize()
    assert int(n.item()) == 0


def test_warm_call_does_not_block_the_host():
    rng = np.random.default_rng(12)
    x, lens = batch([noise(rng, (LOUD, 3000), (QUIET, 2000)), noise(rng, (LOUD, 2000))])
    lib = engine.load_library()
    h = handle(**P)
    xd = torch.from_numpy(x).cuda()
    ln = torch.tensor(lens, dtype=torch.int32).cuda()
    out = torch.empty((1, sum(lens)), device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    sp = torch.zeros((2, 3), dtype=torch.int32, device="cuda")

    def call():
        assert lib.zv_wavjoin_apply(h, engine._ptr(xd), x.shape[2], engine._ptr(ln), None, 2, 1,
                                    engine._ptr(out), out.shape[1], out.shape[1], engine._ptr(n),
                                    engine._ptr(sp), engine._stream()) == 0
    call()                                               # warm-up: the scratch may grow here
    torch.cuda.synchronize()
    before = lib.zv_host_block_count()
    call()
    assert lib.zv_host_block_count() == before
    torch.cuda.synchronize()
    assert int(n.item()) == int(ref.wavjoin(x, lens, None, **P).out.shape[1])


# ------------------------------------------------------------------------ end to end
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


def test_generate_long_end_to_end(stack):
    m, voc, fx = stack
    rng = np.random.default_rng(0)
    BREAK, SOFT = (3, 4), (5,)
    tokens = [int(t) for t in rng.integers(10, 90, 120)]
    for i in (17, 33, 41, 58, 79, 96, 110):
        tokens[i] = BREAK[i % 2]
    for i in (8, 25, 50, 70, 101):
        tokens[i] = SOFT[0]
    prompt_tokens = list(range(40, 52))
    pw = (0.05 * rng.standard_normal(24000)).astype(np.float32)     # 1 s, quieter than target
    max_seconds, batch_size = 5.0, 2
    budget = chunk_budget(len(prompt_tokens), 1.0, max_seconds)
    assert budget == 48
    chunks = chunk_tokens(tokens, BREAK, budget, SOFT)
    K = len(chunks)
    assert K >= 3
    groups = [chunks[i:i + batch_size] for i in range(0, K, batch_size)]
    assert len(groups) == 2

    # the same prompt features, groups and initial noise, called directly
    w, rms = _prompt_rms_normalise(torch.from_numpy(pw)[None], 0.1)
    assert rms < 0.1
    pf = ((fx.extract(w.cuda(), sampling_rate=24000).unsqueeze(0) + 0.0) * 0.1)
    Pn = pf.size(1)
    gen = torch.Generator().manual_seed(0)
    x0, direct = [], []
    for grp in groups:
        fl = predict_features_lens(torch.full((len(grp),), Pn), torch.full((len(grp),), 12),
                                   torch.tensor([len(c) for c in grp]), 1.0)
        x0.append(torch.randn(len(grp), int(fl.max()), 100, generator=gen).cuda())
    for grp, z in zip(groups, x0):
        pred, pl, _, _ = m.sample(tokens=grp, prompt_tokens=[prompt_tokens] * len(grp),
                                  prompt_features=pf.expand(len(grp), -1, -1).contiguous(),
                                  prompt_features_lens=torch.full((len(grp),), Pn), speed=1.0,
                                  t_shift=0.5, duration="predict", num_step=4,
                                  guidance_scale=1.0, x0=z)
        wv = voc.decode_features(pred, pl, feat_scale=0.1, feat_bias=0.0, clamp=True)
        direct += [wv[i, :int(pl[i]) * 256] for i in range(len(grp))]

    wav, met, cw, spans = generate_long(tokens, prompt_tokens, pw, m, voc, fx, BREAK, SOFT,
                                        max_seconds=max_seconds, batch_size=batch_size, x0=x0,
                                        return_chunks=True, num_step=4)
    assert met["num_chunks"] == K and met["num_batches"] == 2
    for k in ("t", "wav_seconds", "rtf"):
        assert met[k] > 0
    assert len(cw) == K
    for a, b in zip(cw, direct):
        assert a.shape == b.shape and a.numel() > 0 and torch.equal(a, b)

    j = WavJoiner()
    xs = [c.cpu().numpy() for c in cw]
    r = ref.wavjoin(xs, [len(c) for c in xs], [rms / 0.1] * K, j.frame, j.thr, j.keep_edge,
                    j.max_gap, j.fade)
    print(f"generate_long: K={K} lens={[len(c) for c in xs]} m={r.m.tolist()} F={r.F.tolist()} "
          f"margin {r.margin:.3e}")
    assert r.margin >= 1e-3, r.margin
    assert wav.shape == (1, r.out.shape[1]) and torch.isfinite(wav).all()
    assert np.array_equal(spans.cpu().numpy(), np.stack([r.m, r.off, r.F], 1))
    peak = max(float(np.abs(c).max()) for c in xs) * rms / 0.1
    assert np.abs(wav.cpu().numpy() - r.out).max(initial=0.0) <= 4 * 2.0 ** -23 * peak
    assert abs(met["wav_seconds"] - wav.shape[1] / 24000) < 1e-9
