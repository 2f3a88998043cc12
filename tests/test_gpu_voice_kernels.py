"""The voice store's kernels (zv_prompt_rms, zv_prompt_scale, zv_voice_gather) against tests/voice_ref.py,
bit for bit: the header fixes the order of every operation, so there is no tolerance.

* rms: rows of 1, 255, 256, 257, 4097 and 33000 samples in one batch at ld = 33008, NaN in every column
  past a row's length (a read there would poison the sum), levels on both sides of the target and within
  a few ulp of it; each row alone (B = 1, ld = len) gives the same bits.
* scale: the same rows, the output pre-filled with NaN; ld = 33008 takes the 16-byte form, ld = 33002 the
  one-sample form.
* gather: voices of 5, 37 and 38 frames at non-adjacent offsets, five rows with repeats, T in
  {38, 41, 97}; bitwise the numpy gather and engine.speech_condition on the padded prompts; F = 99 for the
  one-value form; rejections launch nothing and leave the handle usable."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_fullsize as fs  # noqa: E402
import voice_ref  # noqa: E402
from zipvoice_amd import voices  # noqa: E402

TARGET = 0.1
LENS = [1, 255, 256, 257, 4097, 33000]
LD = 33008


def rows():
    """Row levels: 0.03 | target - 2 ulp | target | target + 2 ulp | 0.3 | 0.03.  The three rows around the
    target hold +-a with random signs, whose rms is a to the last bit or next to it."""
    rng = np.random.default_rng(61)
    t = np.float32(TARGET)
    below = np.nextafter(np.nextafter(t, np.float32(0)), np.float32(0))
    above = np.nextafter(np.nextafter(t, np.float32(1)), np.float32(1))
    out = [np.array([0.03], np.float32)]
    for n, a in zip(LENS[1:4], (below, t, above)):
        out.append((a * rng.choice([-1.0, 1.0], n)).astype(np.float32))
    out.append((0.3 * rng.standard_normal(LENS[4])).astype(np.float32))
    out.append((0.03 * rng.standard_normal(LENS[5])).astype(np.float32))
    return out


def padded(xs, ld, fill=np.nan):
    wb = np.full((len(xs), ld), fill, np.float32)
    for i, x in enumerate(xs):
        wb[i, :x.size] = x
    return wb


@pytest.fixture(scope="module")
def measured():
    xs = rows()
    rms, gin, gout, ln = voices.prompt_rms(fs.cuda(padded(xs, LD)), LENS, TARGET)
    return xs, rms.cpu().numpy(), gin.cpu().numpy(), gout.cpu().numpy()


def test_prompt_rms_is_the_header_order(measured):
    xs, rms, gin, gout = measured
    want = np.array([voice_ref.prompt_rms(x) for x in xs], np.float32)
    print("rms:", rms, "reference:", want)
    assert np.array_equal(rms.view(np.int32), want.view(np.int32))
    assert (rms[[0, 1, 5]] < np.float32(TARGET)).all() and (rms[[3, 4]] >= np.float32(TARGET)).all()
    win, wout = voice_ref.gains(rms, TARGET)
    assert np.array_equal(gin.view(np.int32), win.view(np.int32))
    assert np.array_equal(gout.view(np.int32), wout.view(np.int32))
    assert (gin[[3, 4]] == 1).all() and (gout[[3, 4]] == 1).all() and gin[0] > 3 and gout[0] < 0.31


def test_prompt_rms_row_alone_is_the_row_in_the_batch(measured):
    xs, rms, gin, gout = measured
    for i, x in enumerate(xs):
        r, gi, go, _ = voices.prompt_rms(fs.cuda(x[None]), [x.size], TARGET)
        got = np.array([r.item(), gi.item(), go.item()], np.float32)
        assert np.array_equal(got.view(np.int32), np.array([rms[i], gin[i], gout[i]], np.float32).view(np.int32)), i


@pytest.mark.parametrize("ld", [LD, 33002])
def test_prompt_scale(measured, ld):
    xs, _, _, _ = measured
    wav = fs.cuda(padded(xs, ld))
    rms, _, _, ln = voices.prompt_rms(wav, LENS, TARGET)
    out = torch.full_like(wav, float("nan"))
    voices.prompt_scale(wav, LENS, ln, rms, TARGET, out=out)
    got, r = out.cpu().numpy(), rms.cpu().numpy()
    for i, x in enumerate(xs):
        want = voice_ref.prompt_scale(x, r[i], TARGET, ld)
        assert np.array_equal(got[i].view(np.int32), want.view(np.int32)), (ld, i)
        assert (got[i, x.size:] == 0).all()
        if r[i] >= np.float32(TARGET):
            assert np.array_equal(got[i, :x.size].view(np.int32), x.view(np.int32))      # a bit copy
        else:
            assert np.array_equal(got[i, :x.size], (x * np.float32(TARGET)) / r[i])
    # in place, as the store runs it
    voices.prompt_scale(wav, LENS, ln, rms, TARGET, out=wav)
    assert torch.equal(wav, out)


def test_prompt_kernels_reject_bad_lengths():
    wav = torch.zeros((2, 8), device="cuda:0")
    for lens in ([0, 4], [4, 9], [-1, 4]):
        with pytest.raises(RuntimeError, match="length"):
            voices.prompt_rms(wav, lens, TARGET)
    with pytest.raises(RuntimeError, match="target"):
        voices.prompt_rms(wav, [4, 4], 0.0)


VOICES = [(3, 5), (20, 37), (77, 38)]                 # (offset, frames) in a pool of 128 rows
ROWS = [1, 0, 2, 1, 0]


def raw_gather(g, pool, table, T, gpool=None):
    """zv_voice_gather into buffers that hold NaN before the call: the kernel must write every element."""
    from zipvoice_amd import engine
    n, F = len(table), pool.shape[1]
    out = torch.full((n, T, F), float("nan"), device="cuda:0")
    gains = None if gpool is None else torch.full((n,), float("nan"), device="cuda:0")
    tab = np.ascontiguousarray(np.asarray(table, np.int32))
    rc = g.lib.zv_voice_gather(g.h, engine._ptr(pool), pool.shape[0], F, tab.ctypes.data, n, T, engine._ptr(out),
                               engine._ptr(gpool), engine._ptr(gains), engine._stream())
    assert rc == 0, g.lib.zv_last_error().decode()
    return out, gains


@pytest.mark.parametrize("T", [38, 41, 97])
def test_voice_gather(T):
    rng = np.random.default_rng(62 + T)
    pool = rng.standard_normal((128, 100), dtype=np.float32)
    gpool = rng.standard_normal(128, dtype=np.float32)
    table = [VOICES[v] for v in ROWS]
    g = voices.VoiceGather("cuda:0")
    assert g.device_bytes() == 0
    out, gains = raw_gather(g, fs.cuda(pool), table, T, fs.cuda(gpool))
    want, wg = voice_ref.voice_gather(pool, table, T, gpool)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(gains.cpu().numpy().view(np.int32), wg.view(np.int32))
    # what zv_speech_condition makes of the padded prompt batch
    prompts = np.zeros((len(ROWS), 38, 100), np.float32)
    for r, (off, fr) in enumerate(table):
        prompts[r, :fr] = pool[off:off + fr]
    sc = fs.model("zipvoice", "fp32").engine.speech_condition(
        fs.cuda(prompts), torch.tensor([fr for _, fr in table], device="cuda:0"), T)
    assert torch.equal(out, sc)
    assert g.device_bytes() > 0
    # the Python entry on the warm handle, with and without gains
    out2, g2 = g(fs.cuda(pool), table, T, fs.cuda(gpool))
    out3, none = g(fs.cuda(pool), table[:2], T)
    assert torch.equal(out2, out) and torch.equal(g2, gains) and none is None and torch.equal(out3, out[:2])
    g.close()


def test_voice_gather_one_value_form():
    """F = 99 is no multiple of 4: one value per thread."""
    rng = np.random.default_rng(63)
    pool = rng.standard_normal((128, 99), dtype=np.float32)
    table = [VOICES[v] for v in ROWS]
    g = voices.VoiceGather("cuda:0")
    out, _ = raw_gather(g, fs.cuda(pool), table, 41)
    want, _ = voice_ref.voice_gather(pool, table, 41)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    g.close()


def test_voice_gather_rejections_leave_the_handle_usable():
    pool = torch.arange(128 * 100, dtype=torch.float32, device="cuda:0").reshape(128, 100)
    g = voices.VoiceGather("cuda:0")
    for table, T in (([(100, 29)], 38),               # a range past the pool
                     ([(3, 5), (20, 37)], 36),         # frames > T
                     ([(-1, 5)], 38), ([(3, 0)], 38),
                     ([], 38)):                         # n = 0
        with pytest.raises(ValueError, match="voice table"):
            g(pool, table, T)
    out, _ = g(pool, [(100, 28)], 38)                 # the last rows of the pool: just inside
    assert torch.equal(out[0, :28], pool[100:]) and (out[0, 28:] == 0).all()
    g.close()
