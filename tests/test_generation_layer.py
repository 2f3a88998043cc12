"""The shared steps of the generation layer: the two level restores (infer.restore_level, infer.output_gain),
the batched wave front (infer._prompts_at_rate) on prompts that need no resampling, and the one noise draw
(noise.initial_noise)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from zipvoice_amd import infer  # noqa: E402
from zipvoice_amd.noise import initial_noise, seeded_normal  # noqa: E402

TARGET = 0.1


def test_restore_level_is_the_two_step_form():
    w = torch.from_numpy(np.random.default_rng(0).standard_normal(1001).astype(np.float32))
    for rms in (TARGET, 0.25):
        assert infer.restore_level(w, rms, TARGET) is w
    rms = 0.037
    assert torch.equal(infer.restore_level(w, rms, TARGET), w * rms / TARGET)


def test_output_gain_is_the_python_expression():
    for rms in (0.037, 0.0999, TARGET, 0.3):
        want = rms / TARGET if rms < TARGET else 1.0
        got = infer.output_gain(rms, TARGET)
        assert type(got) is float and got == want


def test_wave_front_leaves_prompts_at_the_models_rate_on_the_host(monkeypatch):
    def no_resampler(*a):
        raise AssertionError("a prompt at the model's rate was sent to the resampler")
    monkeypatch.setattr(infer, "_resampler", no_resampler)
    rng = np.random.default_rng(1)
    wavs = [rng.standard_normal(n).astype(np.float32) for n in (5, 1, 9)]
    rows = infer._prompts_at_rate(wavs, [None, 24000, None], 24000, "cuda:0")
    assert len(rows) == 3
    for w, r in zip(wavs, rows):
        assert r.device.type == "cpu" and r.dtype == torch.float32 and r.shape == w.shape
        assert r.data_ptr() == w.ctypes.data and np.array_equal(r.numpy(), w)


B, T, F = 3, 5, 4


@pytest.mark.gpu
def test_noise_mixed_rows():
    torch.manual_seed(0)
    got = initial_noise(B, T, F, "cuda:0", seeds=[7, None, 9])
    torch.manual_seed(0)
    plain = torch.randn(B, T, F, device="cuda:0")
    keyed = seeded_normal([7, 9], (T, F), device="cuda:0")
    assert got.shape == (B, T, F) and got.dtype == torch.float32
    assert torch.equal(got[0], keyed[0]) and torch.equal(got[2], keyed[1]) and torch.equal(got[1], plain[1])


@pytest.mark.gpu
def test_noise_all_rows_seeded():
    seeds, streams = [7, 8, (1 << 64) - 1], [0, 3, 1]
    assert torch.equal(initial_noise(B, T, F, "cuda:0", seeds=seeds), seeded_normal(seeds, (T, F), device="cuda:0"))
    assert torch.equal(initial_noise(B, T, F, "cuda:0", seeds=seeds, streams=streams),
                       seeded_normal(seeds, (T, F), streams, device="cuda:0"))


@pytest.mark.gpu
def test_noise_argument_checks():
    x0 = torch.zeros(B, T, F, device="cuda:0")
    assert initial_noise(B, T, F, "cuda:0", x0=x0) is x0
    with pytest.raises(ValueError, match="shape"):
        initial_noise(B, T + 1, F, "cuda:0", x0=x0)
    with pytest.raises(ValueError, match="not both"):
        initial_noise(B, T, F, "cuda:0", x0=x0, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="needs seeds"):
        initial_noise(B, T, F, "cuda:0", streams=[0, 1, 2])
