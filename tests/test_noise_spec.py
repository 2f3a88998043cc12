"""The seeded-noise definition (include/zipvoice_hip.h, zv_noise_normal) without a GPU: the numpy
restatement tests/noise_ref.py and the library's host functions (zv_noise_check, where = 0)
against the Random123 known answers, the counter carry, the edge words of the Box-Muller step,
the moments of the definition, and the argument checks of the Python layer that precede the
engine."""
import numpy as np
import pytest

import noise_ref
from noise_cases import CARRY, KAT, check_normals, edge_words, lib_bits, lib_normals

torch = pytest.importorskip("torch")


def test_known_answers_reference():
    for counter, key, want in KAT:
        assert noise_ref.philox4x32_10(counter, key).tolist() == list(want)
        assert noise_ref.philox_blocks(counter, key, 1)[0].tolist() == list(want)


def test_known_answers_host():
    for counter, key, want in KAT:
        assert lib_bits(counter, key, 1)[0].tolist() == list(want)


def test_counter_carry_host():
    counter, key, nb = CARRY
    want = noise_ref.philox_blocks(counter, key, nb)
    # the second block's counter is (0, 1, 7, 0): the carry went into word 1
    assert want[1].tolist() == noise_ref.philox4x32_10((0, 1, 7, 0), key).tolist()
    assert want[2].tolist() == noise_ref.philox4x32_10((1, 1, 7, 0), key).tolist()
    assert np.array_equal(lib_bits(counter, key, nb), want)


def test_edge_word_radius():
    """The edge values the definition names: u(0) = 2^-33 (r ~ 6.76), u(0xffffffff) rounds to 1."""
    assert noise_ref.unit(0) == np.float32(2.0 ** -33)
    assert noise_ref.unit(0xffffffff) == np.float32(1.0)
    _, r = noise_ref.box_muller(np.array([0, 0, 0xffffffff, 0], np.uint32))
    assert abs(r[0] - 6.7637) < 1e-3 and r[2] == 0.0


def test_normals_host_edges():
    words = edge_words()
    frac = check_normals(lib_normals(words), words)
    print(f"host normals, edge words: largest fraction of the bound {frac:.3f}")


def test_reference_moments():
    """Seed 1234, stream 0, 2^22 blocks: the definition itself draws standard normals."""
    z = noise_ref.normal(1234, 0, 1 << 24)
    N = z.size
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    print(f"mean {mean:.3e} var {var:.6f} kurtosis {kurt:.4f} max |z| {np.abs(z).max():.3f}")
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1) <= 5 * np.sqrt(2 / N)
    assert abs(kurt - 3) <= 0.02
    # the figures recorded with the definition
    assert abs(mean - 1.9e-4) < 0.1e-4 and abs(var - 0.99998) < 1e-5
    assert abs(kurt - 2.998) < 1e-3 and abs(np.abs(z).max() - 6.13) < 0.01


def test_reference_row_is_prefix_stable():
    """Element e depends on (seed, stream, e) alone: a shorter row is a prefix of a longer one."""
    a, b = noise_ref.normal(5, 3, 37 * 100), noise_ref.normal(5, 3, 20 * 100 + 1)
    assert np.array_equal(a[:b.size], b)
    assert not np.array_equal(noise_ref.normal(5, 4, 64), a[:64])
    assert not np.array_equal(noise_ref.normal(6, 3, 64), a[:64])


def test_noise_normal_rejects_bad_arguments():
    from zipvoice_amd import engine
    lib = engine.load_library()
    for B, n, ld, msg in ((0, 4, 4, "B must be"), (-1, 4, 4, "B must be"), (1, -1, 4, "n must be"),
                          (1, 8, 7, "ld < n")):
        assert lib.zv_noise_normal(None, None, B, n, ld, None, None) != 0
        assert msg in lib.zv_last_error().decode()
    assert lib.zv_noise_normal(None, None, 1, 0, 0, None, None) == 0      # n == 0: nothing to do


def test_seeded_normal_argument_errors():
    from zipvoice_amd.noise import check_keys, seeded_normal, seeded_normal_into
    for bad in ([-1], [1 << 64], [1.5], ["7"], [True], [], 7, "12", torch.tensor([1, 2])):
        with pytest.raises(ValueError):
            seeded_normal(bad, (4, 100))
    with pytest.raises(ValueError):
        seeded_normal([1, 2], (4, 100), streams=[0])             # one stream per seed
    with pytest.raises(ValueError):
        seeded_normal([1], (4, 100), streams=[-1])
    with pytest.raises(ValueError):
        seeded_normal([1], (4, 100), streams=[1 << 32])
    with pytest.raises(ValueError):
        seeded_normal([1], (-4, 100))
    with pytest.raises(ValueError):
        seeded_normal_into(torch.zeros(3, 8), [1, 2])            # one seed per row
    assert check_keys([0, (1 << 64) - 1], [0, (1 << 32) - 1], 2) == ([0, (1 << 64) - 1],
                                                                     [0, (1 << 32) - 1])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                        # no CPU fallback
            seeded_normal([1], (4, 100))


def test_sample_argument_errors():
    """The checks of sample() that precede the engine (the model is not on a GPU)."""
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    m = build_model(default_config("zipvoice"))
    kw = dict(tokens=[[1, 2, 3], [4, 5]], prompt_tokens=[[6], [7]],
              prompt_features=torch.zeros(2, 10, 100), prompt_features_lens=torch.tensor([10, 8]))
    with pytest.raises(ValueError, match="not both"):
        m.sample(**kw, x0=torch.zeros(2, 30, 100), seeds=[1, 2])
    with pytest.raises(ValueError, match="needs seeds"):
        m.sample(**kw, seed_streams=[0, 1])
    with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
        m.sample(**kw, seeds=[1, -2])
    with pytest.raises(ValueError, match="one seed per row"):
        m.sample(**kw, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="one stream per seed"):
        m.sample(**kw, seeds=[1, 2], seed_streams=[0])
    with pytest.raises(RuntimeError):                            # valid seeds reach the engine check
        m.sample(**kw, seeds=[1, 2])
