#!/usr/bin/env python3
"""Generate tests/golden/sample_intermediate.npz by running the REFERENCE's
``ZipVoice.sample_intermediate`` (zipvoice/models/zipvoice.py:488-534) on CPU.

Container-only tool, as make_golden.py, whose ``build`` (reference model + the engine's
synthetic weights) it reuses; it writes only its own fixture and leaves MANIFEST.json alone.
Default config, B = 2 with 37 and 29 frames, one interior masked span per row aligned to
nothing, num_step = 2, a (B, 1, 1) guidance tensor, t_start = 0, t_end = 1.  The fixture holds
the inputs and the output only.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_edit.py
"""
import numpy as np

import make_golden as mg  # (stubs tensorboard, puts the reference on sys.path)

import torch  # noqa: E402


@torch.inference_mode()
def main():
    torch.set_num_threads(8)
    cfg, model = mg.build("zipvoice")
    rng = np.random.default_rng(21)
    B, F = 2, cfg.io_feat_dim
    lens = np.array([37, 29], np.int64)
    T = int(lens.max())
    tokens = [mg.rand_tokens(rng, n) for n in (9, 7)]
    feats = (0.3 * rng.standard_normal((B, T, F)) - 0.5).astype(np.float32)
    noise = np.random.default_rng(667).standard_normal((B, T, F), dtype=np.float32)
    mask = np.zeros((B, T), bool)
    mask[0, 11:24] = True
    mask[1, 5:18] = True
    for b in range(B):
        feats[b, lens[b]:] = 0.0
    guidance = np.array([1.0, 0.6], np.float32).reshape(B, 1, 1)
    x, x_lens = model.sample_intermediate(
        tokens=tokens, features=torch.from_numpy(feats), features_lens=torch.from_numpy(lens),
        noise=torch.from_numpy(noise), speech_condition_mask=torch.from_numpy(mask),
        t_start=0.0, t_end=1.0, num_step=2, guidance_scale=torch.from_numpy(guidance))
    mg.save("sample_intermediate.npz", tokens=mg.ragged_tokens_array(tokens), features=feats,
            features_lens=lens, noise=noise, speech_condition_mask=mask, t_start=np.float32(0.0),
            t_end=np.float32(1.0), num_step=np.int64(2), guidance_scale=guidance, x=x.numpy(),
            x_lens=x_lens.numpy(), variant=np.array("zipvoice"), seed=np.int64(mg.SEED))


if __name__ == "__main__":
    main()
