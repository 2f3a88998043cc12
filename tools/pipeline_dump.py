#!/usr/bin/env python3
"""Every generation entry's output as .npy files, for comparing two trees bit for bit.

Public entries only, so the same file runs on any commit that has them: run it from two checkouts
into two directories, then compare them (``--compare A B``: file by file with np.array_equal).

Setup: synthetic default-size ZipVoice in bf16, synthetic Vocos, VocosFbank, num_step = 2.  Inputs: the
two items of tests/test_gpu_session.py's ``serving`` fixture, a 16 kHz prompt of 6401 samples, a quiet
prompt (amplitude 0.02), and request 0 / 1 of tests/test_gpu_longform_batch.py for the long-form entries.

usage: pipeline_dump.py OUT_DIR | pipeline_dump.py --compare DIR_A DIR_B"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

BREAK, SOFT = (3, 4), (5,)
SET = dict(num_step=2, guidance_scale=1.0, speed=2.0, t_shift=0.5)


def compare(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = []
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        same = os.path.exists(pa) and os.path.exists(pb) and np.array_equal(np.load(pa), np.load(pb))
        print(f"{'equal   ' if same else 'DIFFERS '} {n}")
        bad += [] if same else [n]
    print(f"{len(names) - len(bad)} of {len(names)} files equal" + (f"; different: {bad}" if bad else ""))
    return 1 if bad or not names else 0


def inputs():
    rng = np.random.default_rng(37)
    items = [([int(t) for t in rng.integers(10, 90, n)], list(range(40, 40 + p)),
              (0.1 * rng.standard_normal(w)).astype(np.float32)) for n, p, w in ((8, 8, 9600), (7, 9, 8000))]
    wav16 = (0.1 * np.random.default_rng(38).standard_normal(6401)).astype(np.float32)
    quiet = (0.02 * np.random.default_rng(39).standard_normal(9000)).astype(np.float32)
    rng = np.random.default_rng(0)
    t0 = [int(t) for t in rng.integers(10, 90, 120)]
    for i in (17, 33, 41, 58, 79, 96, 110):
        t0[i] = BREAK[i % 2]
    for i in (8, 25, 50, 70, 101):
        t0[i] = SOFT[0]
    pw0 = (0.05 * rng.standard_normal(24000)).astype(np.float32)
    rng = np.random.default_rng(1)
    t1 = [int(t) for t in rng.integers(10, 90, 60)]
    t1[27], t1[59] = BREAK
    pw1 = (0.2 * rng.standard_normal(18000)).astype(np.float32)
    pw16 = (0.05 * np.random.default_rng(2).standard_normal(16000)).astype(np.float32)
    return items, wav16, quiet, [(t0, list(range(40, 52)), pw0), (t1, list(range(60, 69)), pw1)], pw16


def main(out):
    import torch
    from zipvoice_amd.config import default_config
    from zipvoice_amd.edit import edit_batch
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.infer import generate_batch, generate_sentence
    from zipvoice_amd.longform import generate_long, generate_long_batch, generate_long_stream
    from zipvoice_amd.models import build_model
    from zipvoice_amd.serving import ContinuousBatcher
    from zipvoice_amd.vocoder import Vocos
    from zipvoice_amd.voices import VoiceStore
    from zipvoice_amd.weights import synthetic_state_dict
    os.makedirs(out, exist_ok=True)
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="bf16")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m = m.to("cuda:0")
    voc, fx = Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()
    items, wav16, quiet, reqs, pw16 = inputs()
    toks, ptoks, _ = items[0]
    count = [0]

    def save(name, tensors):
        for i, t in enumerate(tensors):
            np.save(os.path.join(out, f"{name}.{i}.npy"), t.detach().float().cpu().numpy())
            count[0] += 1

    for name, wav, rate in (("24k", items[0][2], 24000), ("16k", wav16, 16000), ("quiet", quiet, 24000)):
        w, _ = generate_sentence(toks, ptoks, wav, m, voc, fx, prompt_sampling_rate=rate, seed=11, **SET)
        save(f"sentence_{name}", [w])

    mixed = items + [(toks, ptoks, wav16, 16000), (items[1][0], items[1][1], quiet)]
    seeds = [5, 6, 7, 8]
    save("batch_wav", generate_batch(mixed, m, voc, fx, seeds=seeds, **SET)[0])
    save("batch_trim", generate_batch(mixed, m, voc, fx, seeds=seeds, remove_long_sil=True, **SET)[0])
    save("batch_per_item", generate_batch(mixed, m, voc, fx, seeds=seeds, **dict(SET, num_step=[2, 1, 3, 2]))[0])
    store = VoiceStore(fx, 512)
    voices = store.register_batch([(it[2], it[1]) + tuple(it[3:]) for it in mixed])
    vitems = [(it[0], v) for it, v in zip(mixed, voices)]
    save("batch_voice", generate_batch(vitems, m, voc, fx, seeds=seeds, **SET)[0])
    save("batch_voice_trim", generate_batch(vitems, m, voc, fx, seeds=seeds, remove_long_sil=True, **SET)[0])

    long_kw = dict(max_seconds=5.0, batch_size=2, num_step=2)
    t0, pt0, pw0 = reqs[0]
    for name, pw, rate in (("24k", pw0, 24000), ("16k", pw16, 16000)):
        w, _, chunks, spans = generate_long(t0, pt0, pw, m, voc, fx, BREAK, SOFT, seed=3, return_chunks=True,
                                            prompt_sampling_rate=rate, **long_kw)
        save(f"long_{name}", [w, spans] + chunks)
        pieces = []
        for piece, info in generate_long_stream(t0, pt0, pw, m, voc, fx, BREAK, SOFT, seed=3, return_chunks=True,
                                                prompt_sampling_rate=rate, **long_kw):
            pieces += [piece, info["spans"]] + info["chunks"]
        save(f"long_stream_{name}", pieces)
    w, _, chunks, spans = generate_long(t0, pt0, pw0, m, voc, fx, BREAK, SOFT, seed=3, return_chunks=True,
                                        max_seconds=5.0, batch_size=32, num_step=2)      # (one group)
    save("long_one_group", [w, spans] + chunks)
    both = reqs + [(reqs[1][0], pt0, pw16, 16000)]
    for name, srt in (("sorted", True), ("unsorted", False)):
        ws, _, chunks, spans, _ = generate_long_batch(both, m, voc, fx, BREAK, SOFT, seeds=[3, 4, 5],
                                                      sort_by_length=srt, return_chunks=True, **long_kw)
        save(f"long_batch_{name}", ws + [spans] + chunks)

    ws, _ = edit_batch([(toks + toks[:3], wav16, [(10, 20, 12)], 16000), (toks, items[1][2], [])], m, voc, fx,
                       num_step=2, seeds=[9, 10])
    save("edit", ws)
    ws, _ = edit_batch([(toks + toks[:3], quiet, [(5, 9, 6), (20, 20, 3)])], m, voc, fx, num_step=[2], seeds=[9])
    save("edit_quiet_scheduled", ws)

    def batcher(name, submits, **kw):
        cb = ContinuousBatcher(m, voc, fx, max_rows=2, max_frames=97, **kw)
        for s in submits:
            cb.submit(*s[0], **dict(SET, **s[1]))
        got = dict(cb.drain())
        cb.close()
        save(name, [got[t] for t in sorted(got)])

    batcher("batcher_wav", [((it[0], it[1], it[2]) + tuple(it[3:]), dict(seed=s)) for it, s in zip(mixed, seeds)])
    batcher("batcher_voice", [((it[0],), dict(voice=v, seed=s)) for it, v, s in zip(mixed, voices, seeds)], voices=store)
    torch.manual_seed(0)
    batcher("batcher_mixed_seeds", [(items[0], dict(seed=5)), (items[1], dict())])
    torch.manual_seed(0)
    batcher("batcher_voice_mixed_seeds", [((items[0][0],), dict(voice=voices[0])),
                                         ((items[1][0],), dict(voice=voices[1], seed=6))], voices=store)
    torch.cuda.synchronize()
    print(f"pipeline_dump: {count[0]} arrays in {out}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
