#!/usr/bin/env python3
"""Edits through the editing service (recordings in a VoiceStore, ContinuousBatcher.submit_edit) against
edit.edit_batch on wav items, the only form of an edit before the service.  Writes
profiles/edit_service_ab.txt (or --out PATH).

Model: synthetic default-size ZipVoice (the C2 model), bf16, synthetic Vocos, VocosFbank.  Every
measurement alternates its two arms over ROUNDS rounds after a warm-up of each, with a device
synchronise between arms.  Informational: no threshold is set on these figures.

(a) Host stall: a 32-slot x 1219-frame ContinuousBatcher with 24 generation rows (voices) in flight and 8
    ticks queued and not synchronised; then 8 edits of 10 s recordings arrive.  service: submit_edit x 8
    and the host clock inside the next step() (retire nothing, admit 8, tick).  wav: the host clock inside
    edit_batch on the same 8 recordings as wav items with the same ticks queued: a closed batch, which
    synchronises and so waits for everything queued ahead of it.  Per arm also the host clock to a
    synchronise after it (service: the admitting tick done; wav: the 8 edited waveforms done).
(b) Front of one admission: the same 8 edits, from the first host call until 8 slots of a session hold
    them.  wav: edit_batch's front (resample, host RMS, pad, upload, fbank, scale and bias), the plan,
    engine.edit_gather for the speech condition, session.admit.  service: the plans and
    session.admit_edit from the store's arena.  x0 and the text condition are made beforehand in both.

usage: edit_service_bench.py [--out PATH]"""
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import session_bench as sb  # noqa: E402
from voice_bench import timed  # noqa: E402
from zipvoice_amd.edit import edit_batch, plan_edit_batch  # noqa: E402
from zipvoice_amd.infer import _prompt_rms_normalise, _prompts_at_rate  # noqa: E402
from zipvoice_amd.serving import ContinuousBatcher  # noqa: E402
from zipvoice_amd.solver import RowSchedule  # noqa: E402
from zipvoice_amd.voices import VoiceStore  # noqa: E402

ROUNDS, SLOTS, MAX_FRAMES, EDITS = 3, 32, 1219, 8
SAMPLES, SPAN = 240000, (400, 500, 100)          # 10 s at 24 kHz (938 frames); 100 frames regenerated
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def sync():
    torch.cuda.synchronize()


def report(name, rows, labels):
    for k, what in enumerate(labels):
        v = [r[k] for r in rows]
        say(f"  {name:8s} {what:15s} " + " ".join(f"{x:9.3f}" for x in v) + f" ms   median {statistics.median(v):9.3f}")


def make_edits(seed):
    rng = np.random.default_rng(seed)
    return [([int(t) for t in rng.integers(10, 90, 130)], (0.05 * rng.standard_normal(SAMPLES)).astype(np.float32), [SPAN])
            for _ in range(EDITS)]


def stall(m, voc, fx):
    rng = np.random.default_rng(5)
    P = (sb.PROMPT_SAMPLES + 128) // 256
    ntok = (MAX_FRAMES - P) * sb.PROMPT_TOKENS // P
    while sb.predicted(P, ntok) > MAX_FRAMES:
        ntok -= 1
    running = [([int(t) for t in rng.integers(10, 90, ntok)], [int(t) for t in rng.integers(10, 90, sb.PROMPT_TOKENS)],
                (0.05 * rng.standard_normal(sb.PROMPT_SAMPLES)).astype(np.float32)) for _ in range(SLOTS - EDITS)]
    edits = make_edits(6)
    store = VoiceStore(fx, SLOTS * 300 + EDITS * 940)
    vr = store.register_batch([(r[2], r[1]) for r in running])
    recs = store.register_recording_batch([e[1] for e in edits])
    sync()
    say(f"(a) host stall: {SLOTS} slots x {MAX_FRAMES} frames, {SLOTS - EDITS} generation rows in flight, ticks queued and not "
        f"synchronised, then {EDITS} edits of {recs[0].frames}-frame recordings ({SPAN[2]} frames regenerated each, 16 steps)")

    def arm(service, ticks):
        cb = ContinuousBatcher(m, voc, fx, max_rows=SLOTS, max_frames=MAX_FRAMES, voices=store)
        for i, r in enumerate(running):
            cb.submit(r[0], voice=vr[i], seed=i, num_step=64, guidance_scale=1.0, t_shift=0.5)
        cb.step()
        sync()
        for _ in range(ticks):
            cb.step()                                   # (nothing to retire or admit: ticks, queued)
        t = time.perf_counter()
        if service:
            for i, (e, r) in enumerate(zip(edits, recs)):
                cb.submit_edit(e[0], r, e[2], num_step=16, seed=100 + i)
            cb.step()
        else:
            edit_batch(edits, m, voc, fx, num_step=16, seeds=[100 + i for i in range(EDITS)])
        host = (time.perf_counter() - t) * 1e3
        sync()
        wall = (time.perf_counter() - t) * 1e3
        assert cb.pending() == (0, SLOTS if service else SLOTS - EDITS)
        cb.close()
        return host, wall

    for ticks in (8, 4):
        arm(False, ticks), arm(True, ticks)
        res = {"wav": [], "service": []}
        for _ in range(ROUNDS):
            res["wav"].append(arm(False, ticks))
            res["service"].append(arm(True, ticks))
        for name, rows in res.items():
            report(f"{ticks} ticks queued  {name}", rows, ("host in call", "host to sync"))
    say("  (wav: edit_batch returns 8 finished waveforms; service: step() returns with the 8 rows admitted and one tick queued,"
        " their waveforms come 16 ticks later while the other rows keep running)")


def front(m, fx):
    edits = make_edits(7)
    eng, dev = m.engine, m.device
    store = VoiceStore(fx, EDITS * 940)
    sync()
    t = time.perf_counter()
    recs = store.register_recording_batch([e[1] for e in edits])
    sync()
    say(f"(b) front of one admission: {EDITS} edits of 10 s recordings at 24 kHz ({recs[0].frames} frames each) into {EDITS} "
        f"slots of {MAX_FRAMES}; register_recording_batch of the {EDITS} once: {(time.perf_counter() - t) * 1e3:.2f} ms "
        f"(first call, unwarmed)")
    spans = [e[2] for e in edits]
    T = recs[0].frames - (SPAN[1] - SPAN[0]) + SPAN[2]
    rng = np.random.default_rng(8)
    x0 = torch.from_numpy(rng.standard_normal((EDITS, T, 100)).astype(np.float32)).to(dev)
    tc = torch.from_numpy(rng.standard_normal((EDITS, T, 100)).astype(np.float32)).to(dev)
    sched = [RowSchedule(16, 1.0, t_shift=0.5)] * EDITS
    slots = list(range(EDITS))
    state = {}

    def wav():
        ws = [w.cpu() for w in _prompts_at_rate([e[1] for e in edits], [None] * EDITS, fx.config.sampling_rate, dev)]
        Ns = [len(w) for w in ws]
        norm = torch.zeros((EDITS, max(Ns)), dtype=torch.float32)
        for r, w in enumerate(ws):
            norm[r, :Ns[r]] = _prompt_rms_normalise(w, 0.1)[0]
        feats, nfr = fx.extract_batch(norm.to(dev), torch.tensor(Ns))
        features = (feats + 0.0) * 0.1
        plan = plan_edit_batch([int(v) for v in nfr.tolist()], spans)
        sc, _ = eng.edit_gather(features, plan.lens, plan.table, plan.row_ptr, T)
        state["sess"].admit(slots, x0, tc, sc, plan.new_lens.tolist(), sched)

    def service():
        plan = plan_edit_batch([r.frames for r in recs], spans)
        state["sess"].admit_edit(slots, x0, tc, store.arena, [r.offset for r in recs], plan.lens, plan.table,
                                 plan.row_ptr, sched)

    def run(fn):
        state["sess"] = eng.open_session(EDITS, MAX_FRAMES)
        try:
            return timed(fn)
        finally:
            state["sess"].close()

    arms = {"wav": wav, "service": service}
    for fn in arms.values():
        run(fn)
    ms = {name: [] for name in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            ms[name].append(run(fn))
    for name, rows in ms.items():
        report(name, rows, ("host in call", "device events", "host to sync"))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        os.path.dirname(HERE), "profiles", "edit_service_ab.txt")
    from zipvoice_amd.config import default_config
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.models import build_model
    from zipvoice_amd.vocoder import Vocos
    from zipvoice_amd.weights import synthetic_state_dict
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="bf16")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m = m.to("cuda:0")
    voc, fx = Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()
    say(f"edit_service_bench: {torch.cuda.get_device_name(0)}, zipvoice bf16, rounds {ROUNDS}, arms alternated")
    front(m, fx)
    stall(m, voc, fx)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
