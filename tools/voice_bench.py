#!/usr/bin/env python3
"""The prompt front with registered voices (zipvoice_amd/voices.py) against the wav path.
Writes profiles/voice_front_ab.txt (or --out PATH).

Model: synthetic default-size ZipVoice (the C2 model), bf16, synthetic Vocos, VocosFbank.  Every
measurement alternates its two arms over ROUNDS rounds after a warm-up of each, with a device
synchronise between arms.  Informational: no threshold is set on these figures.

(a) Prompt front of one admission: 8 requests with 3 s prompts at 44.1 kHz, from the first host call to
    the end of the producer of the speech condition at T = 1219.  wav: infer._prepare_prompts (resample,
    RMS, pad, upload, fbank), scale and bias, engine.speech_condition.  voice: VoiceStore.gather on the
    registered prompts.  Per arm the host clock inside the call (the device not waited for), the device
    time between two events around it, and the host clock to a synchronise after it.
(b) Host stall: a 32-slot x 1219-frame ContinuousBatcher with 24 rows in flight and 8 ticks queued and not
    synchronised; 8 requests are submitted and the host clock is taken inside the next step() (retire
    nothing, admit 8, tick).  wav requests against voice requests.  The same with 4 ticks queued, to tell
    what the admission waits for from what a host that runs further ahead of the device pays elsewhere (the
    session's table staging allocates a pinned slot per upload in flight beyond those it holds).
(c) The arrival trace of tools/session_bench.py (profiles/session_ab.txt) through ContinuousBatcher with wav
    requests and with voices registered beforehand, in one process on one machine.

usage: voice_bench.py [--out PATH]"""
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
from zipvoice_amd.infer import _prepare_prompts  # noqa: E402
from zipvoice_amd.serving import ContinuousBatcher  # noqa: E402
from zipvoice_amd.voices import VoiceStore  # noqa: E402

ROUNDS, SLOTS, MAX_FRAMES = 3, 32, 1219
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def sync():
    torch.cuda.synchronize()


def timed(fn):
    """(host ms inside fn, device ms between events around it, host ms to a synchronise after it)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    t = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    host = (time.perf_counter() - t) * 1e3
    sync()
    return host, e0.elapsed_time(e1), (time.perf_counter() - t) * 1e3


def table(arms):
    """arms: {name: fn}; alternated ROUNDS times after one warm-up each."""
    for fn in arms.values():
        fn()
    sync()
    ms = {name: [] for name in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            ms[name].append(timed(fn))
    for name, rows in ms.items():
        for k, what in enumerate(("host in call", "device events", "host to sync")):
            v = [r[k] for r in rows]
            say(f"  {name:6s} {what:14s} " + " ".join(f"{x:9.3f}" for x in v) + f" ms   median {statistics.median(v):9.3f}")
    return ms


def front(m, fx):
    rng = np.random.default_rng(4)
    n = 3 * 44100
    items = [([10] * 20, [int(t) for t in rng.integers(10, 90, 30)], (0.05 * rng.standard_normal(n)).astype(np.float32), 44100)
             for _ in range(8)]
    store = VoiceStore(fx, 8 * 300)
    sync()
    t = time.perf_counter()
    voices = store.register_batch([(it[2], it[1], it[3]) for it in items])
    sync()
    say(f"(a) prompt front of one admission: 8 prompts of 3 s at 44.1 kHz ({voices[0].frames} frames each), T = {MAX_FRAMES}; "
        f"register_batch of the 8 once: {(time.perf_counter() - t) * 1e3:.2f} ms (first call, unwarmed)")
    dev = m.device

    def wav():
        feats, nfr, _, _ = _prepare_prompts(items, fx, 0.1, 0.1, 0.0, dev)
        return m.engine.speech_condition(feats, nfr, MAX_FRAMES)

    def voice():
        return store.gather(voices, MAX_FRAMES)[0]

    a, b = wav(), voice()
    fr = voices[0].frames
    say(f"  speech conditions of the two arms: max |diff| {(a - b).abs().max().item():.3e} (quiet prompts: the rms may "
        f"differ in its last bit), zero past frame {fr} in both: {bool((a[:, fr:] == 0).all() and (b[:, fr:] == 0).all())}")
    table({"wav": wav, "voice": voice})


def stall(m, voc, fx):
    rng = np.random.default_rng(5)
    P = (sb.PROMPT_SAMPLES + 128) // 256
    ntok = (MAX_FRAMES - P) * sb.PROMPT_TOKENS // P
    while sb.predicted(P, ntok) > MAX_FRAMES:
        ntok -= 1
    mk = lambda: ([int(t) for t in rng.integers(10, 90, ntok)], [int(t) for t in rng.integers(10, 90, sb.PROMPT_TOKENS)],
                  (0.05 * rng.standard_normal(sb.PROMPT_SAMPLES)).astype(np.float32))
    running, late = [mk() for _ in range(SLOTS - 8)], [mk() for _ in range(8)]
    store = VoiceStore(fx, SLOTS * 300)
    vr = store.register_batch([(r[2], r[1]) for r in running])
    vl = store.register_batch([(r[2], r[1]) for r in late])
    sync()
    say(f"(b) host stall: {SLOTS} slots x {MAX_FRAMES} frames, {SLOTS - 8} rows of {sb.predicted(P, ntok)} frames in flight, "
        f"ticks queued and not synchronised, then 8 requests submitted: host clock inside the next step()")

    def arm(by_voice, ticks):
        cb = ContinuousBatcher(m, voc, fx, max_rows=SLOTS, max_frames=MAX_FRAMES, voices=store)
        kw = dict(num_step=64, guidance_scale=1.0, t_shift=0.5)
        for i, r in enumerate(running):
            cb.submit(r[0], voice=vr[i], seed=i, **kw) if by_voice else cb.submit(*r, seed=i, **kw)
        cb.step()
        sync()
        for _ in range(ticks):
            cb.step()                                   # (nothing to retire or admit: ticks, queued)
        for i, r in enumerate(late):
            cb.submit(r[0], voice=vl[i], seed=100 + i, **kw) if by_voice else cb.submit(*r, seed=100 + i, **kw)
        t = time.perf_counter()
        cb.step()
        host = (time.perf_counter() - t) * 1e3
        sync()
        wall = (time.perf_counter() - t) * 1e3
        assert cb.pending() == (0, SLOTS)
        cb.close()
        return host, wall

    for ticks in (8, 4):
        arm(False, ticks), arm(True, ticks)
        res = {"wav": [], "voice": []}
        for _ in range(ROUNDS):
            res["wav"].append(arm(False, ticks))
            res["voice"].append(arm(True, ticks))
        for name, rows in res.items():
            for k, what in enumerate(("host in step()", "host to sync")):
                v = [r[k] for r in rows]
                say(f"  {ticks} ticks queued  {name:6s} {what:14s} " + " ".join(f"{x:9.3f}" for x in v)
                    + f" ms   median {statistics.median(v):9.3f}")


def arm_trace_voices(m, voc, fx, store, voices, reqs, gap):
    """session_bench.arm_continuous with the requests' prompts registered beforehand."""
    cb = ContinuousBatcher(m, voc, fx, max_rows=SLOTS, max_frames=MAX_FRAMES, voices=store)
    arrive = [i * gap for i in range(len(reqs))]
    ticket, lat, nxt = {}, {}, 0
    sync()
    t0 = time.perf_counter()
    while len(lat) < len(reqs):
        now = time.perf_counter() - t0
        while nxt < len(reqs) and arrive[nxt] <= now:
            ticket[cb.submit(reqs[nxt][0], voice=voices[nxt], num_step=sb.NUM_STEP, guidance_scale=sb.GUIDANCE,
                             t_shift=sb.T_SHIFT, seed=nxt)] = nxt
            nxt += 1
        if not sum(cb.pending()):
            time.sleep(max(arrive[nxt] - (time.perf_counter() - t0), 0.0))
            continue
        done = cb.step()
        sync()
        now = time.perf_counter() - t0
        for tk, _ in done:
            lat[ticket[tk]] = now - arrive[ticket[tk]]
    total = time.perf_counter() - t0
    work = cb.session.stats()[2]
    cb.close()
    return lat, total, work


def trace(m, voc, fx):
    full = [([10] * ((MAX_FRAMES - 281) * sb.PROMPT_TOKENS // 281), [11] * sb.PROMPT_TOKENS,
             np.full(sb.PROMPT_SAMPLES, 0.05, np.float32))] * SLOTS
    cb = ContinuousBatcher(m, voc, fx, max_rows=SLOTS, max_frames=MAX_FRAMES)
    for r in full:
        cb.submit(*r, num_step=3, guidance_scale=sb.GUIDANCE, t_shift=sb.T_SHIFT, seed=0)
    cb.step()
    sync()
    t = time.perf_counter()
    cb.step()
    sync()
    step_time = time.perf_counter() - t
    cb.drain()
    cb.close()
    gap = step_time / 2
    reqs, warm = sb.make_requests(64, MAX_FRAMES, seed=2), sb.make_requests(8, MAX_FRAMES, seed=3)
    store = VoiceStore(fx, (len(reqs) + len(warm)) * 281)
    vw = store.register_batch([(r[2], r[1]) for r in warm])
    vs = store.register_batch([(r[2], r[1]) for r in reqs])
    frames = [sb.predicted(281, len(r[0])) for r in reqs]
    say(f"(c) arrival trace of session_bench.py: step-time {step_time * 1e3:.1f} ms, one arrival every {gap * 1e3:.1f} ms, "
        f"64 requests of {min(frames)} .. {max(frames)} frames (mean {statistics.mean(frames):.0f}), 16 steps; "
        f"{len(vs)} voices of 281 frames registered beforehand")
    sb.arm_continuous(m, voc, fx, warm, gap, SLOTS, MAX_FRAMES)
    arm_trace_voices(m, voc, fx, store, vw, warm, gap)
    for r in range(2):
        for name, run in (("ContinuousBatcher, wav", lambda: sb.arm_continuous(m, voc, fx, reqs, gap, SLOTS, MAX_FRAMES)),
                          ("ContinuousBatcher, voices", lambda: arm_trace_voices(m, voc, fx, store, vs, reqs, gap))):
            lat, total, work = run()
            v = sorted(lat.values())
            p95 = v[min(len(v) - 1, int(np.ceil(0.95 * len(v))) - 1)]
            say(f"  round {r} {name:26s} arrival -> waveform mean {statistics.mean(v):7.3f} s  p95 {p95:7.3f} s  max {v[-1]:7.3f} s   "
                f"trace done in {total:7.3f} s   decoder rows x frames {work}")
    say("  recorded in profiles/session_ab.txt for the wav form (another session, possibly another machine: not comparable "
        "with the lines above): mean 0.317 s, p95 0.385 s, done in 0.934 s")


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        os.path.dirname(HERE), "profiles", "voice_front_ab.txt")
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
    say(f"voice_bench: {torch.cuda.get_device_name(0)}, zipvoice bf16, rounds {ROUNDS}, arms alternated")
    front(m, fx)
    stall(m, voc, fx)
    trace(m, voc, fx)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
