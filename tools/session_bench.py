#!/usr/bin/env python3
"""Continuous batching against batch-at-a-time serving on one arrival trace, and the
per-tick cost of a solve session against the scheduled solve.  Writes profiles/session_ab.txt.

Model: synthetic default-size ZipVoice (the C2 model), bf16, synthetic Vocos.  SLOTS = 32 slots of
MAX_FRAMES = 1219 frames, 16 steps, guidance 1.

Trace: REQUESTS requests with total lengths (prompt + generated frames) drawn from a seeded uniform
range, one arriving every half step-time, where the step-time is one measured tick of the full session
(32 rows at 1219 frames).  Both arms see the same requests at the same offsets on the host clock and
synchronise the device after every step / batch, so a finishing time is a time the waveform exists.
  (a) serving.ContinuousBatcher: every step() retires, admits what has arrived, ticks.
  (b) the way before sessions: infer.generate_batch on whatever has arrived (at most SLOTS requests) when
      the previous batch ends; every row runs padded to the batch's longest.
Reported per arm: mean and p95 of arrival -> waveform, the time to finish the trace, and the decoder's
rows x frames (session stats for (a); 2 rows x 16 steps x B x T_max per batch for (b)).

Per-tick overhead: the same 32 rows admitted at once, ticked STEPS_OV times and retired, against
engine.euler_sample_sched on the same inputs (the decoder batches are the same); ROUNDS alternating
rounds after a warm-up of each, host clock around a device synchronise; the medians, each arm's own
spread and the difference per tick.
Informational: no threshold is set on these figures.

usage: session_bench.py [REQUESTS [SLOTS [MAX_FRAMES]]]   (default 64 32 1219)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from zipvoice_amd.config import default_config  # noqa: E402
from zipvoice_amd.feature import VocosFbank  # noqa: E402
from zipvoice_amd.infer import generate_batch  # noqa: E402
from zipvoice_amd.models import build_model  # noqa: E402
from zipvoice_amd.serving import ContinuousBatcher  # noqa: E402
from zipvoice_amd.solver import RowSchedule  # noqa: E402
from zipvoice_amd.vocoder import Vocos  # noqa: E402
from zipvoice_amd.weights import synthetic_state_dict  # noqa: E402

assert torch.cuda.is_available(), "session_bench.py needs a GPU"
NUM_STEP, GUIDANCE, T_SHIFT = 16, 1.0, 0.5
PROMPT_SAMPLES, PROMPT_TOKENS = 72000, 30          # 3 s at 24 kHz: 281 prompt frames
ROUNDS, STEPS_OV = 3, 4
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "session_ab.txt")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def predicted(P, ntok):
    """The total frames of a request of ntok text tokens on the trace's prompt (speed 1)."""
    from zipvoice_amd.common import predict_features_lens
    return int(predict_features_lens(torch.tensor([P]), torch.tensor([PROMPT_TOKENS]), torch.tensor([ntok]), 1.0)[0])


def make_requests(n, max_frames, seed):
    """n requests whose predicted total lengths are spread over about [max_frames / 3, max_frames]."""
    rng = np.random.default_rng(seed)
    P = (PROMPT_SAMPLES + 128) // 256
    reqs = []
    for _ in range(n):
        want = int(rng.integers(max(max_frames // 3, P + 20), max_frames + 1))
        ntok = max(1, (want - P) * PROMPT_TOKENS // P)            # P + ceil(P / 30 * ntok) <= want
        while ntok > 1 and predicted(P, ntok) > max_frames:       # (the float32 quotient may round up)
            ntok -= 1
        toks = [int(t) for t in rng.integers(10, 90, ntok)]
        ptoks = [int(t) for t in rng.integers(10, 90, PROMPT_TOKENS)]
        wav = (0.1 * rng.standard_normal(PROMPT_SAMPLES)).astype(np.float32)
        reqs.append((toks, ptoks, wav))
    return reqs


def sync():
    torch.cuda.synchronize()


def arm_continuous(m, voc, fx, reqs, gap, slots, max_frames):
    cb = ContinuousBatcher(m, voc, fx, max_rows=slots, max_frames=max_frames)
    arrive = [i * gap for i in range(len(reqs))]
    ticket, lat, nxt = {}, {}, 0
    sync()
    t0 = time.perf_counter()
    while len(lat) < len(reqs):
        now = time.perf_counter() - t0
        while nxt < len(reqs) and arrive[nxt] <= now:
            ticket[cb.submit(*reqs[nxt], num_step=NUM_STEP, guidance_scale=GUIDANCE, t_shift=T_SHIFT, seed=nxt)] = nxt
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


def arm_batches(m, voc, fx, reqs, gap, slots):
    arrive = [i * gap for i in range(len(reqs))]
    lat, nxt, work = {}, 0, 0
    sync()
    t0 = time.perf_counter()
    while nxt < len(reqs):
        now = time.perf_counter() - t0
        if arrive[nxt] > now:
            time.sleep(arrive[nxt] - now)
            continue
        idx = [i for i in range(nxt, len(reqs)) if arrive[i] <= now][:slots]
        nxt = idx[-1] + 1
        generate_batch([reqs[i] for i in idx], m, voc, fx, num_step=NUM_STEP, guidance_scale=GUIDANCE, t_shift=T_SHIFT,
                       seeds=idx)
        sync()
        now = time.perf_counter() - t0
        work += 2 * NUM_STEP * len(idx) * max(predicted((PROMPT_SAMPLES + 128) // 256, len(reqs[i][0])) for i in idx)
        for i in idx:
            lat[i] = now - arrive[i]
    return lat, time.perf_counter() - t0, work


def report(name, lat, total, work):
    v = sorted(lat.values())
    p95 = v[min(len(v) - 1, int(np.ceil(0.95 * len(v))) - 1)]
    say(f"{name:28s} arrival -> waveform mean {statistics.mean(v):7.3f} s  p95 {p95:7.3f} s  max {v[-1]:7.3f} s   "
        f"trace done in {total:7.3f} s   decoder rows x frames {work}")


def overhead(eng, slots, max_frames):
    rng = np.random.default_rng(1)
    torch.manual_seed(1)
    lens = sorted((int(v) for v in rng.integers(max_frames // 3, max_frames + 1, slots)), reverse=True)
    lens[0] = max_frames
    dev = torch.device("cuda:0")
    T = max_frames
    pm = torch.arange(T, device=dev)[None] >= torch.tensor(lens, device=dev)[:, None]
    mk = lambda s, o: ((s * torch.randn(slots, T, 100, device=dev) + o) * ~pm[..., None]).contiguous()
    x, tc, sc = mk(1.0, 0.0), mk(1.0, 0.0), mk(0.3, -0.5)
    sched = [RowSchedule(STEPS_OV, GUIDANCE, t_shift=T_SHIFT)] * slots
    sess = eng.open_session(slots, max_frames)
    all_slots = list(range(slots))

    def session():
        sess.admit(all_slots, x, tc, sc, lens, sched)
        for _ in range(STEPS_OV):
            sess.step()
        return sess.retire(all_slots, T)

    def scheduled():
        return eng.euler_sample_sched(x, tc, sc, pm, sched)

    a, b = session(), scheduled()
    sync()
    same = all(torch.equal(a[i, :n], b[i, :n]) for i, n in enumerate(lens))
    ms = {"session": [], "scheduled": []}
    for r in range(ROUNDS):
        for name, fn in (("session", session), ("scheduled", scheduled)):
            sync()
            t = time.perf_counter()
            fn()
            sync()
            ms[name].append((time.perf_counter() - t) * 1e3)
    say(f"per-tick overhead: {slots} rows (lengths {min(lens)} .. {max(lens)}, padded {T}), {STEPS_OV} steps, guidance {GUIDANCE}; "
        f"results equal on valid frames: {same}")
    for name in ms:
        say(f"  {name:10s} " + " ".join(f"{v:9.2f}" for v in ms[name]) + f" ms   median {statistics.median(ms[name]):9.2f}  "
            f"spread {max(ms[name]) - min(ms[name]):6.2f}")
    d = statistics.median(ms["session"]) - statistics.median(ms["scheduled"])
    say(f"  session - scheduled: {d:+.2f} ms per solve, {d / STEPS_OV:+.3f} ms per tick "
        f"({100 * d / statistics.median(ms['scheduled']):+.2f} %)")
    sess.close()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    slots = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    max_frames = int(sys.argv[3]) if len(sys.argv) > 3 else 1219
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="bf16")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m = m.to("cuda:0")
    voc, fx = Vocos().load_synthetic(0).to("cuda:0"), VocosFbank()
    say(f"session_bench: {torch.cuda.get_device_name(0)}, zipvoice bf16, {slots} slots x {max_frames} frames, "
        f"{NUM_STEP} steps, guidance {GUIDANCE}")
    overhead(m.engine, slots, max_frames)
    # the step-time: one tick of the full session
    full = [([10] * ((max_frames - 281) * PROMPT_TOKENS // 281), [11] * PROMPT_TOKENS,
             np.full(PROMPT_SAMPLES, 0.05, np.float32))] * slots
    cb = ContinuousBatcher(m, voc, fx, max_rows=slots, max_frames=max_frames)
    for r in full:
        cb.submit(*r, num_step=3, guidance_scale=GUIDANCE, t_shift=T_SHIFT, seed=0)
    cb.step()
    sync()
    t = time.perf_counter()
    cb.step()
    sync()
    step_time = time.perf_counter() - t
    cb.drain()
    cb.close()
    gap = step_time / 2
    say(f"step-time (one tick of {slots} rows at about {max_frames} frames): {step_time * 1e3:.1f} ms; one arrival every {gap * 1e3:.1f} ms")
    reqs = make_requests(n, max_frames, seed=2)
    warm = make_requests(min(8, n), max_frames, seed=3)
    arm_continuous(m, voc, fx, warm, gap, slots, max_frames)
    arm_batches(m, voc, fx, warm, gap, slots)
    frames = [predicted(281, len(r[0])) for r in reqs]
    say(f"trace: {n} requests of {min(frames)} .. {max(frames)} frames (mean {statistics.mean(frames):.0f}) on a "
        f"{PROMPT_TOKENS}-token, 281-frame prompt")
    report("(a) ContinuousBatcher", *arm_continuous(m, voc, fx, reqs, gap, slots, max_frames))
    report("(b) generate_batch on arrival", *arm_batches(m, voc, fx, reqs, gap, slots))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
