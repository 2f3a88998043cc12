#!/usr/bin/env python3
"""The time of one scheduled solve of a mixed pool (zv_euler_sample_sched) next to the same
pool run as today's only single-batch alternative: every row at the pool's largest num_step with the
per-row guidance tensor (zv_euler_sample_rows, all rows doubled).  Synthetic default-size ZipVoice, bf16,
B x T x 100 inputs.  Device events around SOLVES solves after WARM warm-up solves per window; the two arms
alternate over ROUNDS rounds, so an arm's own spread is what the other arm is read against.
Informational: no threshold is set on these figures.  The padded length T is the batch's for every step
of both arms.

usage: sched_time.py [T [REPS]]   (the pool is REPS copies of the 8-row pattern below; default 600 1)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from zipvoice_amd.config import default_config  # noqa: E402
from zipvoice_amd.models import build_model  # noqa: E402
from zipvoice_amd.solver import RowSchedule  # noqa: E402
from zipvoice_amd.weights import synthetic_state_dict  # noqa: E402

assert torch.cuda.is_available(), "sched_time.py needs a GPU"
ROUNDS, SOLVES, WARM = 3, 3, 2
STEPS = [4, 32, 16, 8, 4, 32, 16, 8]
SCALES = [1.0, 1.0, 0.0, 2.5, 0.0, 1.0, 1.0, 0.0]


def window(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(SOLVES):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / SOLVES


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    STEPS[:], SCALES[:] = STEPS * reps, SCALES * reps
    B = len(STEPS)
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="bf16")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    eng = m.to("cuda:0").engine
    rng = np.random.default_rng(0)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(rng.standard_normal((B, T, 100), dtype=np.float32)).to(dev)
    tc = torch.from_numpy(rng.standard_normal((B, T, 100), dtype=np.float32)).to(dev)
    sc = torch.from_numpy((0.3 * rng.standard_normal((B, T, 100)) - 0.5).astype(np.float32)).to(dev)
    lens = torch.tensor([T - 37 * (b % 4) for b in range(B)], device=dev)
    pm = torch.arange(T, device=dev)[None] >= lens[:, None]
    sched = [RowSchedule(n, g, t_shift=0.5) for n, g in zip(STEPS, SCALES)]
    gt = torch.tensor(SCALES, device=dev).reshape(B, 1, 1)
    K = max(STEPS)

    def mixed():
        eng.euler_sample_sched(x, tc, sc, pm, sched)

    def uniform():
        eng.euler_sample(x, tc, sc, pm, K, gt, t_shift=0.5)

    mixed()
    rows, steps = eng.sched_stats()
    print(f"pool B={B} T={T} bf16: {reps} x (num_step {STEPS[:8]}, guidance {SCALES[:8]})")
    print(f"decoder rows per solve: scheduled {rows} over {steps} steps; uniform at {K} steps, all rows doubled {2 * B * K}")
    ms = {"scheduled": [], "uniform": []}
    for r in range(ROUNDS):
        for name, fn in (("scheduled", mixed), ("uniform", uniform)):
            ms[name].append(window(fn))
            print(f"round {r} {name:10s} {ms[name][-1]:9.2f} ms per solve")
    a, b = statistics.median(ms["scheduled"]), statistics.median(ms["uniform"])
    print(f"median: scheduled {a:.2f} ms, uniform {b:.2f} ms, ratio {a / b:.3f} (rows ratio {rows / (2 * B * K):.3f})")


if __name__ == "__main__":
    main()
