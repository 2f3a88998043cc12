#!/usr/bin/env python3
"""What the row padding mode costs, and whether it makes a session row bitwise independent of its company
(DESIGN.md §3 "Padding").  Writes profiles/padrow_ab.txt.

Cost: synthetic default-size ZipVoice (the C2 model), bf16, one 16-step solve (engine.euler_sample,
guidance 1, t_shift 0.5) at
  C2      32 rows of 1219 frames, nothing masked (the mask is given, every length is 1219), and
  ragged  32 rows of about 430 .. 1219 frames padded to 1219 (tools/session_bench.py's lengths),
in "batch" and in "row" mode: after one warm-up solve of each arm, ROUNDS rounds alternating the two modes in
one process (the arm that goes first alternates too), host clock around a device synchronise.  Reported: every time, each arm's median and spread,
and row - batch.  Row mode adds one length kernel per decoder call and swaps the three downsample launches
for their row-clamped form; the expectation is a difference inside the batch arm's own spread.

Bitwise: fp32 and bf16, row mode.  A row of 50 frames runs 3 steps (a) alone in a 1-slot session and (b) in
slot 1 of a 3-slot session beside rows of 71 and 62 frames that outlive it; reported is whether its valid
frames are the same bits, and the largest difference if not.  The model's dependence on the company is
gone in row mode; what is left is whether a launch policy follows the batch's rows (N) or length (T_k).
Informational: no threshold is set on these figures.

usage: padrow_ab.py [ROUNDS [ROWS [FRAMES [STEPS]]]]   (default 4 32 1219 16)
       padrow_ab.py trace     the ragged shape's arms alone at 2 rounds of 2 steps, nothing written: run it under
                              rocprofv3 --kernel-trace --stats to compare zv_downsample_kernel (batch arm)
                              with zv_downsample_row_kernel + zv_row_len_kernel (row arm) per launch"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from zipvoice_amd.config import default_config  # noqa: E402
from zipvoice_amd.models import build_model  # noqa: E402
from zipvoice_amd.solver import RowSchedule  # noqa: E402
from zipvoice_amd.weights import synthetic_state_dict  # noqa: E402

assert torch.cuda.is_available(), "padrow_ab.py needs a GPU"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "padrow_ab.txt")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def model(precision):
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision=precision)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    return m.to("cuda:0")


def batch(lens, T, seed):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    pm = torch.arange(T, device=dev)[None] >= torch.tensor(lens, device=dev)[:, None]
    mk = lambda s, o: (s * torch.randn(len(lens), T, 100, device=dev, generator=g) + o).contiguous()
    return mk(1.0, 0.0), mk(1.0, 0.0), mk(0.3, -0.5), pm


def cost(eng, rounds, rows, T, steps, only=None):
    rng = np.random.default_rng(1)
    ragged = sorted((int(v) for v in rng.integers(T // 3, T + 1, rows)), reverse=True)
    ragged[0] = T
    for name, lens in (("C2", [T] * rows), ("ragged", ragged)):
        if only and name != only:
            continue
        x, tc, sc, pm = batch(lens, T, seed=2)
        solve = lambda: eng.euler_sample(x, tc, sc, pm, steps, 1.0, t_shift=0.5)
        ms = {"batch": [], "row": []}
        for mode in ms:                                   # warm-up of each arm
            eng.padding = mode
            solve()
            torch.cuda.synchronize()
        for r in range(rounds):
            for mode in (list(ms) if r % 2 == 0 else list(ms)[::-1]):   # (each arm goes first in every other round)
                eng.padding = mode
                torch.cuda.synchronize()
                t = time.perf_counter()
                solve()
                torch.cuda.synchronize()
                ms[mode].append((time.perf_counter() - t) * 1e3)
        eng.padding = "batch"
        say(f"{name}: {rows} rows of {min(lens)} .. {max(lens)} frames padded to {T}, {steps} steps, guidance 1")
        for mode, v in ms.items():
            say(f"  {mode:6s} " + " ".join(f"{t:9.2f}" for t in v) + f" ms   median {statistics.median(v):9.2f}  "
                f"spread {max(v) - min(v):6.2f}")
        d = statistics.median(ms["row"]) - statistics.median(ms["batch"])
        say(f"  row - batch: {d:+.2f} ms per solve, {d / steps:+.3f} ms per step "
            f"({100 * d / statistics.median(ms['batch']):+.2f} %)")


def bitwise(precision):
    eng = model(precision).engine
    eng.padding = "row"
    rows = {n: batch([n], n, seed=10 + n)[:3] for n in (71, 50, 62)}
    sched = {71: RowSchedule(4, 1.0, t_shift=0.5), 50: RowSchedule(3, 1.0, t_shift=0.5), 62: RowSchedule(4, 0.7, t_shift=0.5)}

    def run(slots, order, want):
        sess = eng.open_session(slots, 97)
        for slot, n in order:
            sess.admit([slot], *rows[n], [n], [sched[n]])
        while max(sess.steps_left()) > 0:
            sess.step()
        out = sess.retire([s for s, _ in order])
        sess.close()
        return out[[n for _, n in order].index(want), :want]

    alone = run(1, [(0, 50)], 50)
    beside = run(3, [(0, 71), (1, 50), (2, 62)], 50)
    torch.cuda.synchronize()
    same = torch.equal(alone, beside)
    say(f"bitwise, {precision}, row mode: a 50-frame row alone in a 1-slot session vs in a 3-slot session beside rows of 71 and "
        f"62 frames: {'the same bits' if same else 'different bits'}, max |diff| {(alone - beside).abs().max().item():.3e}")


def main():
    if sys.argv[1:] == ["trace"]:
        cost(model("bf16").engine, 2, 32, 1219, 2, only="ragged")
        return
    a = [int(v) for v in sys.argv[1:]]
    rounds, rows, T, steps = (a + [4, 32, 1219, 16][len(a):])[:4]
    say(f"padrow_ab: {torch.cuda.get_device_name(0)}, zipvoice bf16")
    cost(model("bf16").engine, rounds, rows, T, steps)
    for precision in ("fp32", "bf16"):
        bitwise(precision)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
