#!/usr/bin/env python3
"""The time of one seeded-noise draw (zv_noise_normal, zipvoice_amd/csrc/zv_noise.inc)
at the C2 shape, 32 x 1219 x 100 fp32 (15.6 MB written), next to torch.randn of the same shape in
the same process.  Device events around 200 calls after 10 warm-up calls, median of 5 windows;
the two arms alternate over ROUNDS rounds, so the distance between an arm's own figures is the
spread the other arm is read against.  Informational: the draw runs once per sample(), outside
the Euler loop.

usage: noise_time.py [B T F]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from zipvoice_amd import engine  # noqa: E402

assert torch.cuda.is_available(), "noise_time.py needs a GPU"
ROUNDS = 3


def events(fn, calls=200, windows=5, warmup=10):
    """Median over `windows` of the mean device time (us) of `calls` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / calls)
    return statistics.median(us), min(us), max(us)


def main():
    B, T, F = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (32, 1219, 100)
    lib = engine.load_library()
    dev = torch.device("cuda:0")
    seeds = torch.arange(1000, 1000 + B, dtype=torch.int64, device=dev)
    out = torch.empty((B, T, F), dtype=torch.float32, device=dev)
    n = T * F
    args = (engine._ptr(seeds), None, B, n, n, engine._ptr(out), engine._stream())

    def seeded():
        assert lib.zv_noise_normal(*args) == 0

    def randn():
        torch.randn((B, T, F), device=dev, out=out)

    mb = 4e-6 * B * n
    print(f"shape {B} x {T} x {F}: {mb:.1f} MB written per call")
    for r in range(ROUNDS):
        for name, fn in (("zv_noise_normal", seeded), ("torch.randn", randn)):
            med, lo, hi = events(fn)
            print(f"round {r} {name:16s} {med:8.2f} us (min {lo:.2f} max {hi:.2f})  "
                  f"{mb / med:.2f} TB/s written")
    seeded()
    torch.cuda.synchronize()
    print(f"mean {float(out.mean()):+.3e} var {float(out.var()):.5f}")


if __name__ == "__main__":
    main()
