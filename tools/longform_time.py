#!/usr/bin/env python3
"""Time the long-form join against the vocoder decode it follows: 64 chunks of 20 s
(30.7 M samples), one zv_wavjoin_apply versus one Vocos decode_features of the same
64 x 1875 frames, both between device events after a warm-up, in one process.

Two join inputs: every frame loud (everything is kept: the most bytes written) and a
speech-like layout (0.4 s of silence at both edges, a 1.5 s pause inside: edge trim and a
cut gap).  Three buffer sets in rotation (~740 MB) keep the Infinity Cache from serving the
reads.  Bytes counted for the join: 4 per input sample read by the energy pass, 4 per kept
sample read by the gather pass, 4 per output column written (kept samples, then zeros up to
the capacity).

usage: longform_time.py [chunks=64] [seconds=20]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.longform import WavJoiner  # noqa: E402
from zipvoice_amd.vocoder import Vocos  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 20.0
HOP, SR, SETS, CALLS, WINDOWS = 256, 24000, 3, 20, 5
T = int(SECONDS * SR) // HOP
n = T * HOP
dev = torch.device("cuda:0")
assert torch.cuda.is_available(), "longform_time.py needs a GPU"


def events(fn, calls=CALLS, windows=WINDOWS, warmup=3):
    """Median over `windows` of the mean device time (ms) of `calls` calls."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return statistics.median(ms), min(ms), max(ms)


def signal(kind, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = 0.1 * torch.randn((B, n), device=dev, generator=g)
    if kind == "speech":
        env = torch.ones(n, device=dev)
        edge, mid, gap = int(0.4 * SR), n // 2, int(0.75 * SR)
        env[:edge] = 1e-3
        env[n - edge:] = 1e-3
        env[mid - gap:mid + gap] = 1e-3
        x *= env
    return x


joiner = WavJoiner()
lib = engine.load_library()
h = joiner._handle(dev)
lens = torch.full((B,), n, dtype=torch.int32, device=dev)
cap = B * n
out_len = torch.zeros(1, dtype=torch.int64, device=dev)
outs = [torch.empty((1, cap), device=dev) for _ in range(SETS)]
for kind in ("all loud", "speech"):
    xs = [signal(kind, s) for s in range(SETS)]

    def join(i):
        k = i % SETS
        assert lib.zv_wavjoin_apply(h, engine._ptr(xs[k]), n, engine._ptr(lens), None, B, 1,
                                    engine._ptr(outs[k]), cap, cap, engine._ptr(out_len), None,
                                    engine._stream()) == 0
    med, lo, hi = events(join)
    N = int(out_len.item())
    spans = joiner(xs[0], [n] * B)[1].cpu()
    kept = int(spans[:, 0].sum())
    moved = 4 * B * n + 4 * kept + 4 * cap
    print(f"join [{kind}] {B} x {SECONDS:.0f} s ({B * n / 1e6:.1f} M samples): {med:.3f} ms "
          f"(min {lo:.3f}, max {hi:.3f}); kept {kept / (B * n):.3f}, N = {N}; "
          f"{moved / 1e6:.0f} MB moved = {moved / med / 1e6:.0f} GB/s "
          f"({moved / (B * n):.1f} B per input sample)", flush=True)
    del xs

voc = Vocos().load_synthetic(0).to(dev)
rng = np.random.default_rng(0)
mels = [torch.from_numpy((0.3 * rng.standard_normal((B, T, 100)) - 0.5).astype(np.float32)).to(dev)
        for _ in range(SETS)]
flens = torch.full((B,), T, dtype=torch.int64, device=dev)
med, lo, hi = events(lambda i: voc.decode_features(mels[i % SETS], flens), calls=5)
print(f"vocos decode_features {B} x {T} frames: {med:.3f} ms (min {lo:.3f}, max {hi:.3f})",
      flush=True)
