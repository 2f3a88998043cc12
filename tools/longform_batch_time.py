#!/usr/bin/env python3
"""Two measurements of pooled long-form synthesis (zipvoice_amd/longform.py).

join   The cost of the segmented join: zv_wavjoin_apply_docs on 64 chunks x 20 s (every
       frame loud, so everything is kept: the most bytes written) as 16 documents x 4 chunks
       and as 64 documents x 1 chunk (the per-row trim), against zv_wavjoin_apply on the same
       data, on this tree's library and, with --parent-lib PATH, on an older build of the
       library in the same process.  The older build is timed twice per round (first and last
       arm), so the distance between its own two figures is the run-to-run spread the other
       arms are read against.  Device events around 20 calls after 3 warm-up calls, median of
       5 windows, three buffer sets in rotation (~740 MB, so the Infinity Cache does not serve
       the reads), as tools/longform_time.py; the arms alternate over ROUNDS rounds.  All
       layouts move the same bytes: 4 read per input sample by the energy pass, 4 read and 4
       written per kept sample.

apply  300 zv_wavjoin_apply calls on the same data and nothing else, for a kernel trace of
       its own (rocprofv3 --kernel-trace --stats -- python tools/longform_batch_time.py apply);
       ZV_LIB_PATH selects an older build of the library (zipvoice_amd/engine.py).

e2e    8 requests x 4 chunks pooled by generate_long_batch (batch_size 32: one model.sample
       call of 32 rows) against 8 sequential generate_long calls (4 rows each), num_step 16,
       full-size synthetic bf16 model and Vocos, prompts of 1 s, chunks of 16 to 24 s.  Each
       side once as warm-up, then alternated ROUNDS times in one process; host clock around a
       device synchronise, around the whole call(s), prompt preparation included.

usage: longform_batch_time.py join [--parent-lib PATH] | apply | e2e"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.longform import WavJoiner, generate_long, generate_long_batch  # noqa: E402

assert torch.cuda.is_available(), "longform_batch_time.py needs a GPU"
dev = torch.device("cuda:0")
ROUNDS = 3


def events(fn, calls=20, windows=5, warmup=3):
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


def join(parent_path, trace_only=False):
    B, SR, HOP, SETS = 64, 24000, 256, 3
    n = int(20.0 * SR) // HOP * HOP
    j = WavJoiner()
    lib = engine.load_library()
    libs = {"this": (lib, j._handle(dev))}
    if parent_path:
        old = engine.load_library(os.path.abspath(parent_path))
        h = old.zv_wavjoin_create(j.frame, j.thr, j.keep_edge, j.max_gap, j.fade)
        assert h, old.zv_last_error().decode()
        libs["parent"] = (old, h)
        print(f"parent: {old.zv_version().decode()}\nthis:   {lib.zv_version().decode()}")
    xs = []
    for s in range(SETS):
        g = torch.Generator(device=dev).manual_seed(s)
        xs.append(0.1 * torch.randn((B, n), device=dev, generator=g))
    outs = [torch.empty(B * n, device=dev) for _ in range(SETS)]
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    out_len = torch.zeros(B, dtype=torch.int64, device=dev)
    ptrs = {D: torch.arange(0, B + 1, B // D, dtype=torch.int32, device=dev) for D in (16, 64)}

    def apply(which):
        lb, h = libs[which]

        def fn(i):
            k = i % SETS
            assert lb.zv_wavjoin_apply(h, engine._ptr(xs[k]), n, engine._ptr(lens), None, B, 1,
                                       engine._ptr(outs[k]), B * n, B * n, engine._ptr(out_len),
                                       None, engine._stream()) == 0
        return fn

    def docs(D):
        cap = B // D * n

        def fn(i):
            k = i % SETS
            assert lib.zv_wavjoin_apply_docs(libs["this"][1], engine._ptr(xs[k]), n,
                                             engine._ptr(lens), None, B, 1, engine._ptr(ptrs[D]), D,
                                             engine._ptr(outs[k]), cap, cap, engine._ptr(out_len),
                                             None, engine._stream()) == 0
        return fn

    if trace_only:
        print(lib.zv_version().decode())
        fn = apply("this")
        for i in range(300):
            fn(i)
        torch.cuda.synchronize()
        return
    arms = [("apply, this tree", apply("this")), ("docs 16 x 4, this tree", docs(16)),
            ("docs 64 x 1 (trim), this tree", docs(64))]
    if parent_path:
        arms = [("apply, parent (first)", apply("parent"))] + arms + [
            ("apply, parent (last)", apply("parent"))]
    res = {name: [] for name, _ in arms}
    for r in range(ROUNDS):
        for name, fn in arms:
            med, lo, hi = events(fn)
            res[name].append(med)
            print(f"round {r} {name}: {med:.4f} ms (min {lo:.4f}, max {hi:.4f})", flush=True)
    moved = 12 * B * n
    for name, _ in arms:
        med = statistics.median(res[name])
        print(f"join [{name}] {B} x 20 s: median of {ROUNDS} rounds {med:.4f} ms "
              f"(rounds {min(res[name]):.4f} .. {max(res[name]):.4f}); {moved / 1e6:.0f} MB = "
              f"{moved / med / 1e6:.0f} GB/s")
    for D in (16, 64):                                    # the timed calls kept everything
        docs(D)(0)
        torch.cuda.synchronize()
        want = B // D * n - (B // D - 1) * j.fade
        assert out_len[:D].tolist() == [want] * D, out_len[:D].tolist()


def e2e():
    from zipvoice_amd.config import default_config
    from zipvoice_amd.feature import VocosFbank
    from zipvoice_amd.models import build_model
    from zipvoice_amd.vocoder import Vocos
    from zipvoice_amd.weights import synthetic_state_dict
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="bf16")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m = m.to(dev)
    voc = Vocos().load_synthetic(0).to(dev)
    fx = VocosFbank()
    BREAK = (3,)
    rng = np.random.default_rng(0)
    reqs = []
    for r in range(8):
        text = []
        for size in (288 - 8 * r, 250 - 5 * r, 220, 190 + 6 * r):   # budget 288: four chunks
            text += [int(t) for t in rng.integers(10, 90, size - 1)] + [BREAK[0]]
        pw = ((0.04 + 0.02 * r) * rng.standard_normal(24000)).astype(np.float32)
        reqs.append((text, [int(t) for t in rng.integers(10, 90, 12)], pw))
    joiner = WavJoiner()
    kw = dict(max_seconds=25.0, batch_size=32, joiner=joiner, num_step=16)

    def pooled():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs, met = generate_long_batch(reqs, m, voc, fx, BREAK, **kw)
        torch.cuda.synchronize()
        assert met["num_chunks"] == 32 and met["num_batches"] == 1
        return time.perf_counter() - t0, met["t"], met["wav_seconds"]

    def sequential():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inner = secs = 0.0
        for text, pt, pw in reqs:
            _, met = generate_long(text, pt, pw, m, voc, fx, BREAK, **kw)
            assert met["num_chunks"] == 4 and met["num_batches"] == 1
            inner += met["t"]
            secs += met["wav_seconds"]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, inner, secs

    res = {"pooled": [], "sequential": []}
    for r in range(-1, ROUNDS):                           # round -1 is the warm-up
        for name, fn in (("pooled", pooled), ("sequential", sequential)):
            wall, inner, secs = fn()
            print(f"round {r} {name}: {wall * 1e3:.1f} ms (sample + decode + join "
                  f"{inner * 1e3:.1f} ms), {secs:.1f} s of audio, rtf {wall / secs:.5f}",
                  flush=True)
            if r >= 0:
                res[name].append(wall)
    p, s = (statistics.median(res[k]) for k in ("pooled", "sequential"))
    print(f"e2e 8 requests x 4 chunks, num_step 16: pooled {p * 1e3:.1f} ms, sequential "
          f"{s * 1e3:.1f} ms (medians of {ROUNDS}), pooled / sequential = {p / s:.3f}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "join":
        join(sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "apply":
        join(None, trace_only=True)
    elif len(sys.argv) > 1 and sys.argv[1] == "e2e":
        e2e()
    else:
        sys.exit(__doc__)
