#!/usr/bin/env python3
"""Two measurements of streaming long-form synthesis (zipvoice_amd/longform.py).
Every line printed is also appended to --out (default profiles/longform_stream.txt).

join   64 chunks x 20 s, every frame loud (30.7 M samples), joined three ways in one process:
       one zv_wavjoin_apply of the parent commit's library (--parent-lib PATH), the same call
       of this tree's library, and this tree's stateful join in 8 pushes of 8 chunks (the
       last one final, then a reset so the next call starts fresh: both inside the timed
       window).  Device events, 3 warm-up calls, median of 5 windows of 10 calls, 3 buffer
       sets in rotation (~740 MB, so the Infinity Cache does not serve the reads), as
       tools/longform_time.py; the arms alternate over ROUNDS rounds, the parent first and
       last, so its own spread is the yardstick for "unchanged".  Before timing, the 8 pieces
       are checked bitwise against the one call.
ttfa   one text of 8 chunks of 16 to 24 s with a 1 s prompt (synthetic bf16 ZipVoice, Vocos,
       num_step 16, a seed): generate_long(batch_size=32), whose `t` is when its caller gets
       the first sample, against generate_long_stream(first_batch=1, batch_size=32): the `t`
       of its first and of its last piece.  One warm-up per arm, then alternated ROUNDS times.
order  the same text with the loop's other order done by hand (group 1 queued before the wait
       for piece 0): host timestamps of every step and of the moment piece 0's event reports
       done, which show why generate_long_stream waits first.

usage: longform_stream_time.py join [--parent-lib PATH] [--out FILE] | ttfa [--out FILE]
                               | order [--out FILE]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.longform import WavJoiner, generate_long, generate_long_stream  # noqa: E402

assert torch.cuda.is_available(), "longform_stream_time.py needs a GPU"
dev = torch.device("cuda:0")
ROUNDS = 3
ARGS = sys.argv[1:]
OUT = ARGS[ARGS.index("--out") + 1] if "--out" in ARGS else os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "longform_stream.txt")


def say(line):
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def events(fn, calls=10, windows=5, warmup=3):
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


def join(parent_path):
    B, G, SR, HOP, SETS = 64, 8, 24000, 256, 3
    n = int(20.0 * SR) // HOP * HOP
    j = WavJoiner()
    lib = engine.load_library()
    h = j._handle(dev)
    libs = {"this": (lib, h)}
    if parent_path:
        old = engine.load_library(os.path.abspath(parent_path))
        ho = old.zv_wavjoin_create(j.frame, j.thr, j.keep_edge, j.max_gap, j.fade)
        assert ho, old.zv_last_error().decode()
        libs["parent"] = (old, ho)
        say(f"# parent: {old.zv_version().decode()}")
    say(f"# this:   {lib.zv_version().decode()}")
    sh = lib.zv_wavjoin_stream_create(h, 1, 1)
    assert sh, lib.zv_last_error().decode()
    xs = []
    for s in range(SETS):
        g = torch.Generator(device=dev).manual_seed(s)
        xs.append(0.1 * torch.randn((B, n), device=dev, generator=g))
    cap = G * n + j.fade                                  # one push: its chunks and a held tail
    outs = [torch.empty(B // G * cap, device=dev) for _ in range(SETS)]
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    out_len = torch.zeros(2 * (B // G), dtype=torch.int64, device=dev)
    final = (ctypes_u8(0), ctypes_u8(1))

    def apply(which):
        lb, hh = libs[which]

        def fn(i):
            k = i % SETS
            assert lb.zv_wavjoin_apply(hh, engine._ptr(xs[k]), n, engine._ptr(lens), None, B, 1,
                                       engine._ptr(outs[k]), B * n, B * n, engine._ptr(out_len),
                                       None, engine._stream()) == 0
        return fn

    def pushes(i):
        k = i % SETS
        for p in range(B // G):
            assert lib.zv_wavjoin_stream_push(
                sh, engine._ptr(xs[k][p * G:]), n, engine._ptr(lens), None, G, None,
                final[p == B // G - 1], engine._ptr(outs[k][p * cap:]), cap, cap,
                engine._ptr(out_len[2 * p:]), None, engine._stream()) == 0
        assert lib.zv_wavjoin_stream_reset(sh, 0, engine._stream()) == 0

    # the pieces are the one call, bit for bit
    pushes(0)
    torch.cuda.synchronize()
    ns = out_len.view(-1, 2)[:, 0].tolist()
    got = torch.cat([outs[0][p * cap:p * cap + ns[p]] for p in range(B // G)]).clone()
    apply("this")(0)
    torch.cuda.synchronize()
    N = int(out_len[0])
    assert sum(ns) == N == B * n - (B - 1) * j.fade, (ns, N)
    assert torch.equal(got.view(torch.int32), outs[0][:N].view(torch.int32))
    say(f"# 8 pieces of {ns} samples = the one call's {N}, bitwise")

    arms = [("apply, this tree", apply("this")), ("8 pushes of 8, this tree", pushes)]
    if parent_path:
        arms = [("apply, parent (first)", apply("parent"))] + arms + [
            ("apply, parent (last)", apply("parent"))]
    res = {name: [] for name, _ in arms}
    for r in range(ROUNDS):
        for name, fn in arms:
            med, lo, hi = events(fn)
            res[name].append(med)
            say(f"round {r} {name}: {med:.4f} ms (min {lo:.4f}, max {hi:.4f})")
    for name, _ in arms:
        say(f"join [{name}] {B} x 20 s: median of {ROUNDS} rounds {statistics.median(res[name]):.4f} "
            f"ms (rounds {min(res[name]):.4f} .. {max(res[name]):.4f})")
    one, eight = (statistics.median(res[k]) for k in ("apply, this tree", "8 pushes of 8, this tree"))
    say(f"8 pushes / one call = {eight / one:.3f} (+{eight - one:.4f} ms)")
    torch.cuda.synchronize()
    lib.zv_wavjoin_stream_destroy(sh)


def ctypes_u8(v):
    import ctypes
    return (ctypes.c_uint8 * 1)(v)


def stack_and_text():
    """The synthetic bf16 model, Vocos, and the text of 8 chunks of 16 to 24 s with its 1 s prompt."""
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
    text = []
    for size in (240, 288, 192, 264, 220, 276, 204, 250):     # budget 288 tokens = 24 s
        text += [int(t) for t in rng.integers(10, 90, size - 1)] + [BREAK[0]]
    pt = [int(t) for t in rng.integers(10, 90, 12)]
    pw = (0.05 * rng.standard_normal(24000)).astype(np.float32)
    return m, voc, fx, BREAK, text, pt, pw


def ttfa():
    m, voc, fx, BREAK, text, pt, pw = stack_and_text()
    joiner = WavJoiner()
    kw = dict(max_seconds=25.0, batch_size=32, joiner=joiner, num_step=16, seed=7)

    def whole():
        _, met = generate_long(text, pt, pw, m, voc, fx, BREAK, **kw)
        assert met["num_chunks"] == 8 and met["num_batches"] == 1
        return met["t"], met["t"], met["wav_seconds"]

    def stream():
        ts, n = [], 0
        for piece, info in generate_long_stream(text, pt, pw, m, voc, fx, BREAK, first_batch=1, **kw):
            ts.append(info["t"])
            n += piece.shape[1]
        assert len(ts) == 2 and info["num_chunks"] == 8 and info["final"]
        return ts[0], ts[-1], n / 24000

    res = {"generate_long": [], "stream": []}
    for r in range(-1, ROUNDS):                           # round -1 is the warm-up
        for name, fn in (("generate_long", whole), ("stream", stream)):
            first, last, secs = fn()
            say(f"round {r} {name}: first audio {first * 1e3:.1f} ms, all audio {last * 1e3:.1f} ms, "
                f"{secs:.1f} s of audio")
            if r >= 0:
                res[name].append((first, last))
    base = statistics.median(t for t, _ in res["generate_long"])
    first = statistics.median(t for t, _ in res["stream"])
    last = statistics.median(t for _, t in res["stream"])
    say(f"ttfa: generate_long(batch_size=32) {base * 1e3:.1f} ms; generate_long_stream("
        f"first_batch=1) first piece {first * 1e3:.1f} ms ({first / base:.3f} x), last piece "
        f"{last * 1e3:.1f} ms ({last / base:.3f} x); medians of {ROUNDS} rounds")


def order():
    """The other order of generate_long_stream's loop, by hand: group 1 is queued BEFORE the
    wait for piece 0.  Host timestamps (ms from the first group's start) of every step, and,
    from a polling thread, the moment piece 0's event reports done."""
    import threading
    import time

    from zipvoice_amd import longform as lf
    m, voc, fx, BREAK, text, pt, pw = stack_and_text()
    pf, rms, chunks = lf._long_prepare(text, pt, pw, m, fx, BREAK, (), 25.0, 1.0, 0.1, 0.1, 0.0,
                                       24000, 24000)
    joiner = WavJoiner()
    marks = []
    real_sample, real_decode = m.sample, voc.decode_features

    def stamped(name, fn):
        def call(*a, **k):
            r = fn(*a, **k)
            marks.append((name, time.perf_counter()))
            return r
        return call

    m.sample = stamped("sample returned", real_sample)
    voc.decode_features = stamped("decode returned", real_decode)

    def push(js, idx, final):
        nb = len(idx)
        wav, pl = lf._long_group(m, voc, [chunks[i] for i in idx], [pt] * nb,
                                 pf.expand(nb, -1, -1).contiguous(),
                                 torch.full((nb,), pf.size(1), dtype=torch.int64, device=dev),
                                 [7] * nb, idx, None, 0.1, 0.0, speed=1.0, t_shift=0.5, num_step=16,
                                 guidance_scale=1.0)
        p = js.push_async(wav, pl.to(dev, torch.int32) * 256, None, final=final)
        marks.append((f"group {idx[0]}..{idx[-1]} pushed", time.perf_counter()))
        return p

    for r in range(-1, ROUNDS):                           # round -1 is the warm-up
        js = joiner.stream(1, device=dev)
        marks.clear()
        done = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p0 = push(js, [0], False)

        def poll():
            while not p0._event.query():
                time.sleep(0.0002)
            done.append(time.perf_counter())

        th = threading.Thread(target=poll)
        th.start()
        p1 = push(js, list(range(1, 8)), True)
        for name, p in (("piece 0 in hand", p0), ("piece 1 in hand", p1)):
            p.wait()
            marks.append((name, time.perf_counter()))
        th.join()
        say(f"order round {r}: " + "; ".join(f"{k} {(v - t0) * 1e3:.1f}" for k, v in marks)
            + f" || piece 0's event done {(done[0] - t0) * 1e3:.1f}")


if __name__ == "__main__":
    mode = ARGS[0] if ARGS else ""
    if mode == "order":
        order()
        sys.exit(0)
    if mode == "join":
        join(ARGS[ARGS.index("--parent-lib") + 1] if "--parent-lib" in ARGS else None)
    elif mode == "ttfa":
        ttfa()
    else:
        sys.exit(__doc__)
