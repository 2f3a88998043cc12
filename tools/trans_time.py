#!/usr/bin/env python3
"""The two transposed-output linears alone at the decoder's shapes: the NonlinAttention
in-projection (N = 1152) and the SelfAttention value projection (N = 64), K = 512, 64 utterances of
1219 / 610 / 305 frames (78016 / 39040 / 19520 rows), through the engine's launch choice
(zv_bench_fused_linear; HIP events around `iters` back-to-back launches after one warm-up launch).

usage: trans_time.py [--iters N] [--reps R] [--arms 0,1]
  --arms: values of ZV_TRANS_ALIGNED to run (default 0,1: row tiles with per-element stores, then
          utterance-aligned tiles with 16-byte stores); ZV_LIB_PATH selects another build of the library
Prints one line per (form, rows, arm): the R repetitions in us, and their minimum.
"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch  # noqa: E402,F401

from zipvoice_amd import engine  # noqa: E402

NA, TRANS = 7, 6
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--arms", default="0,1")
args = ap.parse_args()
lib = engine.load_library()
for form, name, N in ((NA, "na_in", 1152), (TRANS, "value_t", 64)):
    for L in (1219, 610, 305):
        M = 64 * L
        for arm in args.arms.split(","):
            os.environ["ZV_TRANS_ALIGNED"] = arm
            us = []
            for _ in range(args.reps):
                ms = ctypes.c_float()
                rc = lib.zv_bench_fused_linear(form, M, N, 512, L, args.iters, ctypes.byref(ms))
                if rc:
                    sys.exit(f"{name} M={M}: {lib.zv_last_error().decode()}")
                us.append(ms.value * 1e3)
            print(f"{name} M={M} N={N} K=512 L={L} ZV_TRANS_ALIGNED={arm}: "
                  f"{' '.join(f'{u:7.1f}' for u in us)} us  min {min(us):7.1f}", flush=True)
