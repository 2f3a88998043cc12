#!/usr/bin/env python3
"""Benchmark: generated mel-frames/s (whole job) + RTF of ZipVoice sampling.

Workloads (BASELINE.json configs), synthetic seeded weights (no
pretrained weights offline) and synthetic inputs of the configs' shapes:

* C2 (default; the metric's configuration, BASELINE configs[1]): ZipVoice 123M,
  bf16 MFMA, N_steps=16, 32 utterances per GPU, each a 3 s prompt (281 frames, 40
  prompt tokens) + 10 s of generated speech (938 frames, 134 text tokens;
  duration="real"), T = 1219 frames, classifier-free guidance 1.0 (64 decoder rows
  per GPU), t_shift 0.5.  Weak scaling: the global batch is 32 x N utterances.
* C3 (``--config C3``, BASELINE configs[2]): ZipVoice-Distill, N_steps=8, guidance
  3.0 through the guidance embedding (no CFG doubling), a fixed global batch of 128
  utterances of the same shape sharded over the N GPUs (strong scaling).
* C4 (``--config C4``, BASELINE configs[3]): ZipVoice-Dialog, N_steps=16, 16 dialogues per
  GPU, each a 6 s prompt (563 frames, 80 tokens) + 30 s generated (2813 frames, 400 tokens,
  speaker turns [S1] / [S2]), T = 3376, CFG 1.5 (32 decoder rows per GPU); weak scaling.
* C5 (``--config C5``, BASELINE configs[4]): ZipVoice-Dialog-Stereo, N_steps=16, a fixed
  global batch of 32 two-channel dialogues of C4's shape (200-dim features) sharded over the
  N GPUs (4 per GPU on 8), CFG 1.5, fp8 MFMA weights by default (``--precision fp8``, the
  BASELINE mode; bf16 selectable); each channel decoded by the vocoder
  (``infer_zipvoice_dialog.py:478-490``), wav (B, n, 2).

One "step" = what the reference's RTF times (``infer_zipvoice.py:359-386``) for the
whole global batch, run data-parallel (``zipvoice_amd.dist.generate_batch_dp``):
every rank takes its contiguous shard of the global batch, runs ``ZipVoice.sample()``
(text encoder, conditions, the guided Euler loop replayed as one HIP graph) and the
vocoder on the generated features (post-processing + Vocos decode + clamp, ``:374-378``),
and one RCCL all-gather over xGMI reassembles the output wav batch on every rank.
Inputs are resident in HBM before the timed region.

A plain run sets up, warms up, times the K steps and prints the result line.  ``--dump-outputs
DIR`` also writes what the last timed step returned (the wav batch and its lengths) as
``DIR/<name>.npy``; ``--full`` adds the legs that take runs of their own: the per-kernel roofline
pass, the fp32 / fp16 modes (C2 / C3 in bf16) and the CPU baseline.

Launch: python bench.py [--gpus N --steps K --warmup W --config C2|C3|C4|C5 --precision P]
                        [--dump-outputs DIR] [--full]
        (N > 1 under torch.distributed.run, one process per GPU).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# per-utterance shapes: C2 / C3 3 s prompt + 10 s generated; C4 / C5 6 s + 30 s
SHAPE_10S = dict(t_prompt=281, s_prompt=40, s_text=134, t_gen=938)
SHAPE_30S = dict(t_prompt=563, s_prompt=80, s_text=400, t_gen=2813)
T_SHIFT = 0.5
SAMPLE_RATE = 24000
HOP = 256
CONFIGS = {
    "C2": dict(variant="zipvoice", num_step=16, guidance=1.0, per_gpu=32, global_batch=None,
               scaling="weak", cfg_rows=2, precision="bf16", **SHAPE_10S,
               metric="generated mel-frames/s (whole job) + RTF, ZipVoice 123M N_steps=16 batch=32/GPU",
               desc="C2: ZipVoice 123M, N_steps=16, batch=32/GPU x (3 s prompt + 10 s generated; "
                    "T=1219 frames), CFG g=1.0 (64 decoder rows per GPU), t_shift=0.5"),
    "C3": dict(variant="zipvoice_distill", num_step=8, guidance=3.0, per_gpu=None,
               global_batch=128, scaling="strong", cfg_rows=1, precision="bf16", **SHAPE_10S,
               metric="generated mel-frames/s (whole job) + RTF, ZipVoice-Distill N_steps=8 batch=128",
               desc="C3: ZipVoice-Distill 123M, N_steps=8, global batch=128 x (3 s prompt + 10 s "
                    "generated; T=1219 frames) sharded over the GPUs, guidance 3.0 (embedding, "
                    "no CFG doubling), t_shift=0.5"),
    "C4": dict(variant="zipvoice_dialog", num_step=16, guidance=1.5, per_gpu=16, global_batch=None,
               scaling="weak", cfg_rows=2, precision="bf16", **SHAPE_30S,
               metric="generated mel-frames/s (whole job) + RTF, ZipVoice-Dialog N_steps=16 batch=16x30s/GPU",
               desc="C4: ZipVoice-Dialog, N_steps=16, batch=16/GPU x (6 s prompt + 30 s generated "
                    "dialogue with [S1]/[S2] turns; T=3376 frames), CFG g=1.5 (32 decoder rows per "
                    "GPU), t_shift=0.5"),
    "C5": dict(variant="zipvoice_dialog_stereo", num_step=16, guidance=1.5, per_gpu=None,
               global_batch=32, scaling="strong", cfg_rows=2, precision="fp8", **SHAPE_30S,
               metric="generated mel-frames/s (whole job, per channel) + RTF, ZipVoice-Dialog-Stereo "
                      "N_steps=16 batch=32 two-channel",
               desc="C5: ZipVoice-Dialog-Stereo, N_steps=16, global batch=32 two-channel dialogues x "
                    "(6 s prompt + 30 s generated; T=3376 frames, 200-dim features) sharded over "
                    "the GPUs, CFG g=1.5, t_shift=0.5; both channels vocoded"),
}
BF16_DENSE_PEAK_TFLOPS = 2500.0     # MI355X_MICROARCH.md: ~2.5 PF dense bf16
FP8_DENSE_PEAK_TFLOPS = 5000.0      # ... ~5 PF dense fp8 (the MX-fp8 GEMMs of the fp8 mode)
FP32_MFMA_PEAK_TFLOPS = 157.3
HBM_PEAK_GBS = 8000.0
# PMC traffic per launch (tools/pmc_traffic.py) of the kernels the roofline reports, keyed by
# the engine's profiler tag (one symbol per tag since round 3: the residual linears by ROLE, the
# fused FeedForward with / without the BiasNorm epilogue); newest measurement first
# (round 4: measured on the timed three-stream schedule, the same launch set the roofline pass times)
# (round 6: the residual ROLEs' regexes cover every tile form the tag launches -- 128 x 128, 128 x 64
# and 64 x 64 -- so the PMC mean and the algorithmic mean describe the same launch set; the text
# encoder pass is included, which is where ROLE 2 runs)
TRAFFIC_FILES = {"gemm_bf16_resid": ["r06_gemm_resid_r1_traffic.json"],
                 "gemm_bf16_resid_rv": ["r06_gemm_resid_r4_traffic.json"],
                 "gemm_bf16_resid_byp": ["r06_gemm_resid_r2_traffic.json"],
                 "ffn_bf16": ["r06_ffn_traffic.json", "r05_ffn_traffic.json"],
                 "ffn_norm_bf16": ["r06_ffn_norm_traffic.json", "r05_ffn_norm_traffic.json"],
                 "ffn_bf16+ffn_norm_bf16": ["r06_ffn_all_traffic.json", "r05_ffn_all_traffic.json"],
                 "gemm_bf16_glu_dw": ["r06_gemm_glu_dw_traffic.json"]}
# the residual-stream linears by epilogue ROLE (zv_gemm.inc): the HBM-bound family of the path
RESID_TAGS = ("gemm_bf16_resid", "gemm_bf16_resid_rv", "gemm_bf16_resid_byp")
# analytic FLOPs of one decoder sequence-forward (FlopCounterMode fit on the
# reference, within 1 %) and of the vocoder per frame
def decoder_flops(T):
    return 146.3e6 * T + 9920.0 * T * T


VOCODER_FLOPS_PER_FRAME = 27e6


def feat_width(conf):
    return 200 if conf["variant"] == "zipvoice_dialog_stereo" else 100


def item_arrays(conf, i):
    """Utterance i of the synthetic global batch (the same on every rank).  Dialog configs put
    the speaker-turn tokens [S1] (360) / [S2] (361) at the start and the middle of both texts."""
    rng = np.random.default_rng([1000, i])
    dialog = conf["variant"].startswith("zipvoice_dialog")

    def toks(n):
        t = [int(v) for v in rng.integers(1, 360, n)]
        if dialog:
            t[0], t[n // 2] = 360, 361
        return t

    tokens, ptokens = toks(conf["s_text"]), toks(conf["s_prompt"])
    F = feat_width(conf)
    pf = (0.3 * rng.standard_normal((conf["t_prompt"], F)) - 0.5).astype(np.float32)
    x0 = np.random.default_rng([666, i]).standard_normal((conf["t_prompt"] + conf["t_gen"], F),
                                                         dtype=np.float32)
    return tokens, ptokens, pf, x0


def materialize(conf, ids, device):
    """Device-resident inputs of a shard (built before the timed region)."""
    arrs = [item_arrays(conf, i) for i in ids]
    b = len(ids)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return dict(tokens=[a[0] for a in arrs], prompt_tokens=[a[1] for a in arrs],
                prompt_features=to(np.stack([a[2] for a in arrs])) if b else None,
                prompt_features_lens=to(np.full(b, conf["t_prompt"], np.int64)),
                features_lens=to(np.full(b, conf["t_gen"], np.int64)),
                x0=to(np.stack([a[3] for a in arrs])) if b else None)


def build(variant, precision, device):
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    from zipvoice_amd.weights import synthetic_state_dict
    cfg = default_config(variant)
    m = build_model(cfg, precision=precision)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    return m.to(device)


def build_vocoder(device):
    from zipvoice_amd.vocoder import Vocos
    return Vocos(precision="fp32").load_synthetic(0).to(device)


class Job:
    """One benchmark step: generate_batch_dp over the global batch."""

    def __init__(self, conf, model, vocoder, n_items, device):
        from zipvoice_amd.dist import shard_bounds, _world_rank
        self.conf, self.model, self.vocoder, self.device = conf, model, vocoder, device
        self.items = list(range(n_items))
        self.costs = [conf["t_prompt"] + conf["t_gen"]] * n_items      # frames per utterance
        world, rank = _world_rank()
        lo, hi = shard_bounds(self.costs, world)[rank]
        self.inp = materialize(conf, self.items[lo:hi], device)
        self.n_local = hi - lo
        self.channels = 2 if feat_width(conf) == 200 else 1

    def compute(self, shard):
        assert len(shard) == self.n_local
        if not shard:
            return (torch.zeros((0, 1) if self.channels == 1 else (0, 1, self.channels), device=self.device),
                    torch.zeros((0,), dtype=torch.int64, device=self.device))
        inp = self.inp
        gen, gen_lens, _, _ = self.model.sample(
            tokens=inp["tokens"], prompt_tokens=inp["prompt_tokens"],
            prompt_features=inp["prompt_features"],
            prompt_features_lens=inp["prompt_features_lens"],
            features_lens=inp["features_lens"], t_shift=T_SHIFT, duration="real",
            num_step=self.conf["num_step"], guidance_scale=self.conf["guidance"], x0=inp["x0"])
        if self.channels == 1:
            wav = self.vocoder.decode_features(gen, gen_lens, feat_scale=0.1, feat_bias=0.0,
                                               clamp=True)
            return wav, gen_lens * HOP
        # two-channel features: each channel decoded (infer_zipvoice_dialog.py:478-490), both in
        # one vocoder batch, returned channel-last (b, n, 2)
        b = gen.shape[0]
        F = gen.shape[2] // 2
        both = torch.cat([gen[..., :F], gen[..., F:]], 0)
        wav = self.vocoder.decode_features(both, torch.cat([gen_lens, gen_lens]), feat_scale=0.1,
                                           feat_bias=0.0, clamp=True)
        return wav.view(2, b, -1).permute(1, 2, 0), gen_lens * HOP

    def step(self):
        from zipvoice_amd.dist import generate_batch_dp
        return generate_batch_dp(self.items, self.compute, self.costs)


def timed(job, steps, warmup, world, keep=None):
    """Seconds per step over `steps` timed steps after `warmup` untimed ones.  With a list
    `keep`, what the last timed step returned is appended to it."""
    import torch.distributed as dist
    for _ in range(warmup):
        job.step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps - 1):
        job.step()
    last = job.step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if keep is not None:
        keep.append(last)
    return dt / steps


DUMP_LIMIT_BYTES = 64 * 2 ** 20


def dump_outputs(path, wav, lens):
    """What a caller of the timed step receives from its last run, as float32 .npy files: `wav`
    (the (B, n) batch, or (B, n, C)) and `lens` (samples per utterance).  A wav batch over the
    size limit is written as `wav_sample`, its flattened elements at the sorted positions
    `wav_sample_index` (a fixed seeded draw, stored as float64: exact for these indices), so that
    two runs with the same arguments store the same elements."""
    os.makedirs(path, exist_ok=True)
    wav = wav.detach().float().cpu().numpy()
    np.save(os.path.join(path, "lens.npy"), lens.detach().cpu().numpy().astype(np.float32))
    if wav.nbytes <= DUMP_LIMIT_BYTES - 2 ** 20:    # (1 MB left for lens and the .npy headers)
        np.save(os.path.join(path, "wav.npy"), np.ascontiguousarray(wav))
        return
    n = DUMP_LIMIT_BYTES // 32                      # 8 MB of float32 values + 16 MB of indices
    idx = np.sort(np.random.default_rng(2024).integers(0, wav.size, n))
    np.save(os.path.join(path, "wav_sample.npy"), wav.reshape(-1)[idx])
    np.save(os.path.join(path, "wav_sample_index.npy"), idx.astype(np.float64))


def _kernel_roofline(name, r, total_ms):
    """Roofline object of one tagged kernel.  Residual-stream linears (tag *_resid) sit
    below the bf16 ridge point (<= ~250 FLOP/B vs 2500 TF/s / 8 TB/s = 312): bound HBM,
    achieved = algorithmic bytes per launch / average launch duration.  The others are
    priced on the dense MFMA peak of their dtype."""
    hbm = "_resid" in name
    sec = r["ms"] * 1e-3
    if hbm:
        achieved, peak, unit = r["bytes"] / sec / 1e9, HBM_PEAK_GBS, "GB/s"
    else:
        achieved = r["flops"] / sec / 1e12
        peak = (FP8_DENSE_PEAK_TFLOPS if "fp8" in name else
                BF16_DENSE_PEAK_TFLOPS if "bf16" in name else FP32_MFMA_PEAK_TFLOPS)
        unit = "TFLOP/s"
    traffic, tsrc = None, None
    tfile = next((f for f in TRAFFIC_FILES.get(name, [])
                  if os.path.exists(os.path.join(REPO, "profiles", f))), None)
    tpath = os.path.join(REPO, "profiles", tfile) if tfile else None
    if tpath:
        with open(tpath) as f:
            t = json.load(f)
        traffic = t.get("traffic_bytes_per_launch")
        tsrc = (f"profiles/{tfile}: rocprofv3 PMC FETCH_SIZE(x2, gfx950) + WRITE_SIZE "
                f"per launch of {t['kernel_regex']} over one guided forward")
    alg = r["bytes"] / r["launches"] if r["launches"] else 0.0
    ratio = round(traffic / alg, 3) if traffic and alg else None
    if traffic and t.get("traffic_over_algorithmic"):
        # the PMC pass's launch mix differs from the timed step's (text-encoder launches, row
        # blocks): take the ratio on the PMC pass's own launch set and price this launch set with it
        ratio = t["traffic_over_algorithmic"]
        tsrc += (f"; ratio to the algorithmic bytes of that same launch set "
                 f"({t['algorithmic_launches']} launches), applied to this step's launches "
                 f"(measured mean {traffic / 1e6:.1f} MB per PMC launch)")
        traffic = ratio * alg
    out = {
        "kernel": name, "bound": "hbm" if hbm else "mfma", "achieved": round(achieved, 2), "peak": peak,
        "unit": unit, "frac": round(achieved / peak, 4), "traffic": traffic,
        "traffic_unit": "bytes per launch", "traffic_source": tsrc,
        "algorithmic_bytes_per_launch": round(alg),
        "traffic_over_algorithmic": ratio,
        "hbm_frac": round(alg / (r["ms"] * 1e-3 / r["launches"]) / 1e9 / HBM_PEAK_GBS, 4) if r["ms"] else None,
        "launches_per_step": r["launches"], "avg_launch_us": round(r["ms"] * 1e3 / r["launches"], 2),
        "flops_per_launch": r["flops"] / r["launches"],
        "tflops_achieved": round(r["flops"] / sec / 1e12, 2),
        "share_of_profiled_time": round(r["ms"] / total_ms, 3),
    }
    return out


def roofline(job):
    """One extra, untimed step with the engine's per-launch HIP-event profiler on: the timed
    step's launches (the decoder's three row blocks, the same kernels and shapes: the launch set
    the rocprofv3 summary of the bench command and the PMC traffic files also see), run one row
    block after another so that each event pair times its launch alone (overlapping on three
    streams, an event pair also timed the co-running kernels; rocprofv3's kernel trace serialises
    the dispatches the same way).  The dominant kernel's algorithmic work per launch / its
    average duration, and the residual-linear family (the HBM-bound one) per epilogue ROLE as
    `secondary`."""
    from zipvoice_amd import engine
    torch.cuda.synchronize()
    engine.profile(True)
    job.compute(list(range(job.n_local)))
    torch.cuda.synchronize()
    rep = engine.profile_report()
    engine.profile(False)
    total_ms = sum(v["ms"] for v in rep.values())
    # the FeedForward kernel is one symbol family over two tags (with / without the BiasNorm
    # epilogue): the dominant object prices their union
    ff = [k for k in ("ffn_bf16", "ffn_norm_bf16") if k in rep]
    if ff:
        name = "+".join(ff)
        r = {k: sum(rep[t][k] for t in ff) for k in ("ms", "flops", "bytes", "launches")}
    else:
        name, r = max(rep.items(), key=lambda kv: kv[1]["ms"])
    res = _kernel_roofline(name, r, total_ms)
    if len(ff) > 1:
        res["per_tag"] = {t: _kernel_roofline(t, rep[t], total_ms) for t in ff}
    # (+ the fused convolution front, GLU linear + depthwise conv: MFMA + VALU, priced on the MFMA peak)
    res["secondary"] = {t: _kernel_roofline(t, rep[t], total_ms) for t in RESID_TAGS + ("gemm_bf16_glu_dw",)
                        if t in rep}
    res["per_kernel_ms_per_step"] = {k: round(v["ms"], 3) for k, v in rep.items()}
    return res


def cpu_baseline(conf, budget_s=12.0):
    """Oracle (numpy fp32 restatement, oracle/zipvoice_np.py) on the host cores: one
    utterance of the same workload (the config's T and feature width; CFG batch of 2 where the
    model guides), velocity evaluations repeated until ~budget_s, scaled to generated frames/s."""
    variant, guidance, num_step = conf["variant"], conf["guidance"], conf["num_step"]
    from threadpoolctl import threadpool_limits

    from oracle.zipvoice_np import ZipVoiceOracle
    from zipvoice_amd.config import default_config
    from zipvoice_amd.weights import synthetic_state_dict
    cores = min(16, len(os.sched_getaffinity(0)))
    cfg = default_config(variant)
    o = ZipVoiceOracle(cfg, synthetic_state_dict(cfg, 0))
    rng = np.random.default_rng(7)
    T, T_GEN, F = conf["t_prompt"] + conf["t_gen"], conf["t_gen"], feat_width(conf)
    x = rng.standard_normal((1, T, F), dtype=np.float32)
    tc = rng.standard_normal((1, T, 100), dtype=np.float32)
    sc = rng.standard_normal((1, T, F), dtype=np.float32)
    pm = np.zeros((1, T), bool)
    n = 0
    with threadpool_limits(limits=cores):
        t0 = time.perf_counter()
        while True:
            o.velocity(np.float32(0.3), x, tc, sc, pm, guidance)
            n += 1
            if time.perf_counter() - t0 > budget_s or n >= 8:
                break
        dt = (time.perf_counter() - t0) / n
    frames_per_s = T_GEN / (num_step * dt)
    return {"value": round(frames_per_s, 2), "unit": "mel-frames/s", "cores": cores,
            "kind": "port",
            "sample": f"{n} velocity evaluations (T={T}, {variant}, g={guidance}) of one "
                      f"utterance; {dt:.2f} s each; frames/s = {T_GEN} / ({num_step} steps x time "
                      f"per evaluation); vocoder excluded"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="C2", choices=sorted(CONFIGS))
    ap.add_argument("--precision", default=None, choices=["bf16", "fp32", "fp16", "fp8"],
                    help="compute mode (default: the config's, bf16; C5 fp8 as BASELINE names it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (wav, lens) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the per-kernel roofline pass, the fp32 / "
                         "fp16 legs (C2 / C3, bf16) and the CPU baseline, and add them to the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip that leg")
    ap.add_argument("--no-fp32-mode", action="store_true", help="with --full: skip the fp32 / fp16 legs")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    conf = CONFIGS[args.config]
    if args.precision is None:
        args.precision = conf["precision"]

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=device)

    n_items = conf["global_batch"] or conf["per_gpu"] * world
    model = build(conf["variant"], args.precision, device)
    vocoder = build_vocoder(device)
    job = Job(conf, model, vocoder, n_items, device)
    last = [] if args.dump_outputs else None
    ms = timed(job, args.steps, args.warmup, world, keep=last) * 1e3
    T_GEN = conf["t_gen"]
    frames = n_items * T_GEN
    value = frames / (ms * 1e-3)
    audio_s = n_items * T_GEN * HOP / SAMPLE_RATE
    rtf = (ms * 1e-3) / audio_s                      # whole job
    T = conf["t_prompt"] + T_GEN
    path_flops = (n_items * conf["cfg_rows"] * conf["num_step"] * decoder_flops(T)
                  + job.channels * n_items * T_GEN * VOCODER_FLOPS_PER_FRAME)
    path_tfs = path_flops / (ms * 1e-3) / 1e12
    result = {
        "metric": conf["metric"],
        "value": round(value, 1), "unit": "mel-frames/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms, 2), "higher_is_better": True,
        "scaling": conf["scaling"], "vs_baseline": None, "dtype": args.precision,
        "data": "synthetic (seeded weights and inputs of the config's shapes)",
        "rtf": round(rtf, 6), "x_realtime_per_gpu": round(1.0 / (rtf * world), 1),
        "config": {"workload": conf["desc"],
                   "model": f"{conf['variant']} (zipvoice_base.json, synthetic seeded weights)",
                   "global_batch": n_items, "seq_len": T, "parallelism": f"dp{world}"},
        # the path is a dense contraction priced on the bf16 MFMA peak
        "path_roofline": {"algorithmic_tflop_per_step": round(path_flops / 1e12, 2),
                          "achieved_tflops": round(path_tfs, 1),
                          "peak_tflops": BF16_DENSE_PEAK_TFLOPS * world,
                          "frac": round(path_tfs / (BF16_DENSE_PEAK_TFLOPS * world), 4),
                          "flops_source": "F(T)=146.3e6*T+9920*T^2 per decoder sequence-forward "
                                          "(SURVEY.md §6) x rows x steps + 27 MFLOP/frame vocoder"},
    }
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, *last.pop()[:2])
        if args.full:
            result["roofline"] = roofline(job)
        if args.full and world == 1 and not args.no_fp32_mode and args.precision == "bf16" and args.config in ("C2", "C3"):
            del job, model
            torch.cuda.empty_cache()
            m32 = build(conf["variant"], "fp32", device)
            job32 = Job(conf, m32, vocoder, n_items, device)
            ms32 = timed(job32, 1, 2, 1) * 1e3        # after two warm-ups (graph captured)
            result["fp32_accurate_mode"] = {
                "ms_per_step": round(ms32, 2),
                "value": round(frames / (ms32 * 1e-3), 1), "unit": "mel-frames/s",
                "note": "bf16x3 split-product GEMMs; the parity mode (mean |err| ~3e-5 vs reference); "
                        "timed after 2 warm-up steps"}
            del job32, m32
            torch.cuda.empty_cache()
            m16 = build(conf["variant"], "fp16", device)
            job16 = Job(conf, m16, vocoder, n_items, device)
            ms16 = timed(job16, args.steps, 2, 1) * 1e3
            result["fp16_parity_mode"] = {
                "ms_per_step": round(ms16, 2),
                "value": round(frames / (ms16 * 1e-3), 1), "unit": "mel-frames/s",
                "vs_bf16_time": round(ms16 / ms, 3),
                "note": "fp16 MFMA operands in the decoder layers, split products for the "
                        "decoder in/out projections, the attention-score projections and the "
                        "text encoder: meets the north-star "
                        "1e-3 mean |err| bar (tests/test_gpu_parity.py, test_gpu_fullsize.py); "
                        "timed after 2 warm-up steps"}
            # the fastest mode that meets north_star's 1e-3 mean |err| bar (fp32 and fp16 do;
            # bf16 does not: DESIGN.md §4)
            best = min((("fp16", ms16), ("fp32", ms32)), key=lambda kv: kv[1])
            result["fastest_parity_mode"] = {"mode": best[0], "ms_per_step": round(best[1], 2),
                                             "value": round(frames / (best[1] * 1e-3), 1),
                                             "vs_bf16_time": round(best[1] / ms, 3)}
            del job16, m16
            # the fp8 mode (BASELINE configs[4]) is not a leg of this line since round 4: on the fused
            # tree it runs within 2-4 % of bf16 (the explicit stop); its C5 timing is
            # tools/config_bench.py's, its accuracy tests/test_gpu_fp8.py
        if args.full and world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(conf)
        print(json.dumps(result), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
