"""ctypes binding of libzipvoice_hip.so (the C ABI declared in include/zipvoice_hip.h).

PyTorch-ROCm is used only for device memory, streams and distributed plumbing:
every tensor handed to the engine is a contiguous device buffer whose pointer
crosses the C ABI; all arithmetic of the hot path runs in the engine's HIP
kernels.  There is no CPU fallback: if the library or a GPU is missing, the
constructor raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import numpy as np
import torch  # noqa: F401  (imported first so the engine shares torch's HIP runtime)

from .config import ModelConfig
from .weights import check_state_dict

LIB_NAME = "libzipvoice_hip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
# the same engine built with IEEE fp16 MFMA operands (csrc/build.py VARIANTS)
LIB_F16_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libzipvoice_hip_f16.so")
MAX_STACKS = 8
VARIANT_ID = {"zipvoice": 0, "zipvoice_distill": 1, "zipvoice_dialog": 2,
              "zipvoice_dialog_stereo": 3}
PRECISION_ID = {"fp32": 0, "bf16": 1}      # vocoder / BigVGAN precisions (main library)
# decoder precision modes: name -> (library, zv_precision).  "fp16" is the parity-grade fast
# mode: fp16 MFMA operands in the decoder layers, split products for the decoder's input /
# output projections, the attention-score projections and the text encoder (ZV_MIXED in the
# fp16 library)
# "fp8": the BASELINE C5 mode - the decoder layers' feed-forward, convolution-module and
# NonlinAttention output linears on block-scaled MX-fp8 MFMA (ZV_FP8, main library)
MODES = {"fp32": ("bf16", 0), "bf16": ("bf16", 1), "fp16": ("f16", 2),
         "fp16_plain": ("f16", 1), "bf16_mixed": ("bf16", 2), "fp8": ("bf16", 3)}


class ZvConfig(ctypes.Structure):
    _fields_ = [
        ("variant", ctypes.c_int), ("precision", ctypes.c_int), ("feat_dim", ctypes.c_int),
        ("num_stacks", ctypes.c_int),
        ("downsampling_factor", ctypes.c_int * MAX_STACKS),
        ("num_layers", ctypes.c_int * MAX_STACKS),
        ("cnn_module_kernel", ctypes.c_int * MAX_STACKS),
        ("fm_decoder_dim", ctypes.c_int), ("fm_decoder_feedforward_dim", ctypes.c_int),
        ("fm_decoder_num_heads", ctypes.c_int),
        ("text_encoder_num_layers", ctypes.c_int), ("text_encoder_feedforward_dim", ctypes.c_int),
        ("text_encoder_cnn_module_kernel", ctypes.c_int),
        ("text_encoder_num_heads", ctypes.c_int), ("text_encoder_dim", ctypes.c_int),
        ("time_embed_dim", ctypes.c_int), ("text_embed_dim", ctypes.c_int),
        ("query_head_dim", ctypes.c_int), ("value_head_dim", ctypes.c_int),
        ("pos_head_dim", ctypes.c_int), ("pos_dim", ctypes.c_int),
        ("vocab_size", ctypes.c_int), ("pad_id", ctypes.c_int), ("spk_a_id", ctypes.c_int),
        ("spk_b_id", ctypes.c_int),
    ]


class ZvLinearCheckArgs(ctypes.Structure):
    """zv_linear_check_args (test infrastructure; tests/test_gpu_linear_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("M", "N", "K", "split", "form", "act", "rows_per_group",
                                            "rpb", "guard")] + [
        (n, ctypes.c_void_p) for n in ("A", "W", "bias", "resid", "orig", "byp", "rowvec", "rowmask",
                                       "dw_w", "dw_b")] + [
        ("dw_ks", ctypes.c_int), ("dw_L", ctypes.c_int),
        ("C", ctypes.c_void_p), ("ldc", ctypes.c_int64),
        ("Ch", ctypes.c_void_p), ("Cl", ctypes.c_void_p), ("ldch", ctypes.c_int64),
        ("Cth", ctypes.c_void_p), ("Ctl", ctypes.c_void_p), ("ldct", ctypes.c_int64),
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


class ZvFfnCheckArgs(ctypes.Structure):
    """zv_ffn_check_args (test infrastructure; tests/test_gpu_ffn_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("M", "H", "form", "rows_per_group", "part_slots", "guard")] + [
        ("log_scale", ctypes.c_float)] + [
        (n, ctypes.c_void_p) for n in ("x", "W1", "b1", "W2", "b2", "resid", "rowvec", "orig", "byp", "nb")] + [
        ("C", ctypes.c_void_p), ("ldc", ctypes.c_int64),
        ("Ch", ctypes.c_void_p), ("Cl", ctypes.c_void_p), ("C2h", ctypes.c_void_p), ("C2l", ctypes.c_void_p),
        ("ldch", ctypes.c_int64),
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int),
        ("K", ctypes.c_int), ("A", ctypes.c_void_p), ("Wp", ctypes.c_void_p), ("bp", ctypes.c_void_p)]


class ZvDwconvCheckArgs(ctypes.Structure):
    """zv_dwconv_check_args (test infrastructure; tests/test_gpu_dwconv_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("B", "L", "C", "ks", "split", "guard")] + [
        (n, ctypes.c_void_p) for n in ("g", "w", "bias")] + [
        ("ldin", ctypes.c_int64),
        ("Oh", ctypes.c_void_p), ("Ol", ctypes.c_void_p), ("ldout", ctypes.c_int64),
        ("q", ctypes.c_void_p), ("qs", ctypes.c_void_p), ("ldq", ctypes.c_int64),
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


class ZvAttnCheckArgs(ctypes.Structure):
    """zv_attn_check_args (test infrastructure; tests/test_gpu_attn_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "B", "L", "H", "nv", "split", "form", "b2", "guard", "vrows")] + [
        ("stale", ctypes.c_float)] + [
        (n, ctypes.c_void_p) for n in ("qkp", "P", "key_pad", "v", "y", "stats")] + [
        ("oh", ctypes.c_void_p), ("ol", ctypes.c_void_p), ("oh2", ctypes.c_void_p), ("ldo", ctypes.c_int64),
        ("Wh", ctypes.c_void_p), ("Wl", ctypes.c_void_p), ("ldw", ctypes.c_int64),
        ("launch", ctypes.c_int * 8)]


class ZvStackedgeCheckArgs(ctypes.Structure):
    """zv_stackedge_check_args (test infrastructure; tests/test_gpu_stackedge_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "B", "L", "C", "ds", "guard", "rows_per_group")] + [
        ("log_scale", ctypes.c_float)] + [
        (n, ctypes.c_void_p) for n in ("x", "w", "nb", "orig", "rowvec", "mask", "out", "mout",
                                       "h", "l", "h2", "l2")] + [
        ("ldact", ctypes.c_int64),
        ("q2", ctypes.c_void_p), ("qs2", ctypes.c_void_p), ("ldq", ctypes.c_int64),
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


class ZvPadrowCheckArgs(ctypes.Structure):
    """zv_padrow_check_args (test infrastructure; tests/test_gpu_padrow_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("B", "L", "C", "ds", "guard")] + [
        (n, ctypes.c_void_p) for n in ("mask", "x", "w", "lens", "out")] + [
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


class ZvBigvganCheckArgs(ctypes.Structure):
    """zv_bigvgan_check_args (test infrastructure; tests/test_gpu_bigvgan_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "split", "mode", "guard", "B", "Lmax", "Ls", "halo", "scale",
                                            "C", "Cout", "ks", "d", "u", "n", "layout", "flag")] + [
        (n, ctypes.c_float) for n in ("div", "sub", "bias0")] + [
        ("stale", ctypes.c_uint)] + [
        (n, ctypes.c_void_p) for n in ("lens", "x", "x1", "x2", "w", "bias", "alpha", "ibeta", "w2", "bias2",
                                       "alpha2", "ibeta2", "taps", "resid", "ah", "al", "out", "oh", "ol")] + [
        ("ld", ctypes.c_int64),
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


class ZvSolveCheckArgs(ctypes.Structure):
    """zv_solve_check_args (test infrastructure; tests/test_gpu_solve_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "guard", "form", "B", "T", "S", "C", "Fx", "Ft", "Fs", "copies",
                                            "zero_speech", "cfg", "M", "N", "K", "pre", "inplace")] + [
        (n, ctypes.c_float) for n in ("g", "dt", "gmul", "value")] + [
        (n, ctypes.c_int64) for n in ("n", "per_row", "ld", "ldin", "ldw")] + [
        (n, ctypes.c_void_p) for n in ("x", "tc", "sc", "v", "grows", "W", "bias", "add", "lens", "lens2", "tok",
                                       "spk", "mask", "out", "oh", "ol", "mout")] + [
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


class ZvRowSched(ctypes.Structure):
    """zv_row_sched: one row of a scheduled solve (zv_euler_sample_sched, zv_sched_plan)."""
    _fields_ = [("num_step", ctypes.c_int32), ("t_start", ctypes.c_float), ("t_end", ctypes.c_float),
                ("t_shift", ctypes.c_float), ("guidance_scale", ctypes.c_float)]


class ZvSchedPlanOut(ctypes.Structure):
    """zv_sched_plan_out (tests/test_sched_plan.py)."""
    _fields_ = [("steps", ctypes.c_int32), ("active", ctypes.c_int32), ("copies", ctypes.c_int32),
                ("total_rows", ctypes.c_int64)] + [
        (n, ctypes.c_void_p) for n in ("dec_src", "dec_zero_text", "dec_zero_speech", "dec_t", "act_row", "act_dt",
                                       "act_scale", "act_cond", "act_uncond")]


class ZvSchedCheckArgs(ctypes.Structure):
    """zv_sched_check_args (test infrastructure; tests/test_gpu_sched_ref.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "guard", "B", "T", "N", "A", "Fx", "Ft", "Fs")] + [
        ("ld", ctypes.c_int64), ("per_row", ctypes.c_int64)] + [
        (n, ctypes.c_void_p) for n in ("src", "zero_text", "zero_speech", "x", "tc", "sc", "mask", "v", "row", "dt",
                                       "scale", "cond", "uncond", "out", "oh", "ol", "mout")] + [
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


class ZvSessionCheckArgs(ctypes.Structure):
    """zv_session_check_args (test infrastructure; tests/test_gpu_session_kernels.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "guard", "slots", "max_frames", "n", "T_io", "T_k", "N", "A",
                                            "Fx", "Ft", "Fs")] + [
        ("ld", ctypes.c_int64)] + [
        (n, ctypes.c_void_p) for n in ("slot", "len", "src", "zero_text", "zero_speech", "x", "tc", "sc", "mask", "v",
                                       "row", "dt", "scale", "cond", "uncond", "out", "out_tc", "out_sc", "oh", "ol",
                                       "mout")] + [
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


class ZvSessionEditCheckArgs(ctypes.Structure):
    """zv_session_edit_check_args (test infrastructure; tests/test_gpu_session_edit_kernels.py)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kind", "guard", "slots", "max_frames", "n", "T_io", "Fx", "Ft",
                                            "pool_rows", "keep_original")] + [
        (n, ctypes.c_void_p) for n in ("slot", "offsets", "lens", "table", "row_ptr", "rows", "state_left",
                                       "state_len", "x", "tc", "pool", "out", "out_tc", "out_sc", "mout")] + [
        ("launch", ctypes.c_int * 8), ("num_cus", ctypes.c_int)]


def row_schedule_array(schedule):
    """A sequence of rows with num_step / t_start / t_end / t_shift / guidance_scale attributes (or
    5-tuples in that order) as a ctypes array of zv_row_sched."""
    arr = (ZvRowSched * len(schedule))()
    for i, r in enumerate(schedule):
        if isinstance(r, (tuple, list)):
            n, t0, t1, sh, g = r
        else:
            n, t0, t1, sh, g = r.num_step, r.t_start, r.t_end, r.t_shift, r.guidance_scale
        if int(n) != n:
            raise ValueError(f"schedule row {i}: num_step must be an integer, got {n!r}")
        arr[i] = ZvRowSched(int(n), float(t0), float(t1), float(sh), float(g))
    return arr


class ZvNoiseCheckArgs(ctypes.Structure):
    """zv_noise_check_args (test infrastructure; tests/test_noise_spec.py, tests/test_gpu_noise.py)."""
    _fields_ = [("mode", ctypes.c_int), ("where", ctypes.c_int),
                ("counter", ctypes.c_uint32 * 4), ("key", ctypes.c_uint32 * 2),
                ("count", ctypes.c_int64),
                ("words", ctypes.c_void_p), ("bits", ctypes.c_void_p), ("normals", ctypes.c_void_p)]


# symbol name -> (restype, argtypes); must match include/zipvoice_hip.h
_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
SIGNATURES = {
    "zv_last_error": (ctypes.c_char_p, []),
    "zv_version": (ctypes.c_char_p, []),
    "zv_create": (_P, [ctypes.POINTER(ZvConfig)]),
    "zv_destroy": (None, [_P]),
    "zv_set_weight": (_I, [_P, ctypes.c_char_p, _P, ctypes.c_int64]),
    "zv_finalize": (_I, [_P]),
    "zv_reserve": (_I, [_P, _I, _I]),
    "zv_device_bytes": (ctypes.c_int64, [_P]),
    "zv_set_padding": (_I, [_P, _I]),
    "zv_get_padding": (_I, [_P]),
    "zv_profile": (_I, [_I]),
    "zv_bench_gemm": (_I, [_I, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_float)]),
    "zv_bench_fused_linear": (_I, [_I, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_float)]),
    "zv_gemm_selftest": (_I, [_I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "zv_linear_check": (_I, [ctypes.POINTER(ZvLinearCheckArgs)]),
    "zv_ffn_check": (_I, [ctypes.POINTER(ZvFfnCheckArgs)]),
    "zv_dwconv_check": (_I, [ctypes.POINTER(ZvDwconvCheckArgs)]),
    "zv_stackedge_check": (_I, [ctypes.POINTER(ZvStackedgeCheckArgs)]),
    "zv_padrow_check": (_I, [ctypes.POINTER(ZvPadrowCheckArgs)]),
    "zv_bigvgan_check": (_I, [ctypes.POINTER(ZvBigvganCheckArgs)]),
    "zv_solve_check": (_I, [ctypes.POINTER(ZvSolveCheckArgs)]),
    "zv_time_steps": (_I, [_F, _F, _I, _F, _P]),
    "zv_cfg_plan": (_I, [_F, _F, _I, _I, _I, _P, _P, _P, _P]),
    "zv_profile_report": (_I, [ctypes.c_char_p, _I]),
    "zv_host_block_count": (ctypes.c_int64, []),
    "zv_attn_fallbacks": (_I, [_P, _I, _P]),
    "zv_attn2_check": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P]),
    "zv_attn2_check_stale": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _F, _P, _P]),
    "zv_attn_check": (_I, [ctypes.POINTER(ZvAttnCheckArgs)]),
    "zv_attn_plan": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "zv_mx8_quantize": (_I, [_P, _I, _I, _P, _P]),
    "zv_mx8_gemm_check": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "zv_fm_decoder": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "zv_velocity": (_I, [_P, _F, _F, _P, _P, _P, _P, _I, _I, _P, _P]),
    "zv_euler_sample": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P]),
    "zv_velocity_rows": (_I, [_P, _F, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "zv_euler_sample_rows": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _F, _F, _F, _P]),
    "zv_euler_sample_sched": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "zv_sched_stats": (_I, [_P, _P]),
    "zv_sched_plan": (_I, [_P, _I, _I, _I, ctypes.POINTER(ZvSchedPlanOut)]),
    "zv_sched_check": (_I, [ctypes.POINTER(ZvSchedCheckArgs)]),
    # solve session (HipEngine.open_session, SolveSession)
    "zv_session_create": (_P, [_P, _I, _I]),
    "zv_session_destroy": (None, [_P]),
    "zv_session_admit": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "zv_session_step": (_I, [_P, _P]),
    "zv_session_retire": (_I, [_P, _I, _P, _P, _I, _P]),
    "zv_session_state": (_I, [_P, _P, _P]),
    "zv_session_plan": (_I, [_P, _P, _P, _I, _I, ctypes.POINTER(ZvSchedPlanOut), _P]),
    "zv_session_check": (_I, [ctypes.POINTER(ZvSessionCheckArgs)]),
    # edit rows of a session (SolveSession.admit_edit / retire_edit)
    "zv_session_admit_edit": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "zv_session_retire_edit": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P]),
    "zv_session_edit_check": (_I, [ctypes.POINTER(ZvSessionEditCheckArgs)]),
    "zv_text_encode": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "zv_text_condition": (_I, [_P, _P, _I, _I, _P, _P, _I, _P, _P]),
    "zv_speech_condition": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _P]),
    # vocoder (zipvoice_amd/vocoder.py)
    "zv_vocoder_create": (_P, [_P]),
    "zv_vocoder_destroy": (None, [_P]),
    "zv_vocoder_set_weight": (_I, [_P, ctypes.c_char_p, _P, ctypes.c_int64]),
    "zv_vocoder_finalize": (_I, [_P]),
    "zv_vocoder_decode": (_I, [_P, _P, _I, _F, _F, _P, _I, _I, _P, _I, _P]),
    "zv_vocoder_device_bytes": (ctypes.c_int64, [_P]),
    "zv_bigvgan_create": (_P, [_P]),
    "zv_bigvgan_destroy": (None, [_P]),
    "zv_bigvgan_set_weight": (_I, [_P, ctypes.c_char_p, _P, ctypes.c_int64]),
    "zv_bigvgan_finalize": (_I, [_P]),
    "zv_bigvgan_decode": (_I, [_P, _P, _I, _F, _F, _P, _I, _I, _P, _P]),
    "zv_bigvgan_device_bytes": (ctypes.c_int64, [_P]),
    # prompt feature extractor (zipvoice_amd/feature.py)
    "zv_fbank_create": (_P, [_I, _I, _I, _P, _P]),
    "zv_fbank_destroy": (None, [_P]),
    "zv_fbank_extract": (_I, [_P, _P, ctypes.c_int64, _P, _I, _I, _P, ctypes.c_int64, _P]),
    "zv_fbank_configure": (_I, [_P, _I, _F, _F]),
    # prompt resampler (zipvoice_amd/feature.py Resample)
    "zv_resample_create": (_P, [_I, _I, _I, _P, _P]),
    "zv_resample_destroy": (None, [_P]),
    "zv_resample_apply": (_I, [_P, _P, ctypes.c_int64, _P, _I, _P, ctypes.c_int64, ctypes.c_int64, _P]),
    "zv_resample_device_bytes": (ctypes.c_int64, [_P]),
    # long-form trim and join (zipvoice_amd/longform.py WavJoiner)
    "zv_wavjoin_create": (_P, [_I, _F, _I, _I, _I]),
    "zv_wavjoin_destroy": (None, [_P]),
    "zv_wavjoin_apply": (_I, [_P, _P, ctypes.c_int64, _P, _P, _I, _I, _P, ctypes.c_int64,
                              ctypes.c_int64, _P, _P, _P]),
    "zv_wavjoin_apply_docs": (_I, [_P, _P, ctypes.c_int64, _P, _P, _I, _I, _P, _I, _P,
                                   ctypes.c_int64, ctypes.c_int64, _P, _P, _P]),
    "zv_wavjoin_device_bytes": (ctypes.c_int64, [_P]),
    # the stateful join (zipvoice_amd/longform.py WavJoinStream)
    "zv_wavjoin_stream_create": (_P, [_P, _I, _I]),
    "zv_wavjoin_stream_destroy": (None, [_P]),
    "zv_wavjoin_stream_reset": (_I, [_P, _I, _P]),
    "zv_wavjoin_stream_push": (_I, [_P, _P, ctypes.c_int64, _P, _P, _I, _P, _P, _P, ctypes.c_int64,
                                    ctypes.c_int64, _P, _P, _P]),
    "zv_wavjoin_stream_device_bytes": (ctypes.c_int64, [_P]),
    # speech editing (zipvoice_amd/edit.py, HipEngine.edit_gather / edit_splice)
    "zv_edit_create": (_P, []),
    "zv_edit_destroy": (None, [_P]),
    "zv_edit_device_bytes": (ctypes.c_int64, [_P]),
    "zv_edit_gather": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "zv_edit_splice": (_I, [_P, _P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _I, _I, _P, _P, _P, _I,
                            _P, ctypes.c_int64, ctypes.c_int64, _P]),
    # voice store (zipvoice_amd/voices.py)
    "zv_prompt_rms": (_I, [_P, ctypes.c_int64, _P, _P, _I, _F, _P, _P, _P, _P]),
    "zv_prompt_scale": (_I, [_P, ctypes.c_int64, _P, _P, _P, _I, _F, _P, _P]),
    "zv_voice_create": (_P, []),
    "zv_voice_destroy": (None, [_P]),
    "zv_voice_device_bytes": (ctypes.c_int64, [_P]),
    "zv_voice_gather": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P]),
    # seeded noise (zipvoice_amd/noise.py)
    "zv_noise_normal": (_I, [_P, _P, _I, ctypes.c_int64, ctypes.c_int64, _P, _P]),
    "zv_noise_check": (_I, [ctypes.POINTER(ZvNoiseCheckArgs)]),
}

_libs: Dict[str, ctypes.CDLL] = {}
_lib = None            # the main (bf16-operand) library


def load_library(path: Optional[str] = None, operand: str = "bf16"):
    """dlopen the engine (fails loudly when it has not been built).  operand "f16" loads the
    fp16-operand build.  ZV_LIB_PATH selects an alternative build of the main library (A/B
    measurements), ZV_LIB_F16_PATH one of the fp16-operand library.  Both are loaded RTLD_LOCAL (and linked -Bsymbolic): the two libraries
    export the same entry points and each binds its own."""
    global _lib
    if path is None:
        path = ((os.environ.get("ZV_LIB_F16_PATH") or LIB_F16_PATH) if operand == "f16"
                else (os.environ.get("ZV_LIB_PATH") or LIB_PATH))
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{os.path.basename(path)} not found at {path}: build it with "
            "`python zipvoice_amd/csrc/build.py` (or __graft_entry__.build()). "
            "There is no CPU fallback for the ZipVoice hot path.")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in SIGNATURES.items():
        if path not in (LIB_PATH, LIB_F16_PATH) and not hasattr(lib, name):
            continue        # an older A/B build without this entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _libs[path] = lib
    if operand != "f16" and _lib is None:
        _lib = lib
    return lib


def _check(rc: int, lib=None):
    if rc != 0:
        msg = (lib or _lib).zv_last_error().decode()
        if "missing weight" in msg or "expected" in msg or "unexpected" in msg:
            raise KeyError(msg)
        raise RuntimeError(f"zipvoice_hip: {msg}")


def make_zv_config(cfg: ModelConfig, precision: str) -> ZvConfig:
    c = ZvConfig()
    c.variant = VARIANT_ID[cfg.variant]
    c.precision = MODES[precision][1]
    c.feat_dim = cfg.feat_dim
    n = len(cfg.fm_decoder_downsampling_factor)
    if n > MAX_STACKS:
        raise ValueError(f"at most {MAX_STACKS} decoder stacks supported")
    c.num_stacks = n
    for i in range(n):
        c.downsampling_factor[i] = cfg.fm_decoder_downsampling_factor[i]
        c.num_layers[i] = cfg.fm_decoder_num_layers[i]
        c.cnn_module_kernel[i] = cfg.fm_decoder_cnn_module_kernel[i]
    for f in ("fm_decoder_dim", "fm_decoder_feedforward_dim", "fm_decoder_num_heads",
              "text_encoder_num_layers", "text_encoder_feedforward_dim",
              "text_encoder_cnn_module_kernel", "text_encoder_num_heads", "text_encoder_dim",
              "time_embed_dim", "text_embed_dim", "query_head_dim", "value_head_dim",
              "pos_head_dim", "pos_dim", "vocab_size", "pad_id", "spk_a_id", "spk_b_id"):
        setattr(c, f, int(getattr(cfg, f)))
    return c


def profile(enable: bool, detail: bool = False):
    """Enable/disable (and clear) the engine's per-launch event profiler (in every loaded
    engine library); ``detail`` keys the GEMM records by shape."""
    load_library()
    for lib in list(_libs.values()):
        _check(lib.zv_profile((2 if detail else 1) if enable else 0), lib)


def host_block_count() -> int:
    """Host-blocking HIP runtime calls issued so far, summed over the loaded engine libraries
    (zv_host_block_count: allocations, synchronous copies, synchronisations, ...)."""
    load_library()
    return sum(int(lib.zv_host_block_count()) for lib in list(_libs.values()))


def profile_report() -> dict:
    """{tag: {launches, flops, bytes, ms}} merged over the loaded engine libraries."""
    import json
    load_library()
    rep: dict = {}
    for lib in list(_libs.values()):
        buf = ctypes.create_string_buffer(1 << 20)
        _check(lib.zv_profile_report(buf, len(buf)), lib)
        for k, v in json.loads(buf.value.decode()).items():
            if k in rep:
                for f in ("launches", "flops", "bytes", "ms"):
                    rep[k][f] += v[f]
            else:
                rep[k] = v
    return rep


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# zv_padding
PADDING_MODES = ("batch", "row")


def padding_id(mode) -> int:
    """The zv_padding value of a mode name; any other value is a ValueError."""
    if not isinstance(mode, str) or mode not in PADDING_MODES:
        raise ValueError(f"padding must be one of {list(PADDING_MODES)}, got {mode!r}")
    return PADDING_MODES.index(mode)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class HipEngine:
    """One engine per GPU per process: device weights + workspace."""

    def __init__(self, cfg: ModelConfig, state_dict: Dict[str, np.ndarray],
                 precision: str = "fp32", device: Optional[torch.device] = None):
        if precision not in MODES:
            raise ValueError(f"precision must be one of {list(MODES)}")
        if not torch.cuda.is_available():
            raise RuntimeError("zipvoice_amd needs a ROCm GPU (MI355X); no CPU fallback exists")
        operand, self.mode_id = MODES[precision]
        load_library()                       # the main library (error strings, profiler)
        self.lib = load_library(operand=operand)
        self.cfg = cfg
        self.precision = precision
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        check_state_dict(cfg, state_dict)
        with torch.cuda.device(self.device):
            zc = make_zv_config(cfg, precision)
            self.h = self.lib.zv_create(ctypes.byref(zc))
            if not self.h:
                raise RuntimeError(self.lib.zv_last_error().decode())
            for k, v in state_dict.items():
                a = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
                self._check(self.lib.zv_set_weight(self.h, k.encode(), a.ctypes.data_as(ctypes.c_void_p),
                                              a.size))
            self._check(self.lib.zv_finalize(self.h))

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            e = getattr(self, "_edit", None)
            if e:
                self.lib.zv_edit_destroy(e)
                self._edit = None
            self.lib.zv_destroy(h)
            self.h = None

    def _check(self, rc: int):
        _check(rc, self.lib)

    # ------------------------------------------------------------------ checks
    def _f32(self, t: torch.Tensor, name: str, shape=None) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.device != self.device:
            t = t.to(self.device)
        t = t.to(torch.float32).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _mask(self, m: Optional[torch.Tensor], shape) -> Optional[torch.Tensor]:
        if m is None:
            return None
        m = m.to(self.device)
        if tuple(m.shape) != tuple(shape):
            raise ValueError(f"padding_mask: expected shape {tuple(shape)}, got {tuple(m.shape)}")
        return m.to(torch.uint8).contiguous()

    def device_bytes(self) -> int:
        return int(self.lib.zv_device_bytes(self.h))

    @property
    def padding(self) -> str:
        """The decoder's padding mode (zv_get_padding / zv_set_padding): "batch" (default) pads a
        downsampled stack's last group of frames from the padded batch tensor, as the reference does
        on a batch; "row" pads every row with its own last frame, as the reference does on the row
        alone, so a row's valid frames do not depend on its company or on what lies past its end.
        Engine-wide; setting it raises while a solve session of the engine has an occupied slot."""
        return PADDING_MODES[int(self.lib.zv_get_padding(self.h))]

    @padding.setter
    def padding(self, mode: str) -> None:
        self._check(self.lib.zv_set_padding(self.h, padding_id(mode)))

    def attn_fallbacks(self, reset: bool = False) -> tuple:
        """(low, high, total) exact-path runs of the second-generation attention consumers since
        the last reset (zv_attn_fallbacks; synchronises the device)."""
        c = (ctypes.c_int64 * 3)()
        with torch.cuda.device(self.device):
            self._check(self.lib.zv_attn_fallbacks(self.h, int(reset), ctypes.cast(c, ctypes.c_void_p)))
        return int(c[0]), int(c[1]), int(c[2])

    # ------------------------------------------------------------------ ops
    def fm_decoder(self, t: torch.Tensor, xt, text_c, speech_c, padding_mask=None,
                   guidance: Optional[torch.Tensor] = None) -> torch.Tensor:
        N, T, Fx = xt.shape
        xt = self._f32(xt, "xt")
        text_c = self._f32(text_c, "text_condition", (N, T, self.cfg.feat_dim))
        speech_c = self._f32(speech_c, "speech_condition", (N, T, Fx))
        t = self._f32(t.reshape(-1).expand(N) if t.numel() == 1 else t.reshape(N), "t")
        g = None
        if guidance is not None:
            g = self._f32(guidance.reshape(-1).expand(N) if guidance.numel() == 1
                          else guidance.reshape(N), "guidance_scale")
        pm = self._mask(padding_mask, (N, T))
        if self.cfg.stereo:
            out_w = self.cfg.decoder_out_dims()[0 if 2 * Fx + self.cfg.feat_dim ==
                                                self.cfg.decoder_in_dims()[0] else 1]
        else:
            out_w = self.cfg.feat_dim
        v = torch.empty((N, T, out_w), dtype=torch.float32, device=self.device)
        self._check(self.lib.zv_fm_decoder(self.h, _ptr(t), _ptr(g), _ptr(xt), _ptr(text_c),
                                      _ptr(speech_c), _ptr(pm), N, T, Fx, _ptr(v), _stream()))
        return v

    def _guidance_rows(self, guidance_scale, B: int) -> Optional[torch.Tensor]:
        """None for a scalar guidance scale; else the (B,) fp32 device vector of a
        per-utterance guidance tensor ((batch, 1, 1) in the reference, solver.py:61-62)."""
        if not torch.is_tensor(guidance_scale) or guidance_scale.numel() == 1:
            return None
        if guidance_scale.numel() != B:
            raise ValueError(f"guidance_scale: expected 1 or {B} values (shape (batch, 1, 1)), "
                             f"got shape {tuple(guidance_scale.shape)}")
        return guidance_scale.reshape(B).to(self.device, torch.float32).contiguous()

    def velocity(self, t: float, guidance_scale, x, text_c, speech_c,
                 padding_mask=None) -> torch.Tensor:
        B, T, Fx = x.shape
        x = self._f32(x, "x")
        text_c = self._f32(text_c, "text_condition", (B, T, self.cfg.feat_dim))
        speech_c = self._f32(speech_c, "speech_condition", (B, T, Fx))
        pm = self._mask(padding_mask, (B, T))
        v = torch.empty_like(x)
        gr = self._guidance_rows(guidance_scale, B)
        if gr is not None:
            self._check(self.lib.zv_velocity_rows(self.h, float(t), _ptr(gr), _ptr(x), _ptr(text_c),
                                             _ptr(speech_c), _ptr(pm), B, T, _ptr(v), _stream()))
        else:
            self._check(self.lib.zv_velocity(self.h, float(t), float(guidance_scale), _ptr(x),
                                        _ptr(text_c), _ptr(speech_c), _ptr(pm), B, T, _ptr(v),
                                        _stream()))
        return v

    def euler_sample(self, x0, text_c, speech_c, padding_mask, num_step: int,
                     guidance_scale, t_start=0.0, t_end=1.0, t_shift=1.0) -> torch.Tensor:
        B, T, Fx = x0.shape
        x = self._f32(x0, "x").clone()
        text_c = self._f32(text_c, "text_condition", (B, T, self.cfg.feat_dim))
        speech_c = self._f32(speech_c, "speech_condition", (B, T, Fx))
        pm = self._mask(padding_mask, (B, T))
        gr = self._guidance_rows(guidance_scale, B)
        if gr is not None:
            self._check(self.lib.zv_euler_sample_rows(self.h, _ptr(x), _ptr(text_c), _ptr(speech_c),
                                                 _ptr(pm), B, T, int(num_step), _ptr(gr),
                                                 float(t_start), float(t_end), float(t_shift),
                                                 _stream()))
        else:
            self._check(self.lib.zv_euler_sample(self.h, _ptr(x), _ptr(text_c), _ptr(speech_c),
                                            _ptr(pm), B, T, int(num_step), float(guidance_scale),
                                            float(t_start), float(t_end), float(t_shift),
                                            _stream()))
        return x

    def euler_sample_sched(self, x0, text_c, speech_c, padding_mask, schedule) -> torch.Tensor:
        """One solve over rows with their own step counts, grids and guidance scales
        (zv_euler_sample_sched): ``schedule`` holds one row per batch row (solver.RowSchedule, or
        (num_step, t_start, t_end, t_shift, guidance_scale) tuples).  Queued on the current stream;
        the schedule is read on the host before the call returns."""
        B, T, Fx = x0.shape
        if len(schedule) != B:
            raise ValueError(f"schedule: expected {B} rows, got {len(schedule)}")
        x = self._f32(x0, "x").clone()
        text_c = self._f32(text_c, "text_condition", (B, T, self.cfg.feat_dim))
        speech_c = self._f32(speech_c, "speech_condition", (B, T, Fx))
        pm = self._mask(padding_mask, (B, T))
        rows = row_schedule_array(schedule)
        rc = self.lib.zv_euler_sample_sched(self.h, _ptr(x), _ptr(text_c), _ptr(speech_c), _ptr(pm), B, T,
                                            ctypes.cast(rows, ctypes.c_void_p), _stream())
        if rc != 0 and "scheduled solve:" in self.lib.zv_last_error().decode():
            raise ValueError(self.lib.zv_last_error().decode())
        self._check(rc)
        return x

    def sched_stats(self) -> tuple:
        """(decoder rows launched, steps run) of this engine's last scheduled solve (zv_sched_stats)."""
        c = (ctypes.c_int64 * 2)()
        self._check(self.lib.zv_sched_stats(self.h, ctypes.cast(c, ctypes.c_void_p)))
        return int(c[0]), int(c[1])

    def open_session(self, slots: int, max_frames: int) -> "SolveSession":
        """A solve session of ``slots`` rows of up to ``max_frames`` frames on this engine
        (zv_session_create): continuous batching, rows admitted and retired between steps."""
        return SolveSession(self, slots, max_frames)

    # ------------------------------------------------------------------ speech editing
    def _edit_handle(self):
        """The engine's zv_edit handle (device table + pinned staging), made on first use."""
        if not getattr(self, "_edit", None):
            with torch.cuda.device(self.device):
                self._edit = self.lib.zv_edit_create()
            if not self._edit:
                raise RuntimeError(self.lib.zv_last_error().decode())
        return self._edit

    def _edit_check(self, rc: int):
        if rc != 0 and "edit table:" in self.lib.zv_last_error().decode():
            raise ValueError(self.lib.zv_last_error().decode())
        self._check(rc)

    @staticmethod
    def _host_i32(a, shape, name: str) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.int32))
        if a.shape != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {a.shape}")
        return a

    def edit_device_bytes(self) -> int:
        return int(self.lib.zv_edit_device_bytes(self._edit_handle()))

    def edit_gather(self, feat: torch.Tensor, lens, table, row_ptr, T: int,
                    fill: Optional[torch.Tensor] = None):
        """zv_edit_gather: ``feat`` (B, Lmax, F) with ``lens`` (B,) original frame counts and a
        frame table (edit.plan_edit_batch: ``table`` (n, 3) rows (dst, src, len), ``row_ptr``
        (B + 1,), host arrays) -> (out (B, T, F), mask (B, T) bool, True on generated frames).
        Kept frames are copied from ``feat``, generated ones from ``fill`` (B, T, F) or zero, frames
        past a row's new length are zero.  A bad table is a ValueError and launches nothing."""
        feat = self._f32(feat, "feat")
        B, Lmax, F = feat.shape
        lens = self._host_i32(lens, (B,), "lens")
        row_ptr = self._host_i32(row_ptr, (B + 1,), "row_ptr")
        table = self._host_i32(np.asarray(table).reshape(-1, 3), (max(int(row_ptr[-1]), 0), 3), "table")
        if fill is not None:
            fill = self._f32(fill, "fill", (B, T, F))
        out = torch.empty((B, int(T), F), dtype=torch.float32, device=self.device)
        mask = torch.empty((B, int(T)), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._edit_check(self.lib.zv_edit_gather(
                self._edit_handle(), _ptr(feat), B, Lmax, F, lens.ctypes.data, _ptr(fill),
                table.ctypes.data, row_ptr.ctypes.data, int(T), _ptr(out), _ptr(mask), _stream()))
        return out, mask.bool()

    def edit_splice(self, orig: torch.Tensor, lens, gen: torch.Tensor, gen_lens, table, row_ptr,
                    gains=None, fade: int = 240, out_cols: Optional[int] = None) -> torch.Tensor:
        """zv_edit_splice: ``orig`` (B, C, n) with ``lens`` (B,) true sample counts, ``gen``
        (B, C, m) with ``gen_lens`` valid samples and a sample table (edit.sample_table_batch:
        ``table`` (n, 4) rows (out, src, len, kind), ``row_ptr``) -> (B, C, out_cols): the table's
        gather with a linear cross-fade of up to ``fade`` samples to either side of every
        junction; ``gains`` (B,) host floats scale the generated samples.  Zero past a row's length;
        out_cols defaults to the longest row."""
        if orig.dim() == 2:
            orig, gen = orig.unsqueeze(1), gen.unsqueeze(1)
        orig, gen = self._f32(orig, "orig"), self._f32(gen, "gen")
        B, C, n = orig.shape
        if gen.dim() != 3 or gen.shape[:2] != (B, C):
            raise ValueError(f"gen: expected ({B}, {C}, m), got {tuple(gen.shape)}")
        lens = self._host_i32(lens, (B,), "lens")
        gen_lens = self._host_i32(gen_lens, (B,), "gen_lens")
        row_ptr = self._host_i32(row_ptr, (B + 1,), "row_ptr")
        table = self._host_i32(np.asarray(table).reshape(-1, 4), (max(int(row_ptr[-1]), 0), 4), "table")
        g = np.ones(B, np.float32) if gains is None else np.ascontiguousarray(np.asarray(gains, np.float32))
        if g.shape != (B,):
            raise ValueError("gains must have shape (B,)")
        if out_cols is None:
            ends = [int(table[row_ptr[b + 1] - 1, 0] + table[row_ptr[b + 1] - 1, 2])
                    for b in range(B) if row_ptr[b + 1] > row_ptr[b]]
            out_cols = max(ends + [1])
        out = torch.empty((B, C, int(out_cols)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._edit_check(self.lib.zv_edit_splice(
                self._edit_handle(), _ptr(orig), n, lens.ctypes.data, _ptr(gen), gen.shape[2],
                gen_lens.ctypes.data, B, C, table.ctypes.data, row_ptr.ctypes.data, g.ctypes.data,
                int(fade), _ptr(out), int(out_cols), int(out_cols), _stream()))
        return out

    def reserve(self, max_batch: int, max_frames: int) -> None:
        """Pre-size the decoder workspace (zv_reserve)."""
        self._check(self.lib.zv_reserve(self.h, int(max_batch), int(max_frames)))

    def text_encode(self, tokens: torch.Tensor, padding_mask: torch.Tensor,
                    spk: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, S = tokens.shape
        tokens = tokens.to(self.device, torch.int64).contiguous()
        pm = self._mask(padding_mask, (B, S))
        if spk is not None:
            spk = spk.to(self.device, torch.int8).contiguous()
        out = torch.empty((B, S, self.cfg.feat_dim), dtype=torch.float32, device=self.device)
        self._check(self.lib.zv_text_encode(self.h, _ptr(tokens), _ptr(pm), _ptr(spk), B, S, _ptr(out),
                                       _stream()))
        return out

    def text_condition(self, embed, tokens_lens, features_lens, num_frames: int):
        B, S, C = embed.shape
        embed = self._f32(embed, "embed")
        tl = tokens_lens.to(self.device, torch.int32).contiguous()
        fl = features_lens.to(self.device, torch.int32).contiguous()
        out = torch.empty((B, num_frames, C), dtype=torch.float32, device=self.device)
        self._check(self.lib.zv_text_condition(self.h, _ptr(embed), B, S, _ptr(tl), _ptr(fl),
                                          int(num_frames), _ptr(out), _stream()))
        return out

    def speech_condition(self, prompt_features, prompt_lens, num_frames: int):
        B, Tp, F = prompt_features.shape
        pf = self._f32(prompt_features, "prompt_features")
        pl = prompt_lens.to(self.device, torch.int32).contiguous()
        out = torch.empty((B, num_frames, F), dtype=torch.float32, device=self.device)
        self._check(self.lib.zv_speech_condition(self.h, _ptr(pf), B, Tp, F, _ptr(pl), int(num_frames),
                                            _ptr(out), _stream()))
        return out


class SolveSession:
    """Continuous batching on one engine (zv_session_*): ``slots`` row slots of ``max_frames`` frames
    that live across calls.  Between any two decoder steps finished rows are retired and waiting rows
    admitted into the free slots; every row integrates its own grid from its own step 0 and ends as
    ``EulerSolver.sample`` would leave it when run on that row alone.  All calls are queued on the
    current stream; slot numbers, lengths and schedules are host values, and the host knows which rows
    finish from the schedules alone (``steps_left``), so a warm admit / step / retire neither blocks
    the host nor reads from the device.  The engine must outlive the session."""

    def __init__(self, eng: "HipEngine", slots: int, max_frames: int):
        self.eng, self.lib, self.device = eng, eng.lib, eng.device
        self.slots, self.max_frames = int(slots), int(max_frames)
        self.Fx = (2 if eng.cfg.stereo else 1) * eng.cfg.feat_dim
        self._lens = [0] * self.slots
        self.h = None
        with torch.cuda.device(self.device):
            self.h = self.lib.zv_session_create(eng.h, self.slots, self.max_frames)
        if not self.h:
            msg = self.lib.zv_last_error().decode()
            raise ValueError(msg) if "session: " in msg else RuntimeError(f"zipvoice_hip: {msg}")

    def close(self) -> None:
        h = getattr(self, "h", None)
        if h:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            self.lib.zv_session_destroy(h)
            self.h = None

    __del__ = close

    def _check(self, rc: int):
        if rc != 0 and "session: " in self.lib.zv_last_error().decode():
            raise ValueError(self.lib.zv_last_error().decode())
        _check(rc, self.lib)

    def _handle(self):
        if not self.h:
            raise RuntimeError("the solve session is closed")
        return self.h

    def admit(self, slots, x0, text_c, speech_c, lens, schedule) -> None:
        """Row i of ``x0`` / ``speech_c`` (n, T_in, Fx) and ``text_c`` (n, T_in, feat_dim) goes into the
        free slot ``slots[i]`` with ``lens[i]`` valid frames and the settings ``schedule[i]``
        (solver.RowSchedule or a 5-tuple, as ``euler_sample_sched``).  A bad request is a ValueError
        and changes nothing."""
        n, T_in, _ = x0.shape
        if not (len(slots) == len(lens) == len(schedule) == n):
            raise ValueError(f"admit: expected {n} slots, lens and schedule rows, got {len(slots)}, {len(lens)}, "
                             f"{len(schedule)}")
        x0 = self.eng._f32(x0, "x0", (n, T_in, self.Fx))
        text_c = self.eng._f32(text_c, "text_condition", (n, T_in, self.eng.cfg.feat_dim))
        speech_c = self.eng._f32(speech_c, "speech_condition", (n, T_in, self.Fx))
        sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
        ln = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
        rows = row_schedule_array(list(schedule))
        with torch.cuda.device(self.device):
            self._check(self.lib.zv_session_admit(self._handle(), n, sl.ctypes.data, ln.ctypes.data,
                                                  ctypes.cast(rows, ctypes.c_void_p), _ptr(x0), _ptr(text_c),
                                                  _ptr(speech_c), T_in, _stream()))
        for s, l in zip(sl.tolist(), ln.tolist()):
            self._lens[s] = l

    def step(self) -> None:
        """One tick: every slot with steps left runs one Euler step at its own step index."""
        with torch.cuda.device(self.device):
            self._check(self.lib.zv_session_step(self._handle(), _stream()))

    def retire(self, slots, T_out: Optional[int] = None) -> torch.Tensor:
        """The finished rows of ``slots`` as (n, T_out, Fx), zero past each row's length (``T_out``
        defaults to the longest of them); the slots are free afterwards."""
        sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
        n = int(sl.size)
        if T_out is None:
            T_out = max([self._lens[s] for s in sl.tolist() if 0 <= s < self.slots] + [1])
        out = torch.empty((n, int(T_out), self.Fx), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.zv_session_retire(self._handle(), n, sl.ctypes.data, _ptr(out), int(T_out),
                                                   _stream()))
        for s in sl.tolist():
            self._lens[s] = 0
        return out

    def _edit_tables(self, slots, pool, offsets, lens, table, row_ptr):
        """The host arrays of an edit request, shaped and typed for the C ABI, and each row's new length."""
        sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        n = int(sl.size)
        if pool.dim() != 2 or pool.shape[1] != self.Fx:
            raise ValueError(f"pool: expected (rows, {self.Fx}), got {tuple(pool.shape)}")
        if pool.dtype != torch.float32 or not pool.is_contiguous() or pool.device != self.device:
            raise ValueError("pool must be a contiguous fp32 tensor on the session's device")
        off = HipEngine._host_i32(offsets, (n,), "offsets")
        ln = HipEngine._host_i32(lens, (n,), "lens")
        rp = HipEngine._host_i32(row_ptr, (n + 1,), "row_ptr")
        tab = HipEngine._host_i32(np.asarray(table).reshape(-1, 3), (max(int(rp[-1]), 0) if n else 0, 3), "table")
        new = [int(tab[rp[i + 1] - 1, 0] + tab[rp[i + 1] - 1, 2]) if 0 <= rp[i] < rp[i + 1] <= len(tab) else 0
               for i in range(n)]
        return sl, off, ln, tab, rp, new

    def admit_edit(self, slots, x0, text_c, pool, offsets, lens, table, row_ptr, schedule) -> None:
        """Rows of a speech edit into free slots, their speech condition straight from ``pool`` (rows, Fx)
        (zv_session_admit_edit): row i's original frames are pool rows ``offsets[i] + [0, lens[i])`` and its
        frame table (``edit.plan_edit_batch``: ``table`` (m, 3) rows (dst, src, len), ``row_ptr`` (n + 1,),
        host arrays) says which of them the new row keeps; ``x0`` (n, T_in, Fx) and ``text_c`` (n, T_in,
        feat_dim) are read up to each row's new length.  A bad request is a ValueError, changes nothing and
        launches nothing."""
        n, T_in, _ = x0.shape
        if not (len(slots) == len(schedule) == n):
            raise ValueError(f"admit_edit: expected {n} slots and schedule rows, got {len(slots)}, {len(schedule)}")
        x0 = self.eng._f32(x0, "x0", (n, T_in, self.Fx))
        text_c = self.eng._f32(text_c, "text_condition", (n, T_in, self.eng.cfg.feat_dim))
        sl, off, ln, tab, rp, new = self._edit_tables(slots, pool, offsets, lens, table, row_ptr)
        rows = row_schedule_array(list(schedule))
        with torch.cuda.device(self.device):
            self._check(self.lib.zv_session_admit_edit(
                self._handle(), n, sl.ctypes.data, ctypes.cast(rows, ctypes.c_void_p), _ptr(x0), _ptr(text_c), T_in,
                _ptr(pool), pool.shape[0], off.ctypes.data, ln.ctypes.data, tab.ctypes.data, rp.ctypes.data,
                _stream()))
        for s, l in zip(sl.tolist(), new):
            self._lens[s] = l

    def retire_edit(self, slots, pool, offsets, lens, table, row_ptr, T_out: Optional[int] = None,
                    keep_original: bool = True):
        """The finished edit rows of ``slots`` (zv_session_retire_edit) -> (x1 (n, T_out, Fx), mask (n, T_out)
        bool): kept frames are the pool's, bitwise, generated ones the solver's (``mask`` True), zero past
        each row's new length; ``keep_original=False`` returns the solver's frames everywhere.  The tables
        are those of the admission.  The slots are free afterwards."""
        sl, off, ln, tab, rp, new = self._edit_tables(slots, pool, offsets, lens, table, row_ptr)
        n = int(sl.size)
        if T_out is None:
            T_out = max(new + [1])
        out = torch.empty((n, int(T_out), self.Fx), dtype=torch.float32, device=self.device)
        mask = torch.empty((n, int(T_out)), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.zv_session_retire_edit(
                self._handle(), n, sl.ctypes.data, _ptr(pool), pool.shape[0], off.ctypes.data, ln.ctypes.data,
                tab.ctypes.data, rp.ctypes.data, int(bool(keep_original)), _ptr(out), _ptr(mask), int(T_out),
                _stream()))
        for s in sl.tolist():
            self._lens[s] = 0
        return out, mask.bool()

    def _state(self):
        left = (ctypes.c_int32 * self.slots)()
        st = (ctypes.c_int64 * 4)()
        self._check(self.lib.zv_session_state(self._handle(), ctypes.cast(left, ctypes.c_void_p),
                                              ctypes.cast(st, ctypes.c_void_p)))
        return list(left), tuple(int(v) for v in st)

    def steps_left(self) -> list:
        """Per slot, the steps it still has to run; -1 for a free slot (host state, no GPU call)."""
        return self._state()[0]

    def stats(self) -> tuple:
        """(ticks run, decoder rows launched, sum over the ticks of decoder rows x T_k, the last tick's T_k)."""
        return self._state()[1]
