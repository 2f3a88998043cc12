"""Seeded initial noise: standard normals keyed per request, drawn on the device.

The reference takes one global ``--seed`` (``infer_zipvoice.py:240``, ``fix_random_seed``)
and speaks one sentence per call; this engine batches, pools and shards requests, so a
request's noise is keyed by the request instead: element e of a row is a pure function of
(seed, stream, e) (``zv_noise_normal``, definition in include/zipvoice_hip.h; Philox4x32-10
and Box-Muller).  A row's values do not depend on the batch size, on its position in the
batch, on the longest row or on the row stride, so ``model.sample(seeds=...)`` starts a
request from the same noise whatever it is batched with.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as _eng
from .common import to_device


def _ints(values, what: str, bits: int) -> List[int]:
    """A non-empty sequence of ints in [0, 2^bits) as a list (ValueError otherwise)."""
    if isinstance(values, (str, bytes)) or torch.is_tensor(values) or isinstance(values, np.ndarray):
        raise ValueError(f"{what} must be a sequence of Python ints")
    try:
        values = list(values)
    except TypeError:
        raise ValueError(f"{what} must be a sequence of Python ints") from None
    if not values:
        raise ValueError(f"{what} must not be empty")
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what} must be Python ints, got {type(v).__name__}")
        if not 0 <= int(v) < (1 << bits):
            raise ValueError(f"{what} must lie in [0, 2^{bits}), got {v}")
    return [int(v) for v in values]


def check_keys(seeds, streams=None, rows: Optional[int] = None
               ) -> Tuple[List[int], Optional[List[int]]]:
    """The (seed, stream) keys of ``rows`` rows as host lists, checked: ``seeds`` ints in
    [0, 2^64), one per row; ``streams`` None (all 0) or ints in [0, 2^32), one per seed.
    Raises ValueError; touches no GPU."""
    seeds = _ints(seeds, "seeds", 64)
    if rows is not None and len(seeds) != rows:
        raise ValueError(f"seeds must hold one seed per row ({rows}), got {len(seeds)}")
    if streams is not None:
        streams = _ints(streams, "streams", 32)
        if len(streams) != len(seeds):
            raise ValueError(f"streams must hold one stream per seed ({len(seeds)}), got "
                             f"{len(streams)}")
    return seeds, streams


def check_noise(rows: int, x0=None, seeds=None, streams=None):
    """The checks every entry that takes ``x0`` / ``seeds`` / ``seed_streams`` makes before it touches
    the GPU: ``x0`` or ``seeds``, not both; ``streams`` only with ``seeds``; then ``check_keys``.
    ``seeds`` may hold None for rows without a key.  Returns (seeds, streams) as checked lists."""
    if seeds is not None and x0 is not None:
        raise ValueError("give x0 or seeds, not both")
    if streams is not None and seeds is None:
        raise ValueError("seed_streams needs seeds")
    if seeds is None:
        return None, None
    holes = isinstance(seeds, (list, tuple)) and None in seeds
    keys, streams = check_keys([0 if s is None else s for s in seeds] if holes else seeds, streams, rows)
    return ([None if s is None else k for s, k in zip(seeds, keys)] if holes else keys), streams


def _twos(v: int, bits: int) -> int:
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


@torch.inference_mode()
def seeded_normal_into(out: torch.Tensor, seeds: Sequence[int],
                       streams: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Fill the rows of ``out`` ((B, ...) float32 on the device; every row out[b] contiguous,
    rows may be strided views into a larger buffer) with the noise of (seeds[b], streams[b]):
    one ``zv_noise_normal`` call on the current stream.  Nothing outside the rows is written.
    Returns ``out``."""
    if not torch.is_tensor(out) or out.dim() < 1:
        raise ValueError("out must be a (B, ...) tensor")
    seeds, streams = check_keys(seeds, streams, out.shape[0])
    if out.dtype != torch.float32:
        raise ValueError(f"out must be float32, got {out.dtype}")
    if not out.is_cuda:
        raise RuntimeError("zipvoice_amd seeded noise is drawn on a ROCm GPU; no CPU fallback")
    B = out.shape[0]
    n = out[0].numel()
    ld = out.stride(0) if B > 1 else n
    if (n and not out[0].is_contiguous()) or ld < n:
        raise ValueError("every row of out must be contiguous and rows must not overlap")
    lib = _eng.load_library()
    dev = out.device
    sd = to_device(torch.tensor([_twos(s, 64) for s in seeds], dtype=torch.int64), dev)
    st = None
    if streams is not None:
        st = to_device(torch.tensor([_twos(s, 32) for s in streams], dtype=torch.int32), dev)
    with torch.cuda.device(dev):
        _eng._check(lib.zv_noise_normal(_eng._ptr(sd), _eng._ptr(st), B, n, ld, _eng._ptr(out),
                                        _eng._stream()), lib)
    return out


def seeded_normal(seeds: Sequence[int], shape, streams: Optional[Sequence[int]] = None,
                  device=None) -> torch.Tensor:
    """A (B, *shape) float32 device tensor, B = len(seeds): row b is the noise of
    (seeds[b], streams[b]) (``streams`` None: stream 0), element index in row-major order
    over ``shape``.  ``seeds`` are Python ints in [0, 2^64) (values >= 2^63 cross the C ABI
    as their two's-complement int64), ``streams`` ints in [0, 2^32); anything else raises
    ValueError.  One ``zv_noise_normal`` call on the current stream of ``device`` (default:
    the current GPU)."""
    seeds, streams = check_keys(seeds, streams)
    try:
        shape = tuple(int(v) for v in ((shape,) if isinstance(shape, int) else shape))
    except TypeError:
        raise ValueError("shape must be an int or a sequence of ints") from None
    if any(v < 0 for v in shape):
        raise ValueError(f"shape must be non-negative, got {shape}")
    if not torch.cuda.is_available():
        raise RuntimeError("zipvoice_amd seeded noise is drawn on a ROCm GPU; no CPU fallback")
    dev = torch.device(device if device is not None else "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((len(seeds),) + shape, dtype=torch.float32, device=dev)
    return seeded_normal_into(out, seeds, streams)


def initial_noise(B: int, T: int, F: int, device, x0=None, seeds=None, streams=None) -> torch.Tensor:
    """The (B, T, F) initial noise of a solve, after ``check_noise``: ``x0`` itself (a ValueError at
    another shape); every row keyed: ``seeded_normal``; none keyed: ``torch.randn`` on ``device``, as the
    reference draws it; some keyed (``seeds`` holds None for the others): ``torch.randn`` for the whole
    batch, then each keyed row overwritten in place (no index tensor goes up; a key's noise is its own)."""
    seeds, streams = check_noise(B, x0, seeds, streams)
    if x0 is not None:
        if tuple(x0.shape) != (B, T, F):
            raise ValueError(f"x0 must have shape {(B, T, F)}, got {tuple(x0.shape)}")
        return x0
    keyed = [b for b, s in enumerate(seeds or ()) if s is not None]
    if keyed and len(keyed) == B:
        return seeded_normal(seeds, (T, F), streams, device=device)
    x = torch.randn(B, T, F, device=device)
    for b in keyed:
        seeded_normal_into(x[b:b + 1], [seeds[b]], None if streams is None else [streams[b]])
    return x
