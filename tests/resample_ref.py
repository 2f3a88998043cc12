"""Float64 references for torchaudio.transforms.Resample (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99); a helper, not a test.  torchaudio is not installed:
both forms restate ``torchaudio.functional.resample`` (``_get_sinc_resample_kernel`` +
``_apply_sinc_resample_kernel``).  The taps are torchaudio's float32 values; the sums run
in float64, so the references carry no accumulation error of their own.

dense_kernel / resample_dense: the [n, 2 width + o] table and F.conv1d at stride o, as
torchaudio does it.  resample_direct: one output at a time from the tap formula, without
ever building the dense table (usable for near-coprime rates)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

LW = 6
ROLLOFF = 0.99


def reduced(orig, new):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * ROLLOFF
    return o, n, base, math.ceil(LW * o / base)


def _taps(t):
    """float64 t (already scaled by base, unclamped) -> torchaudio's float64 kernel values
    without the base / o scale."""
    t = t.clamp(-LW, LW)
    window = torch.cos(t * math.pi / LW / 2) ** 2
    t = t * math.pi
    return torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window


def dense_t(orig, new):
    """The dense table's unclamped argument t[j, k], float64."""
    o, n, base, width = reduced(orig, new)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx
    return t * base


def dense_kernel(orig, new):
    """torchaudio's kernel [n, 2 width + o], float32."""
    o, n, base, width = reduced(orig, new)
    return (_taps(dense_t(orig, new)) * (base / o)).to(torch.float32)


def out_len(orig, new, length):
    o, n, _, _ = reduced(orig, new)
    return int(math.ceil(n * length / o))


def resample_dense(x, orig, new):
    """x (L,) -> float64 (ceil(n L / o),) by the padded strided convolution."""
    o, n, base, width = reduced(orig, new)
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    L = x.numel()
    k = dense_kernel(orig, new).to(torch.float64)
    xp = F.pad(x[None, None], (width, width + o))
    y = F.conv1d(xp, k[:, None], stride=o)                    # (1, n, blocks)
    return y.transpose(1, 2).reshape(-1)[:out_len(orig, new, L)].numpy()


def resample_direct(x, orig, new, return_abs_sum=False):
    """x (L,) -> float64 (ceil(n L / o),): output y = i n + j sums the taps of phase j over
    the samples i o + m with |(m / o - j / n) base| < LW, evaluated per output.  With
    return_abs_sum also max_j sum_k |K[j, k]| (the filter's l1 gain, for error bounds)."""
    o, n, base, width = reduced(orig, new)
    x = np.asarray(x, np.float64)
    L = x.shape[0]
    half = LW * o / base
    nt = 2 * int(math.ceil(half)) + 3
    ny = out_len(orig, new, L)
    y = np.zeros(ny)
    xt = torch.from_numpy(np.concatenate([x, np.zeros(1)]))   # index L reads 0
    gain = 0.0
    step = 1 << 16
    for y0 in range(0, ny, step):
        yy = torch.arange(y0, min(y0 + step, ny), dtype=torch.int64)
        i, j = yy // n, yy % n
        m = torch.floor(j.double() * o / n - half).long()[:, None] - 1 + torch.arange(nt)[None]
        t = (-j.double()[:, None] / n + m.double() / o) * base
        k = (_taps(t) * (base / o)).to(torch.float32).double()
        k = torch.where(t.abs() < LW, k, torch.zeros_like(k))
        g = i[:, None] * o + m
        ok = (g >= 0) & (g < L)
        xs = xt[torch.where(ok, g, torch.full_like(g, L))]
        y[y0:y0 + len(yy)] = (k * xs).sum(1).numpy()
        gain = max(gain, float(k.abs().sum(1).max()))
    return (y, gain) if return_abs_sum else y
