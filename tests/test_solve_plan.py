"""Host-only checks of the solve's two host decisions (no GPU): zv_time_steps, the Euler grid the
engine integrates over, and zv_cfg_plan, the guidance branches of one velocity call.

zv_time_steps must equal oracle.zipvoice_np.get_time_steps (torch.linspace's float32 forward / backward
halves, then the shift) bit for bit, and lie within 16 fp32 ulps of 1 of the float64 formula.  The count
(u = 2^-24; every quantity below is at most 1 in magnitude for the grids tested, and 0.5 <= s <= 1):
  u_i = start + step * i (or end - step * (n - i)), with i (or n - i) <= (n + 1) / 2: step carries the
  roundings of the difference and of the quotient (2 u relative, so at most 2 u |t1 - t0| (n + 1) / (2 n) <=
  2 u on step * i), the product and the sum one rounding each: |du| <= 4 u.
  t = s u / (1 + (s - 1) u): a = fl(s - 1), b = fl(a u), den = fl(1 + b), num = fl(s u), t = fl(num / den).
  |d den| <= |s - 1| (|du| + 2 u) + u <= |du| / 2 + 2 u;  |d num| <= s |du| + u;  den >= s, num / den <= 1, so
  |dt| <= |d num| / den + |d den| / den + u <= |du| (1 + 1 / (2 s)) + 3 u / s + u <= 8 u + 6 u + u = 15 u at s = 0.5.

zv_cfg_plan's expectations are the branches of the oracle's velocity(): g == 0 (or all per-row scales
zero) runs the rows once; otherwise the rows are doubled, the unconditional copy's speech is zeroed
for t > 0.5, else the scale is doubled; distill never doubles."""
import ctypes

import numpy as np
import pytest

from oracle import zipvoice_np as zvo


@pytest.fixture(scope="module")
def lib():
    from zipvoice_amd.csrc.build import build
    build(verbose=False)
    from zipvoice_amd import engine
    return engine.load_library()


@pytest.mark.parametrize("t0,t1", [(0.0, 1.0), (0.25, 0.9)])
@pytest.mark.parametrize("shift", [1.0, 0.5, 0.7])
@pytest.mark.parametrize("num_step", [1, 2, 3, 4, 5, 8, 16, 17])
def test_time_steps(lib, num_step, shift, t0, t1):
    out = np.full(num_step + 2, np.float32(-7.0))
    rc = lib.zv_time_steps(t0, t1, num_step, shift, out.ctypes.data)
    assert rc == 0, lib.zv_last_error()
    assert out[-1] == np.float32(-7.0), "wrote past num_step + 1 values"
    want = zvo.get_time_steps(t0, t1, num_step, shift)
    assert want.dtype == np.float32 and np.array_equal(out[:-1].view(np.uint32), want.view(np.uint32)), (out[:-1], want)
    # the float64 formula, on the fp32 arguments the call received
    a, b, s = (float(np.float32(v)) for v in (t0, t1, shift))
    u = a + (b - a) * np.arange(num_step + 1) / num_step
    exact = s * u / (1.0 + (s - 1.0) * u)
    assert np.abs(out[:-1].astype(np.float64) - exact).max() <= 16 * 2.0 ** -24
    assert out[0] == np.float32(exact[0]) and (np.diff(out[:-1]) > 0).all()


def plan(lib, t, g, has_rows=0, rows_nonzero=0, distill=0):
    copies, zs = ctypes.c_int(-1), ctypes.c_int(-1)
    go, gm = ctypes.c_float(-1), ctypes.c_float(-1)
    rc = lib.zv_cfg_plan(t, g, has_rows, rows_nonzero, distill, ctypes.byref(copies), ctypes.byref(zs),
                         ctypes.byref(go), ctypes.byref(gm))
    assert rc == 0, lib.zv_last_error()
    return copies.value, zs.value, go.value, gm.value


HALF = np.float32(0.5)
T_EDGE = [float(np.nextafter(HALF, np.float32(0))), 0.5, float(np.nextafter(HALF, np.float32(1)))]


def oracle_branch(t, g):
    """What ZipVoiceOracle.velocity does with (t, g): (copies, speech zeroed, the combine's g)."""
    g = np.float32(g)
    if g == 0.0:
        return 1, 0, g
    if float(t) > 0.5:
        return 2, 1, g
    return 2, 0, np.float32(g * np.float32(2.0))


@pytest.mark.parametrize("t", T_EDGE + [0.0, 1.0])
@pytest.mark.parametrize("g", [0.0, 0.7, -0.5, 3.0])
def test_cfg_plan_scalar(lib, t, g):
    copies, zs, go, gm = plan(lib, t, g)
    wc, wz, wg = oracle_branch(np.float32(t), g)
    assert (copies, zs) == (wc, wz)
    assert np.float32(go) == wg
    assert gm == (2.0 if (wc == 2 and not wz) else 1.0)


@pytest.mark.parametrize("t", T_EDGE)
def test_cfg_plan_rows_and_distill(lib, t):
    # per-row scales that are all zero: the unguided branch, whatever the scalar argument says
    assert plan(lib, t, 0.0, has_rows=1, rows_nonzero=0)[:2] == (1, 0)
    assert plan(lib, t, 3.0, has_rows=1, rows_nonzero=0)[:2] == (1, 0)
    # some nonzero: doubled, and the per-row factor follows the t branch (the scalar is not used)
    copies, zs, _, gm = plan(lib, t, 0.0, has_rows=1, rows_nonzero=1)
    assert (copies, zs, gm) == ((2, 1, 1.0) if np.float32(t) > HALF else (2, 0, 2.0))
    # distill: one copy, nothing zeroed, the scale as it is
    for kw in ({}, {"has_rows": 1, "rows_nonzero": 1}):
        assert plan(lib, t, 0.7, distill=1, **kw) == (1, 0, float(np.float32(0.7)), 1.0)
