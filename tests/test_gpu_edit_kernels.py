"""The speech-editing kernels (zv_edit_gather, zv_edit_splice; csrc/zv_edit.inc) through the C
ABI against the numpy restatement tests/edit_ref.py.

Gather: bitwise, with and without fill, at F = 100 / 200 (16-byte form) and F = 6 and a
misaligned F = 100 (scalar form), T one past a multiple of the 16-frame tile, Lmax above and
below T.  Frames of feat past a row's length and samples past a waveform's length are NaN, so a
read outside a row shows in the output.
Splice: samples outside the junction windows are the source's bits (generated ones times the
gain, one fp32 product); inside a window |out - ref| <= 4 * 2^-23 * max(|g_a a|, |g_b b|), the
bound tests/test_gpu_longform.py puts on its cross-faded samples: two products, one add, the
rounding of w, and the compiler's freedom to fuse a product into the add."""
import ctypes

import numpy as np
import pytest

import edit_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from zipvoice_amd import engine  # noqa: E402

CANARY = 12345.0
TILE = 16                      # EG_TILE, csrc/zv_edit.inc
HOP = 256


@pytest.fixture(scope="module")
def lib():
    return engine.load_library()


@pytest.fixture()
def handle(lib):
    h = lib.zv_edit_create()
    assert h
    yield h
    torch.cuda.synchronize()
    lib.zv_edit_destroy(h)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ----------------------------------------------------------------------------- gather
def gather_rows(lens):
    """Three rows: one without spans; one with a span at frame 0, 1-frame kept and generated
    segments, an insertion and a deletion; one with a span ending at L that makes it the longest."""
    l0, l1, l2 = lens
    spans = [[], [(0, 3, 1), (4, 5, 2), (10, 10, 2), (l1 - 14, l1 - 4, 0)], [(l2 - 5, l2, 13)]]
    return [edit_ref.plan(L, sp) for L, sp in zip(lens, spans)]


def run_gather(lib, h, feat, lens, tables, T, fill=None, misalign=False):
    """-> (rc, out (B, T, F), mask (B, T), tail of out, tail of mask); the device buffers carry a
    canary past the last row."""
    B, Lmax, F = feat.shape
    table, ptr = edit_ref.stack(tables, 3)
    lens = np.asarray(lens, np.int32)
    off = 1 if misalign else 0
    fd = torch.empty(feat.size + off, dtype=torch.float32, device="cuda")[off:].copy_(cuda(feat).reshape(-1))
    fl = None if fill is None else cuda(fill)
    out = torch.full((B * T * F + 64 + off,), CANARY, dtype=torch.float32, device="cuda")[off:]
    mask = torch.full((B * T + 64,), 7, dtype=torch.uint8, device="cuda")
    rc = lib.zv_edit_gather(h, fd.data_ptr(), B, Lmax, F, lens.ctypes.data,
                            None if fl is None else fl.data_ptr(), table.ctypes.data,
                            ptr.ctypes.data, T, out.data_ptr(), mask.data_ptr(), stream())
    o, m = out.cpu().numpy(), mask.cpu().numpy()
    return rc, o[:B * T * F].reshape(B, T, F), m[:B * T].reshape(B, T), o[B * T * F:], m[B * T:]


def gather_case(F, lens, Lmax, seed=0):
    rng = np.random.default_rng(seed)
    tables = gather_rows(lens)
    T = max(int(t[-1, 0] + t[-1, 2]) for t in tables)
    feat = rng.standard_normal((3, Lmax, F)).astype(np.float32)
    for b, L in enumerate(lens):
        feat[b, L:] = np.nan
    fill = rng.standard_normal((3, T, F)).astype(np.float32)
    return feat, fill, tables, T


@pytest.mark.parametrize("lens,Lmax", [((30, 40, 25), 40), ((20, 28, 25), 28)],
                         ids=["Lmax>T", "Lmax<T"])
@pytest.mark.parametrize("F,misalign", [(100, False), (200, False), (6, False), (100, True)],
                         ids=["F100", "F200", "F6", "F100-misaligned"])
def test_gather_bitwise(lib, handle, F, misalign, lens, Lmax):
    feat, fill, tables, T = gather_case(F, lens, Lmax)
    assert T % TILE == 1 and (Lmax > T) == (Lmax == 40)
    Tb = [int(t[-1, 0] + t[-1, 2]) for t in tables]
    assert Tb[0] == lens[0] and Tb[2] == T and len({*Tb}) == 3
    assert any((t[:, 2] == 1).any() for t in tables)
    for fl in (None, fill):
        rc, out, mask, otail, mtail = run_gather(lib, handle, feat, lens, tables, T, fl, misalign)
        assert rc == 0, lib.zv_last_error()
        ref, rmask = edit_ref.gather(feat, fl, tables, T)
        assert np.array_equal(bits(out), bits(ref))
        assert np.array_equal(mask, rmask.astype(np.uint8))
        for b in range(3):
            assert not out[b, Tb[b]:].any() and not mask[b, Tb[b]:].any()     # zeros past T_b
            assert mask[b].sum() == int(tables[b][tables[b][:, 1] < 0, 2].sum())
        assert (otail == CANARY).all() and (mtail == 7).all()
    assert lib.zv_edit_device_bytes(handle) > 0


def test_gather_in_place_over_fill_and_without_mask(lib, handle):
    """out may be fill itself (every element is read and written by one thread); mask is optional."""
    feat, fill, tables, T = gather_case(100, (30, 40, 36), 40, seed=1)
    table, ptr = edit_ref.stack(tables, 3)
    lens = np.asarray((30, 40, 36), np.int32)
    fd, x = cuda(feat), cuda(fill)
    assert lib.zv_edit_gather(handle, fd.data_ptr(), 3, 40, 100, lens.ctypes.data, x.data_ptr(),
                              table.ctypes.data, ptr.ctypes.data, T, x.data_ptr(), None, stream()) == 0
    assert np.array_equal(bits(x.cpu().numpy()), bits(edit_ref.gather(feat, fill, tables, T)[0]))


def test_same_call_twice_and_back_to_back_tables(lib, handle):
    """Two calls queued on one handle without a wait between them, with different tables: the
    second must not overwrite staging the first one's copy may still be reading.  Then the first
    call again: the same bits."""
    feat, fill, tables, T = gather_case(100, (30, 40, 36), 40, seed=2)
    other = [edit_ref.plan(30, [(2, 9, 10)]), edit_ref.plan(40, []), edit_ref.plan(36, [(0, 36, 5), (36, 36, 1)])]
    lens = np.asarray((30, 40, 36), np.int32)
    fd = cuda(feat)
    outs = []
    torch.cuda.synchronize()
    for tabs in (tables, other, tables):
        table, ptr = edit_ref.stack(tabs, 3)
        o = torch.full((3, T, 100), CANARY, dtype=torch.float32, device="cuda")
        assert lib.zv_edit_gather(handle, fd.data_ptr(), 3, 40, 100, lens.ctypes.data, None,
                                  table.ctypes.data, ptr.ctypes.data, T, o.data_ptr(), None, stream()) == 0
        table[:] = -7                                     # the caller's arrays are free on return
        ptr[:] = -7
        outs.append(o)
    torch.cuda.synchronize()
    a, b, c = (o.cpu().numpy() for o in outs)
    assert np.array_equal(bits(a), bits(edit_ref.gather(feat, None, tables, T)[0]))
    assert np.array_equal(bits(b), bits(edit_ref.gather(feat, None, other, T)[0]))
    assert np.array_equal(bits(a), bits(c))
    assert not np.array_equal(bits(a), bits(b))


def gather_rejects():
    good = [[(0, 0, 5), (5, -1, 3), (8, 7, 2)], [(0, 0, 6)]]        # lens (9, 6), T = 10
    def case(tables=good, ptr=None, lens=(9, 6), T=10, Lmax=9):
        return tables, ptr, lens, T, Lmax
    return {
        "row_ptr[0] must be 0": case(ptr=[1, 3, 4]),
        "row_ptr must not fall (row 1)": case(ptr=[0, 3, 2]),
        "segment lengths must be positive (row 0)": case([[(0, 0, 5), (5, -1, 0), (5, 7, 2)], good[1]]),
        "must tile [0, T_b) in order (row 0)": case([[(0, 0, 5), (6, -1, 3), (9, 7, 1)], good[1]]),
        "must tile [0, T_b) in order (row 1)": case([good[0], [(1, 0, 5)]]),
        "kept segment outside [0, L_b) (row 0)": case([[(0, 0, 5), (5, -1, 3), (8, 7, 3)], good[1]], T=11),
        "kept segment outside [0, L_b) (row 1)": case([good[0], [(0, -2, 6)]]),
        "row longer than T (row 0)": case(T=9),
        "lens must be in [0, Lmax] (row 0)": case(Lmax=8),
    }


@pytest.mark.parametrize("msg", list(gather_rejects()))
def test_gather_rejects_bad_tables_and_launches_nothing(lib, handle, msg):
    tables, ptr, lens, T, Lmax = gather_rejects()[msg]
    table, p = edit_ref.stack([np.asarray(t, np.int32).reshape(-1, 3) for t in tables], 3)
    if ptr is not None:
        p = np.asarray(ptr, np.int32)
    lens = np.asarray(lens, np.int32)
    feat = torch.zeros((2, 16, 8), device="cuda")                  # larger than any Lmax here
    out = torch.full((2, 16, 8), CANARY, device="cuda")
    mask = torch.full((2, 16), 7, dtype=torch.uint8, device="cuda")
    rc = lib.zv_edit_gather(handle, feat.data_ptr(), 2, Lmax, 8, lens.ctypes.data, None, table.ctypes.data,
                            p.ctypes.data, T, out.data_ptr(), mask.data_ptr(), stream())
    assert rc != 0 and msg in lib.zv_last_error().decode()
    torch.cuda.synchronize()
    assert (out == CANARY).all() and (mask == 7).all()
    assert lib.zv_edit_device_bytes(handle) == 0                   # not even the table was uploaded


def test_create_destroy_and_argument_checks(lib):
    h = lib.zv_edit_create()
    assert h and lib.zv_edit_device_bytes(h) == 0
    x = torch.zeros(64, device="cuda")
    one = np.asarray([0, 1], np.int32)
    seg = np.asarray([[0, 0, 1]], np.int32)
    L = np.asarray([1], np.int32)
    for B, Lmax, F, T, msg in ((0, 1, 1, 1, "B must be in"), (70000, 1, 1, 1, "B must be in"),
                               (1, 0, 1, 1, "at least 1"), (1, 1, 0, 1, "at least 1"), (1, 1, 1, 0, "at least 1")):
        assert lib.zv_edit_gather(h, x.data_ptr(), B, Lmax, F, L.ctypes.data, None, seg.ctypes.data,
                                  one.ctypes.data, T, x.data_ptr(), None, stream()) != 0
        assert msg in lib.zv_last_error().decode()
    assert lib.zv_edit_gather(h, None, 1, 1, 1, L.ctypes.data, None, seg.ctypes.data, one.ctypes.data, 1,
                              x.data_ptr(), None, stream()) != 0
    assert "null argument" in lib.zv_last_error().decode()
    assert lib.zv_edit_device_bytes(h) == 0
    lib.zv_edit_destroy(h)
    lib.zv_edit_destroy(None)


# ----------------------------------------------------------------------------- splice
SPLICE_ROWS = [   # (L, N - L * HOP, spans, gain)
    (12, -101, [(3, 5, 4), (12, 12, 2)], 0.5),         # an insertion at L: the kept side cannot run on
    (10, 100, [(0, 2, 1), (6, 10, 2)], 1.0),            # generated at both ends, gain 1
    (14, 37, [(0, 0, 1), (4, 9, 0), (11, 11, 1), (12, 13, 3)], 1.7),   # insertion at 0, a deletion
]


def splice_case(C, seed=0):
    rng = np.random.default_rng(seed)
    Ls = [r[0] for r in SPLICE_ROWS]
    Ns = [r[0] * HOP + r[1] for r in SPLICE_ROWS]
    assert all((N + HOP // 2) // HOP == L and N % HOP for N, L in zip(Ns, Ls))
    plans = [edit_ref.plan(L, r[2]) for L, r in zip(Ls, SPLICE_ROWS)]
    gl = [int(p[-1, 0] + p[-1, 2]) * HOP for p in plans]
    tables = [edit_ref.sample_table(p, N, HOP, L) for p, N, L in zip(plans, Ns, Ls)]
    ld, ldg = max(Ns) + 5, max(gl) + 3
    orig = rng.standard_normal((3, C, ld)).astype(np.float32)
    gen = rng.standard_normal((3, C, ldg)).astype(np.float32)
    for b in range(3):
        orig[b, :, Ns[b]:] = np.nan
        gen[b, :, gl[b]:] = np.nan
    return orig, Ns, gen, gl, tables, [r[3] for r in SPLICE_ROWS]


def run_splice(lib, h, orig, Ns, gen, gl, tables, gains, fade, out_cols, pad=3):
    B, C, ld = orig.shape
    table, ptr = edit_ref.stack(tables, 4)
    Ns, gl = np.asarray(Ns, np.int32), np.asarray(gl, np.int32)
    g = np.asarray(gains, np.float32)
    od, gd = cuda(orig), cuda(gen)
    out_ld = out_cols + pad
    out = torch.full((B * C * out_ld + 64,), CANARY, dtype=torch.float32, device="cuda")
    rc = lib.zv_edit_splice(h, od.data_ptr(), ld, Ns.ctypes.data, gd.data_ptr(), gen.shape[2], gl.ctypes.data,
                            B, C, table.ctypes.data, ptr.ctypes.data, g.ctypes.data, fade, out.data_ptr(),
                            out_ld, out_cols, stream())
    o = out.cpu().numpy()
    return rc, o[:B * C * out_ld].reshape(B, C, out_ld), o[B * C * out_ld:]


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("fade", [0, 7, 240, 100000])
def test_splice(lib, handle, fade, C):
    orig, Ns, gen, gl, tables, gains = splice_case(C)
    n = [int(t[-1, 0] + t[-1, 2]) for t in tables]
    out_cols = max(n) + 9
    ref, inside, amp = edit_ref.splice(orig, Ns, gen, gl, tables, gains, fade, out_cols)
    hs = [edit_ref.half_windows(t, N, g, fade) for t, N, g in zip(tables, Ns, gl)]
    # the cases the table is built for: clamped by the buffers (h = 0 where the kept side ends
    # at N or the kept side starts at sample 0), by len / 2 at the largest fade, a kept | kept
    # junction, and windows that never overlap
    assert hs[0][2] == 0 and hs[2][0] == 0
    assert tables[2][1, 3] == 0 and tables[2][2, 3] == 0           # the deletion's junction
    if fade:
        assert inside.any(1).all() and hs[2][1] == min(fade, tables[2][1, 2] // 2, tables[2][2, 2] // 2)
    else:
        assert not inside.any()
    if fade == 100000:
        assert any(h == min(a[2], b[2]) // 2 for t, hh in zip(tables, hs) for a, b, h in zip(t, t[1:], hh))
    for t, hh in zip(tables, hs):
        for i, s in enumerate(t):
            assert (hh[i - 1] if i else 0) + hh[i] <= s[2]
    rc, out, tail = run_splice(lib, handle, orig, Ns, gen, gl, tables, gains, fade, out_cols)
    assert rc == 0, lib.zv_last_error()
    assert np.isfinite(out).all()
    for b in range(3):
        o, r = out[b, :, :n[b]], ref[b, :, :n[b]]
        w = inside[b, :n[b]]
        assert np.array_equal(bits(o[:, ~w]), bits(r[:, ~w]))                  # bitwise outside
        err, tol = np.abs(o[:, w] - r[:, w]), 4 * 2.0 ** -23 * amp[b][:, :n[b]][:, w]
        print(f"fade {fade} C {C} row {b}: {int(w.sum())} window samples, max err / tol "
              f"{float((err / np.maximum(tol, 1e-30)).max(initial=0.0)):.3f}")
        assert (err <= tol).all()
        assert not out[b, :, n[b]:out_cols].any()                              # zero past the length
        assert (out[b, :, out_cols:] == CANARY).all()
        # original samples away from the windows are the recording's own bits
        for o0, src, ln, kind in tables[b].tolist():
            if kind == 0:
                keep = ~w[o0:o0 + ln]
                assert np.array_equal(bits(out[b, :, o0:o0 + ln][:, keep]), bits(orig[b, :, src:src + ln][:, keep]))
    assert (tail == CANARY).all()
    # the same call again: the same bits
    rc, out2, _ = run_splice(lib, handle, orig, Ns, gen, gl, tables, gains, fade, out_cols)
    assert rc == 0 and np.array_equal(bits(out), bits(out2))


def test_splice_exact_width(lib, handle):
    """out_cols equal to the longest row and no multiple of 4: the last thread's samples go one by one."""
    orig, Ns, gen, gl, tables, gains = splice_case(1, seed=3)
    n = [int(t[-1, 0] + t[-1, 2]) for t in tables]
    out_cols = max(n)
    assert out_cols % 4
    ref, inside, amp = edit_ref.splice(orig, Ns, gen, gl, tables, gains, 240, out_cols)
    rc, out, tail = run_splice(lib, handle, orig, Ns, gen, gl, tables, gains, 240, out_cols, pad=0)
    assert rc == 0 and (tail == CANARY).all()
    w = inside[:, None, :]
    assert np.array_equal(bits(np.where(w, 0, out)), bits(np.where(w, 0, ref)))
    assert (np.abs(np.where(w, out - ref, 0)) <= 4 * 2.0 ** -23 * amp).all()


def splice_rejects():
    good = [[(0, 0, 600, 0), (600, 512, 256, 1), (856, 700, 300, 0)]]       # lens 1000, gen 768
    def case(tables=good, ptr=None, lens=1000, gen_lens=768, out_cols=1200, C=1, fade=10, out_ld=1200):
        return tables, ptr, lens, gen_lens, out_cols, C, fade, out_ld
    return {
        "row_ptr[0] must be 0": case(ptr=[2, 3]),
        "segment lengths must be positive (row 0)": case([[(0, 0, 600, 0), (600, 512, 0, 1), (600, 700, 300, 0)]]),
        "must tile [0, N_b) in order (row 0)": case([[(0, 0, 600, 0), (601, 512, 256, 1), (857, 700, 300, 0)]]),
        "kind must be 0 (original) or 1 (generated) (row 0)": case([[(0, 0, 600, 2)]]),
        "segment outside its source (row 0)": case(lens=999),
        "segment outside its source (row 0) ": case(gen_lens=767),
        "segment outside its source (row 0)  ": case([[(0, -1, 600, 0)]]),
        "row longer than out_cols (row 0)": case(out_cols=1155, out_ld=1155),
        "lens must be in [0, ld] (row 0)": case(lens=1025),
        "gen_lens must be in [0, ldg] (row 0)": case(gen_lens=1025),
        "C must be 1 or 2": case(C=3),
        "fade must be non-negative": case(fade=-1),
        "out_cols must be in [1, out_ld]": case(out_ld=1199),
    }


@pytest.mark.parametrize("msg", list(splice_rejects()))
def test_splice_rejects_bad_tables_and_launches_nothing(lib, handle, msg):
    tables, ptr, lens, gen_lens, out_cols, C, fade, out_ld = splice_rejects()[msg]
    table, p = edit_ref.stack([np.asarray(t, np.int32).reshape(-1, 4) for t in tables], 4)
    if ptr is not None:
        p = np.asarray(ptr, np.int32)
    lens, gen_lens = np.asarray([lens], np.int32), np.asarray([gen_lens], np.int32)
    g = np.ones(1, np.float32)
    x = torch.zeros((1, 3, 1024), device="cuda")                   # every source here has ld = 1024
    out = torch.full((1, 3, 1200), CANARY, device="cuda")
    rc = lib.zv_edit_splice(handle, x.data_ptr(), 1024, lens.ctypes.data, x.data_ptr(), 1024,
                            gen_lens.ctypes.data, 1, C, table.ctypes.data, p.ctypes.data, g.ctypes.data, fade,
                            out.data_ptr(), out_ld, out_cols, stream())
    assert rc != 0 and msg.strip() in lib.zv_last_error().decode()
    torch.cuda.synchronize()
    assert (out == CANARY).all() and lib.zv_edit_device_bytes(handle) == 0
