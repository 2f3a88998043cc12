"""The attention kernels, one launch at a time, against a float64 softmax (tests/kernel_ref.py, section
"attention"; input classes and case lists in tests/attn_cases.py).

First generation (csrc/zv_flash.inc, through zv_attn_check): zv_attn_stats_kernel (split 1 VALU /
Toeplitz, split 3), zv_attn_na_kernel for the same three at 8 / 8 / 4 query tiles and the widths 384 /
144 / 128 / 40 (3, 2, 1 value tiles per wave and a ragged last tile), zv_attn_sa_kernel<1> / <3>,
zv_attn_sa_tp_kernel<0, 2> / <0, 1>, and the materialising zv_attn_softmax_kernel (csrc/zv_attn.inc;
split 1 / 3, natural and base-2 scores).  Second generation (csrc/zv_flash2.inc, through
zv_attn2_check_stale): the SelfAttention forms 1-5 and the NonlinAttention forms 1-2, forced at every
length.  Both operand libraries.

The first-generation launch functions record which instantiation ran (kernel, SPLIT, value tiles per
wave, query tiles per block, TPM, grid); every zv_attn_check call asserts that record.  The SelfAttention
forms also run once with 16 V^T rows per head (the padded value projection's layout, rows 12..15 stale).

Every launch holds three utterances (full, a single kept key, a middle length), padded keys carry
values of +-1000, V^T columns past L hold +-1000, and every output is checked inside canary guards.
The one-hot class is judged at tolerance 0; the shift and general classes by the derived bound through
the interval rule round16(ref - tol) <= got <= round16(ref + tol).

Second generation, fast path: counts == (0, 0, 0) is asserted for the general class and, in bf16, for
the one-hot class -- where the kernels' stated range promises it.  It cannot be promised for the rest:
a shift-class row without a kept target has every kept score at -64, so its bf16 denominator n 2^-64
falls under 2^-60 (the low edge, counted, redone on the exact path); in fp16 a one-hot row whose match
lies in neither the first key step nor the query's own step has its offset 64 or more below the match
(p overflows fp16, counted, exact path).  There the counters are printed and the low / high edge that
cannot fire is asserted to be zero; the outputs are held to the same bounds on either path.
"""
import ctypes
import functools

import numpy as np
import pytest

import attn_cases as ac
import kernel_ref as kr

pytestmark = pytest.mark.gpu

CAN16 = np.uint16(0x7FA5)
CAN32 = np.float32(-7.25e33)
GUARD = 2
KIND = {"stats": 0, "na": 1, "sa": 2, "softmax": 3}
# form -> (split, zv_attn_check form)
V1 = {"stats1": (1, 0), "stats1_tp": (1, 1), "stats3": (3, 0),
      "na1": (1, 0), "na1_tp": (1, 1), "na3": (3, 0),
      "sa1": (1, 0), "sa3": (3, 0), "sa_tp2": (1, 1), "sa_tp1": (1, 2),
      "softmax1": (1, 0), "softmax3": (3, 0), "softmax1_b2": (1, 0), "softmax3_b2": (3, 0)}

# (class, lengths, mask): a test is one launch per length of its group -- the lengths below, at and above
# one edge -- so the file stays a modest number of tests.  The one-hot and shift classes run every length
# of ac.LENGTHS, the general class the thinned list, and each class once with key_pad = NULL.
EDGE_GROUPS = ((1, 2, 321), (15, 16, 17), (31, 32, 33), (63, 64, 65), (127, 128, 129), (191, 192, 193),
               (255, 256, 257))
GENERAL_GROUPS = ((1, 2, 17), (33, 64, 65), (129, 192), (257, 321))
assert sorted(L for g in EDGE_GROUPS for L in g) == sorted(ac.LENGTHS)
assert sorted(L for g in GENERAL_GROUPS for L in g) == sorted(ac.GENERAL_LENGTHS)
CASES = [(k, g, True) for k in ("onehot", "shift") for g in EDGE_GROUPS] + \
        [("general", g, True) for g in GENERAL_GROUPS] + \
        [(k, (65,), False) for k in ("onehot", "shift", "general")]
# the narrower NonlinAttention widths (fewer value tiles per wave, a ragged last tile; each is an
# instantiation of its own): the one-hot and shift classes at every length, the general class at three
CASES_NARROW = [(k, g, True) for k in ("onehot", "shift") for g in EDGE_GROUPS] + \
               [("general", (17, 129, 321), True)] + [(k, (65,), False) for k in ("onehot", "shift", "general")]
# a value projection built padded: 16 V^T rows per head, rows 12..15 stale (the first-generation
# SelfAttention kernels behind the engine's fallback and ZV_ATTN2=0 arms)
CASES_VROWS16 = [("onehot", (63, 64, 65), True), ("general", (129,), True)]
CASES_NV5 = [("onehot", (129,), True), ("general", (129,), True)]
CASES_EXACT = [("onehot", (321,), True), ("general", (129,), True)]
case_id = lambda c: f"{c[0]}-L{'_'.join(map(str, c[1]))}" + ("" if c[2] else "-nopad")  # noqa: E731
one_id = lambda c: f"{c[0]}-L{c[1]}" + ("" if c[2] else "-nopad")  # noqa: E731


def each_length(case):
    """The group's cases one length at a time: (class, L, mask)."""
    return [(case[0], L, case[2]) for L in case[1]]


WORST = {}


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    from zipvoice_amd import engine
    yield request.param, engine.load_library(operand=request.param)
    inputs.cache_clear()
    consumer_ref.cache_clear()
    rows = sorted((k, v) for k, v in WORST.items() if k[1] == request.param)
    if rows:
        print(f"\nworst |got - ref| / (tol + half an ulp) per kernel form [{request.param}]:")
        for (form, _, klass), r in rows:
            print(f"  {form:14s} {klass:8s} {r:.3f}")


def note(form, fmt, klass, r):
    WORST[(form, fmt, klass)] = max(WORST.get((form, fmt, klass), 0.0), r)


@functools.lru_cache(maxsize=2)
def inputs(klass, L, kernel, nv, fmt, split, mask, hot):
    return ac.attn_inputs(klass, L, kernel, nv, fmt, split, mask, hot)


@functools.lru_cache(maxsize=2)
def consumer_ref(form, fmt, klass, L, kernel, nv, split, mask, hot):
    inp = inputs(klass, L, kernel, nv, fmt, split, mask, hot)
    ref, tol = kr.attn_consumer_ref(form, fmt, inp["qkp"], inp["P"], inp["pad"], inp["v"], inp["y"], ac.H, nv)
    if klass == "onehot":
        exp = ac.onehot_expected(inp, kernel, nv)
        assert np.abs(ref - exp).max() <= 2.0 ** -50 * np.abs(exp).max()
        ref, tol = exp, np.zeros_like(tol)
    return ref, tol


def f32(a):
    k = np.ascontiguousarray(a, np.float32)
    assert np.array_equal(k.astype(np.float64), a), "inputs must be fp32 values"
    return k


def check_rc(rc, Lb):
    """A failed call fails the test; a HIP error ends the run (nothing more is launched on a device that
    has reported a fault)."""
    if rc != 0:
        msg = Lb.zv_last_error().decode()
        if "HIP error" in msg:
            pytest.exit(f"HIP error, run ended: {msg}", returncode=3)
        raise AssertionError(msg)


def interior(buf, rows, width, can, what):
    """The (rows, width) output of a canary-guarded buffer; everything else must be untouched."""
    m = np.ones(buf.shape, bool)
    m[GUARD:GUARD + rows, :width] = False
    touched = int((buf[m].view(np.uint32 if buf.dtype == np.float32 else buf.dtype)
                   != np.array(can).view(np.uint32 if buf.dtype == np.float32 else buf.dtype)).sum())
    assert touched == 0, f"{what}: {touched} elements outside the output were written"
    return buf[GUARD:GUARD + rows, :width]


def expect_launch(form, B, L, nv):
    """What the launch function must have recorded: {kernel, SPLIT, DTW / PLO, QTILES / MINW, TPM, grid}."""
    f = kr.ATTN_FORMS[form]
    split, tpm = f["split"], 1 if f["tp"] else 0
    if f["kind"] == "stats":
        return [0, split, 0, 0, tpm, -(-L // 64), 1, B]
    if f["kind"] == "softmax":
        return [4, split, 0, 0, 0, -(-L // 64), ac.H, B]
    if f["kind"] == "na":
        dtw, qt = (1 if nv <= 128 else 2 if nv <= 256 else 3), (4 if split == 3 else 8)
        return [1, split, dtw, qt, tpm, -(-L // (16 * qt)), 1, B]
    if form in ("sa_tp2", "sa_tp1"):
        return [3, 1, 0, 2 if form == "sa_tp2" else 1, 1, -(-L // 128), ac.H, B]
    return [2, split, 0, 0, 0, -(-L // 128), ac.H, B]


def run_v1(Lb, fmt, form, inp, nv, copies=False, vrows=0):
    """One zv_attn_check call -> dict of decoded outputs; the launch record is asserted."""
    from zipvoice_amd.engine import ZvAttnCheckArgs
    f = kr.ATTN_FORMS[form]
    kind, (split, cform) = f["kind"], V1[form]
    B, L, _ = inp["qkp"].shape
    M, Lpad = B * L, -(-L // 64) * 64
    keep = {n: f32(inp[n]) for n in ("qkp", "P", "v", "y") if inp[n] is not None}
    pad = None if inp["pad"] is None else np.ascontiguousarray(inp["pad"], np.uint8)
    a = ZvAttnCheckArgs()
    a.kind, a.B, a.L, a.H, a.nv, a.split, a.form, a.guard = KIND[kind], B, L, ac.H, nv, split, cform, GUARD
    a.b2 = 1 if f["base"] == "2" else 0
    a.stale = ac.STALE
    a.vrows = vrows
    a.qkp, a.P = keep["qkp"].ctypes.data, keep["P"].ctypes.data
    a.key_pad = None if pad is None else pad.ctypes.data
    bufs = {}
    if kind == "stats":
        bufs["stats"] = np.full((M + 2 * GUARD, 2), CAN32, np.float32)
        a.stats = bufs["stats"].ctypes.data
    elif kind == "softmax":
        a.ldw = Lpad
        for n in ("Wh",) + (("Wl",) if split == 3 else ()):
            bufs[n] = np.full((ac.H * M + 2 * GUARD, Lpad), CAN16, np.uint16)
            setattr(a, n, bufs[n].ctypes.data)
    else:
        cols = ac.H * nv if kind == "sa" else nv
        a.v = keep["v"].ctypes.data
        a.y = keep["y"].ctypes.data if kind == "na" else None
        a.ldo = cols + 4
        for n in ("oh",) + (("ol",) if split == 3 or copies else ()) + (("oh2",) if copies else ()):
            bufs[n] = np.full((M + 2 * GUARD, a.ldo), CAN16, np.uint16)
            setattr(a, n, bufs[n].ctypes.data)
    rc = Lb.zv_attn_check(ctypes.byref(a))
    check_rc(rc, Lb)
    assert list(a.launch) == expect_launch(form, B, L, nv), (form, L, nv, list(a.launch))
    out = {}
    for n, b in bufs.items():
        if n == "stats":
            out[n] = interior(b, M, 2, CAN32, n).astype(np.float64)
        elif kind == "softmax":
            out[n] = kr.decode16(interior(b, ac.H * M, Lpad, CAN16, n), fmt)
        else:
            out[n] = kr.decode16(interior(b, M, cols, CAN16, n), fmt).reshape(B, L, cols)
    return out


def run_v2(Lb, kernel, form, inp, nv, force_exact=0):
    B, L, _ = inp["qkp"].shape
    keep = {n: f32(inp[n]) for n in ("qkp", "P", "v", "y") if inp[n] is not None}
    pad = None if inp["pad"] is None else np.ascontiguousarray(inp["pad"], np.uint8)
    out = np.full(inp["v"].shape, np.nan, np.float32)
    cnt = (ctypes.c_int64 * 3)()
    rc = Lb.zv_attn2_check_stale(0 if kernel == "sa" else 1, form, B, L, ac.H, nv, keep["qkp"].ctypes.data,
                                 keep["P"].ctypes.data, None if pad is None else pad.ctypes.data,
                                 keep["v"].ctypes.data, keep["y"].ctypes.data if kernel == "na" else None,
                                 int(force_exact), ac.STALE, out.ctypes.data, ctypes.cast(cnt, ctypes.c_void_p))
    check_rc(rc, Lb)
    return out.astype(np.float64), tuple(int(x) for x in cnt)


def judge(got, ref, tol, fmt, split, tag, key):
    bad, r = kr.attn_accept(got, ref, tol, fmt, split)
    note(*key, r)
    if bad.any():
        at = np.argwhere(bad)
        i = tuple(at[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.size} outside the interval, worst {r:.3f} x the "
                             f"allowance; first at {at[:4].tolist()}: got {got[i]!r}, ref {ref[i]!r}, tol {tol[i]!r}")


def consumer_case(lib, form, case, kernel, nv, gen, v2form=0, force_exact=0, vrows=0):
    for one in each_length(case):
        consumer_one(lib, form, one, kernel, nv, gen, v2form, force_exact, vrows)


def consumer_one(lib, form, case, kernel, nv, gen, v2form=0, force_exact=0, vrows=0):
    fmt, Lb = lib
    klass, L, mask = case
    f = kr.ATTN_FORMS[form]
    hot = gen == 1                                   # the padded keys' raised scores: first generation
    inp = inputs(klass, L, kernel, nv, fmt, f["split"], mask, hot)
    ref, tol = consumer_ref(form, fmt, klass, L, kernel, nv, f["split"], mask, hot)
    tag = f"{fmt} {form}{'' if gen == 1 else '/' + str(v2form)} nv={nv} {one_id(case)}"
    if gen == 1:
        copies = form in ("sa_tp2", "sa_tp1") and L % 2 == 1
        out = run_v1(Lb, fmt, form, inp, nv, copies, vrows)
        got = out["oh"] + out["ol"] if f["split"] == 3 else out["oh"]
        judge(got, ref, tol, fmt, f["split"], tag, (form, fmt, klass))
        if copies:                                   # [o_hi | o_lo | o_hi]: the same value, split
            assert np.array_equal(out["oh2"], out["oh"]), tag
            judge(out["oh"] + out["ol"], ref, tol, fmt, 3, tag + " hi + lo", (form + "+lo", fmt, klass))
        return
    got, cnt = run_v2(Lb, kernel, v2form, inp, nv, force_exact)
    name = f"{form}/{v2form}" + ("x" if force_exact else "")
    judge(got, ref, tol, fmt, 1, tag + f" counts {cnt}", (name, fmt, klass))
    promised = klass == "general" or (klass == "onehot" and fmt == "bf16")
    if force_exact:                                  # every wave / block, and no edge where none can fire
        per = {1: 2, 2: 3, 3: 2, 4: 3, 5: 4}[v2form] * 64 if kernel == "sa" else {1: 64, 2: 128}[v2form]
        units = (4 * ac.H if kernel == "sa" else 1) * ac.B * -(-L // per)
        assert cnt[2] == units and (not promised or cnt[0] == cnt[1] == 0), (tag, cnt, units)
    elif promised:
        assert cnt == (0, 0, 0), (tag, cnt)
    else:
        print(f"{tag}: exact-path runs (low, high, all) = {cnt}")
        # bf16 has no offsets: nothing here can reach 2^100; fp16's offsets keep the denominator above 1/2
        assert cnt[1 if fmt == "bf16" else 0] == 0, (tag, cnt)


# ------------------------------------------------------------------------------- first generation
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("form", ["sa1", "sa3", "sa_tp2", "sa_tp1"])
def test_sa_v1(lib, form, case):
    consumer_case(lib, form, case, "sa", ac.SA_NV, 1)


@pytest.mark.parametrize("case", CASES_NV5, ids=case_id)
@pytest.mark.parametrize("form", ["sa1", "sa3", "sa_tp2", "sa_tp1"])
def test_sa_v1_nv5(lib, form, case):
    consumer_case(lib, form, case, "sa", ac.SA_NV_ODD, 1)


@pytest.mark.parametrize("case", CASES_VROWS16, ids=case_id)
@pytest.mark.parametrize("form", ["sa1", "sa3", "sa_tp2", "sa_tp1"])
def test_sa_v1_16_rows_per_head(lib, form, case):
    consumer_case(lib, form, case, "sa", ac.SA_NV, 1, vrows=16)


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("form", ["na1", "na1_tp", "na3"])
def test_na_v1(lib, form, case):
    consumer_case(lib, form, case, "na", 384, 1)


@pytest.mark.parametrize("case", CASES_NARROW, ids=case_id)
@pytest.mark.parametrize("hid", ac.NA_HIDS[1:])
@pytest.mark.parametrize("form", ["na1", "na1_tp", "na3"])
def test_na_v1_narrow(lib, form, hid, case):
    consumer_case(lib, form, case, "na", hid, 1)


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("form", ["stats1", "stats1_tp", "stats3"])
def test_stats(lib, form, case):
    """m - log2 r against the float64 base-2 log-sum-exp of head 0, and m against the true row maximum."""
    for one in each_length(case):
        stats_one(lib, form, one)


def stats_one(lib, form, case):
    fmt, Lb = lib
    klass, L, mask = case
    f = kr.ATTN_FORMS[form]
    inp = inputs(klass, L, "na", 40, fmt, f["split"], mask, True)
    st = run_v1(Lb, fmt, form, inp, 0)["stats"].reshape(ac.B, L, 2)
    lse, mx, tol = kr.attn_stats_ref(form, fmt, inp["qkp"], inp["P"], inp["pad"], ac.H)
    assert np.isfinite(st).all() and (st[..., 1] > 0).all()
    e1 = np.abs(st[..., 0] - np.log2(st[..., 1]) - lse) / tol
    e2 = np.abs(st[..., 0] - mx) / tol
    note(form, fmt, klass, float(max(e1.max(), e2.max())))
    assert e1.max() <= 1.0, (form, one_id(case), float(e1.max()), np.unravel_index(e1.argmax(), e1.shape))
    assert e2.max() <= 1.0, (form, one_id(case), float(e2.max()), np.unravel_index(e2.argmax(), e2.shape))


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("form", ["softmax1", "softmax3", "softmax1_b2", "softmax3_b2"])
def test_softmax(lib, form, case):
    """Every weight through the interval rule at relative tolerance E; columns [L, Lpad) exactly 0."""
    for one in each_length(case):
        softmax_one(lib, form, one)


def softmax_one(lib, form, case):
    fmt, Lb = lib
    klass, L, mask = case
    f = kr.ATTN_FORMS[form]
    inp = inputs(klass, L, "sa", ac.SA_NV, fmt, f["split"], mask, True)
    out = run_v1(Lb, fmt, form, inp, 0)
    W, E = kr.attn_softmax_ref(form, fmt, inp["qkp"], inp["P"], inp["pad"], ac.H)
    W = W.reshape(ac.H * ac.B * L, L)
    tol = E.reshape(-1, 1) * W
    for n in ("Wh", "Wl")[:2 if f["split"] == 3 else 1]:
        assert not out[n][:, L:].any(), f"{form} {one_id(case)}: {n} columns past L are not zero"
    got = out["Wh"][:, :L] + (out["Wl"][:, :L] if f["split"] == 3 else 0.0)
    judge(got, W, tol, fmt, f["split"], f"{fmt} {form} {one_id(case)}", (form, fmt, klass))


# ------------------------------------------------------------------------------ second generation
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("form", [1, 2, 3, 4, 5])
def test_sa_v2(lib, form, case):
    consumer_case(lib, "sa2", case, "sa", ac.SA_NV, 2, form)


@pytest.mark.parametrize("case", CASES_NV5, ids=case_id)
@pytest.mark.parametrize("form", [1, 2, 3, 4, 5])
def test_sa_v2_nv5(lib, form, case):
    consumer_case(lib, "sa2", case, "sa", ac.SA_NV_ODD, 2, form)


@pytest.mark.parametrize("case", CASES_EXACT, ids=case_id)
@pytest.mark.parametrize("form", [1, 2, 3, 4, 5])
def test_sa_v2_exact(lib, form, case):
    consumer_case(lib, "sa2", case, "sa", ac.SA_NV, 2, form, force_exact=1)


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("form", [1, 2])
def test_na_v2(lib, form, case):
    consumer_case(lib, "na2", case, "na", 384, 2, form)


@pytest.mark.parametrize("case", CASES_NARROW, ids=case_id)
@pytest.mark.parametrize("hid", ac.NA_HIDS[1:])
@pytest.mark.parametrize("form", [1, 2])
def test_na_v2_narrow(lib, form, hid, case):
    consumer_case(lib, "na2", case, "na", hid, 2, form)


@pytest.mark.parametrize("case", CASES_EXACT, ids=case_id)
@pytest.mark.parametrize("form", [1, 2])
def test_na_v2_exact(lib, form, case):
    consumer_case(lib, "na2", case, "na", 384, 2, form, force_exact=1)
