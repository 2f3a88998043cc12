"""The segmented long-form join on the GPU (zv_wavjoin_apply_docs, csrc/zv_wavjoin.inc;
WavJoiner.join_docs and WavJoiner.trim) against tests/wavjoin_docs_ref.py: the float64
reference tests/wavjoin_ref.wavjoin called once per document on that document's chunks.

Conditions and tolerances are those of tests/test_gpu_longform.py: every comparison first
asserts, on the reference, that no frame's energy lies within 1e-3 (relative) of the
threshold; output samples are held to 4 * 2^-23 * max |g x|; spans and lengths are exact;
samples outside the overlaps with gain 1 must be the input's bits."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import wavjoin_docs_ref as dref  # noqa: E402
from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.longform import WavJoiner  # noqa: E402

THR = 10.0 ** (-42.0 / 20.0)
P = dict(frame=240, thr=THR, keep_edge=2, max_gap=4, fade=480)
LOUD, QUIET = 0.1, 1e-4
L, Q = LOUD, QUIET
CANARY = 7.0


@functools.lru_cache(maxsize=None)
def handle(frame, thr, keep_edge, max_gap, fade):
    h = engine.load_library().zv_wavjoin_create(frame, thr, keep_edge, max_gap, fade)
    assert h, engine.load_library().zv_last_error().decode()
    return h


def noise(rng, *segments):
    """segments: (amplitude, samples), ... -> one float32 chunk of Gaussian noise."""
    return np.concatenate([(a * rng.standard_normal(n)).astype(np.float32) for a, n in segments])


def batch(chunks, pad=13, seed=99):
    """Chunks ((n_b,) or (C, n_b)) -> ((B, C, longest + pad) with garbage past each length,
    lens)."""
    chunks = [c[None] if c.ndim == 1 else c for c in chunks]
    lens = [c.shape[1] for c in chunks]
    x = np.random.default_rng(seed).uniform(-1, 1, (len(chunks), chunks[0].shape[0],
                                                     max(lens) + pad)).astype(np.float32)
    for b, c in enumerate(chunks):
        x[b, :, :lens[b]] = c
    return x, lens


def doc_cap(lens, doc_ptr):
    return max([sum(lens[a:b]) for a, b in zip(doc_ptr, doc_ptr[1:])] + [1])


def apply_docs(x, lens, doc_ptr, gains=None, params=P, out_cap=None, out_ld=None):
    """One zv_wavjoin_apply_docs on canary-filled outputs -> (out (D, C, out_ld), N (D,),
    spans (B, 3)).  doc_ptr None: the NULL / D = 1 form."""
    lib = engine.load_library()
    h = handle(**params)
    B, C, n = x.shape
    D = 1 if doc_ptr is None else len(doc_ptr) - 1
    xd = torch.from_numpy(x).cuda()
    ln = torch.tensor(lens, dtype=torch.int32).cuda()
    g = None if gains is None else torch.tensor(gains, dtype=torch.float32).cuda()
    dp = None if doc_ptr is None else torch.tensor(doc_ptr, dtype=torch.int32).cuda()
    cap = doc_cap(lens, [0, B] if doc_ptr is None else doc_ptr) if out_cap is None else out_cap
    out = torch.full((D, C, cap if out_ld is None else out_ld), CANARY, device="cuda")
    out_len = torch.full((D,), -5, dtype=torch.int64, device="cuda")
    spans = torch.full((max(B, 1), 3), -9, dtype=torch.int32, device="cuda")
    rc = lib.zv_wavjoin_apply_docs(h, engine._ptr(xd), n, engine._ptr(ln), engine._ptr(g), B, C,
                                   engine._ptr(dp), D, engine._ptr(out), out.shape[2], cap,
                                   engine._ptr(out_len), engine._ptr(spans), engine._stream())
    assert rc == 0, lib.zv_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_len.cpu().numpy(), spans[:B].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def reference(case, fade=P["fade"]):
    """The float64 reference of a case, computed once and shared."""
    x, lens, doc_ptr, gains = CASES[case]()
    return x, lens, doc_ptr, gains, dref.wavjoin_docs(x, lens, gains, doc_ptr, **dict(P, fade=fade))


def peak(x, lens, gains=None):
    """max |g x| over the chunks' own samples (not the garbage past each length)."""
    g = np.ones(len(lens)) if gains is None else np.asarray(gains, np.float64)
    return max([float(np.abs(g[b] * x[b, :, :lens[b]]).max()) for b in range(len(lens)) if lens[b]],
               default=0.0)


def compare(x, lens, doc_ptr, gains, r, out, N, spans, cap):
    """Engine results against the reference r, below column cap of every row."""
    assert r.margin >= 1e-3, r.margin                    # a condition on the inputs
    assert np.array_equal(spans, np.stack([r.m, r.off, r.F], 1))
    assert np.array_equal(N, r.N)
    g = np.ones(len(lens)) if gains is None else np.asarray(gains, np.float64)
    tol = 4 * 2.0 ** -23 * peak(x, lens, gains)
    for d in range(len(doc_ptr) - 1):
        n = min(int(r.N[d]), cap)
        err = float(np.abs(out[d, :, :n] - r.outs[d][:, :n]).max(initial=0.0))
        print(f"  doc {d}: N {int(r.N[d])} max err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (d, err, tol)
        assert not out[d, :, n:cap].any()                # zero-filled up to the capacity
        # outside the overlaps, with gain 1: the input's bits
        live = [b for b in range(doc_ptr[d], doc_ptr[d + 1]) if r.m[b]]
        for i, b in enumerate(live):
            if g[b] != 1.0:
                continue
            lo = int(r.F[b])
            hi = int(r.m[b] - (r.F[live[i + 1]] if i + 1 < len(live) else 0))
            hi = min(hi, cap - int(r.off[b]))
            if hi <= lo:
                continue
            src = x[b][:, r.kept[b][lo:hi]]
            assert np.array_equal(bits(out[d, :, r.off[b] + lo:r.off[b] + hi]), bits(src)), b


def check(case, fade=P["fade"]):
    x, lens, doc_ptr, gains, r = reference(case, fade)
    print(f"wavjoin_docs {case}: B={len(lens)} D={len(doc_ptr) - 1} margin {r.margin:.3e} "
          f"N={r.N.tolist()}")
    assert r.margin >= 1e-3, r.margin
    out, N, spans = apply_docs(x, lens, doc_ptr, gains, dict(P, fade=fade))
    compare(x, lens, doc_ptr, gains, r, out, N, spans, out.shape[2])
    return r, out


# ------------------------------------------------------------------------------ the cases
def case_a():
    rng = np.random.default_rng(20)
    x, lens = batch([
        noise(rng, (Q, 1000), (L, 3001), (Q, 5003), (L, 777), (Q, 2500)),
        noise(rng, (Q, 4000)),                           # document 0 ends in an empty chunk
        noise(rng, (Q, 700)),                            # document 2 starts with one
        noise(rng, (L, 1203), (Q, 700), (L, 1500)),
        noise(rng, (L, 100)),
        noise(rng, (L, 6000)),
        noise(rng, (L, 2000), (Q, 900))])                # a one-chunk document
    return x, lens, [0, 2, 2, 6, 7], [1, 1, 1, 0.5, 1, 0.25, 1]


def case_b():
    rng = np.random.default_rng(21)
    x, lens = batch([
        noise(rng, (Q, 900), (L, 1000), (Q, 1300)),
        noise(rng, (Q, 1000)),
        np.zeros(0, np.float32),
        noise(rng, (L, 480), (Q, 1440), (L, 480)),       # a 6-frame pause, cut to 4
        noise(rng, (L, 100))])
    return x, lens, [0, 1, 2, 3, 4, 5], None


def case_c():
    rng = np.random.default_rng(22)
    x, lens = batch([noise(rng, (L, 300)) for _ in range(1033)])
    return x, lens, [0, 1030, 1033], None


def case_d():
    rng = np.random.default_rng(23)
    seg = [1200, 1500, 2000, 900, 1003]
    ch0 = noise(rng, *zip([Q, L, Q, Q, Q], seg))
    ch1 = noise(rng, *zip([Q, Q, Q, L, Q], seg))         # loud where ch0 is quiet
    other = np.stack([noise(rng, (L, 2000)), noise(rng, (Q, 2000))])
    third = np.stack([noise(rng, (Q, 480), (L, 1500)), noise(rng, (L, 1980))])
    x, lens = batch([np.stack([ch0, ch1]), other, third])
    return x, lens, [0, 2, 3], [1, 0.5, 1]


CASES = dict(A=case_a, B=case_b, C=case_c, D=case_d)


def test_document_boundaries():
    r, out = check("A")
    assert r.m.tolist() == [6000, 0, 0, 3403, 100, 6000, 2640]
    assert r.off.tolist() == [0, -1, -1, 0, 3353, 3403, 0]
    # chunk 3 opens its document: a join that fades across the boundary gives 480 here
    assert r.F.tolist() == [0, 0, 0, 0, 50, 50, 0]
    assert r.N.tolist() == [6000, 0, 9403, 2640]
    assert out.shape[:2] == (4, 1) and not out[1].any()  # the empty document's row


def test_trim_every_row_its_own_document():
    r, _ = check("B")
    assert r.m.tolist() == [2160, 0, 0, 1920, 100] and r.N.tolist() == r.m.tolist()
    assert r.off.tolist() == [0, -1, -1, 0, 0] and not r.F.any()


def test_document_longer_than_one_offsets_round():
    r, _ = check("C", fade=100)
    assert r.N.tolist() == [206100, 700]
    first = np.isin(np.arange(1033), [0, 1030])
    assert (r.F[first] == 0).all() and (r.F[~first] == 100).all()


def test_two_channels():
    r, out = check("D")
    assert out.shape[1] == 2
    assert r.m.tolist() == [4800, 2000, 1980] and r.F.tolist() == [0, 480, 0]


def test_small_out_cap_is_respected_and_reported():
    x, lens, doc_ptr, gains, r = reference("A")
    out, N, spans = apply_docs(x, lens, doc_ptr, gains, out_cap=3000, out_ld=10000)
    assert (out[:, :, 3000:] == CANARY).all()            # nothing at or past out_cap
    compare(x, lens, doc_ptr, gains, r, out, N, spans, 3000)   # N is the true N_d


def test_canary_between_out_cap_and_out_ld():
    x, lens, doc_ptr, gains, r = reference("A")
    cap = doc_cap(lens, doc_ptr)
    out, N, spans = apply_docs(x, lens, doc_ptr, gains, out_cap=cap, out_ld=cap + 37)
    assert (out[:, :, cap:] == CANARY).all()
    compare(x, lens, doc_ptr, gains, r, out, N, spans, cap)


def test_same_call_twice_is_bitwise_equal():
    x, lens, doc_ptr, gains, _ = reference("A")
    a = apply_docs(x, lens, doc_ptr, gains)
    b = apply_docs(x, lens, doc_ptr, gains)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(a[0]), bits(b[0]))


def test_null_doc_ptr_is_one_document_of_all_chunks():
    x, lens, _, gains, _ = reference("A")
    a = apply_docs(x, lens, None, gains)
    b = apply_docs(x, lens, [0, len(lens)], gains)
    assert a[0].shape == b[0].shape and a[1][0] > 0
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(a[0]), bits(b[0]))


def test_docs_equal_separate_apply_calls_bit_for_bit():
    """Consistency, besides the reference: every document equals one zv_wavjoin_apply over
    just its chunks."""
    lib = engine.load_library()
    x, lens, doc_ptr, gains, _ = reference("A")
    out, N, spans = apply_docs(x, lens, doc_ptr, gains)
    for d, (lo, hi) in enumerate(zip(doc_ptr, doc_ptr[1:])):
        xd = torch.from_numpy(np.ascontiguousarray(x[lo:hi])).cuda()
        ln = torch.tensor(lens[lo:hi], dtype=torch.int32).cuda()
        g = torch.tensor(gains[lo:hi], dtype=torch.float32).cuda()
        o = torch.full((1, out.shape[2]), CANARY, device="cuda")
        n = torch.full((1,), -5, dtype=torch.int64, device="cuda")
        sp = torch.full((max(hi - lo, 1), 3), -9, dtype=torch.int32, device="cuda")
        assert lib.zv_wavjoin_apply(handle(**P), engine._ptr(xd), x.shape[2], engine._ptr(ln),
                                    engine._ptr(g), hi - lo, 1, engine._ptr(o), o.shape[1],
                                    o.shape[1], engine._ptr(n), engine._ptr(sp),
                                    engine._stream()) == 0
        torch.cuda.synchronize()
        assert int(n.item()) == N[d]
        assert np.array_equal(sp[:hi - lo].cpu().numpy(), spans[lo:hi])
        assert np.array_equal(bits(o.cpu().numpy()), bits(out[d]))


def test_warm_call_does_not_block_the_host():
    x, lens, doc_ptr, gains, r = reference("A")
    lib = engine.load_library()
    h = handle(**P)
    B, D, cap = len(lens), len(doc_ptr) - 1, doc_cap(lens, doc_ptr)
    xd = torch.from_numpy(x).cuda()
    ln = torch.tensor(lens, dtype=torch.int32).cuda()
    dp = torch.tensor(doc_ptr, dtype=torch.int32).cuda()
    out = torch.empty((D, 1, cap), device="cuda")
    n = torch.zeros(D, dtype=torch.int64, device="cuda")
    sp = torch.zeros((B, 3), dtype=torch.int32, device="cuda")

    def call():
        assert lib.zv_wavjoin_apply_docs(h, engine._ptr(xd), x.shape[2], engine._ptr(ln), None, B,
                                         1, engine._ptr(dp), D, engine._ptr(out), cap, cap,
                                         engine._ptr(n), engine._ptr(sp), engine._stream()) == 0
    call()                                               # warm-up: the scratch may grow here
    torch.cuda.synchronize()
    before = lib.zv_host_block_count()
    call()
    assert lib.zv_host_block_count() == before
    torch.cuda.synchronize()
    assert n.cpu().tolist() == r.N.tolist()


def test_rejections():
    lib = engine.load_library()
    err = lambda: lib.zv_last_error().decode()  # noqa: E731
    h = handle(**P)
    x = torch.zeros((2, 1, 512), device="cuda")
    ln = torch.tensor([512, 512], dtype=torch.int32, device="cuda")
    dp = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    out = torch.full((2, 1, 1024), CANARY, device="cuda")
    n = torch.full((2,), -5, dtype=torch.int64, device="cuda")

    def call(B=2, C=1, D=2, out_ld=1024, out_cap=1000, hh=h, ptr=dp):
        return lib.zv_wavjoin_apply_docs(hh, engine._ptr(x), 512, engine._ptr(ln), None, B, C,
                                         engine._ptr(ptr), D, engine._ptr(out), out_ld, out_cap,
                                         engine._ptr(n), None, engine._stream())
    assert call(hh=None) != 0 and "null" in err()
    for C in (0, 3):
        assert call(C=C) != 0 and "C must be 1 or 2" in err()
    assert call(B=-1) != 0 and "B must be non-negative" in err()
    assert call(D=-1) != 0 and "D must be non-negative" in err()
    assert call(D=0) != 0 and "D must be positive when B > 0" in err()
    for D in (0, 2):
        assert call(B=0, D=D, ptr=None) != 0 and "doc_ptr is NULL but D is not 1" in err()
    assert call(out_ld=1000, out_cap=1001) != 0 and "out_cap exceeds out_ld" in err()
    torch.cuda.synchronize()
    assert (out == CANARY).all() and (n == -5).all()     # a rejected call writes nothing
    # B == 0 succeeds for any D >= 0: zero lengths and zero rows
    dz = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert call(B=0, D=0) == 0 and call(B=0, D=2, ptr=dz) == 0 and call(B=0, D=1, ptr=None) == 0
    torch.cuda.synchronize()
    assert n.tolist() == [0, 0] and not out[:, :, :1000].any()
    assert (out[:, :, 1000:] == CANARY).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert n.tolist() == [0, 0]                          # all-zero chunks are empty


# ------------------------------------------------------------------------------ WavJoiner
def joiner():
    return WavJoiner(frame=240, threshold_db=-42.0, keep_edge=2, max_gap=4, fade=480)


def test_python_join_docs():
    x, lens, doc_ptr, gains, r = reference("A")
    sizes = [b - a for a, b in zip(doc_ptr, doc_ptr[1:])]
    j = joiner()
    outs, spans = j.join_docs(torch.from_numpy(x[:, 0]).cuda(), lens, sizes, gains)
    assert len(outs) == 4 and spans.is_cuda and spans.dtype == torch.int32 and spans.shape == (7, 3)
    assert np.array_equal(spans.cpu().numpy(), np.stack([r.m, r.off, r.F], 1))
    tol = 4 * 2.0 ** -23 * peak(x, lens, gains)
    base = outs[0].untyped_storage().data_ptr()
    for d, o in enumerate(outs):
        assert o.is_cuda and o.shape == (1, int(r.N[d]))
        assert o.untyped_storage().data_ptr() == base    # views of the one (D, C, cap) tensor
        assert np.abs(o.cpu().numpy() - r.outs[d]).max(initial=0.0) <= tol
    outs2, _ = j.join_docs(torch.from_numpy(x).cuda(), torch.tensor(lens), sizes)  # (B, C, n)
    assert [tuple(o.shape) for o in outs2] == [(1, int(v)) for v in r.N] and j.device_bytes() > 0
    for bad in ([2, 0, 4], [3, 0, 4, 1], [8, -1, 0, 0]):
        with pytest.raises(ValueError):
            j.join_docs(torch.from_numpy(x).cuda(), lens, bad)
    with pytest.raises(ValueError):
        j.join_docs(torch.from_numpy(x).cuda(), lens[:-1] + [x.shape[2] + 1], sizes)
    with pytest.raises(ValueError):
        j.join_docs(torch.from_numpy(x).cuda(), lens, sizes, gains[:-1])
    outs0, spans0 = j.join_docs(torch.zeros((0, 16), device="cuda"), [], [0, 0])
    assert [tuple(o.shape) for o in outs0] == [(1, 0), (1, 0)] and spans0.shape == (0, 3)


def test_python_trim():
    x, lens, doc_ptr, _, r = reference("B")
    j = joiner()
    lib = engine.load_library()
    xd = torch.from_numpy(x[:, 0]).cuda()
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    gains = [1.0, 1.0, 1.0, 0.5, 1.0]
    g = torch.tensor(gains, device="cuda")
    rg = dref.wavjoin_docs(x, lens, gains, doc_ptr, **P)
    j.trim(xd, ln, g)                                    # warm-up: the scratch may grow here
    torch.cuda.synchronize()
    before = lib.zv_host_block_count()
    out, out_lens = j.trim(xd, ln, g)                    # device lens and gains: no host wait
    assert lib.zv_host_block_count() == before
    assert out.is_cuda and out.shape == xd.shape
    assert out_lens.is_cuda and out_lens.dtype == torch.int64 and out_lens.shape == (5,)
    assert out_lens.tolist() == r.N.tolist() == [2160, 0, 0, 1920, 100]
    o = out.cpu().numpy()
    tol = 4 * 2.0 ** -23 * peak(x, lens, gains)
    for b in range(5):
        n = int(rg.N[b])
        assert np.abs(o[b, :n] - rg.outs[b][0]).max(initial=0.0) <= tol
        assert not o[b, n:].any()                        # rows are zero past their length
        if gains[b] == 1.0:
            assert np.array_equal(bits(o[b, :n]), bits(x[b, 0, rg.kept[b]]))
    out3, lens3 = j.trim(torch.from_numpy(x).cuda(), lens)            # (B, C, n), host lens
    assert out3.shape == x.shape and lens3.tolist() == r.N.tolist()
    assert np.array_equal(bits(out3[:, 0].cpu().numpy()[[0, 4]]), bits(o[[0, 4]]))
    with pytest.raises(ValueError):
        j.trim(xd, lens[:-1])
