"""The stateful long-form join on the GPU (zv_wavjoin_stream_*, csrc/zv_wavjoin.inc;
zipvoice_amd/longform.py WavJoiner.stream, generate_long_stream).

The bar: streaming changes when samples are handed over, never their value.  The pieces of
every split of a chunk sequence into pushes, concatenated, are compared at the bit level with
zv_wavjoin_apply on the same data, held to the 4 * 2^-23 * max |g x| of
tests/test_gpu_longform.py against the float64 restatement (tests/wavjoin_stream_ref.py,
tests/wavjoin_ref.py), and n_d, pos_d and spans must equal the reference's.  As there, every
comparison first asserts on the reference that no frame's energy lies within 1e-3 (relative)
of the loud / quiet threshold: a condition on the inputs."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import wavjoin_ref as ref  # noqa: E402
import wavjoin_stream_ref as sref  # noqa: E402
from zipvoice_amd import engine  # noqa: E402
from zipvoice_amd.feature import VocosFbank  # noqa: E402
from zipvoice_amd.longform import (WavJoiner, chunk_budget, chunk_tokens, generate_long,  # noqa: E402
                                   generate_long_stream, stream_groups)

SMALL = sref.SMALL
BIG = dict(frame=240, thr=sref.THR, keep_edge=2, max_gap=4, fade=480)
LOUD, QUIET = sref.LOUD, sref.QUIET
CANARY = 7.0


def lib():
    return engine.load_library()


def err():
    return lib().zv_last_error().decode()


@functools.lru_cache(maxsize=None)
def joiner(frame, thr, keep_edge, max_gap, fade):
    h = lib().zv_wavjoin_create(frame, thr, keep_edge, max_gap, fade)
    assert h, err()
    return h


class Stream:
    """A zv_wavjoin_stream handle with numpy in and out."""

    def __init__(self, params, C=1, D=1):
        self.params, self.C, self.D = params, C, D
        self.h = lib().zv_wavjoin_stream_create(joiner(**params), C, D)
        assert self.h, err()

    def __del__(self):
        torch.cuda.synchronize()
        lib().zv_wavjoin_stream_destroy(self.h)

    def reset(self, d=-1):
        return lib().zv_wavjoin_stream_reset(self.h, d, engine._stream())

    def push(self, chunks, gains=None, final=False, doc_sizes=None, out_cap=None, out_ld=None,
             rc_only=False):
        """chunks: (C, n_b) arrays -> (rows (D, C, out_ld) on a canary ground, out_len (D, 2),
        spans (B, 3)); `final` a bool or one flag per slot."""
        C, D, B = self.C, self.D, len(chunks)
        lens = [c.shape[1] for c in chunks]
        n = max(lens + [0]) + 13                         # garbage past every chunk's length
        x = np.random.default_rng(99).uniform(-1, 1, (max(B, 1), C, n)).astype(np.float32)
        for b, c in enumerate(chunks):
            x[b, :, :lens[b]] = c
        xd = torch.from_numpy(x).cuda()
        ln = torch.tensor(lens + [0] * (B == 0), dtype=torch.int32).cuda()
        g = None if gains is None else torch.tensor(list(gains) + [1.0] * (B == 0),
                                                    dtype=torch.float32).cuda()
        sizes = [B] if doc_sizes is None else list(doc_sizes)
        ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        per_doc = [sum(lens[ptr[d]:ptr[d + 1]]) for d in range(D)]
        cap = self.params["fade"] + max(per_doc) if out_cap is None else out_cap
        ld = max(cap, 1) if out_ld is None else out_ld
        out = torch.full((D, C, ld), CANARY, device="cuda")
        out_len = torch.full((D, 2), -5, dtype=torch.int64, device="cuda")
        spans = torch.full((max(B, 1), 3), -9, dtype=torch.int32, device="cuda")
        fin = np.array([final] * D if isinstance(final, bool) else final, np.uint8)
        rc = lib().zv_wavjoin_stream_push(
            self.h, engine._ptr(xd), n, engine._ptr(ln), engine._ptr(g), B,
            None if doc_sizes is None else ptr.ctypes.data, fin.ctypes.data, engine._ptr(out), ld,
            cap, engine._ptr(out_len), engine._ptr(spans), engine._stream())
        torch.cuda.synchronize()
        if rc_only:
            return rc
        assert rc == 0, err()
        return out.cpu().numpy(), out_len.cpu().numpy(), spans[:B].cpu().numpy()


def one_shot(chunks, gains, params, C, doc_sizes=None):
    """zv_wavjoin_apply_docs on the same data -> (list of rows (C, N_d), spans (B, 3))."""
    B = len(chunks)
    lens = [c.shape[1] for c in chunks]
    n = max(lens) + 5
    x = np.random.default_rng(7).uniform(-1, 1, (B, C, n)).astype(np.float32)
    for b, c in enumerate(chunks):
        x[b, :, :lens[b]] = c
    sizes = [B] if doc_sizes is None else list(doc_sizes)
    D = len(sizes)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32).cuda()
    cap = max(sum(lens), 1)
    xd, ln = torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    g = None if gains is None else torch.tensor(gains, dtype=torch.float32).cuda()
    out = torch.full((D, C, cap), CANARY, device="cuda")
    out_len = torch.zeros(D, dtype=torch.int64, device="cuda")
    spans = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
    rc = lib().zv_wavjoin_apply_docs(joiner(**params), engine._ptr(xd), n, engine._ptr(ln),
                                     engine._ptr(g), B, C, engine._ptr(ptr), D, engine._ptr(out),
                                     cap, cap, engine._ptr(out_len), engine._ptr(spans),
                                     engine._stream())
    assert rc == 0, err()
    torch.cuda.synchronize()
    N = out_len.tolist()
    return [out[d, :, :N[d]].cpu().numpy() for d in range(D)], spans.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def peak_of(chunks, gains):
    g = np.ones(len(chunks)) if gains is None else np.asarray(gains, np.float64)
    return max([float(np.abs(g[b] * c).max()) for b, c in enumerate(chunks) if c.size], default=0.0)


def stream_split(st, chunks, gains, sizes, params, C):
    """Push the chunks in parts of `sizes` (the last one final) through the engine and the
    float64 slot side by side, comparing n, pos and spans push by push -> the engine's pieces
    and the reference's, each concatenated."""
    slot = sref.Slot(C, **params)
    parts = list(zip(sref.cut(chunks, sizes), sref.cut(gains, sizes)))
    got, want = [], []
    for i, (cs, gs) in enumerate(parts):
        final = i == len(parts) - 1
        r = slot.push(cs, [c.shape[1] for c in cs], gs, final=final)
        assert r.margin >= 1e-3, r.margin                # a condition on the inputs
        out, out_len, spans = st.push(cs, gs, final=final)
        assert out_len.tolist() == [[r.n, r.pos]], (sizes, i, out_len, r.n, r.pos)
        assert np.array_equal(spans, r.spans), (sizes, i)
        assert not out[0, :, r.n:].any(), (sizes, i)     # zero-filled up to the capacity
        got.append(out[0, :, :r.n])
        want.append(r.out)
    return np.concatenate(got, axis=1), np.concatenate(want, axis=1)


# ------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("C", [1, 2])
def test_split_invariance(C):
    chunks, gains = sref.eight_chunks(C)
    lens = [c.shape[1] for c in chunks]
    whole = ref.wavjoin(chunks, lens, gains, **SMALL)
    assert whole.margin >= 1e-3, whole.margin
    (row,), spans = one_shot(chunks, gains, SMALL, C)
    assert np.array_equal(spans, np.stack([whole.m, whole.off, whole.F], 1))
    tol = 4 * 2.0 ** -23 * peak_of(chunks, gains)
    st = Stream(SMALL, C)
    for sizes in sref.SPLITS:
        assert st.reset() == 0
        got, want = stream_split(st, chunks, gains, sizes, SMALL, C)
        assert got.shape == row.shape, sizes
        assert np.array_equal(bits(got), bits(row)), sizes          # bitwise the one-shot join
        e = float(np.abs(got - want).max())
        print(f"split {sizes} C={C}: N={got.shape[1]} max err {e:.3e} tol {tol:.3e}")
        assert e <= tol, (sizes, e, tol)
        assert np.array_equal(want, whole.out)


def test_held_tail_rule():
    chunks, gains = sref.eight_chunks(1)
    fade = SMALL["fade"]
    whole = ref.wavjoin(chunks, [c.shape[1] for c in chunks], gains, **SMALL)
    assert whole.margin >= 1e-3
    st = Stream(SMALL)
    last = 0
    for b, c in enumerate(chunks):
        _, out_len, _ = st.push([c], [gains[b]])
        n, pos = out_len[0].tolist()
        last = int(whole.m[b]) or last
        so_far = ref.wavjoin(chunks[:b + 1], [x.shape[1] for x in chunks[:b + 1]], gains[:b + 1],
                             **SMALL)
        assert pos + n == so_far.out.shape[1] - min(fade, last // 2), b
    # a 1-sample chunk holds nothing
    assert whole.m[2] == 1
    st.reset()
    out, out_len, spans = st.push([chunks[2]], [0.5])
    assert out_len.tolist() == [[1, 0]] and spans.tolist() == [[1, 0, 0]]
    assert np.array_equal(bits(out[0, :, :1]), bits(np.float32(0.5) * chunks[2]))
    out, out_len, _ = st.push([], final=True)
    assert out_len.tolist() == [[0, 1]]
    # a closing push with no chunks emits exactly the held samples, gained
    st.reset()
    c = chunks[5]
    m = int(whole.m[5])
    assert m == c.shape[1]                               # all loud: y is the chunk itself
    H = min(fade, m // 2)
    _, out_len, _ = st.push([c], [0.25])
    assert out_len.tolist() == [[m - H, 0]]
    out, out_len, _ = st.push([], final=True)
    assert out_len.tolist() == [[H, m - H]]
    assert np.array_equal(bits(out[0, :, :H]), bits(np.float32(0.25) * c[:, m - H:]))
    assert not out[0, :, H:].any()


def test_default_frame_chunks_cross_gather_tiles():
    """frame 240, fade 480: 6000-sample chunks span several 1024-sample gather tiles, so the
    16-byte path runs on both sides of the held region, and the held tail (480 samples) is
    saved and emitted 4 columns at a time."""
    rng = np.random.default_rng(21)
    chunks = [sref.noise(rng, 1, (LOUD, 6000)), sref.noise(rng, 1, (LOUD, 3000), (QUIET, 3000)),
              sref.noise(rng, 1, (QUIET, 1000), (LOUD, 5000)), sref.noise(rng, 1, (LOUD, 6000))]
    gains = [1.0, 0.5, 1.0, 1.0]
    whole = ref.wavjoin(chunks, [6000] * 4, gains, **BIG)
    assert whole.margin >= 1e-3 and whole.F.tolist()[1:] == [480] * 3
    (row,), _ = one_shot(chunks, gains, BIG, 1)
    got, want = stream_split(Stream(BIG), chunks, gains, [2, 2], BIG, 1)
    assert np.array_equal(bits(got), bits(row))
    assert np.abs(got - want).max() <= 4 * 2.0 ** -23 * peak_of(chunks, gains)
    assert np.array_equal(want, whole.out)


def test_three_slots():
    rng = np.random.default_rng(22)
    a = [sref.noise(rng, 1, (LOUD, 500), (QUIET, 200)), sref.noise(rng, 1, (LOUD, 333)),
         sref.noise(rng, 1, (QUIET, 100), (LOUD, 421))]
    b = [sref.noise(rng, 1, (LOUD, 257))]
    c = [sref.noise(rng, 1, (LOUD, 90)), sref.noise(rng, 1, (QUIET, 64), (LOUD, 700))]
    ga, gb, gc = [1.0, 0.5, 1.0], [0.25], [1.0, 1.0]
    docs, sizes = a + b + c, [3, 1, 2]
    whole = [ref.wavjoin(x, [v.shape[1] for v in x], g, **SMALL) for x, g in ((a, ga), (b, gb), (c, gc))]
    assert min(w.margin for w in whole) >= 1e-3
    rows, _ = one_shot(docs, ga + gb + gc, SMALL, 1, sizes)
    st = Stream(SMALL, 1, 3)
    # round one: two chunks of a, all of b (which closes), all of c
    o1, n1, s1 = st.push(a[:2] + b + c, ga[:2] + gb + gc, final=[0, 1, 0], doc_sizes=[2, 1, 2])
    # round two: the rest of a and its end; nothing for c but its end
    o2, n2, s2 = st.push(a[2:], ga[2:], final=[1, 0, 1], doc_sizes=[1, 0, 0])
    assert n1[:, 1].tolist() == [0, 0, 0] and n2[:, 1].tolist() == n1[:, 0].tolist()
    assert n2[1, 0] == 0 and not o2[1].any()             # the closed slot's row: nothing, zeros
    for d in range(3):
        got = np.concatenate([o1[d, :, :n1[d, 0]], o2[d, :, :n2[d, 0]]], axis=1)
        assert got.shape == rows[d].shape and np.array_equal(bits(got), bits(rows[d])), d
        tol = 4 * 2.0 ** -23 * peak_of(*((a, ga), (b, gb), (c, gc))[d])
        assert np.abs(got - whole[d].out).max() <= tol, d
    want = np.stack([whole[0].m[:2], whole[0].off[:2], whole[0].F[:2]], 1)
    assert np.array_equal(s1[:2], want)
    assert s2.tolist() == [[whole[0].m[2], whole[0].off[2] - n1[0, 0], whole[0].F[2]]]
    # every slot is closed now: chunks for one, or a second final, are rejected
    assert st.push(b, gb, final=[0, 0, 0], doc_sizes=[0, 1, 0], rc_only=True) != 0
    assert "closed" in err()
    assert st.push([], final=[0, 1, 0], doc_sizes=[0, 0, 0], rc_only=True) != 0 and "closed" in err()
    assert st.push([], final=[0, 0, 0], doc_sizes=[0, 0, 0], rc_only=True) == 0
    # after reset the slot works again, from position 0
    assert st.reset(1) == 0
    o3, n3, _ = st.push(b, gb, final=[0, 1, 0], doc_sizes=[0, 1, 0])
    assert n3.tolist() == [[0, n1[0, 0] + n2[0, 0]], [rows[1].shape[1], 0],
                           [0, n1[2, 0] + n2[2, 0]]]
    assert np.array_equal(bits(o3[1, :, :n3[1, 0]]), bits(rows[1]))


def test_two_streams_on_one_joiner_interleaved():
    c1, g1 = sref.eight_chunks(1, seed=0)
    c2, g2 = sref.eight_chunks(1, seed=5)
    c2, g2 = c2[::-1], g2[::-1]
    for cs, gs in ((c1, g1), (c2, g2)):
        assert ref.wavjoin(cs, [c.shape[1] for c in cs], gs, **SMALL).margin >= 1e-3
    s1, s2 = Stream(SMALL), Stream(SMALL)
    p1, p2 = [], []
    for b in range(8):
        for st, cs, gs, ps in ((s1, c1, g1, p1), (s2, c2, g2, p2)):
            out, out_len, _ = st.push([cs[b]], [gs[b]], final=b == 7)
            ps.append(out[0, :, :out_len[0, 0]])
    for cs, gs, ps in ((c1, g1, p1), (c2, g2, p2)):
        (row,), _ = one_shot(cs, gs, SMALL, 1)
        assert np.array_equal(bits(np.concatenate(ps, axis=1)), bits(row))


def test_small_out_cap_is_respected_and_the_state_advances():
    chunks, gains = sref.eight_chunks(2)
    whole = ref.wavjoin(chunks, [c.shape[1] for c in chunks], gains, **SMALL)
    assert whole.margin >= 1e-3
    (row,), _ = one_shot(chunks, gains, SMALL, 2)
    st = Stream(SMALL, 2)
    slot = sref.Slot(2, **SMALL)
    parts = list(zip(sref.cut(chunks, [3, 5]), sref.cut(gains, [3, 5])))
    for cap in (1000, 7, 0):
        st.reset()
        slot.reset()
        first = slot.push(parts[0][0], [c.shape[1] for c in parts[0][0]], parts[0][1])
        assert first.n > 1000
        out, out_len, spans = st.push(*parts[0], out_cap=cap, out_ld=4000)
        assert out_len.tolist() == [[first.n, 0]]        # the true length
        assert np.array_equal(spans, first.spans)
        assert (out[:, :, cap:] == CANARY).all()         # nothing at or past out_cap
        assert np.array_equal(bits(out[0, :, :cap]), bits(row[:, :cap]))
        # the state advanced all the same: the next push continues the one-shot row
        out, out_len, _ = st.push(*parts[1], final=True)
        assert out_len[0, 1] == first.n
        assert np.array_equal(bits(out[0, :, :out_len[0, 0]]), bits(row[:, first.n:]))
    # a capacity between n and the row's end: zeros in [n, out_cap), the canary beyond
    st.reset()
    out, out_len, _ = st.push([chunks[6]], [1.0], out_cap=400, out_ld=512)
    n = int(out_len[0, 0])
    assert n == 300 - SMALL["fade"]
    assert not out[0, :, n:400].any() and (out[0, :, 400:] == CANARY).all()


def test_rejections():
    L = lib()
    j = joiner(**SMALL)
    for C in (0, 3):
        assert not L.zv_wavjoin_stream_create(j, C, 1) and "C must be 1 or 2" in err()
    assert not L.zv_wavjoin_stream_create(j, 1, 0) and "D must be at least 1" in err()
    assert not L.zv_wavjoin_stream_create(None, 1, 1) and "null" in err()
    assert L.zv_wavjoin_stream_device_bytes(None) == 0
    assert L.zv_wavjoin_stream_reset(None, 0, engine._stream()) != 0 and "null" in err()
    one, two = Stream(SMALL), Stream(SMALL, 1, 2)
    assert L.zv_wavjoin_stream_device_bytes(one.h) >= 4 * SMALL["fade"]
    for d in (-2, 1):
        assert one.reset(d) != 0 and "slot out of range" in err()
    assert one.reset(-1) == 0 and one.reset(0) == 0
    x = torch.zeros((2, 1, 512), device="cuda")
    ln = torch.tensor([512, 512], dtype=torch.int32, device="cuda")
    out = torch.zeros((2, 1, 2048), device="cuda")
    n = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    ptr = (ctypes.c_int32 * 3)(0, 1, 2)

    def call(h, B, doc_ptr, out_ld, out_cap):
        return L.zv_wavjoin_stream_push(h, engine._ptr(x), 512, engine._ptr(ln), None, B, doc_ptr,
                                        None, engine._ptr(out), out_ld, out_cap, engine._ptr(n),
                                        None, engine._stream())
    assert call(None, 2, None, 2048, 2048) != 0 and "null" in err()
    assert call(one.h, -1, None, 2048, 2048) != 0 and "B must be non-negative" in err()
    assert call(two.h, 2, None, 2048, 2048) != 0 and "doc_ptr is NULL" in err()
    assert call(one.h, 2, None, 1000, 1001) != 0 and "out_cap exceeds out_ld" in err()
    for bad in ((0, 1, 1), (1, 1, 2), (0, 2, 1)):
        assert call(two.h, 2, (ctypes.c_int32 * 3)(*bad), 2048, 2048) != 0 and "doc_ptr" in err()
    assert call(two.h, 2, ptr, 2048, 2048) == 0 and call(one.h, 2, None, 2048, 2048) == 0
    torch.cuda.synchronize()
    # a push to a closed slot
    assert one.push([], final=True, rc_only=True) == 0
    assert call(one.h, 2, None, 2048, 2048) != 0 and "closed" in err()
    assert one.reset(0) == 0 and call(one.h, 2, None, 2048, 2048) == 0
    torch.cuda.synchronize()


def test_warm_push_does_not_block_the_host():
    rng = np.random.default_rng(23)
    chunks = [sref.noise(rng, 1, (LOUD, 3000), (QUIET, 2000)), sref.noise(rng, 1, (LOUD, 2000))]
    L = lib()
    st = Stream(BIG)
    x = np.zeros((2, 1, 5000), np.float32)
    for b, c in enumerate(chunks):
        x[b, :, :c.shape[1]] = c
    xd = torch.from_numpy(x).cuda()
    ln = torch.tensor([5000, 2000], dtype=torch.int32).cuda()
    out = torch.empty((1, 1, 7480), device="cuda")
    n = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    sp = torch.zeros((2, 3), dtype=torch.int32, device="cuda")

    def call():
        assert L.zv_wavjoin_stream_push(st.h, engine._ptr(xd), 5000, engine._ptr(ln), None, 2, None,
                                        None, engine._ptr(out), 7480, 7480, engine._ptr(n),
                                        engine._ptr(sp), engine._stream()) == 0
    call()                                               # warm-up: the joiner's scratch may grow
    torch.cuda.synchronize()
    first = n.tolist()
    before = L.zv_host_block_count()
    call()
    assert st.reset() == 0                               # stream-ordered, not blocking either
    assert L.zv_host_block_count() == before
    torch.cuda.synchronize()
    assert n[0, 1].item() == first[0][0] and n[0, 0].item() > 0


def test_python_stream():
    chunks, gains = sref.eight_chunks(1)
    lens = [c.shape[1] for c in chunks]
    j = WavJoiner(frame=16, threshold_db=-42.0, keep_edge=1, max_gap=2, fade=24)
    n = max(lens)
    x = np.zeros((8, n), np.float32)
    for b, c in enumerate(chunks):
        x[b, :lens[b]] = c[0]
    xd = torch.from_numpy(x).cuda()
    want, spans = j(xd, lens, gains)
    js = j.stream()
    assert js.position == 0 and js.device_bytes() >= 4 * 24
    pieces = []
    for lo, hi in ((0, 3), (3, 3), (3, 8)):
        piece, sp = js.push(xd[lo:hi], lens[lo:hi], gains[lo:hi])
        assert piece.is_cuda and piece.dim() == 2 and sp.shape == (hi - lo, 3)
        pieces.append(piece)
        assert js.position == sum(p.shape[1] for p in pieces)
    tail, _ = js.close()
    pieces.append(tail)
    assert tail.shape[1] == min(24, int(spans[7, 0]) // 2) and js.closed
    assert torch.equal(torch.cat(pieces, 1), want)
    with pytest.raises(RuntimeError):
        js.push(xd[:1], lens[:1])
    js.reset()
    assert js.position == 0
    # lens on the device cost no host wait and give the same piece
    pend = js.push_async(xd, torch.tensor(lens, dtype=torch.int32).cuda(), gains, final=True)
    piece, sp = pend.wait()
    assert pend.position == 0 and torch.equal(piece, want) and torch.equal(sp, spans)
    with pytest.raises(ValueError):
        j.stream(2).push(xd, lens)                       # (B, n) is one channel


# ------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def stack():
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    from zipvoice_amd.vocoder import Vocos
    from zipvoice_amd.weights import synthetic_state_dict
    cfg = default_config("zipvoice")
    m = build_model(cfg, precision="bf16")
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m = m.to("cuda:0")
    voc = Vocos().load_synthetic(0).to("cuda:0")
    return m, voc, VocosFbank()


BREAK, SOFT, SEED = (3, 4), (5,), 1234


@pytest.fixture(scope="module")
def text():
    """The 120-token text and 1 s prompt of tests/test_gpu_longform.py."""
    rng = np.random.default_rng(0)
    tokens = [int(t) for t in rng.integers(10, 90, 120)]
    for i in (17, 33, 41, 58, 79, 96, 110):
        tokens[i] = BREAK[i % 2]
    for i in (8, 25, 50, 70, 101):
        tokens[i] = SOFT[0]
    prompt_tokens = list(range(40, 52))
    pw = (0.05 * rng.standard_normal(24000)).astype(np.float32)     # quieter than the target
    K = len(chunk_tokens(tokens, BREAK, chunk_budget(12, 1.0, 5.0), SOFT))
    assert K >= 3
    return tokens, prompt_tokens, pw, K


@pytest.fixture(scope="module")
def one_call(stack, text):
    """generate_long(batch_size=2, seed): computed once, shared, left unchanged."""
    m, voc, fx = stack
    tokens, prompt_tokens, pw, K = text
    return generate_long(tokens, prompt_tokens, pw, m, voc, fx, BREAK, SOFT, max_seconds=5.0,
                         batch_size=2, seed=SEED, return_chunks=True, num_step=4)


def run_stream(stack, text, **kw):
    m, voc, fx = stack
    tokens, prompt_tokens, pw, K = text
    return list(generate_long_stream(tokens, prompt_tokens, pw, m, voc, fx, BREAK, SOFT,
                                     max_seconds=5.0, seed=SEED, num_step=4, **kw))


def check_infos(ys, K, groups):
    assert len(ys) == len(groups)                        # one piece per group
    pos, t = 0, 0.0
    for gi, (piece, info) in enumerate(ys):
        assert piece.is_cuda and piece.shape[0] == 1
        pos += piece.shape[1]
        assert info["group"] == gi and info["num_chunks"] == K
        assert info["chunks_done"] == groups[gi][-1] + 1
        assert info["position"] == pos                   # position adds up
        assert info["final"] == (gi == len(groups) - 1)
        assert info["t"] > t                             # t is increasing
        t = info["t"]


def test_stream_same_groups_equals_generate_long(stack, text, one_call):
    wav, met, cw, spans = one_call
    K = text[3]
    ys = run_stream(stack, text, first_batch=2, batch_size=2, return_chunks=True)
    check_infos(ys, K, stream_groups(K, 2, 2))
    assert len(ys) == met["num_batches"]
    got = [c for _, info in ys for c in info["chunks"]]
    assert len(got) == K
    for a, b in zip(got, cw):
        assert a.shape == b.shape and a.numel() > 0 and torch.equal(a, b)
    assert torch.equal(torch.cat([p for p, _ in ys], 1), wav)
    # the spans are those of the one call, relative to each piece
    pos = 0
    rel = []
    for piece, info in ys:
        sp = info["spans"].clone().to(torch.int64)
        sp[sp[:, 1] >= 0, 1] += pos
        rel.append(sp)
        pos += piece.shape[1]
    assert torch.equal(torch.cat(rel), spans.to(torch.int64))


def test_stream_small_first_batch_equals_the_join_of_its_own_chunks(stack, text):
    K = text[3]
    ys = run_stream(stack, text, first_batch=1, batch_size=2, return_chunks=True)
    check_infos(ys, K, stream_groups(K, 1, 2))
    cw = [c for _, info in ys for c in info["chunks"]]
    n = max(c.shape[0] for c in cw)
    batch = torch.zeros((K, n), device="cuda")
    for i, c in enumerate(cw):
        batch[i, :c.shape[0]] = c
    from zipvoice_amd.infer import _prompt_rms_normalise
    _, rms = _prompt_rms_normalise(torch.from_numpy(text[2])[None], 0.1)
    assert rms < 0.1
    want, _ = WavJoiner()(batch, [c.shape[0] for c in cw], [rms / 0.1] * K)
    got = torch.cat([p for p, _ in ys], 1)
    assert got.shape == want.shape and torch.equal(got, want)


def test_stream_one_group_equals_generate_long(stack, text):
    m, voc, fx = stack
    tokens, prompt_tokens, pw, K = text
    ys = run_stream(stack, text, first_batch=K + 3, batch_size=2)
    check_infos(ys, K, [list(range(K))])
    wav, _ = generate_long(tokens, prompt_tokens, pw, m, voc, fx, BREAK, SOFT, max_seconds=5.0,
                           batch_size=32, seed=SEED, num_step=4)
    assert torch.equal(ys[0][0], wav)
