"""The editing service without a GPU: the C ABI of the session's edit rows, the rules both entries check on
the host, the numpy restatement of the two kernels, and the host logic of ContinuousBatcher.submit_edit on a
stub session.

* ABI: zv_session_admit_edit / zv_session_retire_edit / zv_session_edit_check are declared in
  include/zipvoice_hip.h with the documented signatures, bound in engine.SIGNATURES with matching argument
  lists and exported by both operand builds.
* Rules: every rejection of tests/session_edit_cases.py through zv_session_edit_check, which runs the rules
  before it touches a device: return 1, the row named, outputs and state untouched.  session_edit_ref.validate
  rejects the same requests.
* tests/session_edit_ref.py against the composition it replaces: edit_ref.gather into session_ref.admit_ref,
  and session_ref.retire_ref into edit_ref.gather(fill=), bit for bit, on the kernel tests' cases.
* submit_edit: bad spans, max_frames + 1 against max_frames, a foreign or dropped recording and a bad seed
  are rejected at submit; a queue mixing wav, voice and edit requests is admitted in leading runs of one kind;
  a recording is held from submit to retirement and can be dropped only after."""
import ctypes
import os
import re

import numpy as np
import pytest

import edit_ref
import session_edit_cases as sc
import session_edit_ref as ser
import session_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "zipvoice_hip.h")

DECLS = {
    "zv_session_admit_edit": "int zv_session_admit_edit(zv_session_handle s, int n, const int32_t* host_slots, "
                             "const zv_row_sched* host_rows, const float* x0, const float* text_c, int T_in, "
                             "const float* pool, int pool_rows, const int32_t* host_offsets, "
                             "const int32_t* host_lens, const int32_t* host_table, const int32_t* host_row_ptr, "
                             "void* stream);",
    "zv_session_retire_edit": "int zv_session_retire_edit(zv_session_handle s, int n, const int32_t* host_slots, "
                              "const float* pool, int pool_rows, const int32_t* host_offsets, "
                              "const int32_t* host_lens, const int32_t* host_table, const int32_t* host_row_ptr, "
                              "int keep_original, float* out, uint8_t* mask_out, int T_out, void* stream);",
    "zv_session_edit_check": "int zv_session_edit_check(zv_session_edit_check_args* a);",
}


def header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.sub(r"\s+", " ", src)


def test_header_declares_the_documented_signatures():
    h = header()
    for name, decl in DECLS.items():
        assert decl in h, name
    assert "} zv_session_edit_check_args;" in h
    # zv_session_check_args is as it was: the edit rows have a check entry of their own
    assert "const int32_t* offsets" not in h[h.index("enum zv_session_kind"):h.index("} zv_session_check_args;")]


def test_ctypes_table_matches_the_header():
    from zipvoice_amd.engine import SIGNATURES, ZvSessionEditCheckArgs
    for name, decl in DECLS.items():
        res, args = SIGNATURES[name]
        params = decl[decl.index("(") + 1:decl.rindex(")")]
        want = []
        for p in params.split(", "):
            ty = p.rsplit(" ", 1)[0]
            if ty == "zv_session_edit_check_args*":
                want.append(ctypes.POINTER(ZvSessionEditCheckArgs))
            else:
                want.append(ctypes.c_void_p if "*" in ty or ty.endswith("_handle") else ctypes.c_int)
        assert args == want and res == ctypes.c_int, name
    # the struct, field by field, against the header's
    h = header()
    body = h[h.index("enum zv_session_edit_kind"):h.index("} zv_session_edit_check_args;")]
    body = body[body.index("typedef struct {") + len("typedef struct {"):]
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.rsplit(" ", 1)[0], decl
        if "*" in decl:
            fields.append((decl.rsplit(" ", 1)[1], ctypes.c_void_p))
        elif decl.startswith("int launch[8]"):
            fields.append(("launch", ctypes.c_int * 8))
        else:
            assert ty.startswith("int"), decl
            fields += [(n.strip(), ctypes.c_int) for n in names[len("int "):].split(",")]
    assert [(n, t) for n, t in ZvSessionEditCheckArgs._fields_] == fields


def both_libraries():
    from zipvoice_amd.csrc.build import build
    build(verbose=False)
    from zipvoice_amd import engine
    return engine.load_library(), engine.load_library(operand="f16")


def test_both_libraries_export_the_symbols():
    for lib in both_libraries():
        for name in DECLS:
            assert hasattr(lib, name), name
        # a null session is refused with a message, before anything touches a device
        assert lib.zv_session_admit_edit(None, 1, None, None, None, None, 1, None, 1, None, None, None, None, None) != 0
        assert b"null session handle" in lib.zv_last_error()
        assert lib.zv_session_retire_edit(None, 1, None, None, 1, None, None, None, None, 1, None, None, 1, None) != 0
        assert b"null session handle" in lib.zv_last_error()
        assert lib.zv_session_edit_check(None) != 0


REJECTIONS, GOOD, PTR = sc.rejections()


@pytest.mark.parametrize("case", range(len(REJECTIONS)), ids=[f"{k}: {w}" for w, k, _, _ in REJECTIONS])
def test_rules_run_on_the_host_before_a_device_is_touched(case):
    what, kind, fields, row = REJECTIONS[case]
    lib = both_libraries()[0]
    sc.run_rejection(lib, what, kind, fields, row, GOOD, PTR)
    # the restatement refuses the same request
    f = dict(fields)
    left, cur = ([-1, -1, 3], [0, 0, 9]) if kind == "admit" else ([0, 0, 3], [1, 7, 9])
    for s in f.pop("free", []):
        left[s], cur[s] = -1, 0
    table, ptr = f.get("table", GOOD), f.get("row_ptr", PTR)
    n = f.get("n", 2)
    if ptr[0] != 0 or (np.diff(ptr) < 0).any():
        return                                              # (a malformed row_ptr has no per-row tables to restate)
    tabs = [table[ptr[i]:ptr[i + 1]] for i in range(n)]
    with pytest.raises(ValueError):
        ser.validate(kind, tabs, list(f.get("offsets", [10, 30]))[:n], list(f.get("lens", [9, 6]))[:n], sc.POOL_ROWS,
                     list(f.get("slot", [1, 0]))[:n], left, cur, sc.MAXT, f.get("T_io", 23 if kind == "admit" else 12),
                     f.get("sched", [sc.SCHED, sc.SCHED]))


def test_the_good_request_of_the_rejections_passes_the_restated_rules():
    tabs = [GOOD[PTR[i]:PTR[i + 1]] for i in range(2)]
    assert ser.validate("admit", tabs, [10, 30], [9, 6], 64, [1, 0], [-1, -1, 3], [0, 0, 9], 23, 23, [sc.SCHED] * 2) == [7, 1]
    assert ser.validate("retire", tabs, [10, 30], [9, 6], 64, [1, 0], [0, 0, 3], [1, 7, 9], 23, 12) == [7, 1]


def test_the_cases_hold_what_they_are_meant_to():
    segs = {n: len(sc.table(n)) for n in sc.ROWS}
    assert segs == {"seven": 7, "generated": 1, "two": 2, "five": 5, "one": 1}
    T = {n: ser.new_length(sc.table(n)) for n in sc.ROWS}
    assert T == {"seven": sc.MAXT, "generated": 5, "two": 7, "five": 10, "one": 1}
    seven = sc.table("seven").tolist()
    assert seven[0][1] == -1                                          # a generated segment first
    assert [s[1] for s in seven[2:5]] == [-1, 4, -1] and seven[3][2] == 1   # one kept frame between generated ones
    assert seven[5][1] >= 0 and seven[6][1] > seven[5][1] + seven[5][2]    # kept | kept: the deletion's junction
    assert sc.ROWS["seven"][0] + sc.ROWS["seven"][1] == sc.POOL_ROWS
    assert sc.ROWS["two"][:2] == sc.ROWS["five"][:2]
    for rows, slots, T_in, T_out in sc.CALLS.values():
        assert len(set(slots)) == len(slots) <= sc.SLOTS and T_in >= max(T[n] for n in rows) <= T_out
    assert min(T[n] for n in sc.CALLS["A"][0]) < sc.CALLS["A"][2]      # T_in > T_i


@pytest.mark.parametrize("call", sorted(sc.CALLS))
@pytest.mark.parametrize("widths", sorted(sc.WIDTHS))
def test_restatement_is_the_unfused_composition(widths, call):
    Fx, Ft = sc.WIDTHS[widths]
    names, slots, T_in, T_out = sc.CALLS[call]
    tabs, offsets, lens, _, _ = sc.call_tables(call)
    n, S, maxT = len(names), sc.SLOTS, sc.MAXT
    rng = np.random.default_rng([ord(c) for c in widths + call])
    pool = sc.pool_for(rng, Fx)
    x0 = rng.standard_normal((n, T_in, Fx)).astype(np.float32)
    tc0 = (8.0 + rng.standard_normal((n, T_in, Ft))).astype(np.float32)
    can = lambda F: np.full((S, maxT, F), sc.CAN32, np.uint32).view(np.float32)
    pad = np.full((S, maxT), sc.CAN8, np.uint8)
    feat = np.zeros((n, max(lens), Fx), np.float32)
    for i in range(n):
        feat[i, :lens[i]] = pool[offsets[i]:offsets[i] + lens[i]]
    sc0, gmask = edit_ref.gather(feat, None, tabs, T_in)
    Ts = [ser.new_length(t) for t in tabs]
    want = sr.admit_ref(can(Fx), can(Ft), can(Fx), pad, slots, Ts, x0, tc0, sc0)
    got = ser.admit_edit_ref(can(Fx), can(Ft), can(Fx), pad, slots, x0, tc0, pool, offsets, tabs)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
    assert not np.isnan(got[2][slots]).any()
    # retire: the slots hold finished rows
    x = rng.standard_normal((S, maxT, Fx)).astype(np.float32)
    plain = sr.retire_ref(x, slots, Ts, T_out)
    want_out, want_mask = edit_ref.gather(feat, plain, tabs, T_out)
    out, mask = ser.retire_edit_ref(x, slots, pool, offsets, tabs, T_out)
    assert np.array_equal(out.view(np.uint32), want_out.view(np.uint32)) and np.array_equal(mask.astype(bool), want_mask)
    assert np.array_equal(mask[:, :T_in].astype(bool), gmask[:, :mask.shape[1]])
    raw, mask2 = ser.retire_edit_ref(x, slots, pool, offsets, tabs, T_out, keep_original=False)
    assert np.array_equal(raw.view(np.uint32), plain.view(np.uint32)) and np.array_equal(mask2, mask)


# ---------------------------------------------------------------------------------------------- submit_edit
torch = pytest.importorskip("torch")


class StubSession:
    """Host state only: which slots hold a row and how many steps it has left."""

    def __init__(self, slots):
        self.left, self.calls = [-1] * slots, []

    def steps_left(self):
        return list(self.left)

    def admit(self, slots, x0, tc, sc_, lens, schedule):
        self.calls.append(("admit", list(slots)))
        for s, r in zip(slots, schedule):
            self.left[s] = r.num_step

    def admit_edit(self, slots, x0, tc, pool, offsets, lens, table, row_ptr, schedule):
        self.calls.append(("admit_edit", list(slots), list(offsets), list(lens), np.asarray(table).copy(), list(row_ptr)))
        for s, r in zip(slots, schedule):
            self.left[s] = r.num_step

    def retire_edit(self, slots, pool, offsets, lens, table, row_ptr, T_out=None, keep_original=True):
        self.calls.append(("retire_edit", list(slots), list(offsets)))
        for s in slots:
            self.left[s] = -1
        return torch.zeros((len(slots), T_out or 1, 4)), torch.zeros((len(slots), T_out or 1), dtype=torch.bool)

    def step(self):
        self.left = [v - 1 if v > 0 else v for v in self.left]

    def close(self):
        pass


def stub_store(recordings):
    """A VoiceStore with host bookkeeping only (its constructor allocates on a GPU) and recordings of the
    given (frames, samples)."""
    from zipvoice_amd.voices import FrameAllocator, Recording, VoiceStore
    st = VoiceStore.__new__(VoiceStore)
    st.target_rms, st.feat_scale, st.feat_bias, st.n_mels = 0.1, 0.1, 0.0, 4
    st.alloc = FrameAllocator(256)
    st._live, st._uses, st._wavs = {}, {}, {}
    st.arena, st.gains = torch.zeros((256, 4)), torch.ones(256)
    recs = []
    for i, (frames, samples) in enumerate(recordings):
        r = Recording(i, st.alloc.alloc(frames), frames, samples, st)
        st._live[r.id], st._uses[r.id], st._wavs[r.id] = r, 0, torch.arange(samples, dtype=torch.float32)
        recs.append(r)
    return st, recs


class StubModel:
    class cfg:
        stereo = False
    device = torch.device("cpu")

    def __init__(self, slots):
        self.session = StubSession(slots)
        self.solver = self

    def open_session(self, slots, max_frames):
        return self.session


class StubVocoder:
    class cfg:
        hop_length = 256


def make_batcher(store, max_rows=2, max_frames=40):
    from zipvoice_amd.serving import ContinuousBatcher
    m = StubModel(max_rows)
    return ContinuousBatcher(m, StubVocoder(), None, max_rows=max_rows, max_frames=max_frames, voices=store), m.session


def test_submit_edit_checks_what_the_host_can_know():
    store, (rec,) = stub_store([(30, 30 * 256)])
    other, (foreign,) = stub_store([(30, 30 * 256)])
    cb, sess = make_batcher(store)
    toks = [1, 2, 3]
    for spans, msg in (([(5, 31, 2)], "row 0 span 0"), ([(5, 3, 2)], "row 0 span 0"), ([(5, 8, -1)], "non-negative"),
                       ([(5, 8, 2), (7, 9, 1)], "sorted and disjoint"), ([(4, 4, 0)], "generates nothing")):
        with pytest.raises(ValueError, match=msg):
            cb.submit_edit(toks, rec, spans)
    with pytest.raises(ValueError, match="exceeds the batcher's max_frames"):
        cb.submit_edit(toks, rec, [(10, 10, 11)])                    # 41 = max_frames + 1
    with pytest.raises(ValueError, match="another store"):
        cb.submit_edit(toks, foreign, [(10, 12, 2)])
    with pytest.raises(ValueError, match="expected a Recording"):
        cb.submit_edit(toks, np.zeros(9000, np.float32), [(10, 12, 2)])
    with pytest.raises(ValueError):
        cb.submit_edit(toks, rec, [(10, 12, 2)], seed=-1)
    with pytest.raises(ValueError):
        cb.submit_edit(toks, rec, [(10, 12, 2)], seed=2 ** 64)
    with pytest.raises(ValueError, match="num_step"):
        cb.submit_edit(toks, rec, [(10, 12, 2)], num_step=0)
    assert cb.pending() == (0, 0) and store.uses(rec) == 0 and sess.calls == []
    assert cb.submit_edit(toks, rec, [(10, 10, 10)]) == 0            # 40 = max_frames: accepted
    assert cb.pending() == (1, 0) and store.uses(rec) == 1
    gone, (dropped,) = stub_store([(30, 30 * 256)])
    cb2, _ = make_batcher(gone)
    gone.drop(dropped)
    with pytest.raises(ValueError, match="dropped"):
        cb2.submit_edit(toks, dropped, [(10, 12, 2)])
    cb.close()
    assert store.uses(rec) == 0                                      # close gives the queued edit up

    class Stereo(StubModel):
        class cfg:
            stereo = True
    from zipvoice_amd.serving import ContinuousBatcher
    with pytest.raises(NotImplementedError):
        ContinuousBatcher(Stereo(1), StubVocoder(), None, 1, 40, voices=store).submit_edit(toks, rec, [(1, 2, 1)])
    with pytest.raises(ValueError, match="no voice store"):
        ContinuousBatcher(StubModel(1), StubVocoder(), None, 1, 40).submit_edit(toks, rec, [(1, 2, 1)])


def test_a_request_without_spans_never_reaches_the_session():
    store, (rec,) = stub_store([(30, 7700)])
    cb, sess = make_batcher(store)
    t = cb.submit_edit([1, 2], rec, [])
    assert cb.pending() == (0, 0) and store.uses(rec) == 0
    (ticket, wav), = cb.step()
    assert ticket == t and wav.shape == (1, 7700) and torch.equal(wav[0], store.waveform(rec))
    assert sess.calls == []


def test_groups_are_leading_runs_of_one_kind(monkeypatch):
    """wav, edit, edit, voice, edit in the queue and four free slots: four admissions, one kind each, in order."""
    from zipvoice_amd import serving
    from zipvoice_amd.voices import Voice
    store, (rec,) = stub_store([(30, 7700)])
    voice = Voice(99, store.alloc.alloc(5), 5, 1280, (1, 2), store)
    store._live[99], store._uses[99] = voice, 0
    cb, sess = make_batcher(store, max_rows=4)
    seen = []
    monkeypatch.setattr(cb, "_admit_edits", lambda free, reqs: (seen.append(("edit", len(reqs))),
                                                                [cb._queue.popleft() for _ in reqs]))
    cb._queue.append(serving._Request(100, ([1], [2], np.zeros(4)), 1, 1.0, 1.0, 0.5, None, 9))
    for _ in range(2):
        cb.submit_edit([1, 2], rec, [(3, 5, 2)])
    cb._queue.append(serving._Request(101, ([1], voice), 1, 1.0, 1.0, 0.5, None, 9))
    cb.submit_edit([1, 2], rec, [(3, 5, 2)])
    kinds = [serving._kind(q) for q in cb._queue]
    assert kinds == ["wav", "edit", "edit", "voice", "edit"]
    cb._queue.popleft()                                              # (the wav group needs a real front: taken as admitted)
    cb._admit()
    assert seen == [("edit", 2)] and [serving._kind(q) for q in cb._queue] == ["voice", "edit"]
    cb._queue.popleft()
    cb._admit()
    assert seen == [("edit", 2), ("edit", 1)] and not cb._queue


def test_a_recording_is_held_from_submit_to_retirement(monkeypatch):
    store, (rec, rec2) = stub_store([(30, 7700), (20, 5000)])
    cb, sess = make_batcher(store, max_rows=2)
    m = cb.model
    # the device work of an admission and a retirement, stubbed: the host bookkeeping is what runs
    m.forward_text_embed = lambda tokens: (torch.zeros((len(tokens), 3, 4)), torch.tensor([len(t) for t in tokens]))
    m.forward_text_condition = lambda e, tl, fl, num_frames=None: (torch.zeros((e.shape[0], num_frames, 4)), None)
    from zipvoice_amd import serving
    monkeypatch.setattr(serving, "initial_noise", lambda n, T, F, dev, seeds=None: torch.zeros((n, T, F)))
    cb.vocoder.decode_features = lambda x, lens, **kw: torch.zeros((x.shape[0], x.shape[1] * 256))

    class Eng:
        @staticmethod
        def edit_splice(orig, lens, gen, gen_lens, table, row_ptr, gains, fade):
            assert gains is None
            return torch.zeros((orig.shape[0], 1, max(int(table[row_ptr[b + 1] - 1, 0] + table[row_ptr[b + 1] - 1, 2])
                                                      for b in range(orig.shape[0]))))
    m.engine = Eng()
    t0 = cb.submit_edit([1, 2], rec, [(3, 5, 4)], num_step=2)
    t1 = cb.submit_edit([3], rec, [(0, 0, 1)], num_step=1)
    t2 = cb.submit_edit([4], rec2, [(5, 15, 0)], num_step=1)
    assert store.uses(rec) == 2 and store.uses(rec2) == 1
    with pytest.raises(ValueError, match="still used by 2 queued or in-flight"):
        store.drop(rec)
    assert cb.step() == []                                           # admits the first two (two slots), ticks
    assert cb.pending() == (1, 2) and store.uses(rec) == 2           # in flight: still held
    call = sess.calls[0]
    assert call[0] == "admit_edit" and call[1] == [0, 1] and call[2] == [rec.offset] * 2 and call[3] == [30, 30]
    assert np.array_equal(call[4], np.concatenate([edit_ref.plan(30, [(3, 5, 4)]), edit_ref.plan(30, [(0, 0, 1)])]))
    with pytest.raises(ValueError, match="in-flight"):
        store.drop(rec)
    done = cb.step()                                                 # retires t1, admits t2 into its slot, ticks
    assert [t for t, _ in done] == [t1] and done[0][1].shape == (1, 7700 + 256)
    assert store.uses(rec) == 1 and cb.pending() == (0, 2)
    assert [c[0] for c in sess.calls] == ["admit_edit", "retire_edit", "admit_edit"] and sess.calls[2][1] == [1]
    rest = cb.step()                                                 # both remaining rows finish together
    assert sorted(t for t, _ in rest) == [t0, t2]
    assert dict(rest)[t2].shape == (1, 5000 - 10 * 256) and dict(rest)[t0].shape == (1, 7700 + 2 * 256)
    assert store.uses(rec) == 0 and store.uses(rec2) == 0 and cb.pending() == (0, 0)
    assert [t for t, _ in cb.last_mel] == [t0, t2]
    store.drop(rec)                                                  # free to go now
    with pytest.raises(ValueError, match="dropped"):
        cb.submit_edit([1], rec, [(1, 2, 1)])
    assert store.alloc.free_ranges()[0] == (0, 30)
