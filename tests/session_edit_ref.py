"""Numpy restatement of the edit rows of a solve session (include/zipvoice_hip.h zv_session_admit_edit /
zv_session_retire_edit), written from the definitions, frame by frame: no table is searched, every frame
asks which segment it lies in.  A row's original frame f is pool row offset + f; its frame table has rows
(dst, src, len) with src == -1 a generated segment (edit_ref.plan builds them).

`validate` restates the rules of the two entries on the host state (left[b]: the steps slot b has left, -1
for a free slot; cur[b]: its row's length) and returns the new lengths, or raises ValueError naming the row."""
import numpy as np

import edit_ref  # noqa: F401  (the tables these functions take are edit_ref.plan's)

F32 = np.float32


def new_length(tab):
    return int(sum(int(r[2]) for r in np.asarray(tab).reshape(-1, 3)))


def frame_source(tab, t):
    """The original frame new frame t copies, -1 on a generated segment, None at or past the row's end."""
    for dst, src, ln in np.asarray(tab).reshape(-1, 3).tolist():
        if dst <= t < dst + ln:
            return -1 if src < 0 else src + (t - dst)
    return None


def validate(kind, tables, offsets, lens, pool_rows, slots, left, cur, max_frames, T_io, schedule=None):
    """kind "admit" / "retire".  tables: per-row (m, 3) arrays."""
    n = len(slots)
    if n < 1:
        raise ValueError("at least one row")
    T = []
    for i, tab in enumerate(tables):
        if lens[i] < 0 or offsets[i] < 0 or offsets[i] + lens[i] > pool_rows:
            raise ValueError(f"row {i}: pool range")
        pos = 0
        for dst, src, ln in np.asarray(tab).reshape(-1, 3).tolist():
            if ln <= 0:
                raise ValueError(f"row {i}: segment lengths must be positive")
            if dst != pos:
                raise ValueError(f"row {i}: segments must tile")
            if src != -1 and not (src >= 0 and src + ln <= lens[i]):
                raise ValueError(f"row {i}: kept segment outside [0, L)")
            pos += ln
        T.append(pos)
    seen = set()
    for i, s in enumerate(slots):
        if not 0 <= s < len(left):
            raise ValueError(f"row {i}: slot outside [0, slots)")
        if kind == "admit":
            if left[s] >= 0:
                raise ValueError(f"row {i}: slot is not free")
        elif left[s] < 0:
            raise ValueError(f"row {i}: slot is free")
        elif left[s] > 0:
            raise ValueError(f"row {i}: slot has steps left")
        if s in seen:
            raise ValueError(f"row {i}: slot named twice")
        seen.add(s)
        if kind == "admit":
            if not (1 <= T[i] <= T_io and T[i] <= max_frames):
                raise ValueError(f"row {i}: length")
            num_step, t0, t1, shift, g = schedule[i]
            if not (1 <= num_step <= 65536) or not np.isfinite([t0, t1, shift, g]).all() or shift <= 0:
                raise ValueError(f"row {i}: schedule")
        else:
            if T[i] != cur[s]:
                raise ValueError(f"row {i}: the table's length is not the slot's")
            if T_io < T[i]:
                raise ValueError(f"row {i}: T_out is shorter than the row")
    return T


def admit_edit_ref(x, tc, sc, pad, slots, x0, tc0, pool, offsets, tables):
    """Row i into slot slots[i]: x and the text condition are frames [0, T_i) of the request rows, zero past
    them; the speech condition is the pool frame on a kept segment and zero elsewhere; pad[t] = t >= T_i.
    The other slots are left.  Returns new arrays."""
    x, tc, sc, pad = x.copy(), tc.copy(), sc.copy(), pad.copy()
    maxT = x.shape[1]
    for i, (s, tab) in enumerate(zip(slots, tables)):
        T = new_length(tab)
        for t in range(maxT):
            src = frame_source(tab, t)
            x[s, t] = x0[i, t] if t < T else 0
            tc[s, t] = tc0[i, t] if t < T else 0
            sc[s, t] = pool[offsets[i] + src] if src is not None and src >= 0 else 0
            pad[s, t] = t >= T
    return x, tc, sc, pad


def retire_edit_ref(x, slots, pool, offsets, tables, T_out, keep_original=True):
    """(out (n, T_out, Fx), mask (n, T_out) uint8): the pool frame on a kept segment (the slot's x without
    keep_original), the slot's x on a generated one, zero from T_i on; mask 1 on generated frames."""
    out = np.zeros((len(slots), T_out, x.shape[2]), x.dtype)
    mask = np.zeros((len(slots), T_out), np.uint8)
    for i, (s, tab) in enumerate(zip(slots, tables)):
        for t in range(T_out):
            src = frame_source(tab, t)
            if src is None:
                continue
            mask[i, t] = src < 0
            out[i, t] = pool[offsets[i] + src] if (src >= 0 and keep_original) else x[s, t]
    return out, mask
