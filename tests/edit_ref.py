"""numpy restatement of the speech-editing definitions in include/zipvoice_hip.h (zv_edit_*)
and zipvoice_amd/edit.py: the frame plan, the sample table, the gather and the splice.  Written
from the definitions, frame by frame and sample by sample, not from the kernels: no tables are
searched, every output element asks which segment it lies in."""
import numpy as np

F32 = np.float32


def plan(L, spans):
    """Frame table (dst, src, len) of a row from spans (s, e, n): mark every original frame as
    kept or cut, walk the frames, and emit runs."""
    cut = np.zeros(L, bool)
    ins = {}                                   # original frame index -> frames generated before it
    for s, e, n in spans:
        cut[s:e] = True
        ins[s] = ins.get(s, 0) + n
    seq = []                                   # the new row: original frame index, or -1
    for f in range(L + 1):
        seq += [-1] * ins.get(f, 0)
        if f < L and not cut[f]:
            seq.append(f)
    rows, i = [], 0
    while i < len(seq):
        j = i + 1
        if seq[i] < 0:
            while j < len(seq) and seq[j] < 0:
                j += 1
        else:
            while j < len(seq) and seq[j] == seq[j - 1] + 1 and seq[j] >= 0:
                j += 1
        rows.append((i, seq[i] if seq[i] >= 0 else -1, j - i))
        i = j
    return np.asarray(rows, np.int32).reshape(-1, 3)


def sample_table(table, N, hop, L):
    rows, out = [], 0
    for dst, src, ln in table.tolist():
        if src < 0:
            seg = (out, dst * hop, ln * hop, 1)
        else:
            end = N if src + ln == L else (src + ln) * hop
            seg = (out, src * hop, end - src * hop, 0)
        if seg[2] > 0:
            rows.append(seg)
            out += seg[2]
    return np.asarray(rows, np.int32).reshape(-1, 4)


def stack(tables, width):
    ptr = np.zeros(len(tables) + 1, np.int32)
    ptr[1:] = np.cumsum([len(t) for t in tables])
    return np.concatenate(tables).reshape(-1, width).astype(np.int32), ptr


def gather(feat, fill, tables, T):
    """out (B, T, F) and mask (B, T) from per-row frame tables."""
    B, _, F = feat.shape
    out = np.zeros((B, T, F), F32)
    mask = np.zeros((B, T), bool)
    for b, tab in enumerate(tables):
        for dst, src, ln in tab.tolist():
            if src >= 0:
                out[b, dst:dst + ln] = feat[b, src:src + ln]
            else:
                mask[b, dst:dst + ln] = True
                if fill is not None:
                    out[b, dst:dst + ln] = fill[b, dst:dst + ln]
    return out, mask


def half_windows(tab, lim_orig, lim_gen, fade):
    """h of the junction after each segment of a row's sample table (0 after the last)."""
    hs = []
    for i in range(len(tab)):
        if i + 1 == len(tab):
            hs.append(0)
            continue
        _, src, ln, kind = (int(v) for v in tab[i])
        _, src2, ln2, _ = (int(v) for v in tab[i + 1])
        lim = lim_gen if kind else lim_orig
        hs.append(max(min(fade, ln // 2, ln2 // 2, lim - (src + ln), src2), 0))
    return hs


def splice(orig, lens, gen, gen_lens, tables, gains, fade, out_cols):
    """out (B, C, out_cols) fp32 and inside (B, out_cols) bool: True inside a junction's window.
    The mix is evaluated in fp32, one rounding per operation, in the order of the definition."""
    B, C, _ = orig.shape
    out = np.zeros((B, C, out_cols), F32)
    inside = np.zeros((B, out_cols), bool)
    amp = np.zeros((B, C, out_cols), F32)      # max(|a|, |b|) of the two gained sources in a window
    for b, tab in enumerate(tables):
        g = F32(gains[b])
        hs = half_windows(tab, int(lens[b]), int(gen_lens[b]), fade)
        src_of = lambda kind: gen[b] if kind else orig[b]
        for i, (o, src, ln, kind) in enumerate(tab.tolist()):
            x = src_of(kind)[:, src:src + ln]
            out[b, :, o:o + ln] = x * g if kind else x
        for i in range(len(tab) - 1):
            h = hs[i]
            if h == 0:
                continue
            oa, sa, la, ka = tab[i].tolist()
            p, sb, _, kb = tab[i + 1].tolist()
            ga, gb = (g if ka else F32(1)), (g if kb else F32(1))
            q = np.arange(p - h, p + h)
            w = ((q - (p - h)).astype(F32) + F32(0.5)) / F32(2 * h)
            a = src_of(ka)[:, sa + (q - oa)]
            bb = src_of(kb)[:, sb + (q - p)]
            out[b, :, q] = ((ga * a) * (F32(1) - w) + (gb * bb) * w).T
            inside[b, q] = True
            amp[b, :, q] = np.maximum(np.abs(ga * a), np.abs(gb * bb)).T
    return out, inside, amp
