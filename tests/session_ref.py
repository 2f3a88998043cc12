"""Numpy restatements of the solve session (include/zipvoice_hip.h zv_session_*): admit, retire, the
three per-step kernels at their two strides, and the tick's host plan.

The session keeps `slots` rows of `max_frames` frames: x (slots, max_frames, Fx), tc (.., Ft), sc (.., Fx),
pad (slots, max_frames).  A tick's decoder batch has T_k <= max_frames frames per row."""
import numpy as np

from oracle import zipvoice_np as zvo

F32 = np.float32


def admit_ref(x, tc, sc, pad, slots, lens, x0, tc0, sc0):
    """Row i of the request tensors (n, T_in, F) into slot slots[i]: frames [0, len) copied, the rest of
    the slot zero, pad[t] = t >= len.  The other slots are left.  Returns new arrays."""
    x, tc, sc, pad = x.copy(), tc.copy(), sc.copy(), pad.copy()
    for i, (s, n) in enumerate(zip(slots, lens)):
        for dst, src in ((x, x0), (tc, tc0), (sc, sc0)):
            dst[s] = 0
            dst[s, :n] = src[i, :n]
        pad[s] = np.arange(pad.shape[1]) >= n
    return x, tc, sc, pad


def retire_ref(x, slots, lens, T_out):
    """out (n, T_out, Fx): frames [0, len) of slot slots[i], zero past them."""
    out = np.zeros((len(slots), T_out, x.shape[2]), x.dtype)
    for i, (s, n) in enumerate(zip(slots, lens)):
        out[i, :n] = x[s, :n]
    return out


def build_input_ref(x, tc, sc, src, zt, zs, Tk):
    """Decoder row j, frames [0, T_k) = cat[x, tc, sc] of slot src[j], the text zeroed where zt[j], the speech
    where zs[j] -> (N T_k, Fx + Ft + Fs)."""
    rows = []
    for b, t0, s0 in zip(src, zt, zs):
        t = np.zeros_like(tc[b, :Tk]) if t0 else tc[b, :Tk]
        s = np.zeros_like(sc[b, :Tk]) if s0 else sc[b, :Tk]
        rows.append(np.concatenate([x[b, :Tk], t, s], axis=1))
    return np.concatenate(rows, axis=0)


def mask_gather_ref(pad, src, Tk):
    return np.stack([pad[b, :Tk] for b in src])


def euler_update_ref(x, v, row, dt, scale, cond, unc, Tk):
    """x (slots, max_frames, Fx) float32, v (N, T_k, Fx): frames [0, T_k) of slot row[i] take x + vv dt with
    vv = (1 + g) v[cond] - g v[unc], or v[cond] where unc < 0; everything else is left.  Evaluated in
    float64 and rounded once: bit-exact where every fp32 step is exact (dyadic operands)."""
    out = x.copy()
    for i, b in enumerate(row):
        vc = v[cond[i]].astype(np.float64)
        g, h = float(F32(scale[i])), float(F32(dt[i]))
        vv = (1.0 + g) * vc - g * v[unc[i]].astype(np.float64) if unc[i] >= 0 else vc
        out[b, :Tk] = (x[b, :Tk].astype(np.float64) + vv * h).astype(F32)
    return out


def tick_plan(rows, done, lens, distill):
    """The tick of a slot state.  rows[b] = (num_step, t_start, t_end, t_shift, g), num_step 0 a free slot;
    slot b is active while done[b] < num_step and runs step k = done[b] of its own grid.  The scheduled
    solve's step rule over the active slots in slot order: a copy iff g != 0 (never in distill), the copy's
    speech zeroed iff the row's own t > 0.5, else the scale doubled; the copies first.  T_k = the longest
    active row.  Returns (dict of the plan's arrays, A, U, T_k)."""
    active = [b for b, r in enumerate(rows) if r[0] > 0 and done[b] < r[0]]
    ts = {b: zvo.get_time_steps(rows[b][1], rows[b][2], rows[b][0], rows[b][3]) for b in active}
    t_of = {b: ts[b][done[b]] for b in active}
    guided = [b for b in active if not distill and F32(rows[b][4]) != 0]
    U, A = len(guided), len(active)
    scale, unc = [], []
    for b in active:
        g = F32(rows[b][4])
        if distill:
            scale.append(g)
            unc.append(-1)
        elif b in guided:
            scale.append(g if t_of[b] > F32(0.5) else F32(g * F32(2.0)))
            unc.append(guided.index(b))
        else:
            scale.append(F32(0.0))
            unc.append(-1)
    plan = dict(dec_src=guided + active, dec_zero_text=[1] * U + [0] * A,
                dec_zero_speech=[int(t_of[b] > F32(0.5)) for b in guided] + [0] * A,
                dec_t=[t_of[b] for b in guided + active], act_row=active,
                act_dt=[F32(ts[b][done[b] + 1] - ts[b][done[b]]) for b in active], act_scale=scale,
                act_cond=[U + i for i in range(A)], act_uncond=unc)
    return plan, A, U, max([lens[b] for b in active] + [0])
