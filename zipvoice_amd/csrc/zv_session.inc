// Solve session for gfx950: the kernels, launches and host plan of continuous batching
// (zv_session_*, include/zipvoice_hip.h; the session body is zv_engine::session_* in zv_engine.hip).
// No reference counterpart: the reference's solver integrates one batch from step 0 to its end.  The
// behaviour is defined in the header and restated in numpy by tests/session_ref.py.
//
// A session owns `slots` rows of `max_frames` frames: x, text condition, speech condition and padding
// mask.  A row is put into a free slot (admit), integrated one Euler step per tick on its own grid,
// and read out when its steps are done (retire); rows never move between slots.  A tick's decoder
// batch is gathered from the active slots through the scheduled solve's row map (sched_step,
// zv_elem.inc) at the tick's own length T_k = max length of the active rows, so the slot buffers are
// read and written at stride max_frames and the decoder batch at stride T_k:
//   admit    one admitted row per blockIdx.y: frames [0, len) of the request's x0 / text / speech rows
//            copied, [len, max_frames) zero-filled, pad[t] = t >= len.  A row's frames are contiguous
//            on both sides, so each tensor is one flat copy followed by one flat fill; f32x4 where the
//            widths are multiples of 4 and the bases 16-byte aligned, one float per item otherwise.
//            (slots' bytes written once, len frames read.)
//   retire   the same copy the other way: frames [0, len) of x into row i of out, [len, T_out) zero.
//   build    zv_build_input_map(4)_kernel with the source at stride max_frames, frames [0, T_k)
//   mask     zv_gather_u8_kernel likewise, T_k bytes per decoder row
//   update   zv_euler_update_sched_kernel on frames [0, T_k) of the listed slots (euler_combine /
//            euler_step: the same FMAs); frames >= T_k and unlisted slots are not touched
// No atomics; every output element is written once, by one thread.
#pragma once

struct SessRow { int slot, len; };   // one row of an admit / retire table

// dst[0, ncopy) = src[0, ncopy), dst[ncopy, ntotal) = 0 over the x-blocks of one grid row
template <bool QUAD>
__device__ __forceinline__ void sess_copy_zero(float* dst, const float* src, int ncopy, int ntotal) {
  if (QUAD) {
    const int nc = ncopy >> 2, nt = ntotal >> 2;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += gridDim.x * blockDim.x) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < nc) v = reinterpret_cast<const f32x4*>(src)[i];
      reinterpret_cast<f32x4*>(dst)[i] = v;
    }
  } else {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ntotal; i += gridDim.x * blockDim.x)
      dst[i] = i < ncopy ? src[i] : 0.f;
  }
}

// request rows (n, T_in, F) -> the slots of tab (slots, maxT, F); pad (slots, maxT) bytes
template <bool QUAD>
__global__ __launch_bounds__(256) void zv_session_admit_kernel(
    const float* x0, const float* tc0, const float* sc0, int T_in, float* x, float* tc, float* sc, uint8_t* pad,
    const SessRow* tab, int maxT, int Fx, int Ft) {
  const SessRow r = tab[blockIdx.y];
  const long src = (long)blockIdx.y * T_in, dst = (long)r.slot * maxT;
  sess_copy_zero<QUAD>(x + dst * Fx, x0 + src * Fx, r.len * Fx, maxT * Fx);
  sess_copy_zero<QUAD>(tc + dst * Ft, tc0 + src * Ft, r.len * Ft, maxT * Ft);
  sess_copy_zero<QUAD>(sc + dst * Fx, sc0 + src * Fx, r.len * Fx, maxT * Fx);
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < maxT; t += gridDim.x * blockDim.x)
    pad[dst + t] = t >= r.len;
}
// the slots of tab -> out rows (n, T_out, Fx)
template <bool QUAD>
__global__ __launch_bounds__(256) void zv_session_retire_kernel(const float* x, float* out, const SessRow* tab,
                                                                int maxT, int T_out, int Fx) {
  const SessRow r = tab[blockIdx.y];
  sess_copy_zero<QUAD>(out + (long)blockIdx.y * T_out * Fx, x + (long)r.slot * maxT * Fx, r.len * Fx, T_out * Fx);
}

// decoder row j, frames [0, Tk) = cat[x, tc, sc] of slot map[j] >> 2 (stride maxT), text / speech
// zeroed by the entry's flags (sched_map_entry)
template <bool QUAD>
__global__ __launch_bounds__(256) void zv_session_build_input_kernel(
    const float* x, const float* tc, const float* sc, bf16* oh, bf16* ol, long ld, const int* map, int Tk,
    int maxT, int Fx, int Ft, int Fs) {
  const int Fin = Fx + Ft + Fs;
  const int e = map[blockIdx.y];
  const long src = (long)(e >> 2) * maxT, dst = (long)blockIdx.y * Tk;
  const bool zt = e & 1, zs = e & 2;
  if (QUAD) {
    const int q = Fin >> 2;
    const int total = Tk * q;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
      const int t = i / q, f = (i - t * q) << 2;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < Fx) v = *reinterpret_cast<const f32x4*>(x + (src + t) * Fx + f);
      else if (f < Fx + Ft) { if (!zt) v = *reinterpret_cast<const f32x4*>(tc + (src + t) * Ft + (f - Fx)); }
      else if (!zs) v = *reinterpret_cast<const f32x4*>(sc + (src + t) * Fs + (f - Fx - Ft));
      float vv[4] = {v[0], v[1], v[2], v[3]};
      store_split4(oh, ol, (dst + t) * ld + f, vv);
    }
  } else {
    const int total = Tk * Fin;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
      const int t = i / Fin, f = i - t * Fin;
      float v;
      if (f < Fx) v = x[(src + t) * Fx + f];
      else if (f < Fx + Ft) v = zt ? 0.f : tc[(src + t) * Ft + (f - Fx)];
      else v = zs ? 0.f : sc[(src + t) * Fs + (f - Fx - Ft)];
      split_store(oh, ol, (dst + t) * ld + f, v);
    }
  }
}
// the padding mask of the decoder rows: out[j, 0 .. Tk) = pad[map[j] >> 2, 0 .. Tk)
__global__ __launch_bounds__(256) void zv_session_gather_u8_kernel(const uint8_t* in, uint8_t* out, const int* map,
                                                                   int Tk, int maxT) {
  const long src = (long)(map[blockIdx.y] >> 2) * maxT, dst = (long)blockIdx.y * Tk;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < Tk; t += gridDim.x * blockDim.x) out[dst + t] = in[src + t];
}
// the Euler step of the active slots: the first per_row values (T_k frames) of slot u.row, whose rows
// are x_stride values apart; v: the decoder batch's velocities, per_row values each
__global__ __launch_bounds__(256) void zv_session_euler_update_kernel(float* x, const float* v, const SchedUpd* upd,
                                                                      long per_row, long x_stride) {
  const SchedUpd u = upd[blockIdx.y];
  float* xr = x + (long)u.row * x_stride;
  const float* vc = v + (long)u.vc * per_row;
  const float* vu = v + (long)(u.vu < 0 ? 0 : u.vu) * per_row;
  const bool cfg = u.vu >= 0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < per_row; i += (long)gridDim.x * blockDim.x) {
    const float vv = cfg ? euler_combine(vc[i], vu[i], u.g) : vc[i];
    xr[i] = euler_step(xr[i], vv, u.dt);
  }
}

// ---- launches (zv_engine::session_* and zv_session_check).  The tables are device arrays whose
// every index the host has checked; grids as the scheduled solve's (sched_grid) ----
static bool sess_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}
static void sess_check_sizes(int maxT, int Fx, int Ft) {
  ZV_REQUIRE(maxT > 0 && Fx > 0 && Ft > 0 && (long)maxT * (2L * Fx + Ft) < (1L << 30),
             "session: frames times input width must stay under 2^30");
}
// form 1: the quad kernel (Fx, Ft multiples of 4, so T_in * F is too, and 16-byte aligned bases)
static EdgeLaunch launch_session_admit(const float* x0, const float* tc0, const float* sc0, int n, int T_in, float* x,
                                       float* tc, float* sc, uint8_t* pad, const SessRow* tab, int maxT, int Fx,
                                       int Ft, hipStream_t s) {
  sess_check_sizes(maxT, Fx, Ft);
  ZV_REQUIRE(T_in > 0 && (long)T_in * std::max(Fx, Ft) < (1L << 30), "session: T_in times width must stay under 2^30");
  const bool quad = Fx % 4 == 0 && Ft % 4 == 0 && sess_aligned16(x0, tc0, sc0) && sess_aligned16(x, tc, sc);
  const long per = (long)maxT * std::max(Fx, Ft);
  const dim3 grid = sched_grid(quad ? per / 4 : per, n);
  if (quad)
    hipLaunchKernelGGL(zv_session_admit_kernel<true>, grid, dim3(256), 0, s, x0, tc0, sc0, T_in, x, tc, sc, pad, tab,
                       maxT, Fx, Ft);
  else
    hipLaunchKernelGGL(zv_session_admit_kernel<false>, grid, dim3(256), 0, s, x0, tc0, sc0, T_in, x, tc, sc, pad, tab,
                       maxT, Fx, Ft);
  ZV_LAUNCH_CHECK();
  return {quad ? 1 : 0, (int)grid.x, 256};
}
static EdgeLaunch launch_session_retire(const float* x, float* out, int n, int T_out, const SessRow* tab, int maxT,
                                        int Fx, hipStream_t s) {
  sess_check_sizes(maxT, Fx, 1);
  ZV_REQUIRE(T_out > 0 && (long)T_out * Fx < (1L << 30), "session: T_out times width must stay under 2^30");
  const bool quad = Fx % 4 == 0 && sess_aligned16(x, out);
  const long per = (long)T_out * Fx;
  const dim3 grid = sched_grid(quad ? per / 4 : per, n);
  if (quad)
    hipLaunchKernelGGL(zv_session_retire_kernel<true>, grid, dim3(256), 0, s, x, out, tab, maxT, T_out, Fx);
  else
    hipLaunchKernelGGL(zv_session_retire_kernel<false>, grid, dim3(256), 0, s, x, out, tab, maxT, T_out, Fx);
  ZV_LAUNCH_CHECK();
  return {quad ? 1 : 0, (int)grid.x, 256};
}
// map (device, N entries, sched_map_entry over slots): decoder rows [0, N) of Tk <= maxT frames
static EdgeLaunch launch_session_build_input(const float* x, const float* tc, const float* sc, bf16* oh, bf16* ol,
                                             long ld, const int* map, int N, int Tk, int maxT, int Fx, int Ft, int Fs,
                                             hipStream_t s) {
  const int Fin = Fx + Ft + Fs;
  ZV_REQUIRE(Tk > 0 && Tk <= maxT && (long)maxT * Fin < (1L << 30),
             "session: 0 < T_k <= max_frames, frames times input width under 2^30");
  const bool quad = Fx % 4 == 0 && Ft % 4 == 0 && Fs % 4 == 0 && ld % 4 == 0;
  const dim3 grid = sched_grid(quad ? (long)Tk * Fin / 4 : (long)Tk * Fin, N);
  if (quad)
    hipLaunchKernelGGL(zv_session_build_input_kernel<true>, grid, dim3(256), 0, s, x, tc, sc, oh, ol, ld, map, Tk, maxT,
                       Fx, Ft, Fs);
  else
    hipLaunchKernelGGL(zv_session_build_input_kernel<false>, grid, dim3(256), 0, s, x, tc, sc, oh, ol, ld, map, Tk, maxT,
                       Fx, Ft, Fs);
  ZV_LAUNCH_CHECK();
  return {quad ? 1 : 0, (int)grid.x, 256};
}
static EdgeLaunch launch_session_gather_u8(const uint8_t* in, uint8_t* out, const int* map, int N, int Tk, int maxT,
                                           hipStream_t s) {
  ZV_REQUIRE(Tk > 0 && Tk <= maxT && maxT < (1 << 30), "session: 0 < T_k <= max_frames < 2^30");
  const dim3 grid = sched_grid(Tk, N);
  hipLaunchKernelGGL(zv_session_gather_u8_kernel, grid, dim3(256), 0, s, in, out, map, Tk, maxT);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
// upd (device, A entries, row: the slot): per_row = T_k Fx values of each, slots x_stride = max_frames Fx apart
static EdgeLaunch launch_session_euler_update(float* x, const float* v, const SchedUpd* upd, int A, long per_row,
                                              long x_stride, hipStream_t s) {
  ZV_REQUIRE(per_row > 0 && per_row <= x_stride, "session: 0 < T_k <= max_frames");
  const dim3 grid = sched_grid(per_row, A);
  hipLaunchKernelGGL(zv_session_euler_update_kernel, grid, dim3(256), 0, s, x, v, upd, per_row, x_stride);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}

// ---- the tick's host plan (zv_engine::session_step, zv_session_plan) ----
// Slot b holds a row when rows[b].num_step > 0; it is active while done[b] < num_step.  The tick is the
// scheduled solve's step (sched_step) over the active slots, in slot order, each at its own index
// k_b = done[b] of its own grid; T_k = the longest active row, exactly (no rounding granule).
struct SessTick {
  SchedStep st;
  int Tk = 0;
};
static SessTick session_tick(const SchedRow* rows, const int* done, const int* lens,
                             const std::vector<std::vector<float>>& ts, int slots, bool distill) {
  SessTick tk;
  std::vector<SchedAct> act;
  for (int b = 0; b < slots; ++b)
    if (rows[b].num_step > 0 && done[b] < rows[b].num_step) {
      act.push_back(SchedAct{b, ts[b][done[b]], ts[b][done[b] + 1], rows[b].g});
      tk.Tk = std::max(tk.Tk, lens[b]);
    }
  tk.st = sched_step(act, distill);
  return tk;
}
constexpr int SESSION_MAX_SLOTS = 32767;   // 2 * slots decoder rows stay inside one grid.y

// ---------------------------------------------------------------------------------------------------
// Edit rows (zv_session_admit_edit / zv_session_retire_edit): a row of a speech edit enters and leaves
// its slot straight from a pool of stored feature frames (the voice store's arena), driven by the
// edit's frame table as zv_edit_gather defines it: rows (dst, src, len), src == -1 a generated segment.
// No (n, T, F) speech condition is built.  Row i's original frame f is pool row off_i + f.
//   admit    x and the text condition as zv_session_admit_kernel (sess_copy_zero); the speech condition
//            by tiles of SE_TILE frames: the first SE_TILE threads find their frame's segment by
//            bisection in the row's table, once per frame, and leave the source frame in LDS (>= 0 a
//            frame of the row's pool range, SE_GEN generated, SE_PAD at or past T_i); then every thread
//            moves 4 features per item (16-byte loads and stores) or one.  The tiles of a row are
//            strided over the grid's x-blocks, so any grid writes the same bytes.
//   retire   the same tiles over [0, T_out): the pool frame on a kept segment, the slot's x on a
//            generated one (everywhere without keep), zero from T_i on; mask = 1 on generated frames.
// No atomics; every output element is written once, by one thread; the pool is read only at the frames
// the host has checked to lie inside [off_i, off_i + L_i).
constexpr int SE_TILE = 16;               // frames per tile
constexpr int SE_GEN = -1, SE_PAD = -2;   // LDS marks: generated frame, frame at or past T_i

// one row of an admit_edit / retire_edit table: T_i = len, the row's segments are seg[3 lo, 3 hi)
struct SessEditRow { int slot, len, off, lo, hi; };

// the source of new frame t of a row: the last segment in [lo, hi) whose dst is <= t (hi > lo: len >= 1)
__device__ __forceinline__ int sess_edit_src(const SessEditRow& r, const int* seg, int t) {
  if (t >= r.len) return SE_PAD;
  int lo = r.lo, hi = r.hi;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg[3L * mid] <= t) lo = mid; else hi = mid;
  }
  const int* sg = seg + 3L * lo;
  return sg[1] < 0 ? SE_GEN : sg[1] + (t - sg[0]);
}

// request rows x0 (n, T_in, Fx), tc0 (n, T_in, Ft) and the pool (pool_rows, Fx) -> the slots of tab
template <bool QUAD>
__global__ __launch_bounds__(256) void zv_session_admit_edit_kernel(
    const float* x0, const float* tc0, int T_in, const float* pool, float* x, float* tc, float* sc, uint8_t* pad,
    const SessEditRow* tab, const int* seg, int maxT, int Fx, int Ft) {
  __shared__ int s_src[SE_TILE];
  const SessEditRow r = tab[blockIdx.y];
  const long src = (long)blockIdx.y * T_in, dst = (long)r.slot * maxT;
  sess_copy_zero<QUAD>(x + dst * Fx, x0 + src * Fx, r.len * Fx, maxT * Fx);
  sess_copy_zero<QUAD>(tc + dst * Ft, tc0 + src * Ft, r.len * Ft, maxT * Ft);
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < maxT; t += gridDim.x * blockDim.x)
    pad[dst + t] = t >= r.len;
  const int per = QUAD ? Fx >> 2 : Fx, W = QUAD ? 4 : 1;   // items per frame, features per item
  const float* pr = pool + (long)r.off * Fx;
  float* so = sc + dst * Fx;
  for (int t0 = blockIdx.x * SE_TILE; t0 < maxT; t0 += gridDim.x * SE_TILE) {   // (uniform over the block)
    if (threadIdx.x < SE_TILE) s_src[threadIdx.x] = sess_edit_src(r, seg, t0 + threadIdx.x);
    __syncthreads();
    for (int i = threadIdx.x; i < SE_TILE * per; i += blockDim.x) {
      const int fr = i / per, c = (i - fr * per) * W;
      const int t = t0 + fr;
      if (t >= maxT) break;                                // fr rises with i
      const int v = s_src[fr];
      const long o = (long)t * Fx + c;
      if (QUAD) {
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (v >= 0) q = *reinterpret_cast<const f32x4*>(pr + (long)v * Fx + c);
        *reinterpret_cast<f32x4*>(so + o) = q;
      } else {
        so[o] = v >= 0 ? pr[(long)v * Fx + c] : 0.f;
      }
    }
    __syncthreads();
  }
}

// the slots of tab -> out rows (n, T_out, Fx) and mask rows (n, T_out) (mask may be null)
template <bool QUAD>
__global__ __launch_bounds__(256) void zv_session_retire_edit_kernel(
    const float* x, const float* pool, float* out, uint8_t* mask, const SessEditRow* tab, const int* seg, int maxT,
    int T_out, int Fx, int keep) {
  __shared__ int s_src[SE_TILE];
  const SessEditRow r = tab[blockIdx.y];
  const int per = QUAD ? Fx >> 2 : Fx, W = QUAD ? 4 : 1;
  const float* pr = pool + (long)r.off * Fx;
  const float* xr = x + (long)r.slot * maxT * Fx;
  float* orow = out + (long)blockIdx.y * T_out * Fx;
  for (int t0 = blockIdx.x * SE_TILE; t0 < T_out; t0 += gridDim.x * SE_TILE) {
    if (threadIdx.x < SE_TILE) {
      const int t = t0 + threadIdx.x;
      const int v = sess_edit_src(r, seg, t);
      s_src[threadIdx.x] = v;
      if (mask && t < T_out) mask[(long)blockIdx.y * T_out + t] = v == SE_GEN;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SE_TILE * per; i += blockDim.x) {
      const int fr = i / per, c = (i - fr * per) * W;
      const int t = t0 + fr;
      if (t >= T_out) break;
      const int v = s_src[fr];
      const long o = (long)t * Fx + c;
      // (t < T_i <= max_frames wherever the slot is read)
      const float* from = v == SE_PAD ? nullptr : (v >= 0 && keep ? pr + (long)v * Fx + c : xr + o);
      if (QUAD) {
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (from) q = *reinterpret_cast<const f32x4*>(from);
        *reinterpret_cast<f32x4*>(orow + o) = q;
      } else {
        orow[o] = from ? *from : 0.f;
      }
    }
    __syncthreads();
  }
}

// ---- the host side of the edit rows: the rules, the table and the launches (zv_engine::session_admit_edit
// / session_retire_edit and zv_session_edit_check run these same functions) ----
// What the rules need of a session: per slot the steps left (-1: free) and the row's length.
struct SessView { int slots, maxT; const int* left; const int* len; };
struct SessEditReq {
  int n;
  const int32_t *slot, *off, *L, *table, *row_ptr;
  int pool_rows;
};
// The table's own rules (zv_edit_gather's, and the pool range); T[i] = the new length of row i.
static void sess_edit_check_tables(const std::string& who, const SessEditReq& e, std::vector<int>& T) {
  ZV_REQUIRE(e.n >= 1, who + " takes at least one row");
  ZV_REQUIRE(e.slot && e.off && e.L && e.row_ptr, who + ": null argument");
  ZV_REQUIRE(e.pool_rows >= 1, who + ": pool_rows must be at least 1");
  ZV_REQUIRE(e.row_ptr[0] == 0, who + ": row_ptr[0] must be 0");
  for (int i = 0; i < e.n; ++i)
    ZV_REQUIRE(e.row_ptr[i + 1] >= e.row_ptr[i], who + " row " + std::to_string(i) + ": row_ptr must not fall");
  ZV_REQUIRE(e.table || e.row_ptr[e.n] == 0, who + ": null table");
  T.assign(e.n, 0);
  for (int i = 0; i < e.n; ++i) {
    const std::string at = who + " row " + std::to_string(i) + ": ";
    const long off = e.off[i], L = e.L[i];
    ZV_REQUIRE(L >= 0 && off >= 0 && off + L <= e.pool_rows, at + "pool range outside [0, pool_rows)");
    long pos = 0;
    for (int k = e.row_ptr[i]; k < e.row_ptr[i + 1]; ++k) {
      const long dst = e.table[3L * k], src = e.table[3L * k + 1], len = e.table[3L * k + 2];
      ZV_REQUIRE(len > 0, at + "segment lengths must be positive");
      ZV_REQUIRE(dst == pos, at + "segments must tile [0, T_i) in order");
      ZV_REQUIRE(src == -1 || (src >= 0 && src + len <= L), at + "kept segment outside [0, L_i)");
      pos += len;
      ZV_REQUIRE(pos < (1L << 30), at + "row longer than 2^30 frames");
    }
    T[i] = (int)pos;
  }
}
static void sess_edit_check_admit(const SessView& q, const SessEditReq& e, const SchedRow* rows, int T_in,
                                  std::vector<int>& T) {
  const std::string who = "session: admit_edit";
  ZV_REQUIRE(rows != nullptr, who + ": null argument");
  ZV_REQUIRE(T_in >= 1, who + ": T_in must be at least 1");
  sess_edit_check_tables(who, e, T);
  std::vector<char> seen(q.slots, 0);
  for (int i = 0; i < e.n; ++i) {
    const std::string at = who + " row " + std::to_string(i) + ": ";
    ZV_REQUIRE(e.slot[i] >= 0 && e.slot[i] < q.slots, at + "slot outside [0, slots)");
    ZV_REQUIRE(q.left[e.slot[i]] < 0, at + "slot is not free");
    ZV_REQUIRE(!seen[e.slot[i]], at + "slot named twice");
    seen[e.slot[i]] = 1;
    ZV_REQUIRE(T[i] >= 1 && T[i] <= T_in && T[i] <= q.maxT, at + "length must be in [1, min(T_in, max_frames)]");
    sched_check_row(rows[i], at);
  }
}
static void sess_edit_check_retire(const SessView& q, const SessEditReq& e, int T_out, std::vector<int>& T) {
  const std::string who = "session: retire_edit";
  sess_edit_check_tables(who, e, T);
  std::vector<char> seen(q.slots, 0);
  for (int i = 0; i < e.n; ++i) {
    const std::string at = who + " row " + std::to_string(i) + ": ";
    ZV_REQUIRE(e.slot[i] >= 0 && e.slot[i] < q.slots, at + "slot outside [0, slots)");
    ZV_REQUIRE(q.left[e.slot[i]] >= 0, at + "slot is free");
    ZV_REQUIRE(q.left[e.slot[i]] == 0, at + "slot has steps left");
    ZV_REQUIRE(!seen[e.slot[i]], at + "slot named twice");
    seen[e.slot[i]] = 1;
    ZV_REQUIRE(T[i] == q.len[e.slot[i]], at + "the table's length is not the slot's");
    ZV_REQUIRE(T_out >= T[i], at + "T_out is shorter than the row");
  }
}
// the device table of a checked request: rows [n] (SessEditRow) | segments [3 nseg]
static size_t sess_edit_words(const SessEditReq& e) { return 5 * (size_t)e.n + 3 * (size_t)e.row_ptr[e.n]; }
static void sess_edit_fill(unsigned* words, const SessEditReq& e, const std::vector<int>& T) {
  static_assert(sizeof(SessEditRow) == 20, "SessEditRow is five 4-byte words");
  SessEditRow* rows = reinterpret_cast<SessEditRow*>(words);
  for (int i = 0; i < e.n; ++i) rows[i] = SessEditRow{e.slot[i], T[i], e.off[i], e.row_ptr[i], e.row_ptr[i + 1]};
  if (e.row_ptr[e.n] > 0) memcpy(words + 5 * (size_t)e.n, e.table, 3 * (size_t)e.row_ptr[e.n] * sizeof(int));
}
// dtab: the device copy of that table.  Forms as launch_session_admit / launch_session_retire.
static EdgeLaunch launch_session_admit_edit(const float* x0, const float* tc0, int n, int T_in, const float* pool,
                                            float* x, float* tc, float* sc, uint8_t* pad, const unsigned* dtab,
                                            int maxT, int Fx, int Ft, hipStream_t s) {
  sess_check_sizes(maxT, Fx, Ft);
  ZV_REQUIRE(T_in > 0 && (long)T_in * std::max(Fx, Ft) < (1L << 30), "session: T_in times width must stay under 2^30");
  const bool quad = Fx % 4 == 0 && Ft % 4 == 0 && sess_aligned16(x0, tc0, pool) && sess_aligned16(x, tc, sc);
  const long per = (long)maxT * std::max(Fx, Ft);
  const dim3 grid = sched_grid(quad ? per / 4 : per, n);
  const SessEditRow* tab = reinterpret_cast<const SessEditRow*>(dtab);
  const int* seg = reinterpret_cast<const int*>(dtab + 5 * (size_t)n);
  if (quad)
    hipLaunchKernelGGL(zv_session_admit_edit_kernel<true>, grid, dim3(256), 0, s, x0, tc0, T_in, pool, x, tc, sc, pad,
                       tab, seg, maxT, Fx, Ft);
  else
    hipLaunchKernelGGL(zv_session_admit_edit_kernel<false>, grid, dim3(256), 0, s, x0, tc0, T_in, pool, x, tc, sc, pad,
                       tab, seg, maxT, Fx, Ft);
  ZV_LAUNCH_CHECK();
  return {quad ? 1 : 0, (int)grid.x, 256};
}
static EdgeLaunch launch_session_retire_edit(const float* x, const float* pool, float* out, uint8_t* mask, int n,
                                             int T_out, const unsigned* dtab, int maxT, int Fx, bool keep,
                                             hipStream_t s) {
  sess_check_sizes(maxT, Fx, 1);
  ZV_REQUIRE(T_out > 0 && (long)T_out * Fx < (1L << 30), "session: T_out times width must stay under 2^30");
  const bool quad = Fx % 4 == 0 && sess_aligned16(x, pool, out);
  const long per = (long)T_out * Fx;
  const dim3 grid = sched_grid(quad ? per / 4 : per, n);
  const SessEditRow* tab = reinterpret_cast<const SessEditRow*>(dtab);
  const int* seg = reinterpret_cast<const int*>(dtab + 5 * (size_t)n);
  if (quad)
    hipLaunchKernelGGL(zv_session_retire_edit_kernel<true>, grid, dim3(256), 0, s, x, pool, out, mask, tab, seg, maxT,
                       T_out, Fx, keep ? 1 : 0);
  else
    hipLaunchKernelGGL(zv_session_retire_edit_kernel<false>, grid, dim3(256), 0, s, x, pool, out, mask, tab, seg, maxT,
                       T_out, Fx, keep ? 1 : 0);
  ZV_LAUNCH_CHECK();
  return {quad ? 1 : 0, (int)grid.x, 256};
}
