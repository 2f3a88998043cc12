// Memory-bound helper kernels of the ZipVoice decoder layer and Euler loop.
// All are HBM-bound (bytes per element >> flops): vectorised 16-B accesses
// where the row width allows, one wave per row for row reductions.
#pragma once
#include <cmath>

#include "zv_common.h"
#include "zv_gemm.inc"

// ---- decoder input: xt = cat[x, text_c, speech_c] with CFG batch doubling --
// (this kernel, its quad form, the Euler / CFG, fill, timestep, posP and small-linear kernels below and
// the mask copy and text-side kernels at the end of the file are pinned against float64 through their
// launch functions: zv_solve_check, tests/test_gpu_solve_ref.py)
// DiffusionModel.forward (solver.py:83-98) + forward_fm_decoder (zipvoice.py:163).
// rows [0,B) = uncond (text zeroed; speech zeroed iff zero_speech_uncond),
// rows [B,2B) = cond.  Without CFG (ncopies = 1) row b = cond.  Written as the
// bf16 hi/lo GEMM operand of in_proj (row stride ld >= Fin, pad columns 0).
__global__ void zv_build_input_kernel(const float* x, const float* tc, const float* sc,
                                      bf16* oh, bf16* ol, long ld, int B, int T, int Fx, int Ft,
                                      int Fs, int ncopies, int zero_speech_uncond) {
  const int Fin = Fx + Ft + Fs;
  const long total = (long)ncopies * B * T * Fin;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int f = (int)(idx % Fin);
    const long row = idx / Fin;          // (copy*B + b)*T + t
    const long bt = row % ((long)B * T);
    const int copy = (int)(row / ((long)B * T));
    const bool uncond = (ncopies == 2 && copy == 0);
    float v;
    if (f < Fx) v = x[bt * Fx + f];
    else if (f < Fx + Ft) v = uncond ? 0.f : tc[bt * Ft + (f - Fx)];
    else v = (uncond && zero_speech_uncond) ? 0.f : sc[bt * Fs + (f - Fx - Ft)];
    split_store(oh, ol, row * ld + f, v);
  }
}

// the same with 4 consecutive features per thread (Fx, Ft, Fs and ld multiples of 4: every
// quad lies inside one source segment, f32x4 loads, one 8-byte store per half); one row
// per 32-bit quotient instead of the 64-bit division per element above.  C2 (64 x 1219 x
// 300): 67.5 us -> (with posP reuse) C2 step -2.6 ms, profiles/r05_posp_reuse_ab.txt
__global__ __launch_bounds__(256) void zv_build_input4_kernel(
    const float* x, const float* tc, const float* sc, bf16* oh, bf16* ol, long ld, int B, int T,
    int Fx, int Ft, int Fs, int ncopies, int zero_speech_uncond) {
  const int q = (Fx + Ft + Fs) >> 2;              // quads per row
  const int bt_rows = B * T;
  const long total = (long)ncopies * bt_rows * q;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int row = (int)(i / q);                 // (copy*B + b)*T + t
    const int f = (int)(i - (long)row * q) << 2;
    const bool uncond = ncopies == 2 && row < bt_rows;
    const int bt = uncond || ncopies == 1 ? row : row - bt_rows;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (f < Fx) v = *reinterpret_cast<const f32x4*>(x + (long)bt * Fx + f);
    else if (f < Fx + Ft) { if (!uncond) v = *reinterpret_cast<const f32x4*>(tc + (long)bt * Ft + (f - Fx)); }
    else if (!(uncond && zero_speech_uncond))
      v = *reinterpret_cast<const f32x4*>(sc + (long)bt * Fs + (f - Fx - Ft));
    float vv[4] = {v[0], v[1], v[2], v[3]};
    store_split4(oh, ol, (long)row * ld + f, vv);
  }
}

// ---- Euler step with CFG combine (solver.py:100-110, :239) -----------------
// v = (1+g) v_cond - g v_uncond;  x = x + v * dt     (cfg)
// x = x + v * dt                                      (no cfg)
// g per row when grows is given (guidance_scale of shape (batch, 1, 1), solver.py:61-62):
// g_b = grows[b] * gmul (gmul = 2 where t <= 0.5 doubles the scale, solver.py:95)
// (the arithmetic as device functions: this kernel and the scheduled one below inline the same
// expressions, so the compiler contracts both into the same FMAs)
__device__ __forceinline__ float euler_combine(float vc, float vu, float g) { return (1.0f + g) * vc - g * vu; }
__device__ __forceinline__ float euler_step(float x, float vv, float dt) { return x + vv * dt; }

__global__ void zv_euler_update_kernel(float* x, const float* v, long n, int cfg, float g,
                                       float dt, const float* grows, float gmul, long per_row) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    float vv;
    if (cfg) {
      const float gi = grows ? grows[i / per_row] * gmul : g;
      vv = euler_combine(v[n + i], v[i], gi);
    } else {
      vv = v[i];
    }
    x[i] = euler_step(x[i], vv, dt);
  }
}

// ---- the scheduled solve's kernels (zv_engine::euler_sample_sched) ----------
// One call integrates rows with their own step counts, grids and guidance scales: a step's decoder
// batch holds only the rows that still have steps left, the needed unconditional copies first.  The
// host plans every step (sched_plan below) and uploads the tables once per solve; these kernels do
// zv_build_input_kernel's / zv_copy_u8_kernel's / zv_euler_update_kernel's job through them.  One
// decoder (or active) row per blockIdx.y: its table entry is a wave-uniform load, once per block.
// A row map entry: (source input row << 2) | zero_speech << 1 | zero_text.
__host__ __device__ static inline int sched_map_entry(int src, bool zero_text, bool zero_speech) {
  return (src << 2) | (zero_speech ? 2 : 0) | (zero_text ? 1 : 0);
}
// An active row's update: x[row] += vv dt with vv = (1 + g) v[vc] - g v[vu], or v[vc] where vu < 0.
struct SchedUpd { int row; float dt, g; int vc, vu; };

// decoder row j = cat[x, text_c, speech_c] of input row map[j] >> 2, text / speech zeroed by its flags
__global__ __launch_bounds__(256) void zv_build_input_map_kernel(
    const float* x, const float* tc, const float* sc, bf16* oh, bf16* ol, long ld, const int* map, int T,
    int Fx, int Ft, int Fs) {
  const int Fin = Fx + Ft + Fs;
  const int e = map[blockIdx.y];
  const long src = (long)(e >> 2) * T, dst = (long)blockIdx.y * T;
  const bool zt = e & 1, zs = e & 2;
  const int total = T * Fin;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int t = i / Fin, f = i - t * Fin;
    float v;
    if (f < Fx) v = x[(src + t) * Fx + f];
    else if (f < Fx + Ft) v = zt ? 0.f : tc[(src + t) * Ft + (f - Fx)];
    else v = zs ? 0.f : sc[(src + t) * Fs + (f - Fx - Ft)];
    split_store(oh, ol, (dst + t) * ld + f, v);
  }
}
// the quad form (Fx, Ft, Fs and ld multiples of 4), as zv_build_input4_kernel
__global__ __launch_bounds__(256) void zv_build_input_map4_kernel(
    const float* x, const float* tc, const float* sc, bf16* oh, bf16* ol, long ld, const int* map, int T,
    int Fx, int Ft, int Fs) {
  const int q = (Fx + Ft + Fs) >> 2;              // quads per frame
  const int e = map[blockIdx.y];
  const long src = (long)(e >> 2) * T, dst = (long)blockIdx.y * T;
  const bool zt = e & 1, zs = e & 2;
  const int total = T * q;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int t = i / q, f = (i - t * q) << 2;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (f < Fx) v = *reinterpret_cast<const f32x4*>(x + (src + t) * Fx + f);
    else if (f < Fx + Ft) { if (!zt) v = *reinterpret_cast<const f32x4*>(tc + (src + t) * Ft + (f - Fx)); }
    else if (!zs) v = *reinterpret_cast<const f32x4*>(sc + (src + t) * Fs + (f - Fx - Ft));
    float vv[4] = {v[0], v[1], v[2], v[3]};
    store_split4(oh, ol, (dst + t) * ld + f, vv);
  }
}
// the padding mask of the decoder rows: out[j] = in[map[j] >> 2], T bytes each
__global__ __launch_bounds__(256) void zv_gather_u8_kernel(const uint8_t* in, uint8_t* out, const int* map, int T) {
  const long src = (long)(map[blockIdx.y] >> 2) * T, dst = (long)blockIdx.y * T;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T; t += gridDim.x * blockDim.x) out[dst + t] = in[src + t];
}
// the Euler step of the active rows, scattered into x at their input rows (v: the decoder batch's
// velocities, per_row values each); rows outside the list are not touched
__global__ __launch_bounds__(256) void zv_euler_update_sched_kernel(float* x, const float* v, const SchedUpd* upd,
                                                                    long per_row) {
  const SchedUpd u = upd[blockIdx.y];
  float* xr = x + (long)u.row * per_row;
  const float* vc = v + (long)u.vc * per_row;
  const float* vu = v + (long)(u.vu < 0 ? 0 : u.vu) * per_row;
  const bool cfg = u.vu >= 0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < per_row; i += (long)gridDim.x * blockDim.x) {
    const float vv = cfg ? euler_combine(vc[i], vu[i], u.g) : vc[i];
    xr[i] = euler_step(xr[i], vv, u.dt);
  }
}
// completion mark of a staged upload: a host-mapped word takes the upload's sequence number
__global__ void zv_mark_kernel(unsigned* word, unsigned seq) {
  *reinterpret_cast<volatile unsigned*>(word) = seq;
  __threadfence_system();
}

// CFG combine only (forward_fm_decoder-level API): out = (1+g) vc - g vu
__global__ void zv_cfg_combine_kernel(float* out, const float* v, long n, float g,
                                      const float* grows, float gmul, long per_row) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float gi = grows ? grows[i / per_row] * gmul : g;
    out[i] = (1.0f + gi) * v[n + i] - gi * v[i];
  }
}

__global__ void zv_fill_kernel(float* p, float v, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- sinusoidal timestep embedding (zipformer.py:47-69) --------------------
// out[m, :half] = cos(t_m f_k), out[m, half:] = sin(t_m f_k); f_k passed in.
__global__ void zv_timestep_embed_kernel(const float* t, const float* freqs, float* out,
                                         int M, int dim) {
  const int half = dim / 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * dim) return;
  const int m = idx / dim, k = idx % dim;
  float v = 0.f;
  if (k < half) v = cosf(t[m] * freqs[k]);
  else if (k < 2 * half) v = sinf(t[m] * freqs[k - half]);
  out[idx] = v;
}

// ---- relative positional encoding + linear_pos of every layer of a stack -----
// CompactRelPositionalEncoding.extend_pe (zipformer.py:983-1032, float32: row n encodes
// offset x = n - (L-1); x_c = c sgn(x) (ln(|x| + c) - ln c), c = sqrt(D); a = atan(x_c /
// (D / 2pi)); pe[2k] = cos(a (k+1)), pe[2k+1] = sin(a (k+1)); pe[D-1] = 1) followed by
// linear_pos (no bias, zipformer.py:1239).  One thread per (layer, row, output column):
// the D-wide pe row is recomputed per thread in registers (cheap next to the latency of
// a serial 16-column loop; 16x the threads fill the chip), out[l][n][c] = sum_k pe[k] W_l[c][k]
// in the same k order as before.
constexpr int POSP_MAXD = 64;
__global__ __launch_bounds__(256) void zv_posp_kernel(const float* __restrict__ W, float* out,
                                                      int L, int nl, int HPD, int D) {
  const long R = 2L * L - 1;
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= R * nl * HPD) return;
  const int cc = (int)(idx % HPD);
  const long ln = idx / HPD;
  const int l = (int)(ln / R);
  const long n = ln % R;
  const float x = (float)(n - (L - 1));
  const float c = sqrtf((float)D);
  const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
  const float xc = c * sg * (logf(fabsf(x) + c) - logf(c));
  const float xa = atanf(xc / (float)((double)D / (2.0 * M_PI)));
  const float* w = W + ((long)l * HPD + cc) * D;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < POSP_MAXD / 2; ++k) {
    if (2 * k < D) {
      const float a = xa * (float)(k + 1);
      const float pc = cosf(a), ps = sinf(a);
      acc = fmaf(2 * k == D - 1 ? 1.0f : pc, w[2 * k], acc);
      if (2 * k + 1 < D) acc = fmaf(2 * k + 1 == D - 1 ? 1.0f : ps, w[2 * k + 1], acc);
    }
  }
  out[ln * HPD + cc] = acc;
}

// ---- small fp32 linear for the time / guidance / positional MLPs -----------
// out[m,n] = sum_k pre(in[m,k]) W[n,k] + b[n] (+ add[m,n]);  pre: 0 id, 1 SwooshR(logaddexp)
// one wave per output: lanes stride K (coalesced weight rows), shuffle reduction
__global__ __launch_bounds__(256) void zv_small_linear_kernel(
    const float* in, int ldin, const float* W, int ldw, const float* b, const float* add,
    float* out, int ldout, int M, int N, int K, int pre) {
  const long o = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= (long)M * N) return;
  const int m = (int)(o / N), n = (int)(o % N);
  const float* xr = in + (long)m * ldin;
  const float* wr = W + (long)n * ldw;
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) {
    float xv = xr[k];
    if (pre == 1) xv = swoosh_r_lae(xv);
    acc = fmaf(xv, wr[k], acc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) {
    if (b) acc += b[n];
    if (add) acc += add[(long)m * ldout + n];
    out[(long)m * ldout + n] = acc;
  }
}

// The same linear, one block per (input row, 32 outputs): the row (SwooshR-activated when
// pre == 1) is staged in LDS once per block and the 4 waves take 8 outputs each; per output
// the identical lane-strided sum and xor-tree as zv_small_linear_kernel (bitwise equal),
// with the activation evaluated N / 32 times per input element instead of N times.
constexpr int SL_NB = 32;
__global__ __launch_bounds__(256) void zv_small_linear_rows_kernel(
    const float* in, int ldin, const float* W, int ldw, const float* b, const float* add,
    float* out, int ldout, int M, int N, int K, int pre) {
  extern __shared__ float xs_row[];
  const int m = blockIdx.x, n0 = blockIdx.y * SL_NB;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float xv = in[(long)m * ldin + k];
    xs_row[k] = pre == 1 ? swoosh_r_lae(xv) : xv;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // a wave's 8 outputs n0 + wave + 4 j side by side: their weight loads are in flight together
  // (one output after another, each waited for its own loads: ~20 us per launch of a few rows)
  constexpr int NPW = SL_NB / 4;
  float acc[NPW];
  const float* wr[NPW];
#pragma unroll
  for (int j = 0; j < NPW; ++j) {
    acc[j] = 0.f;
    wr[j] = W + (long)min(n0 + wave + 4 * j, N - 1) * ldw;
  }
  for (int k = lane; k < K; k += 64) {
    const float xv = xs_row[k];
#pragma unroll
    for (int j = 0; j < NPW; ++j) acc[j] = fmaf(xv, wr[j][k], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < NPW; ++j) {
    const int n = n0 + wave + 4 * j;
    float a = acc[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0 && n < N) {
      if (b) a += b[n];
      if (add) a += add[(long)m * ldout + n];
      out[(long)m * ldout + n] = a;
    }
  }
}

// ---- depthwise conv1d ("same" padding, bias) + SwooshR (zipformer.py:1672, ----
// scaling.py:1185-1191).  in/out: bf16 hi/lo activations (B, L, C), row stride ld.
// The four kernels below are pinned against float64 through launch_dwconv's own dispatch
// (zv_dwconv_check, tests/test_gpu_dwconv_ref.py): every kernel-size instantiation, every
// utterance edge, the LDS forms' tile and chunk edges.
// One workgroup = (64 frames, 64 channels, item): the input window incl. the
// (ks-1) halo frames is staged once in LDS as fp32, each thread then produces
// 16 frames of one channel from registers-held taps.
constexpr int DW_TL = 64, DW_TC = 64, DW_MAXK = 63;
template <int KS>   // KS = 0: runtime kernel size (taps read from L1)
__global__ __launch_bounds__(256) void zv_dwconv_swooshr_kernel(
    const bf16* ih, const bf16* il, long ldin, const float* w, const float* bias, bf16* oh,
    bf16* ol, long ldout, int L, int C, int ks_rt) {
  __shared__ float tile[(DW_TL + DW_MAXK) * DW_TC];
  const int ks = KS ? KS : ks_rt;
  const int l0 = blockIdx.x * DW_TL, c0 = blockIdx.y * DW_TC, b = blockIdx.z;
  const int pad = ks / 2, rows = DW_TL + ks - 1;
  const long base = (long)b * L;
  for (int idx = threadIdx.x; idx < rows * DW_TC; idx += 256) {
    const int rr = idx / DW_TC, cc = idx % DW_TC;
    const int l = l0 - pad + rr, c = c0 + cc;
    float v = 0.f;
    if (l >= 0 && l < L && c < C) v = ld_split(ih, il, (base + l) * ldin + c);
    tile[idx] = v;
  }
  __syncthreads();
  const int cc = threadIdx.x & 63, c = c0 + cc;
  if (c >= C) return;
  const float* wc = w + (long)c * ks;
  const float bc = bias[c];
  if constexpr (KS > 0) {
    float wr[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t) wr[t] = wc[t];
    for (int q = threadIdx.x >> 6; q < DW_TL; q += 4) {
      const int l = l0 + q;
      if (l >= L) break;
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < KS; ++t) acc = fmaf(tile[(q + t) * DW_TC + cc], wr[t], acc);
      split_store(oh, ol, (base + l) * ldout + c, swoosh_r(acc + bc));
    }
  } else {
    for (int q = threadIdx.x >> 6; q < DW_TL; q += 4) {
      const int l = l0 + q;
      if (l >= L) break;
      float acc = 0.f;
      for (int t = 0; t < ks; ++t) acc = fmaf(tile[(q + t) * DW_TC + cc], wc[t], acc);
      split_store(oh, ol, (base + l) * ldout + c, swoosh_r(acc + bc));
    }
  }
}

// Register-window form for the model's kernel sizes: one thread = 2 adjacent
// channels x DW_R consecutive frames; its (DW_R + KS - 1)-frame input window is
// read straight from global (4-B bf16 pairs, the halo re-reads hit L1/L2) into
// registers, so every input feeds KS FMAs without LDS traffic.
constexpr int DW_R = 8;
// Q8 (fp8 mode): also the output's MX-fp8 copy (q (rows, ldq), scales qs): a 32-channel
// block is 16 adjacent lanes of one frame (C % 128 == 0: whole waves, host checks)
template <int KS, bool LO, bool Q8 = false>
__global__ __launch_bounds__(256) void zv_dwconv_win_kernel(
    const bf16* ih, const bf16* il, long ldin, const float* w, const float* bias, bf16* oh,
    bf16* ol, long ldout, int L, int C, uint8_t* q = nullptr, uint8_t* qs = nullptr, long ldq = 0) {
  constexpr int NW = DW_R + KS - 1, PAD = KS / 2;
  const int c = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2;
  const int f0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * DW_R;
  const int b = blockIdx.z;
  if (c >= C || f0 >= L) return;
  const long base = (long)b * L;
  // unconditional (clamped) loads, zeroed outside the item: all in flight at once
  bf16x2 vh[NW], vl[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int l = min(max(f0 - PAD + i, 0), L - 1);
    vh[i] = *reinterpret_cast<const bf16x2*>(ih + (base + l) * ldin + c);
    if constexpr (LO) vl[i] = *reinterpret_cast<const bf16x2*>(il + (base + l) * ldin + c);
  }
  float w0[KS], w1[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) { w0[t] = w[(long)c * KS + t]; w1[t] = w[(long)(c + 1) * KS + t]; }
  const float b0 = bias[c], b1 = bias[c + 1];
  float x0[NW], x1[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int l = f0 - PAD + i;
    const bool in = l >= 0 && l < L;
    float a = (float)vh[i][0], bb = (float)vh[i][1];
    if constexpr (LO) { a += (float)vl[i][0]; bb += (float)vl[i][1]; }
    x0[i] = in ? a : 0.f;
    x1[i] = in ? bb : 0.f;
  }
#pragma unroll
  for (int r = 0; r < DW_R; ++r) {
    if (f0 + r >= L) break;
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int t = 0; t < KS; ++t) { a0 = fmaf(x0[r + t], w0[t], a0); a1 = fmaf(x1[r + t], w1[t], a1); }
    const float y0 = swoosh_r(a0 + b0), y1 = swoosh_r(a1 + b1);
    const long o = (base + f0 + r) * ldout + c;
    const bf16 h0 = (bf16)y0, h1 = (bf16)y1;
    *reinterpret_cast<bf16x2*>(oh + o) = bf16x2{h0, h1};
    if constexpr (LO)
      *reinterpret_cast<bf16x2*>(ol + o) = bf16x2{(bf16)(y0 - (float)h0), (bf16)(y1 - (float)h1)};
    if constexpr (Q8) {
      unsigned sb;
      const float yy[2] = {(float)h0, (float)h1};   // from the bf16 output: == packing it
      const unsigned q2 = mx8_quant2(yy, sb);
      const long row = base + f0 + r;
      *reinterpret_cast<unsigned short*>(q + row * ldq + c) = (unsigned short)q2;
      if ((c & 31) == 0) qs[row * (ldq / MX8_BLOCK) + c / MX8_BLOCK] = (uint8_t)sb;
    }
  }
}

// LDS-staged form (16-bit single operands, C % 128 == 0): a 512-thread block covers 128
// channels x 64 frames; its (64 + KS - 1)-row input window (256 B per row) is staged by
// LDS-DMA (one HBM read per input row; rows outside the item read a zero row), then each
// thread runs the register-window arithmetic above on 2 channels x 8 frames from LDS
// (same FMA order: bitwise equal).  The global form re-read every row 4.75x from L2 with
// 4-B loads and sat on their latency.
constexpr int DWL_FT = 64;
template <int KS>
__global__ __launch_bounds__(512) void zv_dwconv_lds_kernel(const bf16* ih, long ldin, const float* w,
                                                            const float* bias, bf16* oh, long ldout, int L,
                                                            const bf16* zero_row) {
  constexpr int NW = DW_R + KS - 1, PAD = KS / 2, R = DWL_FT + KS - 1, NI = (R + 3) / 4;
  __shared__ __attribute__((aligned(16))) unsigned char tile[NI * 1024];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = blockIdx.x * 128, f0 = blockIdx.y * DWL_FT, b = blockIdx.z;
  const long base = (long)b * L;
#pragma unroll
  for (int i = wave; i < NI; i += 8) {          // DMA piece i: rows 4i .. 4i + 3
    const int l = f0 - PAD + 4 * i + (lane >> 4);
    const bf16* src = (l >= 0 && l < L && 4 * i + (lane >> 4) < R)
                          ? ih + (base + l) * ldin + c0 + (lane & 15) * 8
                          : zero_row + (lane & 15) * 8;
    glds16(src, tile + i * 1024);
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  const int c = c0 + 2 * lane, fw = wave * DW_R;
  if (f0 + fw >= L) return;
  // the channel pair as packed f32 (v_pk_fma_f32: both channels per instruction); all DW_R
  // frames computed unconditionally (rows past the item are zeros in LDS) so the DW_R
  // independent chains interleave — a per-frame exit had serialised them into one dependent
  // chain with hazard nops between the packed FMAs; only the stores are guarded
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  f32x2_t w2[KS], x2[NW], a2[DW_R];
#pragma unroll
  for (int t = 0; t < KS; ++t) w2[t] = f32x2_t{w[(long)c * KS + t], w[(long)(c + 1) * KS + t]};
  const f32x2_t b2 = {bias[c], bias[c + 1]};
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const bf16x2 v = *reinterpret_cast<const bf16x2*>(tile + (fw + i) * 256 + lane * 4);
    x2[i] = f32x2_t{(float)v[0], (float)v[1]};
  }
#pragma unroll
  for (int r = 0; r < DW_R; ++r) a2[r] = f32x2_t{0.f, 0.f};
#pragma unroll
  for (int t = 0; t < KS; ++t) {
#pragma unroll
    for (int r = 0; r < DW_R; ++r) a2[r] = __builtin_elementwise_fma(x2[r + t], w2[t], a2[r]);
    __builtin_amdgcn_sched_barrier(0);   // keep the tap-major order (the scheduler would serialise a chain)
  }
#pragma unroll
  for (int r = 0; r < DW_R; ++r) {
    const f32x2_t z = a2[r] + b2;
    const float y0 = swoosh_r(z[0]), y1 = swoosh_r(z[1]);
    if (f0 + fw + r < L)
      *reinterpret_cast<bf16x2*>(oh + (base + f0 + fw + r) * ldout + c) = bf16x2{(bf16)y0, (bf16)y1};
  }
}

// Pipelined LDS form: one block per (128-channel tile, frame chunk of nft 64-frame tiles,
// utterance) keeps its channels' taps in registers and double-buffers the tile windows: the
// DMA of tile i + 1 is in flight while tile i computes (the one-tile-per-block form above ran
// load, barrier, compute in sequence at one 8-wave block per CU: 90 us at k = 31 against
// ~30 us of HBM traffic).  Same FMA order per output as the forms above (bitwise equal).
template <int KS>
__global__ __launch_bounds__(512) void zv_dwconv_pipe_kernel(const bf16* ih, long ldin, const float* w,
                                                             const float* bias, bf16* oh, long ldout, int L,
                                                             int nft, const bf16* zero_row) {
  constexpr int NW = DW_R + KS - 1, PAD = KS / 2, R = DWL_FT + KS - 1, NI = (R + 3) / 4;
  constexpr int PW = (NI + 7) / 8;               // DMA pieces per wave per tile (some waves idle)
  __shared__ __attribute__((aligned(16))) unsigned char tile[2][PW * 8 * 1024];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = blockIdx.x * 128, b = blockIdx.z;
  const int t0 = blockIdx.y * nft, nt = min(nft, cdiv(L, DWL_FT) - t0);
  if (nt <= 0) return;
  const long base = (long)b * L;
  auto issue = [&](int t, int buf) {
    const int f0 = (t0 + t) * DWL_FT;
#pragma unroll
    for (int k = 0; k < PW; ++k) {
      const int i = wave + 8 * k;                // piece i: window rows 4i .. 4i + 3
      const int row = 4 * i + (lane >> 4), l = f0 - PAD + row;
      const bf16* src = (i < NI && row < R && l >= 0 && l < L) ? ih + (base + l) * ldin + c0 + (lane & 15) * 8
                                                               : zero_row + (lane & 15) * 8;
      // pieces past the window (i >= NI: every wave issues PW, so vmcnt counts are uniform)
      // load the zero row into slots nothing reads
      glds16(src, tile[buf] + i * 1024);
    }
  };
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const int c = c0 + 2 * lane, fw = wave * DW_R;
  f32x2_t w2[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) w2[t] = f32x2_t{w[(long)c * KS + t], w[(long)(c + 1) * KS + t]};
  const f32x2_t b2 = {bias[c], bias[c + 1]};
  issue(0, 0);
  for (int i = 0; i < nt; ++i) {
    if (i + 1 < nt) {
      issue(i + 1, (i + 1) & 1);
      wait_vmcnt<PW>();                          // tile i landed (and every older store)
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    const int f0 = (t0 + i) * DWL_FT;
    const unsigned char* tb = tile[i & 1];
    f32x2_t x2[NW], a2[DW_R];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const bf16x2 v = *reinterpret_cast<const bf16x2*>(tb + (fw + j) * 256 + lane * 4);
      x2[j] = f32x2_t{(float)v[0], (float)v[1]};
    }
#pragma unroll
    for (int r = 0; r < DW_R; ++r) a2[r] = f32x2_t{0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KS; ++t) {
#pragma unroll
      for (int r = 0; r < DW_R; ++r) a2[r] = __builtin_elementwise_fma(x2[r + t], w2[t], a2[r]);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int r = 0; r < DW_R; ++r) {
      const f32x2_t z = a2[r] + b2;
      const float y0 = swoosh_r(z[0]), y1 = swoosh_r(z[1]);
      if (f0 + fw + r < L)
        *reinterpret_cast<bf16x2*>(oh + (base + f0 + fw + r) * ldout + c) = bf16x2{(bf16)y0, (bf16)y1};
    }
    __builtin_amdgcn_s_barrier();                // every wave is done with this buffer (tile i + 2 lands there)
  }
}

// ZV_DWCONV_PIPE: the pipelined LDS form for 16-bit single operands (1 auto chunk, > 1 fixed chunk)
static int dwconv_pipe_default() {
  const char* e = getenv("ZV_DWCONV_PIPE");
  return e ? atoi(e) : 1;
}

// ZV_DWCONV_LDS=0: the register-window kernel reading global memory (A/B arm)
static bool dwconv_lds_default() {
  const char* e = getenv("ZV_DWCONV_LDS");    // read per launch: A/B tests switch it in-process
  return !e || atoi(e) != 0;
}

static void launch_dwconv(const bf16* ih, const bf16* il, long ldin, const float* w,
                          const float* bias, bf16* oh, bf16* ol, long ldout, int B, int L, int C,
                          int ks, hipStream_t s, uint8_t* q = nullptr, uint8_t* qs = nullptr, long ldq = 0) {
  if (ks > DW_MAXK || ks % 2 == 0) throw std::invalid_argument("conv kernel size must be odd <= 63");
  dim3 grid(cdiv(L, DW_TL), cdiv(C, DW_TC), B);
  dim3 wgrid(cdiv(C / 2, 64), cdiv(cdiv(L, DW_R), 4), B);
  const bool win = C % 2 == 0 && ldin % 2 == 0 && ldout % 2 == 0;
  // algorithmic bytes: bf16 in + out (hi/lo pairs in the fp32-accurate mode)
  ZvProfScope prof(il ? "dwconv_fp32" : "dwconv_bf16", 2.0 * ks * (double)B * L * C,
                   (il ? 8.0 : 4.0) * (double)B * L * C, s);
#define ZV_DW(K) hipLaunchKernelGGL((zv_dwconv_swooshr_kernel<K>), grid, dim3(256), 0, s, ih, il, \
                                    ldin, w, bias, oh, ol, ldout, L, C, ks)
#define ZV_DWW(K)                                                                               \
  do {                                                                                          \
    if (il) hipLaunchKernelGGL((zv_dwconv_win_kernel<K, true>), wgrid, dim3(256), 0, s, ih, il, \
                               ldin, w, bias, oh, ol, ldout, L, C, nullptr, nullptr, 0L);       \
    else if (q) hipLaunchKernelGGL((zv_dwconv_win_kernel<K, false, true>), wgrid, dim3(256), 0, \
                                   s, ih, il, ldin, w, bias, oh, ol, ldout, L, C, q, qs, ldq);  \
    else hipLaunchKernelGGL((zv_dwconv_win_kernel<K, false>), wgrid, dim3(256), 0, s, ih, il,   \
                            ldin, w, bias, oh, ol, ldout, L, C, nullptr, nullptr, 0L);          \
  } while (0)
  ZV_REQUIRE(!q || (win && !il && C % 128 == 0 && ldq % MX8_KSTEP == 0 &&
                    (ks == 7 || ks == 9 || ks == 15 || ks == 31)),
             "depthwise conv fp8 copy: register-window kernel, C % 128 == 0");
  // LDS-staged kernel: bf16 operands, whole 128-channel tiles, 16-B aligned rows
  // (k = 31: the register-window kernel is faster: 78 vs 90 us per full-length launch,
  // profiles/r03_prof2_kernel_stats.csv; k <= 15: the LDS form, 25.8 vs 27.8 us)
  const bool lds = dwconv_lds_default() && ks <= 15 && !il && !q && C % 128 == 0 && ldin % 8 == 0 &&
                   ldout % 2 == 0;
#define ZV_DWL(K) hipLaunchKernelGGL((zv_dwconv_lds_kernel<K>), dim3(C / 128, cdiv(L, DWL_FT), B), dim3(512), 0, s, \
                                     ih, ldin, w, bias, oh, ldout, L, reinterpret_cast<const bf16*>(zv_epi_zero()))
  const int pipe = dwconv_pipe_default();
  const bool pok = pipe && !il && !q && C % 128 == 0 && ldin % 8 == 0 && ldout % 2 == 0;
  // frame chunk: enough blocks to fill the chip (>= ~2 per CU), at least 2 tiles each
  const int ntile = cdiv(L, DWL_FT);
  int nft = std::max(2, (int)std::min<long>(ntile, (long)ntile * (C / 128) * B / (2 * zv_num_cus())));
  if (pipe > 1) nft = pipe;                      // A/B: a fixed chunk
  const dim3 pgrid(C / 128, cdiv(ntile, nft), B);
#define ZV_DWP(K) hipLaunchKernelGGL((zv_dwconv_pipe_kernel<K>), pgrid, dim3(512), 0, s, ih, ldin, w, bias, \
                                     oh, ldout, L, nft, reinterpret_cast<const bf16*>(zv_epi_zero()))
  // (the LDS form has no k = 31 instantiation: `lds` requires ks <= 15)
  const bool model_ks = ks == 7 || ks == 9 || ks == 15 || ks == 31;
  const int kind = pok && model_ks ? 3 : lds && model_ks ? 2 : win && model_ks ? 1 : 0;
  if (pok && ks == 7) ZV_DWP(7);
  else if (pok && ks == 9) ZV_DWP(9);
  else if (pok && ks == 15) ZV_DWP(15);
  else if (pok && ks == 31) ZV_DWP(31);
  else if (lds && ks == 7) ZV_DWL(7);
  else if (lds && ks == 9) ZV_DWL(9);
  else if (lds && ks == 15) ZV_DWL(15);
  else if (win && ks == 7) ZV_DWW(7);
  else if (win && ks == 9) ZV_DWW(9);
  else if (win && ks == 15) ZV_DWW(15);
  else if (win && ks == 31) ZV_DWW(31);
  else ZV_DW(0);
  {   // which kernel and grid (test infrastructure, zv_dwconv_check): {0 generic / 1 register-window /
      // 2 LDS / 3 pipe, k, lo halves, fp8 copy, grid x, y, z, frame tiles per pipe chunk}
    const dim3 gk = kind == 3 ? pgrid : kind == 2 ? dim3(C / 128, cdiv(L, DWL_FT), B) : kind == 1 ? wgrid : grid;
    g_zv_last_launch = ZvLaunchRec{kind, ks, il ? 3 : 1, q ? 1 : 0, (int)gk.x, (int)gk.y, (int)gk.z, kind == 3 ? nft : 0};
  }
#undef ZV_DW
#undef ZV_DWW
#undef ZV_DWL
#undef ZV_DWP
  ZV_LAUNCH_CHECK();
}

// ---- BiasNorm + bypass (scaling.py:330-355, zipformer.py:635-637) ----------
// out = orig + (x * mean((x-b)^2)^-1/2 * exp(log_scale) - orig) * c   (fp32 + hi/lo)
// out2 (optional) = out + rowvec[m / rows_per_group]   (next layer's src + temb)
__global__ __launch_bounds__(256) void zv_biasnorm_bypass_kernel(
    const float* x, const float* orig, const float* nb, float log_scale, const float* c,
    float* out, bf16* outh, bf16* outl, float* out2, bf16* out2h, bf16* out2l, long ldact,
    const float* rowvec, int rows_per_group, long M, int C, uint8_t* q2 = nullptr,
    uint8_t* qs2 = nullptr, long ldq = 0) {
  // one wave per row, 4 consecutive channels per lane and chunk (C % 4 == 0); q2 (fp8 mode):
  // out2's MX-fp8 copy, a 32-channel block = 8 adjacent lanes (C % 256 == 0, host checks)
  const long m = blockIdx.x * (long)(blockDim.x / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const float* xr = x + m * C;
  float ss = 0.f;
  for (int k = lane * 4; k < C; k += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(xr + k);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(nb + k);
    const f32x4 d = v - bb;
    ss += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  const float scale = rsqrtf(ss / (float)C) * expf(log_scale);
  const float* orow = orig + m * C;
  const float* rv = rowvec ? rowvec + (m / rows_per_group) * C : nullptr;
  for (int k = lane * 4; k < C; k += 256) {
    const f32x4 o = *reinterpret_cast<const f32x4*>(orow + k);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + k);
    const f32x4 cv = *reinterpret_cast<const f32x4*>(c + k);
    const f32x4 y = o + (xv * scale - o) * cv;
    *reinterpret_cast<f32x4*>(out + m * C + k) = y;
    float yv[4] = {y[0], y[1], y[2], y[3]};
    store_split4(outh, outl, m * ldact + k, yv);
    if (out2h) {   // the next layer's working stream: bf16 copy (+ fp32 where out2 is given)
      f32x4 y2 = y;
      if (rv) y2 = y2 + *reinterpret_cast<const f32x4*>(rv + k);
      if (out2) *reinterpret_cast<f32x4*>(out2 + m * C + k) = y2;
      float y2v[4] = {y2[0], y2[1], y2[2], y2[3]};
      store_split4(out2h, out2l, m * ldact + k, y2v);
      if (q2) {   // from the bf16 copy's values: bitwise equal to packing that copy
        float yb[4] = {(float)(bf16)y2v[0], (float)(bf16)y2v[1], (float)(bf16)y2v[2], (float)(bf16)y2v[3]};
        unsigned sb;
        *reinterpret_cast<unsigned*>(q2 + m * ldq + k) = mx8_quant4(yb, sb);
        if ((lane & 7) == 0) qs2[m * (ldq / MX8_BLOCK) + k / MX8_BLOCK] = (uint8_t)sb;
      }
    }
  }
}

// The same for C = 256 * NCH (the decoder's 512 channels): every load of the row (x, orig,
// the bias and scale vectors) issued before the reduction, so a wave waits one memory latency
// instead of two (the two-pass form above re-reads x after the row sum and sat parked on
// its loads ~70 % of the time); 8 rows per 512-thread block.  Same arithmetic and order.
template <int NCH>
__global__ __launch_bounds__(512) void zv_biasnorm_bypass_v_kernel(
    const float* x, const float* orig, const float* nb, float log_scale, const float* c,
    float* out, bf16* outh, bf16* outl, float* out2, bf16* out2h, bf16* out2l, long ldact,
    const float* rowvec, int rows_per_group, long M, uint8_t* q2, uint8_t* qs2, long ldq) {
  constexpr int C = 256 * NCH;
  const long m = blockIdx.x * (long)(blockDim.x / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const float* xr = x + m * C;
  const float* orow = orig + m * C;
  f32x4 xv[NCH], ov[NCH], bv[NCH], cv[NCH], rvv[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int k = lane * 4 + 256 * j;
    xv[j] = *reinterpret_cast<const f32x4*>(xr + k);
    bv[j] = *reinterpret_cast<const f32x4*>(nb + k);
    ov[j] = *reinterpret_cast<const f32x4*>(orow + k);
    cv[j] = *reinterpret_cast<const f32x4*>(c + k);
  }
  const float* rv = rowvec ? rowvec + (m / rows_per_group) * C : nullptr;
  if (out2h && rv) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) rvv[j] = *reinterpret_cast<const f32x4*>(rv + lane * 4 + 256 * j);
  }
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const f32x4 d = xv[j] - bv[j];
    ss += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  const float scale = rsqrtf(ss / (float)C) * expf(log_scale);
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int k = lane * 4 + 256 * j;
    const f32x4 y = ov[j] + (xv[j] * scale - ov[j]) * cv[j];
    *reinterpret_cast<f32x4*>(out + m * C + k) = y;
    float yv[4] = {y[0], y[1], y[2], y[3]};
    store_split4(outh, outl, m * ldact + k, yv);
    if (out2h) {
      f32x4 y2 = y;
      if (rv) y2 = y2 + rvv[j];
      if (out2) *reinterpret_cast<f32x4*>(out2 + m * C + k) = y2;
      float y2v[4] = {y2[0], y2[1], y2[2], y2[3]};
      store_split4(out2h, out2l, m * ldact + k, y2v);
      if (q2) {
        float yb[4] = {(float)(bf16)y2v[0], (float)(bf16)y2v[1], (float)(bf16)y2v[2], (float)(bf16)y2v[3]};
        unsigned sb;
        *reinterpret_cast<unsigned*>(q2 + m * ldq + k) = mx8_quant4(yb, sb);
        if ((lane & 7) == 0) qs2[m * (ldq / MX8_BLOCK) + k / MX8_BLOCK] = (uint8_t)sb;
      }
    }
  }
}

// Pair-residual form (bf16 mode): the layer's working stream x and its input
// orig are bf16 hi/lo pairs (8 B per element instead of fp32 + a bf16 copy);
// writes the layer output as a pair in place of orig (+ fp32 only for the last
// layer of a stack, whose output the next stack reads) and the next layer's
// x = out + rowvec as a pair in place of x.
__global__ __launch_bounds__(256) void zv_biasnorm_bypass_pair_kernel(
    const bf16* xh, const bf16* xl, const bf16* oh, const bf16* ol, long ld, const float* nb,
    float log_scale, const float* c, float* out32, bf16* outh, bf16* outl, bf16* out2h, bf16* out2l,
    const float* rowvec, int rows_per_group, long M, int C) {
  // one wave per row, 8 consecutive channels per lane and chunk (C % 8 == 0)
  const long m = blockIdx.x * (long)(blockDim.x / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const long r = m * ld;
  float ss = 0.f;
  for (int k = lane * 8; k < C; k += 512) {
    const bf16x8 h = *reinterpret_cast<const bf16x8*>(xh + r + k);
    const bf16x8 l = *reinterpret_cast<const bf16x8*>(xl + r + k);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = ((float)h[e] + (float)l[e]) - nb[k + e];
      ss += d * d;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  const float scale = rsqrtf(ss / (float)C) * expf(log_scale);
  const float* rv = rowvec ? rowvec + (m / rows_per_group) * C : nullptr;
  for (int k = lane * 8; k < C; k += 512) {
    const bf16x8 h = *reinterpret_cast<const bf16x8*>(xh + r + k);
    const bf16x8 l = *reinterpret_cast<const bf16x8*>(xl + r + k);
    const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(oh + r + k);
    const bf16x8 ol8 = *reinterpret_cast<const bf16x8*>(ol + r + k);
    float y[8], y2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float o = (float)o8[e] + (float)ol8[e];
      const float xv = (float)h[e] + (float)l[e];
      y[e] = o + (xv * scale - o) * c[k + e];
      y2[e] = rv ? y[e] + rv[k + e] : y[e];
    }
    store_split8(outh, outl, r + k, y);
    if (out32) {
      *reinterpret_cast<f32x4*>(out32 + m * C + k) = f32x4{y[0], y[1], y[2], y[3]};
      *reinterpret_cast<f32x4*>(out32 + m * C + k + 4) = f32x4{y[4], y[5], y[6], y[7]};
    }
    if (out2h) store_split8(out2h, out2l, r + k, y2);
  }
}

// stack entry: cur = src + rowvec (or src), with hi/lo copies of src and cur
__global__ void zv_stack_entry_kernel(const float* src, const float* rowvec, float* cur,
                                      bf16* srch, bf16* srcl, bf16* curh, bf16* curl, long ldact,
                                      long M, int C, int rows_per_group) {
  // 4 consecutive channels per thread (C % 4 == 0)
  const long total = M * C / 4;
  for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < total;
       i4 += (long)gridDim.x * blockDim.x) {
    const long idx = i4 * 4;
    const long m = idx / C;
    const int c = (int)(idx % C);
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + idx);
    f32x4 y = v;
    if (rowvec) y = y + *reinterpret_cast<const f32x4*>(rowvec + (m / rows_per_group) * C + c);
    if (cur) *reinterpret_cast<f32x4*>(cur + idx) = y;
    float vv[4] = {v[0], v[1], v[2], v[3]}, yv[4] = {y[0], y[1], y[2], y[3]};
    store_split4(srch, srcl, m * ldact + c, vv);
    store_split4(curh, curl, m * ldact + c, yv);
  }
}

// ---- SimpleDownsample (zipformer.py:887-913): weighted sum of ds frames, ----
// right-padded by repeating each item's last frame.  w = softmax(bias) (device, [ds]).
__global__ void zv_downsample_kernel(const float* in, float* out, int B, int L, int dL,
                                     int C, int ds, const float* w) {
  // 4 consecutive channels per thread (C % 4 == 0)
  const long total = (long)B * dL * C / 4;
  for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < total;
       i4 += (long)gridDim.x * blockDim.x) {
    const long idx = i4 * 4;
    const int c = (int)(idx % C);
    const long bi = idx / C;
    const int i = (int)(bi % dL);
    const long b = bi / dL;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < ds; ++k) {
      int l = i * ds + k;
      if (l > L - 1) l = L - 1;
      acc += *reinterpret_cast<const f32x4*>(in + (b * L + l) * C + c) * w[k];
    }
    *reinterpret_cast<f32x4*>(out + idx) = acc;
  }
}
// out = orig + (upsample(d) - orig) * sc (zipformer.py:925-935 SimpleUpsample + BypassModule):
// a block covers whole rows, one f32x4 of a row per thread (32-bit row / channel indices, no
// per-element 64-bit division); each thread walks `rpt` rows spaced a block apart so several
// loads are in flight per thread.  Host guarantees C % 4 == 0 and 256 % (C / 4) == 0.
__global__ __launch_bounds__(256) void zv_upsample_combine_kernel(
    const float* orig, const float* d, const float* sc, float* out, int B, int L, int dL, int C,
    int ds) {
  const int c4n = C >> 2, rpb = 256 / c4n;
  const int c = (threadIdx.x % c4n) * 4;
  const int rows = B * L;
  const f32x4 scv = *reinterpret_cast<const f32x4*>(sc + c);
  constexpr int RPT = 4;
  const int r0 = blockIdx.x * rpb * RPT + threadIdx.x / c4n;
  f32x4 o[RPT], u[RPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int r = r0 + k * rpb;
    if (r < rows) {
      const int b = r / L, l = r - b * L;
      o[k] = *reinterpret_cast<const f32x4*>(orig + (long)r * C + c);
      u[k] = *reinterpret_cast<const f32x4*>(d + ((long)b * dL + l / ds) * C + c);
    }
  }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int r = r0 + k * rpb;
    if (r < rows) *reinterpret_cast<f32x4*>(out + (long)r * C + c) = o[k] + (u[k] - o[k]) * scv;
  }
}

// the same for any channel width (the row-blocked form above needs 256 % (C / 4) == 0: C = 4, 8,
// ..., 1024); one element per thread, grid-stride
__global__ void zv_upsample_combine_any_kernel(const float* orig, const float* d, const float* sc,
                                               float* out, int B, int L, int dL, int C, int ds) {
  const long n = (long)B * L * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    const int b = (int)(r / L), l = (int)(r - (long)b * L);
    const float o = orig[i], u = d[((long)b * dL + l / ds) * C + c];
    out[i] = o + (u - o) * sc[c];
  }
}

// key padding mask subsampling mask[..., ::ds] (zipformer.py:857-858)
__global__ void zv_mask_downsample_kernel(const uint8_t* in, uint8_t* out, int B, int L,
                                          int dL, int ds) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * dL) return;
  const int b = idx / dL, i = idx % dL;
  out[idx] = in[(long)b * L + (long)i * ds];
}

// ---- row padding mode (ZV_PAD_ROW; no reference counterpart: the reference pads the batch tensor) --
// row lengths from the key padding mask: n[b] = 1 + the last l with pad[b, l] == 0, T for a row
// without one.  One wave per row; lane j reads bytes j, j + 64, ... (coalesced) and keeps the largest
// unmasked index it saw, then a butterfly max over the 64 lanes.  A maximum of integers: the result
// does not depend on the order, so not on the launch geometry either.  Lane 0 writes.
__global__ __launch_bounds__(64) void zv_row_len_kernel(const uint8_t* pad, int* n, int T) {
  const uint8_t* row = pad + (long)blockIdx.x * T;
  int last = -1;
  for (int l = threadIdx.x; l < T; l += 64)
    if (row[l] == 0) last = l;   // (l grows: the lane's last hit is its largest)
  for (int off = 32; off > 0; off >>= 1) last = max(last, __shfl_xor(last, off, 64));
  if (threadIdx.x == 0) n[blockIdx.x] = last < 0 ? T : last + 1;
}

// SimpleDownsample of every row as the reference runs it on that row alone at T = n[b]: the frames
// past a row's end are its own last frame, out[b, i] = sum_k w[k] in[b, min(i ds + k, n[b] - 1)] for
// every i < dL.  The form of zv_downsample_kernel (f32x4 per thread, C % 4 == 0, k = 0 .. ds - 1 in
// order); n[b] = L gives that kernel's bits.  Host guarantees 1 <= n[b] <= L (zv_row_len_kernel).
__global__ void zv_downsample_row_kernel(const float* in, float* out, const int* n, int B, int L,
                                         int dL, int C, int ds, const float* w) {
  const long total = (long)B * dL * C / 4;
  for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < total;
       i4 += (long)gridDim.x * blockDim.x) {
    const long idx = i4 * 4;
    const int c = (int)(idx % C);
    const long bi = idx / C;
    const int i = (int)(bi % dL);
    const long b = bi / dL;
    const int last = n[b] - 1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < ds; ++k) {
      int l = i * ds + k;
      if (l > last) l = last;
      acc += *reinterpret_cast<const f32x4*>(in + (b * L + l) * C + c) * w[k];
    }
    *reinterpret_cast<f32x4*>(out + idx) = acc;
  }
}

// ---- the stack-boundary launches (zv_engine and zv_stackedge_check) ---------
// each returns what it launched: kernel form (0 where there is one), grid blocks, block threads
struct EdgeLaunch { int form, blocks, threads; };

static EdgeLaunch launch_downsample(const float* in, float* out, int B, int L, int dL, int C, int ds,
                                    const float* w, hipStream_t s) {
  const dim3 grid = grid1d((long)B * dL * C);
  hipLaunchKernelGGL(zv_downsample_kernel, grid, dim3(256), 0, s, in, out, B, L, dL, C, ds, w);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
// one 64-thread block per row, whatever B and T
static EdgeLaunch launch_row_len(const uint8_t* pad, int* n, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(zv_row_len_kernel, dim3((unsigned)B), dim3(64), 0, s, pad, n, T);
  ZV_LAUNCH_CHECK();
  return {0, B, 64};
}
// n (device, B entries in [1, L]): the table launch_row_len wrote
static EdgeLaunch launch_downsample_row(const float* in, float* out, const int* n, int B, int L, int dL,
                                        int C, int ds, const float* w, hipStream_t s) {
  const dim3 grid = grid1d((long)B * dL * C);
  hipLaunchKernelGGL(zv_downsample_row_kernel, grid, dim3(256), 0, s, in, out, n, B, L, dL, C, ds, w);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
static EdgeLaunch launch_mask_downsample(const uint8_t* in, uint8_t* out, int B, int L, int dL, int ds,
                                         hipStream_t s) {
  const dim3 grid = grid1d((long)B * dL);
  hipLaunchKernelGGL(zv_mask_downsample_kernel, grid, dim3(256), 0, s, in, out, B, L, dL, ds);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
// form 0: row blocks of whole rows (f32x4 per thread); 1: any other width (e.g. 384, 192)
static EdgeLaunch launch_upsample_combine(const float* orig, const float* d, const float* sc, float* out,
                                          int B, int L, int dL, int C, int ds, hipStream_t s) {
  const long M = (long)B * L;
  const bool rowwise = C % 4 == 0 && 256 % (C / 4) == 0;
  const long rows_per_block = rowwise ? 4L * (256 / (C / 4)) : 0;
  const dim3 grid = rowwise ? dim3((unsigned)((M + rows_per_block - 1) / rows_per_block)) : grid1d(M * C);
  if (rowwise)
    hipLaunchKernelGGL(zv_upsample_combine_kernel, grid, dim3(256), 0, s, orig, d, sc, out, B, L, dL, C, ds);
  else
    hipLaunchKernelGGL(zv_upsample_combine_any_kernel, grid, dim3(256), 0, s, orig, d, sc, out, B, L, dL, C, ds);
  ZV_LAUNCH_CHECK();
  return {rowwise ? 0 : 1, (int)grid.x, 256};
}
static EdgeLaunch launch_stack_entry(const float* src, const float* rowvec, float* cur, bf16* srch, bf16* srcl,
                                     bf16* curh, bf16* curl, long ldact, long M, int C, int rows_per_group,
                                     hipStream_t s) {
  const dim3 grid = grid1d(M * C);
  hipLaunchKernelGGL(zv_stack_entry_kernel, grid, dim3(256), 0, s, src, rowvec, cur, srch, srcl, curh, curl,
                     ldact, M, C, rows_per_group);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
// form 1: C = 512, all loads of a row up front; 0: the two-pass kernel
static EdgeLaunch launch_biasnorm_bypass(const float* x, const float* orig, const float* nb, float log_scale,
                                         const float* c, float* out, bf16* outh, bf16* outl, bf16* out2h,
                                         bf16* out2l, long ldact, const float* rowvec, int rows_per_group,
                                         long M, int C, uint8_t* q2, uint8_t* qs2, long ldq, hipStream_t s) {
  const bool v = C == 512;
  const int rows = v ? 8 : 4;                        // one wave per row
  if (v)
    hipLaunchKernelGGL(zv_biasnorm_bypass_v_kernel<2>, dim3(cdiv(M, rows)), dim3(64 * rows), 0, s, x, orig, nb,
                       log_scale, c, out, outh, outl, (float*)nullptr, out2h, out2l, ldact, rowvec,
                       rows_per_group, M, q2, qs2, ldq);
  else
    hipLaunchKernelGGL(zv_biasnorm_bypass_kernel, dim3(cdiv(M, rows)), dim3(64 * rows), 0, s, x, orig, nb,
                       log_scale, c, out, outh, outl, (float*)nullptr, out2h, out2l, ldact, rowvec,
                       rows_per_group, M, C, q2, qs2, ldq);
  ZV_LAUNCH_CHECK();
  return {v ? 1 : 0, cdiv(M, rows), 64 * rows};
}

// duplicate a (B, L) mask for the CFG batch
__global__ void zv_copy_u8_kernel(const uint8_t* in, uint8_t* out, long n, int copies) {
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= n * copies) return;
  out[idx] = in[idx % n];
}

// ---- text side -------------------------------------------------------------
// nn.Embedding lookup (zipvoice.py:205)
__global__ void zv_embed_kernel(const int64_t* tok, const float* table, bf16* oh, bf16* ol,
                                long ld, long n, int C) {
  const long total = n * C;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const long r = idx / C;
    const int c = (int)(idx % C);
    split_store(oh, ol, r * ld + c, table[tok[r] * C + c]);
  }
}

// speaker-turn embedding add (zipvoice_dialog.py:118-125, :153-158); spk[b,s] in {-1,0,1}
__global__ void zv_spk_add_kernel(float* emb, const int8_t* spk, const float* table, long n,
                                  int C) {
  const long total = n * C;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int s = spk[idx / C];
    if (s >= 0) emb[idx] += table[s * C + idx % C];
  }
}

// text condition (zipvoice.py:234-250 + common.py:246-295): frame f of item b
// takes token index min(f / d_b, S_b) (d_b = T_b / S_b; d_b = 0 -> S_b)
__global__ void zv_text_cond_kernel(const float* emb, int S, int C, const int* tok_lens,
                                    const int* feat_lens, float* out, int B, int T) {
  const long total = (long)B * T * C;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const long bt = idx / C;
    const int f = (int)(bt % T);
    const int b = (int)(bt / T);
    const int Sb = tok_lens[b];
    const int d = feat_lens[b] / Sb;
    int k = (d > 0) ? f / d : Sb;
    if (k > Sb) k = Sb;
    out[idx] = emb[((long)b * S + k) * C + c];
  }
}

// speech condition (zipvoice.py:441-451): prompt features padded to T, zeroed
// from prompt_len on.
__global__ void zv_speech_cond_kernel(const float* pf, int Tp, const int* plen, float* out,
                                      int B, int T, int F) {
  const long total = (long)B * T * F;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int f = (int)(idx % F);
    const long bt = idx / F;
    const int t = (int)(bt % T);
    const int b = (int)(bt / T);
    out[idx] = (t < plen[b] && t < Tp) ? pf[((long)b * Tp + t) * F + f] : 0.f;
  }
}

// ---- the solve-boundary launches (zv_engine, zv_text_condition / zv_speech_condition and ---------
// zv_solve_check): what turns (x, text, speech, t, g) into the decoder's operand and velocities back
// into x.  Pinned against float64 one kernel at a time (zv_solve_check, tests/test_gpu_solve_ref.py:
// segment and copy boundaries, row boundaries of the per-row guidance, the grid-stride second trip,
// every column of the positional table, token / prompt boundaries); the host decisions below them
// (cfg_plan, solve_time_steps) in tests/test_solve_plan.py.  Each returns what it launched, as the
// stack-boundary launches above.

// form 1: four features per thread (every segment and the row stride a multiple of 4); 0: one
static EdgeLaunch launch_build_input(const float* x, const float* tc, const float* sc, bf16* oh, bf16* ol, long ld,
                                     int B, int T, int Fx, int Ft, int Fs, int copies, int zero_speech,
                                     hipStream_t s) {
  const long rows = (long)copies * B * T;
  const int Fin = Fx + Ft + Fs;
  const bool quad = Fx % 4 == 0 && Ft % 4 == 0 && Fs % 4 == 0 && ld % 4 == 0;
  const dim3 grid = quad ? grid1d(rows * Fin / 4) : grid1d(rows * Fin);
  if (quad)
    hipLaunchKernelGGL(zv_build_input4_kernel, grid, dim3(256), 0, s, x, tc, sc, oh, ol, ld, B, T, Fx, Ft, Fs,
                       copies, zero_speech);
  else
    hipLaunchKernelGGL(zv_build_input_kernel, grid, dim3(256), 0, s, x, tc, sc, oh, ol, ld, B, T, Fx, Ft, Fs,
                       copies, zero_speech);
  ZV_LAUNCH_CHECK();
  return {quad ? 1 : 0, (int)grid.x, 256};
}
static EdgeLaunch launch_euler_update(float* x, const float* v, long n, int cfg, float g, float dt,
                                      const float* grows, float gmul, long per_row, hipStream_t s) {
  const dim3 grid = grid1d(n);
  hipLaunchKernelGGL(zv_euler_update_kernel, grid, dim3(256), 0, s, x, v, n, cfg, g, dt, grows, gmul, per_row);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
static EdgeLaunch launch_cfg_combine(float* out, const float* v, long n, float g, const float* grows, float gmul,
                                     long per_row, hipStream_t s) {
  const dim3 grid = grid1d(n);
  hipLaunchKernelGGL(zv_cfg_combine_kernel, grid, dim3(256), 0, s, out, v, n, g, grows, gmul, per_row);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
static EdgeLaunch launch_copy_u8(const uint8_t* in, uint8_t* out, long n, int copies, hipStream_t s) {
  const dim3 grid = grid1d(n * copies);
  hipLaunchKernelGGL(zv_copy_u8_kernel, grid, dim3(256), 0, s, in, out, n, copies);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
// the scheduled solve's launches: grid (blocks over one row's elements, rows); a row's blocks are
// capped at SCHED_ROW_BLOCKS (the kernels stride), the rows fill the chip
constexpr int SCHED_ROW_BLOCKS = 1024;
static dim3 sched_grid(long per_row, int rows) {
  ZV_REQUIRE(rows > 0 && rows <= 65535, "scheduled solve: 1 to 65535 decoder rows per step");
  return dim3((unsigned)std::min<long>(std::max<long>(cdiv(per_row, 256), 1), SCHED_ROW_BLOCKS), (unsigned)rows);
}
// map (device, N entries, sched_map_entry): decoder rows [0, N) of T frames.  form as launch_build_input
static EdgeLaunch launch_build_input_map(const float* x, const float* tc, const float* sc, bf16* oh, bf16* ol,
                                         long ld, const int* map, int N, int T, int Fx, int Ft, int Fs,
                                         hipStream_t s) {
  const int Fin = Fx + Ft + Fs;
  ZV_REQUIRE(T > 0 && (long)T * Fin < (1L << 30), "scheduled solve: frames times input width must stay under 2^30");
  const bool quad = Fx % 4 == 0 && Ft % 4 == 0 && Fs % 4 == 0 && ld % 4 == 0;
  const dim3 grid = sched_grid(quad ? (long)T * Fin / 4 : (long)T * Fin, N);
  if (quad)
    hipLaunchKernelGGL(zv_build_input_map4_kernel, grid, dim3(256), 0, s, x, tc, sc, oh, ol, ld, map, T, Fx, Ft, Fs);
  else
    hipLaunchKernelGGL(zv_build_input_map_kernel, grid, dim3(256), 0, s, x, tc, sc, oh, ol, ld, map, T, Fx, Ft, Fs);
  ZV_LAUNCH_CHECK();
  return {quad ? 1 : 0, (int)grid.x, 256};
}
static EdgeLaunch launch_gather_u8(const uint8_t* in, uint8_t* out, const int* map, int N, int T, hipStream_t s) {
  ZV_REQUIRE(T > 0 && T < (1 << 30), "scheduled solve: 1 to 2^30 - 1 frames");
  const dim3 grid = sched_grid(T, N);
  hipLaunchKernelGGL(zv_gather_u8_kernel, grid, dim3(256), 0, s, in, out, map, T);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
// upd (device, A entries): the active rows of one step
static EdgeLaunch launch_euler_update_sched(float* x, const float* v, const SchedUpd* upd, int A, long per_row,
                                            hipStream_t s) {
  ZV_REQUIRE(per_row > 0, "scheduled solve: empty rows");
  const dim3 grid = sched_grid(per_row, A);
  hipLaunchKernelGGL(zv_euler_update_sched_kernel, grid, dim3(256), 0, s, x, v, upd, per_row);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
static EdgeLaunch launch_fill(float* p, float v, int n, hipStream_t s) {
  const dim3 grid(cdiv(n, 256));
  hipLaunchKernelGGL(zv_fill_kernel, grid, dim3(256), 0, s, p, v, n);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
static EdgeLaunch launch_timestep_embed(const float* t, const float* freqs, float* out, int M, int dim,
                                        hipStream_t s) {
  const dim3 grid = grid1d(M * dim);
  hipLaunchKernelGGL(zv_timestep_embed_kernel, grid, dim3(256), 0, s, t, freqs, out, M, dim);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
static EdgeLaunch launch_posp(const float* W, float* out, int L, int nl, int HPD, int D, hipStream_t s) {
  ZV_REQUIRE(D > 0 && D <= POSP_MAXD, "positional dimension above POSP_MAXD");
  const dim3 grid((unsigned)cdiv((long)nl * (2L * L - 1) * HPD, 256L));
  hipLaunchKernelGGL(zv_posp_kernel, grid, dim3(256), 0, s, W, out, L, nl, HPD, D);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
// form 0: one block per (row, 32 outputs) with the row's activation staged in LDS; 1: one wave per
// output, only where the row does not fit LDS.  form < 0: this policy; 0 / 1 force a kernel (tests)
constexpr int SL_ROWS_MAXK = 8192;
static EdgeLaunch launch_small_linear(const float* in, int ldin, const float* W, int ldw, const float* b,
                                      const float* add, float* out, int ldout, int M, int N, int K, int pre,
                                      int form, hipStream_t s) {
  const bool fits = M > 0 && K <= SL_ROWS_MAXK;
  ZV_REQUIRE(form != 0 || fits, "small linear: the row-staged kernel needs M > 0 and K <= 8192");
  const bool rows = form < 0 ? fits : form == 0;
  const dim3 grid = rows ? dim3((unsigned)M, (unsigned)cdiv(N, SL_NB)) : dim3((unsigned)cdiv((long)M * N, 4L));
  if (rows)
    hipLaunchKernelGGL(zv_small_linear_rows_kernel, grid, dim3(256), (size_t)K * sizeof(float), s, in, ldin, W,
                       ldw, b, add, out, ldout, M, N, K, pre);
  else
    hipLaunchKernelGGL(zv_small_linear_kernel, grid, dim3(256), 0, s, in, ldin, W, ldw, b, add, out, ldout, M,
                       N, K, pre);
  ZV_LAUNCH_CHECK();
  return {rows ? 0 : 1, (int)(grid.x * grid.y), 256};
}
static EdgeLaunch launch_embed(const int64_t* tok, const float* table, bf16* oh, bf16* ol, long ld, long n, int C,
                               hipStream_t s) {
  const dim3 grid = grid1d(n * C);
  hipLaunchKernelGGL(zv_embed_kernel, grid, dim3(256), 0, s, tok, table, oh, ol, ld, n, C);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
static EdgeLaunch launch_spk_add(float* emb, const int8_t* spk, const float* table, long n, int C, hipStream_t s) {
  const dim3 grid = grid1d(n * C);
  hipLaunchKernelGGL(zv_spk_add_kernel, grid, dim3(256), 0, s, emb, spk, table, n, C);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
// emb (B, S, C) with the pad slot: 0 < tok_lens[b] < S (device values, not checked here)
static EdgeLaunch launch_text_cond(const float* emb, int S, int C, const int* tok_lens, const int* feat_lens,
                                   float* out, int B, int T, hipStream_t s) {
  ZV_REQUIRE(B > 0 && T > 0 && S > 1 && C > 0, "text condition: B, T, C > 0 and S > 1 (a token and the pad slot)");
  const dim3 grid = grid1d((long)B * T * C);
  hipLaunchKernelGGL(zv_text_cond_kernel, grid, dim3(256), 0, s, emb, S, C, tok_lens, feat_lens, out, B, T);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}
static EdgeLaunch launch_speech_cond(const float* pf, int Tp, const int* plen, float* out, int B, int T, int F,
                                     hipStream_t s) {
  ZV_REQUIRE(B > 0 && T > 0 && Tp > 0 && F > 0, "speech condition: B, T, Tp, F > 0");
  const dim3 grid = grid1d((long)B * T * F);
  hipLaunchKernelGGL(zv_speech_cond_kernel, grid, dim3(256), 0, s, pf, Tp, plen, out, B, T, F);
  ZV_LAUNCH_CHECK();
  return {0, (int)grid.x, 256};
}

// ---- the solve's host decisions (zv_engine::velocity / euler_sample, zv_cfg_plan, zv_time_steps) ----
// DiffusionModel.forward's branches (solver.py:71-98): whether the rows are doubled (conditional +
// unconditional copies), whether the unconditional copy's speech is zeroed (t > 0.5), else the scale
// doubled: g for the scalar form, gmul for per-row scales.  has_rows: per-row scales are given and
// rows_nonzero says whether any is nonzero ((guidance_scale == 0.0).all() selects the unguided
// branch).  Distill: never doubled, the scale feeds the guidance embedding as it is.
struct CfgPlan { int copies, zero_speech; float g, gmul; };
static CfgPlan cfg_plan(float t, float gscale, bool has_rows, bool rows_nonzero, bool distill) {
  const bool on = !distill && (has_rows ? rows_nonzero : gscale != 0.0f);
  CfgPlan p{on ? 2 : 1, 0, gscale, 1.0f};
  if (on) {
    if (t > 0.5f) p.zero_speech = 1;
    else { p.g = gscale * 2.0f; p.gmul = 2.0f; }
  }
  return p;
}
// torch.linspace float32 (forward half / backward half) + shift, solver.py:256-281
static std::vector<float> solve_time_steps(float t_start, float t_end, int num_step, float t_shift) {
  const int steps = num_step + 1;
  std::vector<float> u(steps);
  if (steps == 1) u[0] = t_start;
  else {
    const float step = (t_end - t_start) / (float)(steps - 1);
    const int half = steps / 2;
    for (int i = 0; i < steps; ++i)
      u[i] = (i < half) ? t_start + step * (float)i : t_end - step * (float)(steps - i - 1);
  }
  for (int i = 0; i < steps; ++i) u[i] = t_shift * u[i] / (1.0f + (t_shift - 1.0f) * u[i]);
  return u;
}

// ---- the scheduled solve's host plan (zv_engine::euler_sample_sched, zv_sched_plan) ----
// Row b integrates its own grid solve_time_steps(t_start, t_end, num_step, t_shift) with its own scale,
// as EulerSolver.sample would on that row alone (solver.py:182-240).  Step k of the solve takes the rows
// with k < num_step, in input order (nothing is sorted or permuted); its decoder batch is the
// unconditional copies of the guided ones (g != 0; none in distill), in active order, then the
// conditional rows, in active order.  cfg_plan per row at the row's own t decides whether the copy's
// speech is zeroed (t > 0.5) or the scale doubled.
struct SchedRow { int num_step; float t_start, t_end, t_shift, g; };   // zv_row_sched's layout
struct SchedStep {
  int A = 0, U = 0;
  std::vector<int> src;                      // [U + A] source input row of each decoder row
  std::vector<unsigned char> zt, zs;         // [U + A] text / speech zeroed
  std::vector<float> t;                      // [U + A]
  std::vector<SchedUpd> upd;                 // [A]: input row, dt, effective scale, decoder rows of v_cond / v_uncond
  std::vector<float> gdec;                   // [A]: the row's own scale (distill: the guidance embedding's input)
};
struct SchedPlan {
  int K = 0;
  long total_rows = 0;
  std::vector<std::vector<float>> ts;        // per input row: its grid
  std::vector<SchedStep> steps;
};
// a row's settings, checked (`at` names the row in the message)
static void sched_check_row(const SchedRow& r, const std::string& at) {
  ZV_REQUIRE(r.num_step >= 1, at + "num_step must be at least 1");
  ZV_REQUIRE(r.num_step <= 65536, at + "num_step above 65536");
  ZV_REQUIRE(std::isfinite(r.t_start) && std::isfinite(r.t_end) && std::isfinite(r.t_shift) && std::isfinite(r.g),
             at + "t_start, t_end, t_shift and guidance_scale must be finite");
  ZV_REQUIRE(r.t_shift > 0.0f, at + "t_shift must be positive");
}
// One step's tables from its active rows, in order: each with its input row, its own t and next t and
// its scale.  The scheduled solve gives every row the step's shared index k, a solve session
// (zv_session.inc) the row's own.
struct SchedAct { int row; float t, t_next, g; };
static SchedStep sched_step(const std::vector<SchedAct>& act, bool distill) {
  SchedStep st;
  std::vector<CfgPlan> plan;
  for (const SchedAct& a : act) {
    plan.push_back(cfg_plan(a.t, a.g, false, false, distill));
    if (plan.back().copies == 2) ++st.U;
  }
  st.A = (int)act.size();
  const int N = st.U + st.A;
  st.src.resize(N); st.zt.resize(N); st.zs.resize(N); st.t.resize(N);
  st.upd.resize(st.A); st.gdec.resize(st.A);
  int u = 0;
  for (int i = 0; i < st.A; ++i) {
    const int b = act[i].row, jc = st.U + i;
    const float t = act[i].t;
    st.src[jc] = b; st.zt[jc] = 0; st.zs[jc] = 0; st.t[jc] = t;
    int ju = -1;
    if (plan[i].copies == 2) {
      ju = u++;
      st.src[ju] = b; st.zt[ju] = 1; st.zs[ju] = (unsigned char)plan[i].zero_speech; st.t[ju] = t;
    }
    st.upd[i] = SchedUpd{b, act[i].t_next - t, plan[i].g, jc, ju};
    st.gdec[i] = act[i].g;
  }
  return st;
}
static SchedPlan sched_plan(const SchedRow* rows, int B, bool distill) {
  ZV_REQUIRE(rows != nullptr, "scheduled solve: null schedule");
  ZV_REQUIRE(B >= 1 && B <= 32767, "scheduled solve: B must be in [1, 32767]");
  SchedPlan p;
  p.ts.resize(B);
  for (int b = 0; b < B; ++b) {
    const SchedRow& r = rows[b];
    sched_check_row(r, "scheduled solve: row " + std::to_string(b) + ": ");
    p.ts[b] = solve_time_steps(r.t_start, r.t_end, r.num_step, r.t_shift);
    p.K = std::max(p.K, r.num_step);
  }
  p.steps.resize(p.K);
  for (int k = 0; k < p.K; ++k) {
    std::vector<SchedAct> act;
    for (int b = 0; b < B; ++b)
      if (k < rows[b].num_step) act.push_back(SchedAct{b, p.ts[b][k], p.ts[b][k + 1], rows[b].g});
    p.steps[k] = sched_step(act, distill);
    p.total_rows += p.steps[k].U + p.steps[k].A;
  }
  return p;
}
