// 256 x 256 phased MFMA GEMM for gfx950: the model's large linears.
//
//   C = epilogue( A (M x K, row-major 16-bit) . B^T + bias ),  B stored [N][K]
//
// Why a second mainloop: the 128 x 128 kernel (zv_gemm.inc, 4 waves of 64 x 64) reads
// 0.5 KiB of LDS fragments per MFMA and stages 32 KiB per 128 x 128 x 64 K step; with
// two blocks per CU its fragment reads plus DMA writes take about as many LDS cycles as
// its MFMAs (DESIGN.md §3).  Here 8 waves (2 per SIMD) own 128 x 64 outputs each:
// 0.375 KiB of fragments per MFMA and half the staged bytes per FLOP, so the LDS array
// sits at ~60 % of the MFMA time instead of ~100 %.  One 512-thread block per CU (the
// 128 KiB ring), persistent over an XCD-aware tile order, K pipeline continuous across
// tiles (the next tile's first K steps load under this tile's last MFMAs and epilogue).
//
// Ring: 2 buffers x 4 half-tiles {A rows 0-127, A rows 128-255, B rows 0-127, B rows
// 128-255}, each 128 rows x 128 B (a 64-deep K step), lane-linear glds images with the
// 16-B chunk XOR swizzle chunk ^ (row & 7) applied on the source address (conflict-free
// ds_read_b128).  K step s (buffer s & 1) runs four phases, one C quadrant each (the
// wave's 128 x 64 split into 64-row x 32-column quarters, 16 MFMAs per phase):
//   p0 (0,0): read a0 (rows 0-63), b0 (cols 0-31) | issue B half 0 of step s+1
//   p1 (1,0): read a1 (rows 64-127)               | issue B half 1 of step s+1
//   p2 (1,1): read b1 (cols 32-63)                | issue A half 0 of step s+2
//   p3 (0,1): -                                   | issue A half 1 of step s+2, vmcnt(4)
// A halves are last read in p1, B halves in p2, so every DMA targets a half-slot whose
// readers retired before an earlier phase's closing barrier (WAR); the vmcnt(4) before
// p3's closing barrier leaves only step s+2's A halves in flight, so step s+1 (read
// after that barrier) has landed (RAW).  2 DMA pieces (16 B per lane) per wave per
// half-tile, per-lane offsets fixed for a tile (scalar base per K step, glds16s).
// PB = 1 adds the guide's barrier between the fragment reads and the MFMA cluster of a
// phase (cdna_hip_programming.md §5, the 256^2 phased template); s_setprio(1) brackets
// each cluster (T5: keeps hipcc from moving MFMAs across the barriers).
//
// Epilogue: the counted forms of zv_gemm.inc (same arithmetic, bitwise equal to the
// 128 x 128 kernel: each accumulator sees the same MFMA sequence in K order), staged in
// the just-finished buffer's B half-slots (free until the next tile's p0 refills them;
// unpadded swizzled 16 x 64 strips, 4 KiB per wave).
#pragma once
#include "zv_gemm.inc"

constexpr int G256_HALF = 16384, G256_BUF = 4 * G256_HALF, G256_LDS = 2 * G256_BUF;

// ---------------------------------------------------------------------------
// Direct epilogues (DIRECT = 1).  The MFMA runs with swapped operands (weights as the A
// side, activations as the B side), so a 16 x 16 accumulator gives each lane 4 consecutive
// output COLUMNS of one row: lane (row fr = l & 15, g = l >> 4) holds n = 4g + r.  One
// v_permlane16_swap per register of an n-subtile pair (X = cols 0-15, Y = cols 16-31 of a
// 32-column group) leaves every lane 8 consecutive columns of its row — cols cofs(g)..+7,
// cofs = {0, 16, 8, 24} — as in the staged epilogue's 8-column chunks, with no LDS round
// trip (the staged form writes and re-reads 64 KiB of accumulators per tile).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int g256_cofs(int lane) {
  const int g = lane >> 4;
  return ((g & 1) << 4) | ((g >> 1) << 3);
}
__device__ __forceinline__ void g256_pair8(const f32x4& X, const f32x4& Y, float (&v)[8]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(X[r]), __float_as_uint(Y[r]), false, false);
    v[r] = __uint_as_float(sw[0]);
    v[4 + r] = __uint_as_float(sw[1]);
  }
}
// bias (+ activation) -> bf16 copy (ROLE 3)
template <int TM, int TN>
__device__ __forceinline__ void g256_epi_plain(const GemmParams& p, f32x4 (&acc)[TM][TN], int m0, int n0,
                                               int lane) {
  const int fr = lane & 15, cofs = g256_cofs(lane);
#pragma unroll
  for (int J = 0; J < TN / 2; ++J) {
    const int n = n0 + J * 32 + cofs, nc = min(n, p.N - 8);
    const bool col_ok = n < p.N;
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + nc);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.bias + nc + 4);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float v[8];
      g256_pair8(acc[i][2 * J], acc[i][2 * J + 1], v);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] += b0[e]; v[4 + e] += b1[e]; }
      if (p.act == 1) {        // the only activation of the model's linears (host-checked)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = swoosh_l(v[e]);
      }
      const int m = m0 + i * 16 + fr;
      bf16x8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = (bf16)v[e];
      unsigned long long ha = (col_ok && m < p.M) ? (unsigned long long)(p.Ch + (long)m * p.ldch + n)
                                                  : (unsigned long long)(p.sink + 512 + lane * 4);
      asm volatile("" : "+v"(ha));
      *(GLOBAL bf16x8*)(ha) = h;
    }
  }
}

// residual linears (ROLE 1 / 2 = + bypass original / 4 = + row vector / 5 = 4 without the
// fp32 output): the general epilogue's order, resid + (acc + bias) [+ rowvec], then
// orig + (v - orig) * byp; the residual operands of PD groups ahead held in registers
template <int TM, int TN, bool ORIG, bool RV, bool NOC, int PD>
__device__ __forceinline__ void g256_epi_res(const GemmParams& p, f32x4 (&acc)[TM][TN], int m0, int n0,
                                             int lane) {
  constexpr int NJ = TN / 2, NG = TM * NJ;
  const int fr = lane & 15, cofs = g256_cofs(lane);
  f32x4 bb[NJ][2], sb[ORIG ? NJ : 1][2];
  int nc[NJ];
  bool col_ok[NJ];
#pragma unroll
  for (int J = 0; J < NJ; ++J) {
    const int n = n0 + J * 32 + cofs;
    nc[J] = min(n, p.N - 8);
    col_ok[J] = n < p.N;
    bb[J][0] = *reinterpret_cast<const f32x4*>(p.bias + nc[J]);
    bb[J][1] = *reinterpret_cast<const f32x4*>(p.bias + nc[J] + 4);
    if constexpr (ORIG) {
      sb[J][0] = *reinterpret_cast<const f32x4*>(p.byp + nc[J]);
      sb[J][1] = *reinterpret_cast<const f32x4*>(p.byp + nc[J] + 4);
    }
  }
  f32x4 rr[NG][2], ro[ORIG ? NG : 1][2], rv[RV ? NG : 1][2];
  auto prefetch = [&](int q) {
    if (q < NG) {
      const int i = q / NJ, J = q % NJ;
      const int m = min(m0 + i * 16 + fr, p.M - 1);
      const long ci = (long)m * p.ldc + nc[J];
      rr[q][0] = *reinterpret_cast<const f32x4*>(p.resid + ci);
      rr[q][1] = *reinterpret_cast<const f32x4*>(p.resid + ci + 4);
      if constexpr (RV) {
        const float* vp = p.rowvec + (long)(m / p.rows_per_group) * p.rowvec_ld + nc[J];
        rv[q][0] = *reinterpret_cast<const f32x4*>(vp);
        rv[q][1] = *reinterpret_cast<const f32x4*>(vp + 4);
      }
      if constexpr (ORIG) {
        ro[q][0] = *reinterpret_cast<const f32x4*>(p.orig + ci);
        ro[q][1] = *reinterpret_cast<const f32x4*>(p.orig + ci + 4);
      }
    }
  };
#pragma unroll
  for (int q = 0; q < PD - 1; ++q) prefetch(q);
  static_for<NG>([&](auto Q_) {
    constexpr int q = decltype(Q_)::value, i = q / NJ, J = q % NJ;
    prefetch(q + PD - 1);
    float v[8];
    g256_pair8(acc[i][2 * J], acc[i][2 * J + 1], v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = rr[q][0][e] + (v[e] + bb[J][0][e]);
      v[4 + e] = rr[q][1][e] + (v[4 + e] + bb[J][1][e]);
    }
    if constexpr (RV) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] += rv[q][0][e]; v[4 + e] += rv[q][1][e]; }
    }
    if constexpr (ORIG) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = ro[q][0][e] + (v[e] - ro[q][0][e]) * sb[J][0][e];
        v[4 + e] = ro[q][1][e] + (v[4 + e] - ro[q][1][e]) * sb[J][1][e];
      }
    }
    const int m = m0 + i * 16 + fr, n = n0 + J * 32 + cofs;
    const bool ok = col_ok[J] && m < p.M;
    if constexpr (!NOC) {
      unsigned long long ca = ok ? (unsigned long long)(p.C + (long)m * p.ldc + n)
                                 : (unsigned long long)(p.sink + lane * 8);
      asm volatile("" : "+v"(ca));
      *(GLOBAL f32x4*)(ca) = f32x4{v[0], v[1], v[2], v[3]};
      *(GLOBAL f32x4*)(ca + 16) = f32x4{v[4], v[5], v[6], v[7]};
    }
    bf16x8 h;
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (bf16)v[e];
    unsigned long long ha = ok ? (unsigned long long)(p.Ch + (long)m * p.ldch + n)
                               : (unsigned long long)(p.sink + 512 + lane * 4);
    asm volatile("" : "+v"(ha));
    *(GLOBAL bf16x8*)(ha) = h;
  });
}

// GLU (ROLE 3, weight rows permuted in 32-row groups [x16 | s16]): the pair (X, Y) of a
// group holds x and s of the SAME 4 channels per lane, g = x * sigmoid(s) (0 on masked rows);
// the packed bf16 of two groups are swapped like g256_pair8 into 8 consecutive channels
template <int TM, int TN>
__device__ __forceinline__ void g256_epi_glu(const GemmParams& p, f32x4 (&acc)[TM][TN], int m0, int n0,
                                             int lane) {
  static_assert(TN == 4, "two channel groups per wave");
  const int fr = lane & 15, g = lane >> 4, cofs = g256_cofs(lane);
  // group J's bias: x at nb + 4g, s at nb + 16 + 4g (nb = n0 + 32 J)
  f32x4 bx[2], bs[2];
#pragma unroll
  for (int J = 0; J < 2; ++J) {
    const int nb = min(n0 + J * 32, p.N - 32);
    bx[J] = *reinterpret_cast<const f32x4*>(p.bias + nb + 4 * g);
    bs[J] = *reinterpret_cast<const f32x4*>(p.bias + nb + 16 + 4 * g);
  }
  // output channels: (n0 / 32) * 16 + cofs .. +7 (valid when n0 + 32 <= N, i.e. both groups
  // of the pair exist, or the lane's channels lie in the first group)
  const int cb = (n0 / 32) * 16 + cofs;
  const bool col_ok = (n0 + (cofs >= 16 ? 64 : 32)) <= p.N;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + i * 16 + fr;
    const bool zero = p.rowmask[min(m, p.M - 1) * p.rowmask_step] != 0;
    unsigned w[2][2];
#pragma unroll
    for (int J = 0; J < 2; ++J) {
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xv = acc[i][2 * J][r] + bx[J][r];
        const float sv = acc[i][2 * J + 1][r] + bs[J][r];
        o[r] = zero ? 0.f : xv * sigmoidf_(sv);
      }
      bf16x2 a = {(bf16)o[0], (bf16)o[1]}, b = {(bf16)o[2], (bf16)o[3]};
      w[J][0] = *reinterpret_cast<unsigned*>(&a);
      w[J][1] = *reinterpret_cast<unsigned*>(&b);
    }
    unsigned u[4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const auto sw = __builtin_amdgcn_permlane16_swap(w[0][r], w[1][r], false, false);
      u[r] = sw[0];
      u[2 + r] = sw[1];
    }
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    unsigned long long ha = (col_ok && m < p.M) ? (unsigned long long)(p.Ch + (long)m * p.ldch + cb)
                                                : (unsigned long long)(p.sink + 512 + lane * 4);
    asm volatile("" : "+v"(ha));
    *(GLOBAL u32x4_t*)(ha) = u32x4_t{u[0], u[1], u[2], u[3]};
  }
}

// ---------------------------------------------------------------------------
// GLU + depthwise conv + SwooshR in one launch (DWK = the conv's kernel size k; the
// ConvolutionModule's in_proj -> GLU -> masked_fill -> depthwise_conv -> SwooshR,
// zipformer.py:1638-1672, scaling.py:1185-1191).  An M tile is 256 consecutive rows of the
// flattened batch starting k/2 rows before its 256 - 2 (k/2) output rows (tiles overlap by the
// conv halo; 13 % extra GEMM rows at k = 31, 6 % at 15, 2 % at 7).  The epilogue writes the
// tile's GLU values (bf16, exactly the unfused GLU linear's) to LDS -- the drained K ring, one
// tile per block -- and the block runs the conv on them: lane = channel pair, wave = 8-frame
// output chunks, taps in registers, the same tap-major packed-FMA order as
// zv_dwconv_pipe_kernel, so the output is bitwise the unfused pair's.  Input rows of another
// utterance (or outside the batch) read as zero: the conv's zero padding.  Neither the GLU
// output nor a conv launch exists any more.
// ---------------------------------------------------------------------------
// the GLU tile in LDS as fp32 (the bf16-rounded values widened once: the conv's window loads need
// no conversion), rows of 128 channels + 16 B (conflict-free 16-row column writes)
constexpr int G256_DW_LD = 132;
constexpr int G256_DW_LDS = 256 * G256_DW_LD * 4;

// a[i] = fma(x[i], w, a[i]) for 8 independent channel-pair accumulators, as one asm block: the 8
// packed FMAs stay together in this order (left to itself hipcc emitted each output's whole tap chain
// back to back, one s_nop between every two dependent packed FMAs).  Inside a block nothing depends
// on anything; the next tap's block reads a[0] 7 instructions after it was written.  PRE / POST pad
// the first / last block (the operands' VALU producers and consumers outside the string).
typedef float g256_f32x2 __attribute__((ext_vector_type(2)));
#define G256_PKFMA8                          \
  "v_pk_fma_f32 %0, %8, %16, %0\n\t"       \
  "v_pk_fma_f32 %1, %9, %16, %1\n\t"       \
  "v_pk_fma_f32 %2, %10, %16, %2\n\t"      \
  "v_pk_fma_f32 %3, %11, %16, %3\n\t"      \
  "v_pk_fma_f32 %4, %12, %16, %4\n\t"      \
  "v_pk_fma_f32 %5, %13, %16, %5\n\t"      \
  "v_pk_fma_f32 %6, %14, %16, %6\n\t"      \
  "v_pk_fma_f32 %7, %15, %16, %7"
#define G256_PKFMA8_OPS                                                                                   \
  : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])      \
  : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(w)
template <bool PRE, bool POST>
__device__ __forceinline__ void g256_pk_fma8(g256_f32x2* a, const g256_f32x2* x, g256_f32x2 w) {
  if constexpr (PRE && POST) asm volatile("s_nop 1\n\t" G256_PKFMA8 "\n\ts_nop 1" G256_PKFMA8_OPS);
  else if constexpr (PRE) asm volatile("s_nop 1\n\t" G256_PKFMA8 G256_PKFMA8_OPS);
  else if constexpr (POST) asm volatile(G256_PKFMA8 "\n\ts_nop 1" G256_PKFMA8_OPS);
  else asm volatile(G256_PKFMA8 G256_PKFMA8_OPS);
}
#undef G256_PKFMA8
#undef G256_PKFMA8_OPS

template <int TM, int TN, int DWK>
__device__ __forceinline__ void g256_epi_glu_dw(const GemmParams& p, f32x4 (&acc)[TM][TN], int tm0, int tn,
                                                int wr, int wc, int lane, int tid, unsigned char* smem) {
  static_assert(TN == 4 && TM == 8, "the 256 x 256 tile");
  // (16-frame chunks where the window fits the registers; at k = 31 they spilled)
  constexpr int HALO = DWK / 2, NO = 256 - 2 * HALO, R = DWK >= 31 ? 8 : 16, NW = R + DWK - 1;
  const int fr = lane & 15, g = lane >> 4, cofs = g256_cofs(lane);
  float* T = reinterpret_cast<float*>(smem);
  // ---- GLU values of this wave's 128 rows x 32 channels -> LDS [row][channel]
  const int n0 = tn * 256 + wc * 64;
  f32x4 bx[2], bs[2];
#pragma unroll
  for (int J = 0; J < 2; ++J) {
    const int nb = min(n0 + J * 32, p.N - 32);
    bx[J] = *reinterpret_cast<const f32x4*>(p.bias + nb + 4 * g);
    bs[J] = *reinterpret_cast<const f32x4*>(p.bias + nb + 16 + 4 * g);
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = wr * 128 + i * 16 + fr;
    const int gm = min(max(tm0 + row, 0), p.M - 1);
    const bool zero = p.rowmask[gm * p.rowmask_step] != 0;
    unsigned w[2][2];
#pragma unroll
    for (int J = 0; J < 2; ++J) {
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xv = acc[i][2 * J][r] + bx[J][r];
        const float sv = acc[i][2 * J + 1][r] + bs[J][r];
        o[r] = zero ? 0.f : xv * sigmoidf_(sv);
      }
      bf16x2 a = {(bf16)o[0], (bf16)o[1]}, b = {(bf16)o[2], (bf16)o[3]};
      w[J][0] = *reinterpret_cast<unsigned*>(&a);
      w[J][1] = *reinterpret_cast<unsigned*>(&b);
    }
    unsigned u[4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const auto sw = __builtin_amdgcn_permlane16_swap(w[0][r], w[1][r], false, false);
      u[r] = sw[0];
      u[2 + r] = sw[1];
    }
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bf16x2 h = __builtin_bit_cast(bf16x2, u[e]);
      f[2 * e] = (float)h[0];
      f[2 * e + 1] = (float)h[1];
    }
    float* dst = T + row * G256_DW_LD + wc * 32 + cofs;
    *reinterpret_cast<f32x4*>(dst) = f32x4{f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{f[4], f[5], f[6], f[7]};
  }
  __syncthreads();
  // ---- the conv: lane = channel pair (2 lane, 2 lane + 1 of the tile's 128), wave = output chunks.
  // Every chunk bound below is wave-uniform (the wave index read through readfirstlane): the window
  // loads are unconditional and only a window crossing an utterance edge takes the masking branch
  // (a lane-dependent bound had turned each load into an exec-masked branch with its own wait)
  typedef g256_f32x2 f32x2_t;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = tn * 128 + 2 * lane;                 // global channel
  f32x2_t w2[DWK];
#pragma unroll
  for (int t = 0; t < DWK; ++t) w2[t] = f32x2_t{p.dw_w[(long)c * DWK + t], p.dw_w[(long)(c + 1) * DWK + t]};
  const f32x2_t b2 = {p.dw_b[c], p.dw_b[c + 1]};
  const int L = p.dw_L;
  for (int o0 = wave * R; o0 < NO; o0 += 8 * R) {
    const int om0 = tm0 + HALO + o0;                  // global row of output 0 of the chunk
    if (om0 >= p.M) break;
    const int nval = min(min(R, NO - o0), p.M - om0); // outputs of this chunk
    const int w0 = tm0 + o0;                          // global row of window row 0
    // the utterances this chunk's outputs belong to (two where it crosses a boundary)
    for (int b = om0 / L; b <= (om0 + nval - 1) / L; ++b) {
      const int jlo = max(b * L - w0, 0), jhi = min((b + 1) * L - w0, NW);      // window rows of utterance b
      const int rlo = max(b * L - om0, 0), rhi = min((b + 1) * L - om0, nval);  // its outputs
      f32x2_t x2[NW], a2[R];
#pragma unroll
      for (int j = 0; j < NW; ++j) x2[j] = *reinterpret_cast<const f32x2_t*>(T + (o0 + j) * G256_DW_LD + 2 * lane);
      if (jlo > 0 || jhi < NW) {
#pragma unroll
        for (int j = 0; j < NW; ++j)
          if (j < jlo || j >= jhi) x2[j] = f32x2_t{0.f, 0.f};
      }
#pragma unroll
      for (int r = 0; r < R; ++r) a2[r] = f32x2_t{0.f, 0.f};
      // tap-major, 8 outputs per asm block (the unfused kernel's FMA order per output)
      static_for<DWK>([&](auto T_) {
        constexpr int t = decltype(T_)::value;
        static_for<R / 8>([&](auto G_) {
          constexpr int gq = decltype(G_)::value;
          g256_pk_fma8<t == 0, t == DWK - 1>(a2 + 8 * gq, x2 + 8 * gq + t, w2[t]);
        });
      });
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const f32x2_t z = a2[r] + b2;
        const float y0 = swoosh_r(z[0]), y1 = swoosh_r(z[1]);
        if (r >= rlo && r < rhi)
          *reinterpret_cast<bf16x2*>(p.dw_out + (long)(om0 + r) * p.ld_dw + c) = bf16x2{(bf16)y0, (bf16)y1};
      }
    }
  }
}

template <int EPI, int ROLE, int PB = 0, int MXO = 0, int DIRECT = 1, int DRAIN = 1, int DWK = 0>
__global__ __launch_bounds__(512, DWK ? 1 : 2) void zv_gemm256_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, TM = 8, TN = 4, BK = GEMM_BK;
  // DWK > 0: GLU + depthwise conv (g256_epi_glu_dw); M tiles of 256 rows advance by 256 - 2 (k/2)
  constexpr int MSTEP = BM - 2 * (DWK / 2), MOFS = DWK / 2;
  // ROLE 9: no output (mainloop ablation for the microbenchmark: the accumulators kept live)
  static_assert(ROLE >= 1 && (EPI == EPI_STD || (EPI == EPI_GLU && ROLE == 3)), "counted epilogues only");
  static_assert(DWK == 0 || (EPI == EPI_GLU && DIRECT), "the fused conv follows the direct GLU epilogue");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;           // 2 (M) x 4 (N) waves
  const int ntn = (p.N + BN - 1) / BN, ntm = (p.M + MSTEP - 1) / MSTEP;
  const int ntiles = ntn * ntm;
  const int G = gridDim.x, Q = G >> 3;               // G % 8 == 0 (host)
  const int bslot = (blockIdx.x & 7) * Q + (blockIdx.x >> 3);
  const int my_tiles = (bslot < ntiles) ? (ntiles - 1 - bslot) / G + 1 : 0;
  const int nk = (p.K + BK - 1) / BK;
  const int total = my_tiles * nk;
  if (total == 0) return;                            // block-uniform

  // ---- producers: one cursor per operand (the A loads run one step further ahead)
  const int prow = lane >> 3, ppos = lane & 7;
  const unsigned cswz = (unsigned)((ppos ^ prow) * 16);   // row & 7 == prow in every piece
  unsigned offa[2][2], offb[2][2];                   // [half][piece] per-lane byte offsets
  int a_it = 0, a_kt = 0, a_s = 0, b_it = 0, b_kt = 0, b_s = 0;
  auto set_a = [&](int it) {
    const int m0 = ((it * G + bslot) / ntn) * MSTEP - MOFS;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int gm = min(max(m0 + h * 128 + (wave + 8 * i) * 8 + prow, 0), p.M - 1);
        offa[h][i] = (unsigned)((long)gm * p.lda * 2) + cswz;
      }
  };
  auto set_b = [&](int it) {
    const int n0 = ((it * G + bslot) % ntn) * BN;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int gn = min(n0 + h * 128 + (wave + 8 * i) * 8 + prow, p.Brows - 1);
        offb[h][i] = (unsigned)((long)gn * p.ldb * 2) + cswz;
      }
  };
  // half h of the current A / B producer step; the cursor advances after half 1
  auto issue_a = [&](int h) {
    const unsigned char* base = reinterpret_cast<const unsigned char*>(p.Ah) + (long)a_kt * BK * 2;
    unsigned char* dst = smem + (a_s & 1) * G256_BUF + h * G256_HALF;
    glds16s(base, offa[h][0], dst + wave * 1024);
    glds16s(base, offa[h][1], dst + (wave + 8) * 1024);
    if (h == 1) {
      ++a_s;
      if (++a_kt == nk) { a_kt = 0; if (++a_it < my_tiles) set_a(a_it); }
    }
  };
  auto issue_b = [&](int h) {
    const unsigned char* base = reinterpret_cast<const unsigned char*>(p.Bh) + (long)b_kt * BK * 2;
    unsigned char* dst = smem + (b_s & 1) * G256_BUF + (2 + h) * G256_HALF;
    glds16s(base, offb[h][0], dst + wave * 1024);
    glds16s(base, offb[h][1], dst + (wave + 8) * 1024);
    if (h == 1) {
      ++b_s;
      if (++b_kt == nk) { b_kt = 0; if (++b_it < my_tiles) set_b(b_it); }
    }
  };

  // prologue: A(0), B(0), A(1); step 0 landed before the first reads
  set_a(0);
  set_b(0);
  issue_a(0); issue_a(1);
  issue_b(0); issue_b(1);
  if (total > 1) {
    issue_a(0); issue_a(1);
    wait_vmcnt<4>();
  } else {
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();

  // ---- consumers
  const int fr = lane & 15, fq = lane >> 4;
  auto read_a = [&](const unsigned char* buf, int mi, bf16x8 (&a)[2][4]) {
    const unsigned char* h = buf + wr * G256_HALF;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = mi * 64 + i * 16 + fr;
        a[kk][i] = *reinterpret_cast<const bf16x8*>(h + r * 128 + (((kk * 4 + fq) ^ (r & 7)) << 4));
      }
  };
  auto read_b = [&](const unsigned char* buf, int ni, bf16x8 (&b)[2][2]) {
    const unsigned char* h = buf + (2 + (wc >> 1)) * G256_HALF;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = (wc & 1) * 64 + ni * 32 + j * 16 + fr;
        b[kk][j] = *reinterpret_cast<const bf16x8*>(h + r * 128 + (((kk * 4 + fq) ^ (r & 7)) << 4));
      }
  };
  f32x4 acc[TM][TN];
  auto quad = [&](auto MI, auto NI, const bf16x8 (&a)[2][4], const bf16x8 (&b)[2][2]) {
    constexpr int mi = decltype(MI)::value, ni = decltype(NI)::value;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[mi * 4 + i][ni * 2 + j] =
              DIRECT ? ZV_MFMA_16x16x32(b[kk][j], a[kk][i], acc[mi * 4 + i][ni * 2 + j], 0, 0, 0)
                     : ZV_MFMA_16x16x32(a[kk][i], b[kk][j], acc[mi * 4 + i][ni * 2 + j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  auto pre_mma = [&]() {   // reads issued above; the cluster waits for them
    if constexpr (PB) __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto post_mma = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
  };

  int s = 0;
  for (int it = 0; it < my_tiles; ++it) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt, ++s) {
      const unsigned char* buf = smem + (s & 1) * G256_BUF;
      bf16x8 a0[2][4], a1[2][4], b0[2][2], b1[2][2];
      // p0
      read_a(buf, 0, a0);
      read_b(buf, 0, b0);
      if (s + 1 < total) issue_b(0);
      pre_mma();
      quad(I0{}, I0{}, a0, b0);
      post_mma();
      // p1
      read_a(buf, 1, a1);
      if (s + 1 < total) issue_b(1);
      pre_mma();
      quad(I1{}, I0{}, a1, b0);
      post_mma();
      // p2
      read_b(buf, 1, b1);
      if (s + 2 < total) issue_a(0);
      pre_mma();
      quad(I1{}, I1{}, a1, b1);
      post_mma();
      // p3
      if (s + 2 < total) issue_a(1);
      if constexpr (PB) __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      quad(I0{}, I1{}, a0, b1);
      __builtin_amdgcn_sched_barrier(0);
      if (s + 2 < total) wait_vmcnt<4>();       // step s+1 landed; step s+2's A halves in flight
      else wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
    }
    const int tile = it * G + bslot;
    const int m0 = (tile / ntn) * BM + wr * 128, n0 = (tile % ntn) * BN + wc * 64;
    float* scr = reinterpret_cast<float*>(smem + ((s - 1) & 1) * G256_BUF + 2 * G256_HALF + wave * 4096);
    if constexpr (DWK > 0) {
      // one tile per block (host): the ring has drained (the last step waited vmcnt(0) and
      // every wave passed its closing barrier), so all of it holds the GLU tile
      (void)m0; (void)n0; (void)scr;
      g256_epi_glu_dw<TM, TN, DWK>(p, acc, (tile / ntn) * MSTEP - MOFS, tile % ntn, wr, wc, lane, tid, smem);
    } else if constexpr (ROLE == 9) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(acc[i][j]));
      (void)m0; (void)n0; (void)scr;
    } else if constexpr (DIRECT) {
      static_assert(MXO == 0, "direct epilogues: no fp8 copy");
      (void)scr;
      if constexpr (EPI == EPI_GLU) g256_epi_glu<TM, TN>(p, acc, m0, n0, lane);
      else if constexpr (ROLE == 3) g256_epi_plain<TM, TN>(p, acc, m0, n0, lane);
      else g256_epi_res<TM, TN, ROLE == 2, ROLE == 4 || ROLE == 5, ROLE == 5,
                        ROLE == 2 ? 3 : (ROLE == 4 || ROLE == 5) ? 4 : 8>(p, acc, m0, n0, lane);
    } else if constexpr (EPI == EPI_GLU) {
      gemm_epilogue_glu_c<TM, TN, 1, true>(p, acc, m0, n0, lane, scr);
    } else {
      // residual operands held ahead: 64 VGPRs (acc strips free up as they retire)
      constexpr int PER = 16 * (1 + (ROLE == 2) + (ROLE == 4 || ROLE == 5));
      constexpr int PDM = 64 / PER < 1 ? 1 : 64 / PER;
      gemm_epilogue_res<TM, TN, 1, ROLE == 2, ROLE != 3, MXO, ROLE == 4 || ROLE == 5, ROLE == 5, true, PDM>(
          p, acc, m0, n0, lane, scr);
    }
    // the scratch (this buffer's B halves) is refilled by the next step's p0
    if constexpr (DRAIN) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), visible to hipcc's waitcnt pass
    __builtin_amdgcn_s_barrier();
  }
}

// bench / A-B and engine launcher (16-bit operands, the counted epilogues)
template <int EPI, int ROLE, int PB = 0, int MXO = 0, int DIRECT = 1, int DRAIN = 1, int DWK = 0>
static void launch_gemm256(const GemmParams& p, hipStream_t s, const char* tag, bool persistent = true) {
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_gemm256_kernel<EPI, ROLE, PB, MXO, DIRECT, DRAIN, DWK>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, DWK ? G256_DW_LDS : G256_LDS));
    attr |= 1ull << zv_cur_device();
  }
  static_assert(G256_DW_LDS <= 160 * 1024 && G256_DW_LDS >= G256_LDS, "the GLU tile (and the ring) fit a CU's LDS");
  if constexpr (DWK > 0) {
    ZV_REQUIRE(p.dw_w && p.dw_b && p.dw_out && p.dw_L > 0 && p.M % p.dw_L == 0 && p.N == 2 * 512 &&
                   p.ld_dw % 2 == 0 && !persistent,
               "fused GLU + depthwise conv: taps, bias, output, whole utterances, 512 channels, one tile per block");
  }
  ZV_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "empty GEMM");
  ZV_REQUIRE(!p.Cl && p.nz2 == 1 && !p.As && p.Brows >= p.N,
             "gemm256: 16-bit operands (lo halves ignored), one batch");
  ZV_REQUIRE(p.lda % 8 == 0 && p.ldb % 8 == 0 && p.lda >= round_up(p.K, GEMM_BK) &&
                 p.ldb >= round_up(p.K, GEMM_BK),
             "gemm256: operand rows padded to the 64-deep K step");
  ZV_REQUIRE((long)p.M * p.lda * 2 < (1L << 32) && (long)p.Brows * p.ldb * 2 < (1L << 32),
             "GEMM operand larger than the 4 GiB DMA offset range");
  if constexpr (MXO > 0)
    ZV_REQUIRE(p.Cq && p.Cs && p.ldcq % MX8_KSTEP == 0 && p.N <= p.ldcq,
               "fp8 output copy: values and scales, row stride a multiple of 128");
  GemmParams pr = ROLE == 9 ? p : gemm_prep_epilogue<1, EPI, ROLE, MXO, 0>(p, 1);
  if constexpr (DIRECT && ROLE != 9)
    ZV_REQUIRE(p.N % 8 == 0 && (EPI != EPI_GLU || p.ldch % 8 == 0) && (p.act == 0 || p.act == 1),
               "gemm256 direct epilogue: N % 8 == 0, activation none or SwooshL");
  const int tiles = cdiv(p.N, 256) * cdiv(p.M, 256 - 2 * (DWK / 2));
  // persistent: one block per CU walking the tiles (K pipeline continuous across tiles);
  // else one tile per block (the hardware refills CUs as blocks retire: tail filling)
  int G = persistent ? std::min(zv_num_cus(), tiles) : tiles;
  G = std::max(8, (G + 7) / 8 * 8);
  char dtag[160];
  if (g_zv_prof.detail) {
    snprintf(dtag, sizeof(dtag), "%s M=%d N=%d K=%d z=1 tile=256x256", tag, p.M, p.N, p.K);
    tag = dtag;
  }
  // (fused conv: + its 2 k FLOP per output; algorithmic bytes: A and W once, the conv output's
  // 16-bit copy -- the GLU output no longer exists)
  const double fl = 2.0 * p.M * p.N * (double)p.K + (DWK ? 2.0 * DWK * p.M * (p.N / 2) : 0.0);
  const double by = DWK ? 2.0 * ((double)p.M * p.K + (double)p.N * p.K + (double)p.M * (p.N / 2))
                        : gemm_alg_bytes<1, ROLE, MXO>(p, 1);
  g_zv_last_launch = ZvLaunchRec{256, 256, 1, EPI, ROLE, 1, G, 0};
  ZvProfScope prof(tag, fl, by, s);
  hipLaunchKernelGGL((zv_gemm256_kernel<EPI, ROLE, PB, MXO, DIRECT, DRAIN, DWK>), dim3(G), dim3(512),
                     DWK ? G256_DW_LDS : G256_LDS, s, pr);
  ZV_LAUNCH_CHECK();
}
