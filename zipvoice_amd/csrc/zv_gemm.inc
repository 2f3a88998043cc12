// MFMA GEMM for gfx950 (CDNA4): 16x16x32 bf16 MFMA, 64-wide waves, BK = 64.
//
//   C[z] = epilogue( A[z] (M x K, row-major) . B[z]^T + bias ),  B stored [N][K]
//
// Operands are bf16 in HBM.  In the fp32-accurate mode (SPLIT = 3) every
// operand is a pair of bf16 arrays hi = bf16(x), lo = bf16(x - hi) written by
// the producing kernel, and a.b ~= ah.bh + ah.bl + al.bh (relative error ~2^-16
// per product, fp32 accumulation) — 3 MFMAs per product at 16x the f32-MFMA rate.
//
// Staging: global_load_lds (16 B per lane, lane-linear 1 KiB pieces) into a
// double-buffered LDS image of 128-B rows with the 16-B chunk XOR swizzle
// pos = chunk ^ (row & 7) applied on the SOURCE address (conflict-free
// ds_read_b128 fragment reads); one barrier per 64-deep K step, the next tile's
// loads in flight under the current tile's MFMAs.  Tiles are mapped XCD-aware:
// the 8 XCDs each take a contiguous range of the (m, n) tile grid, n fastest,
// so the n-tiles sharing an A row panel hit the same L2.
//
// Epilogues (the reference's op order):
//   STD : v = acc + bias; act(v); v *= mul; v = resid + v; v += rowvec[row group];
//         v = orig + (v - orig) * byp;  -> C (fp32) and/or Ch/Cl (bf16 hi/lo)
//   TRANS: v = acc + bias -> Ct[m / rpb][n][m % rpb]     (values transposed for the
//         attention consumers: V^T rows are K-contiguous B operands)
//   NA  : weight rows permuted in groups of 48 = [s16 | x16 | y16]:
//         xs = x * tanh(s) -> Ct (transposed), y -> Ch          (NonlinAttention gate)
//   GLU : weight rows permuted in groups of 32 = [x16 | s16]:
//         g = x * sigmoid(s), 0 on padded rows -> Ch            (ConvolutionModule GLU)
//   SPEC: weight rows permuted in groups of 32 = [mag16 | phase16] (vocoder ISTFTHead):
//         m = min(exp(mag), 1e2); re = m cos(phase) -> Ch[:, c], im = m sin(phase)
//         -> Ch[:, spec_im_off + c]                                  (the irfft GEMM's A operand)
//   MAG : weight rows permuted in groups of 32 = [re16 | im16] (STFT basis):
//         |X| = sqrt(re^2 + im^2) -> Ch[:, c]                     (the mel GEMM's A operand)
// STD activations: 1 SwooshL (scaling.py:1174-1180), 2 GELU (erf form, vocos ConvNeXt),
//                  3 log(max(x, 1e-7)) (VocosFbank log-mel);
// STD colscale: v *= colscale[n] after act/mul, before the residual (vocos layer scale).
#pragma once
#include "zv_common.h"
#include "zv_mx8.inc"

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

enum { EPI_STD = 0, EPI_TRANS = 1, EPI_NA = 2, EPI_GLU = 3, EPI_SPEC = 4, EPI_MAG = 5 };

struct GemmParams {
  int M, N, K, nz2;                // blockIdx.z = z1 * nz2 + z2
  int Brows;                       // rows of B that may be read (clamp); >= N
  const bf16* Ah; const bf16* Al; long lda, sA1, sA2;
  const bf16* Bh; const bf16* Bl; long ldb, sB1, sB2;
  const float* bias;
  int act;                         // 0 none, 1 SwooshL, 2 GELU (erf), 3 log-clamp
  const float* colscale;           // per-column scale (after act/mul), or null
  int spec_im_off;                 // SPEC: column offset of the imaginary half
  float* C; long ldc, sC1, sC2;    // fp32 output
  bf16* Ch; bf16* Cl; long ldch, sCh1, sCh2;  // bf16 hi/lo output
  const bf16* mulh; const bf16* mull; long ldmul, smul1, smul2;
  const float* resid;              // indexed like C (may alias C)
  const float* rowvec; long rowvec_ld; int rows_per_group;
  const float* orig; const float* byp;
  bf16* Cth; bf16* Ctl; long ldct; int rpb; long sCt;  // transposed output
  const uint8_t* rowmask;          // GLU: rows to zero
  int rowmask_step;                // counted GLU epilogue: 1, or 0 with rowmask -> a zero byte
  // RP (bf16-mode residual stream as a bf16 hi/lo pair, indexed like Ch): the
  // residual input and the bypass original as pairs instead of fp32
  const bf16* residh; const bf16* residl; const bf16* origh; const bf16* origl;
  // CONV (implicit-GEMM Conv1d): K = taps * conv_c; the A rows of K step k0 are shifted
  // by tap * conv_d - conv_pad (tap = k0 / conv_c), so A is the (rows, conv_c) activation
  // itself with >= conv_pad valid (zero) halo rows around it; conv_c % BK == 0
  int conv_c, conv_d, conv_pad;
  // counted residual epilogue (gemm_epilogue_res): stores of rows / columns outside the
  // output land here (64 KiB, never read)
  float* sink;
  // SPLIT = 8 (MX-fp8 operands, zv_mx8.inc): Ah / Bh point at the e4m3 bytes (lda / ldb in
  // bytes), As / Bs at the E8M0 scale bytes (rows, ldas / ldbs = K / 32 row strides)
  const uint8_t* As; const uint8_t* Bs; long ldas, ldbs;
  // the fp8 copy of the output (counted epilogues; the next fp8 linear's A operand)
  uint8_t* Cq; uint8_t* Cs; long ldcq;
  // fused GLU + depthwise conv (zv_gemm256.inc, DWK > 0): the conv's taps (channels, k) and bias,
  // its SwooshR output (rows, ld_dw) and the frames per utterance (rows of one utterance)
  const float* dw_w; const float* dw_b; bf16* dw_out; long ld_dw; int dw_L;
};

constexpr int GEMM_BK = 64;

// LDS bytes of one ring stage: A and B rows (+ lo halves in the split mode), plus the MX-fp8
// mode's scale bytes (4 per row per 128-deep K step, rows rounded up to the 64-row DMA piece)
template <int BM, int BN, int SPLIT, int BK>
constexpr int gemm_stage_bytes() {
  return SPLIT == 8 ? (BM + BN) * BK + ((BM + 63) / 64 + (BN + 63) / 64) * 256
                    : ((SPLIT == 3 ? 2 : 1) * BM + (SPLIT == 3 || SPLIT == 2 ? 2 : 1) * BN) * BK * 2;
}

// The fp32 value a hi / lo pair is split from, pinned to one register in the fp16-operand build.  There
// the compiler may fold the multiply that produced the value into the hi conversion for one use of hi
// (v_fma_mixlo_f16: the exact product rounded once) and convert the fp32-rounded product for the other
// (rounded twice).  Where the fp32 product lies on an fp16 tie and the exact one beside it, the stored hi
// and the hi that lo was taken against differ by an ulp, and hi + lo is off by that ulp (2^-10 relative):
// zv_attn_na_kernel<3>'s out = acc * y, about one element in 10^5 (tests/test_gpu_attn_ref.py).  The
// empty asm costs no instruction.
__device__ __forceinline__ float split_pin(float v) {
#ifdef ZV_OPERAND_F16
  asm("" : "+v"(v));
#endif
  return v;
}

__device__ __forceinline__ void split_store(bf16* hi, bf16* lo, long i, float v) {
  v = split_pin(v);
  const bf16 h = (bf16)v;
  hi[i] = h;
  if (lo) lo[i] = (bf16)(v - (float)h);
}
__device__ __forceinline__ float ld_split(const bf16* hi, const bf16* lo, long i) {
  float v = (float)hi[i];
  if (lo) v += (float)lo[i];
  return v;
}

// global -> LDS DMA of 16 B per lane (lane-linear destination at lds_base + 16*lane).
// Issued as inline asm so hipcc's waitcnt pass does not treat every later
// ds_read as aliasing the in-flight DMA (it would otherwise insert vmcnt(0)
// before the fragment reads and serialise the pipeline); the kernel orders the
// DMA against its readers itself (counted vmcnt + barrier).
__device__ __forceinline__ void glds16(const void* gptr, const void* lds_base) {
  const unsigned lds = (unsigned)(uintptr_t)lds_base;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
               :: "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(gptr) : "memory", "m0");
}

// The same DMA in the scalar-base form: address = sbase (uniform, SGPR pair) + voff
// (per-lane unsigned byte offset).  The per-lane row offsets are fixed for a tile, so
// a K step only moves the scalar base: no 64-bit address arithmetic per piece.
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, const void* lds_base) {
  const unsigned lds = (unsigned)(uintptr_t)lds_base;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
               :: "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(voff), "s"(sbase) : "memory", "m0");
}
// Four consecutive 1 KiB pieces (source and destination both contiguous) under one M0 write:
// the instruction offset applies to the global and the LDS address alike, so pieces 1-3 are the
// same instruction at offset:1024/2048/3072 (one s_mov/s_nop and no scalar address math for them)
__device__ __forceinline__ void glds16s_x4(const void* sbase, unsigned voff, const void* lds_base) {
  const unsigned lds = (unsigned)(uintptr_t)lds_base;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %1, %2\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:3072"
               :: "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(voff), "s"(sbase) : "memory", "m0");
}
// 4 B per lane (the MX-fp8 scale rows: one lane per row, 64 rows per piece)
__device__ __forceinline__ void glds4s(const void* sbase, unsigned voff, const void* lds_base) {
  const unsigned lds = (unsigned)(uintptr_t)lds_base;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2"
               :: "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(voff), "s"(sbase) : "memory", "m0");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---------------------------------------------------------------------------
// Epilogue.  The accumulator of a 16x16 tile has each lane holding one column
// of 4 rows; storing that directly gives 2-4 B per lane, which is store-issue
// bound.  Instead each wave stages one 16-row strip of its whole sub-tile
// (16 x WN fp32) in LDS and reads it back row-major, 4 consecutive columns per
// lane, so the epilogue loads (bias, resid, orig, mul) and stores (fp32 C 16 B,
// bf16 hi/lo 8 B per lane) are vectorised and each row segment is WN wide.
// The scratch is the ring stage the tile's last K step just consumed (free
// until the next tile's issue, which sits behind the next K-step barrier).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
}
__device__ __forceinline__ float epi_act(int act, float x) {
  return act == 1 ? swoosh_l(x) : (act == 2 ? gelu_erf(x) : (act == 3 ? logf(fmaxf(x, 1e-7f)) : x));
}

template <int TN>
struct EpiScratch {
  static constexpr int W = 16 * TN;
  static constexpr int LDW = W + 4;                   // padded fp32 row (bank spread)
  static constexpr int BYTES = 16 * LDW * 4;
};

__device__ __forceinline__ void store_split4(bf16* hi, bf16* lo, long i, const float (&v)[4]) {
  bf16x4 h, l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x = split_pin(v[j]);
    h[j] = (bf16)x;
    l[j] = (bf16)(x - (float)h[j]);
  }
  *reinterpret_cast<bf16x4*>(hi + i) = h;
  if (lo) *reinterpret_cast<bf16x4*>(lo + i) = l;
}
__device__ __forceinline__ void store_split8(bf16* hi, bf16* lo, long i, const float (&v)[8]) {
  bf16x8 h, l;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = split_pin(v[j]);
    h[j] = (bf16)x;
    l[j] = (bf16)(x - (float)h[j]);
  }
  *reinterpret_cast<bf16x8*>(hi + i) = h;
  if (lo) *reinterpret_cast<bf16x8*>(lo + i) = l;
}
__device__ __forceinline__ void load_split4(const bf16* hi, const bf16* lo, long i, float (&v)[4]) {
  const bf16x4 h = *reinterpret_cast<const bf16x4*>(hi + i);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (float)h[j];
  if (lo) {
    const bf16x4 l = *reinterpret_cast<const bf16x4*>(lo + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += (float)l[j];
  }
}

// SWZ: unpadded strip (16 x WN fp32, WN a power of two >= 64) with the 16-column
// groups XOR-swizzled by row quad instead of the padded row (bank spread at
// 4 KiB per wave for WN = 64: the 256x256 kernel's scratch budget).
// RP: the residual (and bypass original) arrive as bf16 hi/lo pairs (p.residh /
// p.residl, p.origh / p.origl, indexed like Ch) and the result leaves as the pair
// (Ch / Cl): 8 B per residual update instead of fp32 read + write + bf16 copy.
template <int TM, int TN, int EPI, bool SWZ = false, int RP = 0>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x4 (&acc)[TM][TN], int m0,
                                              int n0, int z1, int z2, int lane, float* scr) {
  constexpr int WN = EpiScratch<TN>::W;      // staged columns (the wave's full width)
  constexpr int LDW = SWZ ? WN : EpiScratch<TN>::LDW;
  static_assert(!SWZ || (WN >= 64 && (WN & (WN - 1)) == 0), "swizzled strip needs WN = 2^k >= 64");
  auto sx = [](int row, int col) -> int {
    return SWZ ? row * LDW + (col ^ (((row >> 2) & 3) << 4)) : row * LDW + col;
  };
  static_assert(EPI != EPI_NA || TN % 3 == 0, "NA epilogue needs triples of n-tiles");
  static_assert((EPI != EPI_GLU && EPI != EPI_SPEC && EPI != EPI_MAG) || TN % 2 == 0,
                "GLU/SPEC/MAG epilogues need pairs of n-tiles");
  const long cbase = z1 * p.sC1 + z2 * p.sC2;
  const long hbase = z1 * p.sCh1 + z2 * p.sCh2;
  const bf16* MH = p.mulh ? p.mulh + z1 * p.smul1 + z2 * p.smul2 : nullptr;
  const bf16* ML = p.mull ? p.mull + z1 * p.smul1 + z2 * p.smul2 : nullptr;
  // STD: each lane owns 8 consecutive columns of a row (two LDS quads -> one
  // 16-B bf16 store, two 16-B fp32 loads/stores): half the store instructions
  // of 4-column chunks (the epilogue tail is store-issue bound).
  // The residual reads run ahead of the strips (a window of PD strips, up to PF
  // 16-B loads in flight per lane): the RMW epilogues of the residual-stream
  // linears are HBM-latency bound otherwise.  The window bounds the registers
  // the prefetch holds next to the accumulators (a whole-tile prefetch spills
  // the TM = 8 tiles).
  constexpr int C8 = WN / 8, NCH = 16 * C8, Q8 = (NCH + 63) / 64;
  constexpr int PF = (TM * TN >= 32) ? 8 : 16;   // 16-B loads per lane in flight
  constexpr int PD = (PF / (2 * Q8)) < 1 ? 1 : ((PF / (2 * Q8)) > TM ? TM : (PF / (2 * Q8)));
  constexpr int PTM = EPI == EPI_STD ? TM : 1, PQ = EPI == EPI_STD ? Q8 : 1;
  f32x4 rpre[RP ? 1 : PTM][RP ? 1 : PQ][2];
  bf16x8 rph[RP ? PTM : 1][RP ? PQ : 1], rpl[RP ? PTM : 1][RP ? PQ : 1];
  auto prefetch_strip = [&](int i) {
    if constexpr (EPI == EPI_STD && RP) {
      if (i < TM) {
#pragma unroll
        for (int q = 0; q < Q8; ++q) {
          const int idx = lane + 64 * q;
          const int m = m0 + i * 16 + idx / C8, n = n0 + (idx % C8) * 8;
          if ((NCH % 64 == 0 || idx < NCH) && m < p.M && n + 7 < p.N) {
            const long hi = hbase + (long)m * p.ldch + n;
            rph[i][q] = *reinterpret_cast<const bf16x8*>(p.residh + hi);
            rpl[i][q] = *reinterpret_cast<const bf16x8*>(p.residl + hi);
          }
        }
      }
    } else if constexpr (EPI == EPI_STD) {
      if (p.resid && i < TM) {
#pragma unroll
        for (int q = 0; q < Q8; ++q) {
          const int idx = lane + 64 * q;
          const int m = m0 + i * 16 + idx / C8, n = n0 + (idx % C8) * 8;
          if ((NCH % 64 == 0 || idx < NCH) && m < p.M && n + 7 < p.N) {
            const float* src = p.resid + cbase + (long)m * p.ldc + n;
            rpre[i][q][0] = *reinterpret_cast<const f32x4*>(src);
            rpre[i][q][1] = *reinterpret_cast<const f32x4*>(src + 4);
          }
        }
      }
    }
  };
#pragma unroll
  for (int i = 0; i < PD - 1; ++i) prefetch_strip(i);
  // strips as a compile-time loop: the accumulator and prefetch indices must be
  // constants (a rolled loop over a large body puts acc[] in scratch)
  static_for<TM>([&](auto I_) {
    constexpr int i = decltype(I_)::value;
    prefetch_strip(i + PD - 1);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        scr[sx((lane >> 4) * 4 + r, j * 16 + (lane & 15))] = acc[i][j][r];
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): strip visible to the wave
    __builtin_amdgcn_wave_barrier();
    const int mrow0 = m0 + i * 16;
    if constexpr (EPI == EPI_STD) {
#pragma unroll
      for (int q = 0; q < Q8; ++q) {
        const int idx = lane + 64 * q;
        const int row = idx / C8, c8 = (idx % C8) * 8;
        const int m = mrow0 + row, n = n0 + c8;
        if ((NCH % 64 == 0 || idx < NCH) && m < p.M && n < p.N) {
          float v[8];
          {
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(scr + sx(row, c8));
            const f32x4 t1 = *reinterpret_cast<const f32x4*>(scr + sx(row, c8 + 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = t0[e]; v[4 + e] = t1[e]; }
          }
          if (n + 7 < p.N) {
            if (p.bias) {
              const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + n);
              const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.bias + n + 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) { v[e] += b0[e]; v[4 + e] += b1[e]; }
            }
            // uniform (scalar) branches: one activation evaluated per element
            if (p.act == 1) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = swoosh_l(v[e]);
            } else if (p.act == 2) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = gelu_erf(v[e]);
            } else if (p.act == 3) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = logf(fmaxf(v[e], 1e-7f));
            }
            if (MH) {
              float mv[4];
#pragma unroll
              for (int hh = 0; hh < 2; ++hh) {
                load_split4(MH, ML, (long)m * p.ldmul + n + 4 * hh, mv);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * hh + e] *= mv[e];
              }
            }
            if (p.colscale) {
              const f32x4 c0 = *reinterpret_cast<const f32x4*>(p.colscale + n);
              const f32x4 c1 = *reinterpret_cast<const f32x4*>(p.colscale + n + 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) { v[e] *= c0[e]; v[4 + e] *= c1[e]; }
            }
            const long ci = cbase + (long)m * p.ldc + n;
            if constexpr (RP) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = ((float)rph[i][q][e] + (float)rpl[i][q][e]) + v[e];
            } else if (p.resid) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                v[e] = rpre[i][q][0][e] + v[e];
                v[4 + e] = rpre[i][q][1][e] + v[4 + e];
              }
            }
            if (p.rowvec) {
              const float* rp = p.rowvec + (long)(m / p.rows_per_group) * p.rowvec_ld + n;
              const f32x4 r0 = *reinterpret_cast<const f32x4*>(rp);
              const f32x4 r1 = *reinterpret_cast<const f32x4*>(rp + 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) { v[e] += r0[e]; v[4 + e] += r1[e]; }
            }
            if (RP && p.origh) {
              const long hi = hbase + (long)m * p.ldch + n;
              const bf16x8 oh = *reinterpret_cast<const bf16x8*>(p.origh + hi);
              const bf16x8 ol = *reinterpret_cast<const bf16x8*>(p.origl + hi);
              const f32x4 s0 = *reinterpret_cast<const f32x4*>(p.byp + n);
              const f32x4 s1 = *reinterpret_cast<const f32x4*>(p.byp + n + 4);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float o = (float)oh[e] + (float)ol[e];
                v[e] = o + (v[e] - o) * (e < 4 ? s0[e] : s1[e - 4]);
              }
            } else if (p.orig) {
              const f32x4 o0 = *reinterpret_cast<const f32x4*>(p.orig + ci);
              const f32x4 o1 = *reinterpret_cast<const f32x4*>(p.orig + ci + 4);
              const f32x4 s0 = *reinterpret_cast<const f32x4*>(p.byp + n);
              const f32x4 s1 = *reinterpret_cast<const f32x4*>(p.byp + n + 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                v[e] = o0[e] + (v[e] - o0[e]) * s0[e];
                v[4 + e] = o1[e] + (v[4 + e] - o1[e]) * s1[e];
              }
            }
            if (p.C) {
              *reinterpret_cast<f32x4*>(p.C + ci) = f32x4{v[0], v[1], v[2], v[3]};
              *reinterpret_cast<f32x4*>(p.C + ci + 4) = f32x4{v[4], v[5], v[6], v[7]};
            }
            if (p.Ch) {
              const long hi = hbase + (long)m * p.ldch + n;
              if ((p.ldch & 7) == 0) {
                store_split8(p.Ch, p.Cl, hi, v);
              } else {
                store_split4(p.Ch, p.Cl, hi, *reinterpret_cast<const float(*)[4]>(v));
                store_split4(p.Ch, p.Cl, hi + 4, *reinterpret_cast<const float(*)[4]>(v + 4));
              }
            }
          } else {   // ragged right edge (N % 8 != 0)
            for (int e = 0; e < 8 && n + e < p.N; ++e) {
              const int ne = n + e;
              float x = v[e] + (p.bias ? p.bias[ne] : 0.f);
              if (p.act) x = epi_act(p.act, x);
              if (MH) x *= ld_split(MH, ML, (long)m * p.ldmul + ne);
              if (p.colscale) x *= p.colscale[ne];
              const long ci = cbase + (long)m * p.ldc + ne;
              if (p.resid) x = p.resid[ci] + x;
              if (p.rowvec) x += p.rowvec[(long)(m / p.rows_per_group) * p.rowvec_ld + ne];
              if (p.orig) { const float o = p.orig[ci]; x = o + (x - o) * p.byp[ne]; }
              if (p.C) p.C[ci] = x;
              if (p.Ch) split_store(p.Ch, p.Cl, hbase + (long)m * p.ldch + ne, x);
            }
          }
        }
      }
    } else if constexpr (EPI == EPI_TRANS) {
      // column-major read-back: lane -> (column, 4 consecutive rows)
#pragma unroll
      for (int q = 0; q < (16 * WN) / (64 * 4); ++q) {
        const int idx = lane + 64 * q;
        const int col = idx % WN, rg = idx / WN;
        const int n = n0 + col;
        if (n >= p.N) continue;
        const float bn = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = mrow0 + rg * 4 + e;
          if (m >= p.M) continue;
          const int bb = m / p.rpb, l = m % p.rpb;
          split_store(p.Cth, p.Ctl, bb * p.sCt + (long)n * p.ldct + l,
                      scr[sx(rg * 4 + e, col)] + bn);
        }
      }
    } else if constexpr (EPI == EPI_NA) {
      // groups of 48 permuted columns [s16 | x16 | y16] -> 16 channels
#pragma unroll
      for (int t = 0; t < TN / 3; ++t) {
        const int nb = n0 + t * 48;
        if (nb >= p.N) continue;
        const int cbase16 = (nb / 48) * 16;
        {   // y (row-major): 16 rows x 16 channels = 64 chunks of 4
          const int row = lane >> 2, c4 = (lane & 3) * 4;
          const int m = mrow0 + row;
          if (m < p.M) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
              v[e] = scr[sx(row, t * 48 + 32 + c4 + e)] + p.bias[nb + 32 + c4 + e];
            store_split4(p.Ch, p.Cl, (long)m * p.ldch + cbase16 + c4, v);
          }
        }
        {   // x * tanh(s), transposed: lane -> (channel, 4 rows)
          const int ch = lane & 15, rg = lane >> 4;
          const float bs_ = p.bias[nb + ch], bx = p.bias[nb + 16 + ch];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int row = rg * 4 + e, m = mrow0 + row;
            if (m >= p.M) continue;
            const float sv = scr[sx(row, t * 48 + ch)] + bs_;
            const float xv = scr[sx(row, t * 48 + 16 + ch)] + bx;
            const int bb = m / p.rpb, l = m % p.rpb;
            split_store(p.Cth, p.Ctl, bb * p.sCt + (long)(cbase16 + ch) * p.ldct + l,
                        __fmul_rn(xv, tanh_fast(sv)));
          }
        }
      }
    } else if constexpr (EPI == EPI_MAG) {
      // groups of 32 permuted columns [re16 | im16] -> 16 magnitudes
      constexpr int CPR = WN / 8;
#pragma unroll
      for (int q = 0; q < (16 * CPR) / 64; ++q) {
        const int idx = lane + 64 * q;
        const int row = idx / CPR, cc = idx % CPR;
        const int grp = cc >> 2, c4 = (cc & 3) * 4;
        const int nb = n0 + grp * 32;
        const int m = mrow0 + row;
        if (nb < p.N && m < p.M) {
          float mg[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float re = scr[sx(row, grp * 32 + c4 + e)];
            const float im = scr[sx(row, grp * 32 + 16 + c4 + e)];
            mg[e] = sqrtf(re * re + im * im);
          }
          store_split4(p.Ch, p.Cl, (long)m * p.ldch + (nb / 32) * 16 + c4, mg);
        }
      }
    } else if constexpr (EPI == EPI_SPEC) {
      // groups of 32 permuted columns [mag16 | phase16] -> 16 bins (re, im)
      constexpr int CPR = WN / 8;
#pragma unroll
      for (int q = 0; q < (16 * CPR) / 64; ++q) {
        const int idx = lane + 64 * q;
        const int row = idx / CPR, cc = idx % CPR;
        const int grp = cc >> 2, c4 = (cc & 3) * 4;
        const int nb = n0 + grp * 32;
        const int m = mrow0 + row;
        if (nb < p.N && m < p.M) {
          float re[4], im[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float mg = scr[sx(row, grp * 32 + c4 + e)] + p.bias[nb + c4 + e];
            const float ph = scr[sx(row, grp * 32 + 16 + c4 + e)] + p.bias[nb + 16 + c4 + e];
            const float mag = fminf(expf(mg), 100.0f);
            float sn, cs;
            sincosf(ph, &sn, &cs);
            re[e] = mag * cs;
            im[e] = mag * sn;
          }
          const long o = (long)m * p.ldch + (nb / 32) * 16 + c4;
          store_split4(p.Ch, p.Cl, o, re);
          store_split4(p.Ch, p.Cl, o + p.spec_im_off, im);
        }
      }
    } else {  // EPI_GLU: groups of 32 permuted columns [x16 | s16] -> 16 channels
      constexpr int CPR = WN / 16;        // output 8-channel chunks per row (one 16-B store)
#pragma unroll
      for (int q = 0; q < (16 * CPR + 63) / 64; ++q) {
        const int idx = lane + 64 * q;
        const int row = idx / CPR, cc = idx % CPR;
        const int grp = cc >> 1, c8 = (cc & 1) * 8;
        const int nb = n0 + grp * 32;
        const int m = mrow0 + row;
        if (((16 * CPR) % 64 == 0 || idx < 16 * CPR) && nb < p.N && m < p.M) {
          const bool zero = p.rowmask && p.rowmask[m];
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xv = scr[sx(row, grp * 32 + c8 + e)] + p.bias[nb + c8 + e];
            const float sv = scr[sx(row, grp * 32 + 16 + c8 + e)] + p.bias[nb + 16 + c8 + e];
            v[e] = zero ? 0.f : xv * sigmoidf_(sv);
          }
          const long o = (long)m * p.ldch + (nb / 32) * 16 + c8;
          if ((p.ldch & 7) == 0) {
            store_split8(p.Ch, p.Cl, o, v);
          } else {
            store_split4(p.Ch, p.Cl, o, *reinterpret_cast<const float(*)[4]>(v));
            store_split4(p.Ch, p.Cl, o + 4, *reinterpret_cast<const float(*)[4]>(v + 4));
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();   // strip consumed before the next overwrite
    __builtin_amdgcn_s_waitcnt(0xC07F);
  });
}

// strip scratch index: padded rows (LDW) or, SWZ, unpadded 16 x WN rows with the 16-column
// groups XOR-swizzled by row quad (conflict-free accumulator writes; 8-column reads stay whole)
template <int TN, bool SWZ>
__device__ __forceinline__ int epi_sx(int row, int col) {
  return SWZ ? row * (16 * TN) + (col ^ (((row >> 2) & 3) << 4)) : row * EpiScratch<TN>::LDW + col;
}

// Counted residual epilogue (the residual-stream linears, ROLE >= 1): the same arithmetic
// as gemm_epilogue's STD path for {bias, resid, C, Ch/Cl, orig (ROLE 2)}, with every
// global memory operation issued unconditionally, so hipcc's waitcnt pass counts them
// exactly.  In the general epilogue the residual prefetches sit behind per-lane row
// predicates and the bias / orig / C / Ch accesses behind uniform runtime branches: the
// pass must assume the branches were skipped, so each chunk's bias load waited for
// vmcnt(0) - every prefetched strip and every earlier store - and the prefetch window
// bought nothing.  Here bias (and byp) are loaded once per tile (a lane's 8 columns are
// the same in every strip), the residual (and orig) loads read clamped rows / columns,
// and the stores of rows >= M or columns >= N go to p.sink through an address the
// compiler cannot split into branches.  Requires N % 8 == 0, nz == 1 (host checks).
#define GLOBAL __attribute__((address_space(1)))
// RES = false: the plain linears' form of the same epilogue (ROLE 3): bias, activation,
// bf16 copy only (no residual, no fp32 output) - no loads inside the strips at all.
// MXO (fp8 mode): 1 = also write the MX-fp8 copy (p.Cq / p.Cs: the next fp8 linear's A
// operand; a 32-column block is 4 adjacent lanes), 2 = the fp8 copy instead of the bf16 one.
// RV: also the row-group vector (p.rowvec[m / rows_per_group], the stack's time embedding),
// loaded with the residual rows (the K-concatenated convolution out-projection that also
// finishes the SelfAttention residual update; zv_engine layer())
// NOC: no fp32 output (the SelfAttention out-projection whose fp32 update the conv
// out-projection finishes: residual + row vector -> the bf16 copy only)
// SWZ: the unpadded swizzled strip (epi_sx; the 256x256 kernel's 4 KiB per wave); PDM caps
// the strips whose residual operands are held in registers ahead (the 8-strip tiles)
template <int TM, int TN, int NS, bool ORIG, bool RES = true, int MXO = 0, bool RV = false, bool NOC = false,
          bool SWZ = false, int PDM = 16>
__device__ __forceinline__ void gemm_epilogue_res(const GemmParams& p, f32x4 (&acc)[TM][TN], int m0,
                                                  int n0, int lane, float* scr) {
  constexpr int WN = EpiScratch<TN>::W;
  constexpr int C8 = WN / 8, NCH = 16 * C8, Q8 = NCH / 64;
  static_assert(NCH % 64 == 0 && 64 % C8 == 0, "a lane's column chunk is fixed across strips");
  constexpr int PD0 = ORIG ? (TM < 2 ? TM : 2) : TM;    // strips prefetched ahead (registers)
  constexpr int PD = PD0 < PDM ? PD0 : PDM;
  const int c8 = (lane % C8) * 8, n = n0 + c8, nc = min(n, p.N - 8);
  const bool col_ok = n < p.N;
  f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + nc);
  f32x4 b1 = *reinterpret_cast<const f32x4*>(p.bias + nc + 4);
  f32x4 s0, s1;
  if constexpr (ORIG) {
    s0 = *reinterpret_cast<const f32x4*>(p.byp + nc);
    s1 = *reinterpret_cast<const f32x4*>(p.byp + nc + 4);
  }
  f32x4 rr[RES ? TM : 1][Q8][2], ro[ORIG ? TM : 1][Q8][2], rv[RV ? TM : 1][Q8][2];
  auto prefetch_strip = [&](int i) {
    if (RES && i < TM) {
#pragma unroll
      for (int q = 0; q < Q8; ++q) {
        const int m = min(m0 + i * 16 + (lane + 64 * q) / C8, p.M - 1);
        const long ci = (long)m * p.ldc + nc;
        rr[i][q][0] = *reinterpret_cast<const f32x4*>(p.resid + ci);
        rr[i][q][1] = *reinterpret_cast<const f32x4*>(p.resid + ci + 4);
        if constexpr (RV) {
          const float* vp = p.rowvec + (long)(m / p.rows_per_group) * p.rowvec_ld + nc;
          rv[i][q][0] = *reinterpret_cast<const f32x4*>(vp);
          rv[i][q][1] = *reinterpret_cast<const f32x4*>(vp + 4);
        }
        if constexpr (ORIG) {
          ro[i][q][0] = *reinterpret_cast<const f32x4*>(p.orig + ci);
          ro[i][q][1] = *reinterpret_cast<const f32x4*>(p.orig + ci + 4);
        }
      }
    }
  };
#pragma unroll
  for (int i = 0; i < PD - 1; ++i) prefetch_strip(i);
  static_for<TM>([&](auto I_) {
    constexpr int i = decltype(I_)::value;
    prefetch_strip(i + PD - 1);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[epi_sx<TN, SWZ>((lane >> 4) * 4 + r, j * 16 + (lane & 15))] = acc[i][j][r];
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): strip visible to the wave
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < Q8; ++q) {
      const int row = (lane + 64 * q) / C8;
      const int m = m0 + i * 16 + row;
      float v[8];
      {
        const f32x4 t0 = *reinterpret_cast<const f32x4*>(scr + epi_sx<TN, SWZ>(row, c8));
        const f32x4 t1 = *reinterpret_cast<const f32x4*>(scr + epi_sx<TN, SWZ>(row, c8 + 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = t0[e]; v[4 + e] = t1[e]; }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] += b0[e]; v[4 + e] += b1[e]; }
      if constexpr (!RES) {              // uniform branches, arithmetic only
        if (p.act == 1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = swoosh_l(v[e]);
        } else if (p.act == 2) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = gelu_erf(v[e]);
        } else if (p.act == 3) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = logf(fmaxf(v[e], 1e-7f));
        }
      }
      if constexpr (RES) {
        const int ir = RES ? i : 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = rr[ir][q][0][e] + v[e];
          v[4 + e] = rr[ir][q][1][e] + v[4 + e];
        }
      }
      if constexpr (RV) {                  // the general epilogue's order: resid + v, then + rowvec
        const int iv = RV ? i : 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] += rv[iv][q][0][e];
          v[4 + e] += rv[iv][q][1][e];
        }
      }
      if constexpr (ORIG) {
        const int io = ORIG ? i : 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = ro[io][q][0][e] + (v[e] - ro[io][q][0][e]) * s0[e];
          v[4 + e] = ro[io][q][1][e] + (v[4 + e] - ro[io][q][1][e]) * s1[e];
        }
      }
      const bool ok = col_ok && m < p.M;
      if constexpr (MXO > 0) {
        static_assert(C8 % 4 == 0, "a 32-column block is 4 adjacent lanes");
        unsigned sbyte;
        const u32x2 q8 = mx8_quant8(v, sbyte);
        unsigned long long qa = ok ? (unsigned long long)(p.Cq + (long)m * p.ldcq + n)
                                   : (unsigned long long)(p.sink + 12288 + lane * 2);
        unsigned long long sa = ok && (lane & 3) == 0
                                    ? (unsigned long long)(p.Cs + (long)m * (p.ldcq / MX8_BLOCK) + n / MX8_BLOCK)
                                    : (unsigned long long)(p.sink + 12800 + lane);
        asm volatile("" : "+v"(qa), "+v"(sa));
        *(GLOBAL u32x2*)(qa) = q8;
        *(GLOBAL uint8_t*)(sa) = (uint8_t)sbyte;
      }
      unsigned long long ha = ok ? (unsigned long long)(p.Ch + (long)m * p.ldch + n)
                                 : (unsigned long long)(p.sink + 512 + lane * 4);
      asm volatile("" : "+v"(ha));   // one store per lane, never a branch
      if constexpr (RES && !NOC) {
        unsigned long long ca = ok ? (unsigned long long)(p.C + (long)m * p.ldc + n)
                                   : (unsigned long long)(p.sink + lane * 8);
        asm volatile("" : "+v"(ca));
        // global (not flat) stores: address space 1 spelled out, the asm hides provenance
        *(GLOBAL f32x4*)(ca) = f32x4{v[0], v[1], v[2], v[3]};
        *(GLOBAL f32x4*)(ca + 16) = f32x4{v[4], v[5], v[6], v[7]};
      }
      bf16x8 h, l;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        h[e] = (bf16)v[e];
        l[e] = (bf16)(v[e] - (float)h[e]);
      }
      if constexpr (MXO != 2) *(GLOBAL bf16x8*)(ha) = h;
      if constexpr (NS == 2) {
        unsigned long long la = ok ? (unsigned long long)(p.Cl + (long)m * p.ldch + n)
                                   : (unsigned long long)(p.sink + 1024 + lane * 4);
        asm volatile("" : "+v"(la));
        *(GLOBAL bf16x8*)(la) = l;
      }
    }
    __builtin_amdgcn_wave_barrier();   // strip consumed before the next overwrite
    __builtin_amdgcn_s_waitcnt(0xC07F);
  });
}

// Counted forms of the fused epilogues (ROLE 3 with EPI_GLU / EPI_NA / EPI_TRANS): the same
// arithmetic as gemm_epilogue's branches, with the bias operands loaded once per tile (a
// lane's columns are the same in every strip), the GLU row mask prefetched for all strips,
// every store unconditional (outside the output: p.sink) and the transposed outputs'
// (utterance, frame) position advanced incrementally instead of an integer division per
// element.  Host checks: N % 32 (GLU) / N % 48 (NA) == 0, ldch % 8 == 0, nz == 1.
__device__ __forceinline__ void adv_pos(int& bb, int& l, int d, int rpb) {
  l += d;
  while (l >= rpb) { l -= rpb; ++bb; }
}

template <int TM, int TN, int NS, bool SWZ = false>
__device__ __forceinline__ void gemm_epilogue_glu_c(const GemmParams& p, f32x4 (&acc)[TM][TN],
                                                    int m0, int n0, int lane, float* scr) {
  constexpr int WN = EpiScratch<TN>::W;
  constexpr int CPR = WN / 16, Q = (16 * CPR) / 64;   // output 8-channel chunks per row
  static_assert((16 * CPR) % 64 == 0 && 64 % CPR == 0 && TN % 2 == 0, "GLU chunk layout");
  const int cc = lane % CPR, grp = cc >> 1, c8 = (cc & 1) * 8;
  const int nb = n0 + grp * 32, nbc = min(nb, p.N - 32);
  const bool col_ok = nb < p.N;
  const f32x4 bx0 = *reinterpret_cast<const f32x4*>(p.bias + nbc + c8);
  const f32x4 bx1 = *reinterpret_cast<const f32x4*>(p.bias + nbc + c8 + 4);
  const f32x4 bs0 = *reinterpret_cast<const f32x4*>(p.bias + nbc + 16 + c8);
  const f32x4 bs1 = *reinterpret_cast<const f32x4*>(p.bias + nbc + 16 + c8 + 4);
  uint8_t zr[TM][Q];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int m = min(m0 + i * 16 + (lane + 64 * q) / CPR, p.M - 1);
      zr[i][q] = p.rowmask[m * p.rowmask_step];
    }
  static_for<TM>([&](auto I_) {
    constexpr int i = decltype(I_)::value;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[epi_sx<TN, SWZ>((lane >> 4) * 4 + r, j * 16 + (lane & 15))] = acc[i][j][r];
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int row = (lane + 64 * q) / CPR, m = m0 + i * 16 + row;
      const bool zero = zr[i][q] != 0;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float bxe = e < 4 ? bx0[e] : bx1[e - 4], bse = e < 4 ? bs0[e] : bs1[e - 4];
        const float xv = scr[epi_sx<TN, SWZ>(row, grp * 32 + c8 + e)] + bxe;
        const float sv = scr[epi_sx<TN, SWZ>(row, grp * 32 + 16 + c8 + e)] + bse;
        v[e] = zero ? 0.f : xv * sigmoidf_(sv);
      }
      const bool ok = col_ok && m < p.M;
      const long o = (long)m * p.ldch + (nb / 32) * 16 + c8;
      bf16x8 h, l;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        h[e] = (bf16)v[e];
        l[e] = (bf16)(v[e] - (float)h[e]);
      }
      unsigned long long ha = ok ? (unsigned long long)(p.Ch + o) : (unsigned long long)(p.sink + 512 + lane * 4);
      asm volatile("" : "+v"(ha));
      *(GLOBAL bf16x8*)(ha) = h;
      if constexpr (NS == 2) {
        unsigned long long la = ok ? (unsigned long long)(p.Cl + o) : (unsigned long long)(p.sink + 1024 + lane * 4);
        asm volatile("" : "+v"(la));
        *(GLOBAL bf16x8*)(la) = l;
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
  });
}

// Utterance-aligned transposed stores (UTT tiling, zv_gemm_kernel: a wave's first row is frame l0,
// a multiple of 32, of utterance ub; no tile crosses an utterance).  The accumulator gives a lane
// (column lane & 15, rg = lane >> 4) rows 4 rg .. 4 rg + 3 of a strip: four consecutive frames of
// one row of the transposed output.  The lane rounds them in registers and packs them into two
// dwords; one v_permlane16_swap per dword against the next strip's (the pairing of zv_gemm256.inc's
// direct epilogues) leaves it the 8 consecutive frames that start utt_fofs = {0, 16, 8, 24} past
// the strip pair's first, written with one aligned 16-B store: no LDS round trip, no (utterance,
// frame) walk, one address per store.  Frames at or past the utterance's length are never written
// ([L, ldct) of V^T stays the workspace's zeros, which the attention kernels multiply by P = 0):
// the one group per row that straddles L stores its frames singly, a group wholly outside (or of a
// column >= N) goes to the sink.
__device__ __forceinline__ int utt_fofs(int lane) {
  const int g = lane >> 4;
  return ((g & 1) << 4) | ((g >> 1) << 3);
}
// a lane's four values of one strip, rounded as split_store rounds them, as two packed dwords
template <int NS>
__device__ __forceinline__ void pack_trans4(const float (&v)[4], unsigned (&wh)[2], unsigned (&wl)[2]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const bf16x2 h = {(bf16)v[2 * r], (bf16)v[2 * r + 1]};
    wh[r] = __builtin_bit_cast(unsigned, h);
    if constexpr (NS == 2) {
      const bf16x2 l = {(bf16)(v[2 * r] - (float)h[0]), (bf16)(v[2 * r + 1] - (float)h[1])};
      wl[r] = __builtin_bit_cast(unsigned, l);
    }
  }
}
// {(bf16)(x0 * t0), (bf16)(x1 * t1)} as one dword, as the row-tile NA epilogue rounds the product.
// In the fp16-operand build hipcc compiles that epilogue's (bf16)__fmul_rn(x, t) to one
// v_fma_mixlo_f16, whose fp16 result is not always the fp32 product's rounding (about one element
// in 4,000 differed from a v_pk_mul_f32 + v_cvt_pk_f16_f32 pair on Gaussian operands,
// tests/test_gpu_trans_aligned.py), and the vectoriser makes that pair of two adjacent products;
// so the instruction is spelled out here (lo then hi half of the dword; s_nop: the swap that reads
// the dword next needs two wait states after a VALU write, and hipcc does not look into the asm)
__device__ __forceinline__ unsigned mul_pack16(float x0, float t0, float x1, float t1) {
#ifdef ZV_OPERAND_F16
  unsigned w;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0\n\tv_fma_mixhi_f16 %0, %3, %4, 0\n\ts_nop 1"
      : "=&v"(w) : "v"(x0), "v"(t0), "v"(x1), "v"(t1));
  return w;
#else
  const bf16x2 h = {(bf16)__fmul_rn(x0, t0), (bf16)__fmul_rn(x1, t1)};
  return __builtin_bit_cast(unsigned, h);
#endif
}
// wh / wl [s]: the packed hi / lo dwords of the lane's four frames of strips i + s (i even);
// o: offset of the lane's 8-frame group in Cth / Ctl; nl: how many of its frames lie inside the
// utterance (<= 0: none)
template <int NS>
__device__ __forceinline__ void store_trans8(const GemmParams& p, const unsigned (&wh)[2][2],
                                             const unsigned (&wl)[2][2], long o, int nl, bool col_ok, int lane) {
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  u32x4_t uh, ul;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const auto sw = __builtin_amdgcn_permlane16_swap(wh[0][r], wh[1][r], false, false);
    uh[r] = sw[0];
    uh[2 + r] = sw[1];
    if constexpr (NS == 2) {
      const auto sl = __builtin_amdgcn_permlane16_swap(wl[0][r], wl[1][r], false, false);
      ul[r] = sl[0];
      ul[2 + r] = sl[1];
    }
  }
  const bool full = col_ok && nl >= 8;
  unsigned long long ha = full ? (unsigned long long)(p.Cth + o) : (unsigned long long)(p.sink + 512 + lane * 4);
  asm volatile("" : "+v"(ha));
  *(GLOBAL u32x4_t*)(ha) = uh;
  if constexpr (NS == 2) {
    unsigned long long la = full ? (unsigned long long)(p.Ctl + o) : (unsigned long long)(p.sink + 1024 + lane * 4);
    asm volatile("" : "+v"(la));
    *(GLOBAL u32x4_t*)(la) = ul;
  }
  if (col_ok && nl > 0 && nl < 8) {   // the group that straddles the utterance's end
    uint16_t* th = reinterpret_cast<uint16_t*>(p.Cth) + o;
    uint16_t* tl = NS == 2 ? reinterpret_cast<uint16_t*>(p.Ctl) + o : nullptr;
#pragma unroll
    for (int e = 0; e < 7; ++e)
      if (e < nl) {
        th[e] = (uint16_t)(uh[e >> 1] >> (16 * (e & 1)));
        if constexpr (NS == 2) tl[e] = (uint16_t)(ul[e >> 1] >> (16 * (e & 1)));
      }
  }
}

template <int TM, int TN, int NS, bool UTT = false>
__device__ __forceinline__ void gemm_epilogue_na_c(const GemmParams& p, f32x4 (&acc)[TM][TN],
                                                   int m0, int n0, int ub, int l0, int lane, float* scr) {
  constexpr int LDW = EpiScratch<TN>::LDW;
  static_assert(TN == 3, "one 48-column [s16 | x16 | y16] group per wave");
  const int nbc = min(n0, p.N - 48);
  const bool col_ok = n0 < p.N;
  const int cbase16 = (n0 / 48) * 16;
  // y (row-major): lane -> row lane >> 2 of the strip, channels c4 .. c4 + 3
  const int yrow = lane >> 2, c4 = (lane & 3) * 4;
  const f32x4 by = *reinterpret_cast<const f32x4*>(p.bias + nbc + 32 + c4);
  // x * tanh(s) (transposed): lane -> channel ch, rows 4 rg .. 4 rg + 3 of the strip
  const int ch = lane & 15, rg = lane >> 4;
  const float bs_ = p.bias[nbc + ch], bx = p.bias[nbc + 16 + ch];
  if constexpr (UTT) {
    static_assert(TM % 2 == 0, "aligned transposed stores pair the strips");
    static_assert(NS == 1, "the counted NA epilogue runs the 16-bit product only (launch_na_in)");
    // x * tanh(s) from the accumulators, 8 frames per lane (store_trans8)
    const long orow = (long)ub * p.sCt + (long)(cbase16 + ch) * p.ldct;
    static_for<TM / 2>([&](auto I_) {
      constexpr int i = 2 * decltype(I_)::value;
      unsigned wh[2][2], wl[2][2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float xv[4], tv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          tv[r] = tanh_fast(acc[i + s][0][r] + bs_);
          xv[r] = acc[i + s][1][r] + bx;
        }
        wh[s][0] = mul_pack16(xv[0], tv[0], xv[1], tv[1]);
        wh[s][1] = mul_pack16(xv[2], tv[2], xv[3], tv[3]);
      }
      const int l = l0 + i * 16 + utt_fofs(lane);
      store_trans8<NS>(p, wh, wl, orow + l, p.rpb - l, col_ok, lane);
    });
    // y keeps its staged form (only its 16 columns go through the strip); rows of the tile past
    // the utterance's end belong to the next utterance's tiles
    static_for<TM>([&](auto I_) {
      constexpr int i = decltype(I_)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[(rg * 4 + r) * LDW + 32 + ch] = acc[i][2][r];
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = scr[yrow * LDW + 32 + c4 + e] + by[e];
      bf16x4 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = (bf16)v[e];
      const bool ok = col_ok && l0 + i * 16 + yrow < p.rpb;
      const long o = (long)(m0 + i * 16 + yrow) * p.ldch + cbase16 + c4;
      unsigned long long ha = ok ? (unsigned long long)(p.Ch + o) : (unsigned long long)(p.sink + 512 + lane * 4);
      asm volatile("" : "+v"(ha));
      *(GLOBAL bf16x4*)(ha) = h;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
    });
    return;
  }
  // (utterance, frame) of the lane's first transposed row; strips advance it by 16
  int bb = (m0 + rg * 4) / p.rpb, lf = (m0 + rg * 4) % p.rpb;
  static_for<TM>([&](auto I_) {
    constexpr int i = decltype(I_)::value;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[((lane >> 4) * 4 + r) * LDW + j * 16 + (lane & 15)] = acc[i][j][r];
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    const int mrow0 = m0 + i * 16;
    {
      const int m = mrow0 + yrow;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = scr[yrow * LDW + 32 + c4 + e] + by[e];
      bf16x4 h, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h[e] = (bf16)v[e];
        l[e] = (bf16)(v[e] - (float)h[e]);
      }
      const bool ok = col_ok && m < p.M;
      const long o = (long)m * p.ldch + cbase16 + c4;
      unsigned long long ha = ok ? (unsigned long long)(p.Ch + o) : (unsigned long long)(p.sink + 512 + lane * 4);
      asm volatile("" : "+v"(ha));
      *(GLOBAL bf16x4*)(ha) = h;
      if constexpr (NS == 2) {
        unsigned long long la = ok ? (unsigned long long)(p.Cl + o) : (unsigned long long)(p.sink + 1024 + lane * 4);
        asm volatile("" : "+v"(la));
        *(GLOBAL bf16x4*)(la) = l;
      }
    }
    int b2 = bb, l2 = lf;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = rg * 4 + e, m = mrow0 + row;
      const float sv = scr[row * LDW + ch] + bs_;
      const float xv = scr[row * LDW + 16 + ch] + bx;
      const float v = __fmul_rn(xv, tanh_fast(sv));   // not contracted into the lo half
      const bf16 h = (bf16)v;
      const bool ok = col_ok && m < p.M;
      const long o = b2 * p.sCt + (long)(cbase16 + ch) * p.ldct + l2;
      unsigned long long ha = ok ? (unsigned long long)(p.Cth + o) : (unsigned long long)(p.sink + 2048 + lane);
      asm volatile("" : "+v"(ha));
      *(GLOBAL bf16*)(ha) = h;
      if constexpr (NS == 2) {
        unsigned long long la = ok ? (unsigned long long)(p.Ctl + o) : (unsigned long long)(p.sink + 2560 + lane);
        asm volatile("" : "+v"(la));
        *(GLOBAL bf16*)(la) = (bf16)(v - (float)h);
      }
      if (e < 3) adv_pos(b2, l2, 1, p.rpb);
    }
    adv_pos(bb, lf, 16, p.rpb);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
  });
}

template <int TM, int TN, int NS, bool UTT = false>
__device__ __forceinline__ void gemm_epilogue_trans_c(const GemmParams& p, f32x4 (&acc)[TM][TN],
                                                      int m0, int n0, int ub, int l0, int lane, float* scr) {
  constexpr int WN = EpiScratch<TN>::W, LDW = EpiScratch<TN>::LDW;
  constexpr int Q = (16 * WN) / (64 * 4);
  if constexpr (UTT) {
    static_assert(TM % 2 == 0, "aligned transposed stores pair the strips");
    // from the accumulators, 8 frames of one output row per lane and store (store_trans8)
    const int lf = l0 + utt_fofs(lane);
    static_for<TN>([&](auto J_) {
      constexpr int j = decltype(J_)::value;
      const int n = n0 + j * 16 + (lane & 15);
      const bool col_ok = n < p.N;
      const float bn = p.bias ? p.bias[min(n, p.N - 1)] : 0.f;
      const long orow = (long)ub * p.sCt + (long)n * p.ldct;
      static_for<TM / 2>([&](auto I_) {
        constexpr int i = 2 * decltype(I_)::value;
        unsigned wh[2][2], wl[2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = acc[i + s][j][r] + bn;
          pack_trans4<NS>(v, wh[s], wl[s]);
        }
        const int l = lf + i * 16;
        store_trans8<NS>(p, wh, wl, orow + l, p.rpb - l, col_ok, lane);
      });
    });
    return;
  }
  static_assert(64 % WN == 0 && Q >= 1, "a lane's column is fixed across strips");
  const int col = lane % WN, rg0 = lane / WN;     // q adds 64 / WN row groups
  const int n = n0 + col;
  const bool col_ok = n < p.N;
  const float bn = p.bias ? p.bias[min(n, p.N - 1)] : 0.f;
  int bb[Q], lf[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int m = m0 + (rg0 + q * (64 / WN)) * 4;
    bb[q] = m / p.rpb;
    lf[q] = m % p.rpb;
  }
  static_for<TM>([&](auto I_) {
    constexpr int i = decltype(I_)::value;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[((lane >> 4) * 4 + r) * LDW + j * 16 + (lane & 15)] = acc[i][j][r];
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    const int mrow0 = m0 + i * 16;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int rg = rg0 + q * (64 / WN);
      int b2 = bb[q], l2 = lf[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = mrow0 + rg * 4 + e;
        const float v = scr[(rg * 4 + e) * LDW + col] + bn;
        const bf16 h = (bf16)v;
        const bool ok = col_ok && m < p.M;
        const long o = b2 * p.sCt + (long)n * p.ldct + l2;
        unsigned long long ha = ok ? (unsigned long long)(p.Cth + o) : (unsigned long long)(p.sink + 2048 + lane);
        asm volatile("" : "+v"(ha));
        *(GLOBAL bf16*)(ha) = h;
        if constexpr (NS == 2) {
          unsigned long long la = ok ? (unsigned long long)(p.Ctl + o) : (unsigned long long)(p.sink + 2560 + lane);
          asm volatile("" : "+v"(la));
          *(GLOBAL bf16*)(la) = (bf16)(v - (float)h);
        }
        if (e < 3) adv_pos(b2, l2, 1, p.rpb);
      }
      adv_pos(bb[q], lf[q], 16, p.rpb);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
  });
}

// Persistent kernel: gridDim.x = G blocks (multiple of 8) walk the tile grid; the
// K-step pipeline runs continuously across tile boundaries (the next tile's
// first stages load under the current tile's last MFMAs and epilogue).  Tile
// order: iteration `it` gives the blocks of XCD x (blockIdx % 8 == x under the
// observed round-robin dispatch) a contiguous run of G/8 tiles, n fastest, so
// concurrently running tiles on one XCD share A row panels and the weight panel
// in its L2 (speed only; any placement is correct).
// OCC = waves per SIMD the register allocation must allow: 2 (two 4-wave blocks
// per CU: one block's HBM-bound epilogue overlaps the other's MFMA loop — the
// residual-stream linears) or 1 (one block per CU with up to 512 registers per
// lane: measured faster for the compute-heavy non-residual linears).
// ROLE: 1 = a residual-stream linear (fp32 residual read-modify-write epilogue; HBM-bound
// below the ridge point), 2 = the same with the bypass original (FF2), 3 = a plain linear
// (bias, activation, bf16 copy) on the counted epilogue, 4 = ROLE 1 plus a row-group vector
// (the K-concatenated conv + SelfAttention out-projection), 0 = everything else.
// The residual roles run the counted epilogue (gemm_epilogue_res) and have their own
// symbols, so rocprofv3 kernel stats and PMC passes attribute the two rooflines separately.
#ifndef ZV_GEMM_PRELOAD
#define ZV_GEMM_PRELOAD 1
#endif
template <int BM, int BN, int WGM, int WGN, int SPLIT, int EPI, int STAGES = 2, int OCC = 2,
          int BK = GEMM_BK, int RP = 0, int CONV = 0, int ROLE = 0,
          int PRELOAD = ZV_GEMM_PRELOAD, int MXO = 0, int UTT = 0>
__global__ __launch_bounds__(64 * WGM * WGN, OCC) void zv_gemm_kernel(GemmParams p) {
  constexpr int NW = WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int TM = WM / 16, TN = WN / 16;
  constexpr int NS = (SPLIT == 3) ? 2 : 1;        // output hi/lo (the split mode's copies)
  // SPLIT = 2 (weight-split product a.b ~= ah.bh + ah.bl: a 16-bit activation against the
  // weight's hi/lo pair; the mixed mode's attention-score projection): A single, B hi/lo
  constexpr int NSA = (SPLIT == 3) ? 2 : 1, NSB = (SPLIT == 3 || SPLIT == 2) ? 2 : 1;
  // SPLIT = 8: MX-fp8 operands (1 B per element + a scale byte per 32): a 128-deep K step is
  // the same 128-B staged row as a 64-deep bf16 step, plus 4 scale bytes per row
  constexpr bool MX = SPLIT == 8;
  constexpr int EB = MX ? 1 : 2;                                // bytes per operand element
  static_assert(MX ? (BK == MX8_KSTEP && STAGES == 2 && !CONV && !RP)
                   : (BK == 64 || BK == 32), "K step depth");
  static_assert(MXO == 0 || (ROLE >= 1 && EPI == EPI_STD), "fp8 copy out: counted STD epilogues");
  constexpr int RB = BK * EB, CPRW = RB / 16, RPP = 1024 / RB;  // row bytes, chunks/row, rows/piece
  constexpr int A_BYTES = BM * BK * EB, B_BYTES = BN * BK * EB;
  constexpr int SA_P = MX ? (BM + 63) / 64 : 0, SB_P = MX ? (BN + 63) / 64 : 0;   // scale pieces
  constexpr int SC_OFF = NS * (A_BYTES + B_BYTES);              // scale rows within a stage
  static_assert((SA_P + SB_P) % NW == 0, "MX scale pieces: the same count per wave");
  constexpr int STAGE = gemm_stage_bytes<BM, BN, SPLIT, BK>();
  // unpadded swizzled epilogue strips when the padded ones do not fit a (BK = 32) stage
  constexpr bool SWZ = BK == 32 && NW * EpiScratch<TN>::BYTES > STAGE;
  constexpr int A_PIECES = A_BYTES / 1024, B_PIECES = B_BYTES / 1024;
  constexpr int PER_WAVE = NSA * ((A_PIECES + NW - 1) / NW) + NSB * ((B_PIECES + NW - 1) / NW) + (SA_P + SB_P) / NW;
  static_assert(STAGES == 2 || (A_PIECES % NW == 0 && B_PIECES % NW == 0),
                "multi-stage pipeline needs pieces divisible by the wave count");
  static_assert(BM % 8 == 0 && BN % 8 == 0 && WM % 16 == 0 && WN % 16 == 0, "tile");
  constexpr int SCR = SWZ ? 16 * 16 * TN * 4 : EpiScratch<TN>::BYTES;
  static_assert(NW * SCR <= STAGE, "epilogue scratch must fit one ring stage");
  // 16-B chunk swizzle of a staged row (applied on the DMA source and on the read):
  // conflict-free ds_read_b128 fragment reads for both row widths
  auto swz = [](int row) -> int { return RB == 128 ? (row & 7) : ((120 >> (2 * ((row >> 2) & 3))) & 3); };

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave / WGN) * WM, wn0 = (wave % WGN) * WN;
  static_assert(!UTT || (ROLE == 3 && (EPI == EPI_NA || EPI == EPI_TRANS) && !SWZ),
                "utterance-aligned tiles: the counted NA / transposed epilogues");
  // UTT: utterance-aligned M tiles.  M tile tm covers rows b * rpb + j * BM .. of utterance
  // b = tm / tpu, j = tm % tpu (tpu = cdiv(rpb, BM) tiles per utterance): no tile crosses an
  // utterance and a tile's first frame is a multiple of BM; the rows of an utterance's last tile
  // past its end are loaded (clamped to M - 1 as everywhere) and never stored
  const int tpu = UTT ? (p.rpb + BM - 1) / BM : 1;
  const int ntn = (p.N + BN - 1) / BN, ntm = UTT ? (p.M / p.rpb) * tpu : (p.M + BM - 1) / BM;
  const int ntiles = ntn * ntm;
  // a tile's first row and column (UTT: and its utterance, and the first row's frame in it)
  auto tile_origin = [&](int tile, int& m0, int& n0, int& ub, int& l0) {
    const int tm = tile / ntn;
    n0 = (tile - tm * ntn) * BN;
    if constexpr (UTT) {
      ub = tm / tpu;
      l0 = (tm - ub * tpu) * BM;
      m0 = ub * p.rpb + l0;
    } else {
      ub = 0; l0 = 0;
      m0 = tm * BM;
    }
  };
  const int G = gridDim.x, Q = G >> 3;
  const int bslot = (blockIdx.x & 7) * Q + (blockIdx.x >> 3);
  const int my_tiles = (bslot < ntiles) ? (ntiles - 1 - bslot) / G + 1 : 0;
  const int z1 = blockIdx.z / p.nz2, z2 = blockIdx.z % p.nz2;
  const long aoff = z1 * p.sA1 + z2 * p.sA2, boff = z1 * p.sB1 + z2 * p.sB2;
  const bf16* Ah = p.Ah + aoff;
  const bf16* Al = (SPLIT == 3) ? p.Al + aoff : nullptr;
  const bf16* Bh = p.Bh + boff;
  const bf16* Bl = (NSB == 2) ? p.Bl + boff : nullptr;
  const int nk = (p.K + BK - 1) / BK;
  const int total = my_tiles * nk;

  // producer state (the step whose tiles are loaded next)
  int ld_step = 0, ld_it = 0, ld_kt = 0;
  // per-lane byte offsets of this wave's DMA pieces within the current tile (row and
  // swizzled 16-B chunk: fixed for the tile; the K step moves only the scalar base)
  constexpr int APW = (A_PIECES + NW - 1) / NW, BPW = (B_PIECES + NW - 1) / NW;
  constexpr int SPW = MX ? (SA_P + SB_P) / NW : 1;
  unsigned offa[APW], offb[BPW], offs[SPW];
  const int prow = lane / CPRW, ppos = lane % CPRW;
  auto set_ld_tile = [&]() {
    int ld_m0, ld_n0, ld_ub, ld_l0;
    tile_origin(ld_it * G + bslot, ld_m0, ld_n0, ld_ub, ld_l0);
#pragma unroll
    for (int i = 0; i < APW; ++i) {
      const int row = (wave + i * NW) * RPP + prow;
      const int gm = min(ld_m0 + row, p.M - 1);
      offa[i] = (unsigned)((long)gm * p.lda * EB + (ppos ^ swz(row)) * 16);
    }
#pragma unroll
    for (int i = 0; i < BPW; ++i) {
      const int row = (wave + i * NW) * RPP + prow;
      const int gn = min(ld_n0 + row, p.Brows - 1);
      offb[i] = (unsigned)((long)gn * p.ldb * EB + (ppos ^ swz(row)) * 16);
    }
    if constexpr (MX) {
#pragma unroll
      for (int i = 0; i < SPW; ++i) {     // scale piece sp: 64 rows, one lane per row
        const int sp = wave + i * NW;
        offs[i] = sp < SA_P ? (unsigned)((long)min(ld_m0 + sp * 64 + lane, p.M - 1) * p.ldas)
                            : (unsigned)((long)min(ld_n0 + (sp - SA_P) * 64 + lane, p.Brows - 1) * p.ldbs);
      }
    }
  };
  auto issue_to = [&](unsigned char* base) {   // load step ld_step into `base`, then advance
    const int k0 = ld_kt * BK;
    long ak0 = k0;
    if constexpr (CONV) {
      const int tap = k0 / p.conv_c;
      ak0 = (long)(tap * p.conv_d - p.conv_pad) * p.lda + (k0 - tap * p.conv_c);
    }
    const unsigned char* ah = reinterpret_cast<const unsigned char*>(Ah) + ak0 * EB;
    const bf16* al = (SPLIT == 3) ? Al + ak0 : nullptr;
    const unsigned char* bh = reinterpret_cast<const unsigned char*>(Bh) + (long)k0 * EB;
    const bf16* bl = (NSB == 2) ? Bl + k0 : nullptr;
    if constexpr (MX) {
#pragma unroll
      for (int i = 0; i < SPW; ++i) {
        const int sp = wave + i * NW;
        const uint8_t* sb = sp < SA_P ? p.As + ld_kt * (BK / MX8_BLOCK) : p.Bs + ld_kt * (BK / MX8_BLOCK);
        glds4s(sb, offs[i], base + SC_OFF + sp * 256);
      }
    }
#pragma unroll
    for (int i = 0; i < APW; ++i) {
      const int pc = wave + i * NW;
      if (A_PIECES % NW == 0 || pc < A_PIECES) {
        glds16s(ah, offa[i], base + pc * 1024);
        if constexpr (SPLIT == 3)
          glds16s(al, offa[i], base + A_BYTES + pc * 1024);
      }
    }
#pragma unroll
    for (int i = 0; i < BPW; ++i) {
      const int pc = wave + i * NW;
      if (B_PIECES % NW == 0 || pc < B_PIECES) {
        glds16s(bh, offb[i], base + NSA * A_BYTES + pc * 1024);
        if constexpr (NSB == 2)
          glds16s(bl, offb[i], base + NSA * A_BYTES + B_BYTES + pc * 1024);
      }
    }
    ++ld_step;
    if (++ld_kt == nk) {
      ld_kt = 0;
      ++ld_it;
      if (ld_it < my_tiles) set_ld_tile();
    }
  };
  auto issue = [&]() { issue_to(smem + (ld_step % STAGES) * STAGE); };

  if (total > 0) set_ld_tile();
#pragma unroll
  for (int st = 0; st < STAGES - 1; ++st)
    if (ld_step < total) issue();

  auto mma_step = [&](const unsigned char* base, f32x4 (&acc)[TM][TN]) {
    if constexpr (MX) {
      // one block-scaled MFMA per 16x16 sub-tile and K step.  Lane l (c = l >> 4) holds the
      // 16-B chunks c and c + 4 of its 128-B row (the bf16 kernel's chunks of two K steps)
      // and supplies the scale byte of K block c = [32 c, 32 c + 32) of the row: the
      // hardware pairs scale blocks with K positions itself (tools/probe/mx8_probe*.hip)
      typedef int i32x8 __attribute__((ext_vector_type(8)));
      typedef int i32x4 __attribute__((ext_vector_type(4)));
      const int c = lane >> 4;
      i32x8 fa[TM], fb[TN];
      int sa[TM], sb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm0 + i * 16 + (lane & 15);
        const i32x4 x0 = *reinterpret_cast<const i32x4*>(base + r * RB + ((c ^ swz(r)) << 4));
        const i32x4 x1 = *reinterpret_cast<const i32x4*>(base + r * RB + (((c + 4) ^ swz(r)) << 4));
        fa[i] = i32x8{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        sa[i] = base[SC_OFF + r * 4 + c];
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int r = wn0 + j * 16 + (lane & 15);
        const unsigned char* bb = base + A_BYTES;
        const i32x4 x0 = *reinterpret_cast<const i32x4*>(bb + r * RB + ((c ^ swz(r)) << 4));
        const i32x4 x1 = *reinterpret_cast<const i32x4*>(bb + r * RB + (((c + 4) ^ swz(r)) << 4));
        fb[j] = i32x8{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        sb[j] = base[SC_OFF + SA_P * 256 + r * 4 + c];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 0,
                                                                       sa[i], 0, sb[j]);
      return;
    }
    if constexpr (SPLIT == 1 && PRELOAD) {
      // every fragment of the K step read up front into its own registers, then the
      // MFMAs: the second k-half's LDS reads fly under the first half's MFMAs instead
      // of the compiler's read -> wait -> MFMA chains on reused registers
      constexpr int KK = BK / 32;
      bf16x8 fa[KK][TM], fb[KK][TN];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int r = wm0 + i * 16 + (lane & 15);
          fa[kk][i] = *reinterpret_cast<const bf16x8*>(base + r * RB + ((chunk ^ swz(r)) << 4));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int r = wn0 + j * 16 + (lane & 15);
          fb[kk][j] = *reinterpret_cast<const bf16x8*>(base + NSA * A_BYTES + r * RB +
                                                        ((chunk ^ swz(r)) << 4));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = ZV_MFMA_16x16x32(fa[kk][i], fb[kk][j], acc[i][j], 0, 0, 0);
      return;
    }
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      const int chunk = kk * 4 + (lane >> 4);
      bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm0 + i * 16 + (lane & 15);
        const int o = r * RB + ((chunk ^ swz(r)) << 4);
        ah[i] = *reinterpret_cast<const bf16x8*>(base + o);
        if constexpr (SPLIT == 3) al[i] = *reinterpret_cast<const bf16x8*>(base + A_BYTES + o);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int r = wn0 + j * 16 + (lane & 15);
        const int o = NSA * A_BYTES + r * RB + ((chunk ^ swz(r)) << 4);
        bh[j] = *reinterpret_cast<const bf16x8*>(base + o);
        if constexpr (NSB == 2) bl[j] = *reinterpret_cast<const bf16x8*>(base + B_BYTES + o);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (SPLIT == 3) {
            acc[i][j] = ZV_MFMA_16x16x32(al[i], bh[j], acc[i][j], 0, 0, 0);
            acc[i][j] = ZV_MFMA_16x16x32(ah[i], bl[j], acc[i][j], 0, 0, 0);
          } else if constexpr (SPLIT == 2) {
            acc[i][j] = ZV_MFMA_16x16x32(ah[i], bl[j], acc[i][j], 0, 0, 0);
          }
          acc[i][j] = ZV_MFMA_16x16x32(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
  };

  int step = 0;
  for (int it = 0; it < my_tiles; ++it) {
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt, ++step) {
      {
        const int ahead = min(STAGES - 2, total - 1 - step);   // stages issued after this one
        if (ahead <= 0) wait_vmcnt<0>();
        else if (ahead == 1) wait_vmcnt<PER_WAVE>();
        else if (ahead == 2) wait_vmcnt<2 * PER_WAVE>();
        else wait_vmcnt<3 * PER_WAVE>();
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (ld_step < total) issue();
      mma_step(smem + (step % STAGES) * STAGE, acc);
    }
    int m0, n0, ub, l0;
    tile_origin(it * G + bslot, m0, n0, ub, l0);
    __builtin_amdgcn_s_barrier();          // every wave done reading the last stage
    float* scr = reinterpret_cast<float*>(smem + ((step - 1) % STAGES) * STAGE + wave * SCR);
    if constexpr (ROLE >= 1 && EPI == EPI_STD && !RP && !SWZ)
      gemm_epilogue_res<TM, TN, NS, ROLE == 2, ROLE != 3, MXO, ROLE == 4 || ROLE == 5, ROLE == 5>(
          p, acc, m0 + wm0, n0 + wn0, lane, scr);
    else if constexpr (ROLE == 3 && EPI == EPI_GLU && !SWZ)
      gemm_epilogue_glu_c<TM, TN, NS>(p, acc, m0 + wm0, n0 + wn0, lane, scr);
    else if constexpr (ROLE == 3 && EPI == EPI_NA && !SWZ)
      gemm_epilogue_na_c<TM, TN, NS, UTT != 0>(p, acc, m0 + wm0, n0 + wn0, ub, l0 + wm0, lane, scr);
    else if constexpr (ROLE == 3 && EPI == EPI_TRANS && !SWZ)
      gemm_epilogue_trans_c<TM, TN, NS, UTT != 0>(p, acc, m0 + wm0, n0 + wn0, ub, l0 + wm0, lane, scr);
    else
      gemm_epilogue<TM, TN, EPI, SWZ, RP>(p, acc, m0 + wm0, n0 + wn0, z1, z2, lane, scr);
    // drain the epilogue's own loads/stores with a wait hipcc can see, so its
    // waitcnt pass carries no pending VMEM into the next tile's k-loop (it would
    // otherwise re-wait vmcnt(0) inside every k-step, stalling on the DMA ring)
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  }
}

// per-device process-lifetime buffers (an engine on another GPU of the same process gets
// its own): the counted epilogues' sink (stores outside the output land here, 64 KiB) and a
// zeroed 256-B buffer (the GLU row mask when there is none, the zero row of LDS-DMA halos)
constexpr int ZV_MAX_DEVICES = 64;
static int zv_cur_device() {
  int dev = 0;
  ZV_CHECK(hipGetDevice(&dev));
  ZV_REQUIRE(dev >= 0 && dev < ZV_MAX_DEVICES, "device ordinal out of range");
  return dev;
}
static float* zv_epi_sink() {
  static float* sink[ZV_MAX_DEVICES] = {};
  const int d = zv_cur_device();
  if (!sink[d]) ZV_CHECK(ZV_BLOCKING(hipMalloc(&sink[d], 64 * 1024)));
  return sink[d];
}
// The process's device error word: host memory mapped into every device's address space, so a
// kernel that hits a condition it cannot recover from inside the launch sets a bit and finishes
// (no trap: a trap aborts the process with nothing on the host side), and the host reads the word
// without synchronising (zv_engine's check_ready).  Bit 0: the fused FeedForward's C item outwaited
// its producer (zv_ffn.inc)
static volatile unsigned* zv_dev_err_host() {
  static unsigned* const h = [] {
    unsigned* w = nullptr;
    ZV_CHECK(ZV_BLOCKING(hipHostMalloc((void**)&w, 64, hipHostMallocMapped | hipHostMallocPortable)));
    w[0] = 0;
    return w;
  }();
  return h;
}
static unsigned* zv_dev_err_word() {
  static unsigned* const d = [] {
    unsigned* w = nullptr;
    ZV_CHECK(ZV_BLOCKING(hipHostGetDevicePointer((void**)&w, (void*)zv_dev_err_host(), 0)));
    return w;
  }();
  return d;
}

static void* zv_epi_zero() {
  static void* z[ZV_MAX_DEVICES] = {};
  const int d = zv_cur_device();
  if (!z[d]) {
    ZV_CHECK(ZV_BLOCKING(hipMalloc(&z[d], 256)));
    ZV_CHECK(ZV_BLOCKING(hipMemset(z[d], 0, 256)));
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  }
  return z[d];
}

static int zv_num_cus() {
  static int n[ZV_MAX_DEVICES] = {};
  const int d = zv_cur_device();
  if (!n[d]) {
    ZV_CHECK(hipDeviceGetAttribute(&n[d], hipDeviceAttributeMultiprocessorCount, d));
    if (n[d] <= 0) n[d] = 256;
  }
  return n[d];
}

// the counted epilogues' preconditions and operands (sink, zero row mask), shared by the
// 128x128 and 256x256 launchers
template <int SPLIT, int EPI, int ROLE, int MXO, int RP>
static GemmParams gemm_prep_epilogue(const GemmParams& p, int nz) {
  GemmParams pr = p;
  if constexpr (ROLE == 3 && EPI == EPI_GLU) {
    ZV_REQUIRE(p.bias && p.Ch && p.N % 32 == 0 && p.ldch % 8 == 0 && nz == 1 && p.nz2 == 1 &&
                   (p.Cl != nullptr) == (SPLIT == 3),
               "counted GLU epilogue: bias, bf16 copy, N % 32 == 0");
    pr.sink = zv_epi_sink();
    pr.rowmask_step = p.rowmask ? 1 : 0;
    if (!p.rowmask) pr.rowmask = reinterpret_cast<const uint8_t*>(zv_epi_zero());
  } else if constexpr (ROLE == 3 && (EPI == EPI_NA || EPI == EPI_TRANS)) {
    ZV_REQUIRE((EPI == EPI_TRANS || (p.bias && p.Ch && p.N % 48 == 0 && p.ldch % 4 == 0)) &&
                   p.Cth && p.rpb > 0 && nz == 1 && p.nz2 == 1 &&
                   (p.Ctl != nullptr) == (SPLIT == 3) && (EPI == EPI_TRANS || (p.Cl != nullptr) == (SPLIT == 3)),
               "counted NA / transposed epilogue: bias, outputs present, N % 48 == 0");
    pr.sink = zv_epi_sink();
  } else if constexpr (ROLE == 3 && EPI == EPI_STD && !RP) {
    ZV_REQUIRE(p.bias && (p.Ch || MXO == 2) && !p.C && !p.resid && !p.orig && !p.rowvec && !p.mulh &&
                   !p.colscale && p.N % 8 == 0 && p.ldch % 8 == 0 && nz == 1 && p.nz2 == 1 &&
                   (p.Cl != nullptr) == (SPLIT == 3),
               "counted plain GEMM epilogue: bias (+ activation) -> bf16 copy, N % 8 == 0");
    pr.sink = zv_epi_sink();
    if (MXO == 2) { pr.Ch = reinterpret_cast<bf16*>(pr.sink + 4096); pr.ldch = 0; }   // not written
  } else if constexpr (ROLE >= 1 && EPI == EPI_STD && !RP) {
    ZV_REQUIRE(p.resid && (ROLE == 5) == (p.C == nullptr) && (ROLE != 5 || p.Ch) && p.bias &&
                   (ROLE == 4 || ROLE == 5) == (p.rowvec != nullptr) && p.rows_per_group > 0 &&
                   !p.act && !p.mulh && !p.colscale &&
                   (ROLE == 2) == (p.orig != nullptr) && (ROLE != 2 || p.byp) && p.N % 8 == 0 &&
                   p.ldc % 4 == 0 && nz == 1 && p.nz2 == 1 && (!p.Ch || p.ldch % 8 == 0) &&
                   (p.Cl != nullptr) == (SPLIT == 3 && p.Ch != nullptr),
               "residual GEMM epilogue: bias + residual + fp32 out (+ copy, + bypass), N % 8 == 0");
    pr.sink = zv_epi_sink();
    if (!pr.Ch) { pr.Ch = reinterpret_cast<bf16*>(pr.sink + 4096); pr.ldch = 0; }   // no copy
    if (SPLIT == 3 && !pr.Cl) { pr.Cl = reinterpret_cast<bf16*>(pr.sink + 8192); pr.ldch = 0; }
  }
  return pr;
}

// algorithmic HBM bytes, recorded for the residual-stream linears (their roofline is HBM):
// A and W once (bf16, x2 for hi/lo), per output element the fp32 residual read, the fp32
// write, the bf16 copy (hi[/lo]) and the fp32 bypass original when present
template <int SPLIT, int ROLE, int MXO>
static double gemm_alg_bytes(const GemmParams& p, int nz) {
  if constexpr (ROLE == 1 || ROLE == 2 || ROLE == 4 || ROLE == 5) {
    constexpr int NA = (SPLIT == 3) ? 2 : 1, NB = (SPLIT == 3 || SPLIT == 2) ? 2 : 1;
    constexpr bool MX = SPLIT == 8;
    const double mn = (double)p.M * p.N * nz;
    return (MX ? (1.0 + 1.0 / MX8_BLOCK) * ((double)p.M * p.K + (double)p.N * p.K)
               : 2.0 * (NA * (double)p.M * p.K + NB * (double)p.N * p.K)) * nz +
           mn * (4.0 * (p.resid != nullptr) + 4.0 * (p.C != nullptr) + 4.0 * (p.orig != nullptr) +
                 2.0 * (p.Ch != nullptr && MXO != 2) + 2.0 * (p.Cl != nullptr) +
                 (MXO ? 1.0 + 1.0 / MX8_BLOCK : 0.0));
  }
  return 0.0;
}

// Host-only record of the calling thread's last GEMM / fused FeedForward launch (test
// infrastructure: zv_linear_check / zv_ffn_check return it, so a test can tell which instantiation
// the engine's dispatch chose for a shape).  Written by launch_gemm, launch_gemm256 and
// launch_ffn_t; no kernel reads it.  ffn: EPI = RV | ORIG << 1 | COPY << 2 | TP << 3, ROLE = NORM,
// aux = chunk steps per block (w); GEMMs: aux = STAGES * 16 + OCC (+ 256: utterance-aligned tiles; 0 for
// the 256x256 kernel)
struct ZvLaunchRec { int BM, BN, SPLIT, EPI, ROLE, k256, grid, aux; };
static thread_local ZvLaunchRec g_zv_last_launch = {};

// The utterance-aligned tiling's (UTT) preconditions: whole utterances of rpb rows, and rows of
// the transposed output that start 16-B aligned at every multiple of 8 frames
static bool gemm_utt_ok(const GemmParams& p) {
  return p.rpb > 0 && p.M % p.rpb == 0 && p.ldct >= p.rpb && p.ldct % 8 == 0 && p.sCt % 8 == 0 && p.Cth &&
         (uintptr_t)p.Cth % 16 == 0 && (uintptr_t)p.Ctl % 16 == 0;
}

template <int BM, int BN, int WGM, int WGN, int SPLIT, int EPI, int STAGES = 2, int OCC = 2,
          int BK = GEMM_BK, int RP = 0, int CONV = 0, int ROLE = 0, int MXO = 0, int UTT = 0>
static void launch_gemm(const GemmParams& p, int nz, hipStream_t s, const char* tag,
                        bool persistent = true, int gridx = 0) {
  constexpr int NS = (SPLIT == 3) ? 2 : 1;
  constexpr bool MX = SPLIT == 8;
  constexpr size_t lds = (size_t)STAGES * gemm_stage_bytes<BM, BN, SPLIT, BK>();
  static_assert(lds <= 160 * 1024, "LDS budget");
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute(
        (const void*)zv_gemm_kernel<BM, BN, WGM, WGN, SPLIT, EPI, STAGES, OCC, BK, RP, CONV, ROLE, ZV_GEMM_PRELOAD, MXO, UTT>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr |= 1ull << zv_cur_device();
  }
  ZV_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "empty GEMM");
  if constexpr (MX)
    ZV_REQUIRE(p.As && p.Bs && p.K % MX8_KSTEP == 0 && p.lda % 16 == 0 && p.ldb % 16 == 0 &&
                   p.ldas * MX8_BLOCK >= p.K && p.ldbs * MX8_BLOCK >= p.K && nz == 1 && p.nz2 == 1,
               "MX-fp8 GEMM: scales present, K a multiple of 128, 16-B aligned rows");
  if constexpr (MXO > 0)
    ZV_REQUIRE(p.Cq && p.Cs && p.ldcq % MX8_KSTEP == 0 && p.N <= p.ldcq,
               "fp8 output copy: values and scales, row stride a multiple of 128");
  if constexpr (RP > 0)
    ZV_REQUIRE(p.residh && p.residl && p.Ch && p.Cl && !p.C && !p.resid && !p.orig && p.N % 8 == 0 &&
                   p.ldch % 8 == 0 && EPI == EPI_STD,
               "pair-residual GEMM: hi/lo residual in and out, N and ld multiples of 8");
  GemmParams pr = gemm_prep_epilogue<SPLIT, EPI, ROLE, MXO, RP>(p, nz);
  if constexpr (CONV)
    ZV_REQUIRE(p.conv_c > 0 && p.conv_c % BK == 0 && p.K % p.conv_c == 0 && p.lda == p.conv_c &&
                   p.conv_pad >= 0 && p.conv_d > 0 && p.nz2 == 1,
               "implicit-conv GEMM: channels a multiple of the K step, K = taps * channels");
  // the DMA pieces address A / B as a scalar base + 32-bit per-lane byte offset
  ZV_REQUIRE((long)p.M * p.lda * (MX ? 1 : 2) < (1L << 32) && (long)p.Brows * p.ldb * (MX ? 1 : 2) < (1L << 32),
             "GEMM operand larger than the 4 GiB DMA offset range");
  if constexpr (UTT)
    ZV_REQUIRE(gemm_utt_ok(p), "utterance-aligned tiles: whole utterances, 16-B aligned V^T rows");
  const int tiles = cdiv(p.N, BN) * (UTT ? (p.M / p.rpb) * cdiv(p.rpb, BM) : cdiv(p.M, BM));
  // persistent grid: blocks resident per CU by LDS (and at most 2), across all z
  constexpr int NWB = WGM * WGN;
  const int bpc = std::max(1, std::min({2, (int)((160 * 1024) / lds), std::max(1, OCC * 4 / NWB)}));
  static_assert(lds <= 160 * 1024, "LDS budget (ring + epilogue scratch)");
  // gridx > 0: gridx blocks per CU regardless of residency (the blocks beyond the
  // resident ones start as earlier blocks drain: dynamic balance); < 0: one tile per block
  if (gridx < 0) persistent = false;
  int G = (zv_num_cus() * (gridx > 0 ? gridx : bpc) + nz - 1) / nz;
  G = persistent ? std::min(G, tiles) : tiles;   // non-persistent: one tile per block
  G = std::max(8, (G + 7) / 8 * 8);
  char dtag[160];
  if (g_zv_prof.detail) {
    snprintf(dtag, sizeof(dtag), "%s M=%d N=%d K=%d z=%d tile=%dx%d", tag, p.M, p.N, p.K, nz, BM, BN);
    tag = dtag;
  }
  g_zv_last_launch = ZvLaunchRec{BM, BN, SPLIT, EPI, ROLE, 0, G, STAGES * 16 + OCC + 256 * UTT};
  const double bytes = gemm_alg_bytes<SPLIT, ROLE, MXO>(p, nz);
  ZvProfScope prof(tag, 2.0 * p.M * p.N * (double)p.K * nz, bytes, s);
  hipLaunchKernelGGL((zv_gemm_kernel<BM, BN, WGM, WGN, SPLIT, EPI, STAGES, OCC, BK, RP, CONV, ROLE, ZV_GEMM_PRELOAD, MXO, UTT>), dim3(G, 1, nz),
                     dim3(64 * WGM * WGN), lds, s, pr);
  ZV_LAUNCH_CHECK();
}
