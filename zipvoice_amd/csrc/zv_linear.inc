// The linears' launch policy: which GEMM instantiation (tile, K-ring depth, blocks per CU,
// epilogue) a linear of the Zipformer runs on.  LinearPolicy holds the three run-time knobs the
// choice reads; zv_engine derives from it, and zv_linear_check (test infrastructure) constructs it
// alone.  tests/test_gpu_linear_ref.py predict() mirrors linear16 / attn_in_wsplit arm for arm.
//
// Everywhere: two 4-wave blocks per CU unless an arm says otherwise, and one tile per block (with
// the decoder split over streams, dynamically dispatched tiles fill the CUs another stream's
// kernel leaves idle).
//
// Measured and retired (the arms and their A/B knobs are gone; the records stay in profiles/):
//  - one block per CU (OCC 1) for the plain / residual / fused-epilogue linears: one guided C2
//    forward 41.0-41.1 ms against 38.0-38.3 ms at two, the NonlinAttention in-projection 330 against
//    229 us (r01_gemm_policy_ab.txt)
//  - the persistent resident grid (gridx 0 / n blocks per CU) instead of one tile per block:
//    2.6 % slower per C2 step under the split decoder, 527.4 against 512.6 ms
//    (r02_launch_policy_ab.txt)
//  - the attention-score projection (N = 272) on 128x96 general-epilogue tiles (N96 mode 0) and on
//    128x64 counted tiles at two blocks per CU (mode 1): 12.9 / 10.1 ms per step against 9.1 ms for
//    counted 128x128 (r02_n96_counted_ab.txt); 16-bit mode since on 128x64 at three blocks per CU
//    (below)
//  - deferred epilogue stores (since removed from zv_gemm.inc) for the bf16-only linears on whole tiles:
//    208.4 against 217.4 us alone at 78016 x 1536 x 512, but one guided forward 35.66 against
//    35.34 ms (r01_gemm_defer_ab.txt)
//  - the V^T projection on 128x64 persistent tiles: 44.3 against 37.0 us at 78016 rows
//    (r01_skinny_ab.txt)
//  - the copy-only SelfAttention out-projection on the wave-specialised kernel instead of the
//    counted epilogue (ROLE 5): 474.9-476.1 against 452.1-455.9 ms per C2 step (r02_sa_copy_ab.txt)
//  - fp16 parity mode (r03_mixed_ab.txt, C2 timed step; the arms sat in zv_engine::layer): the lo
//    half of the SelfAttention Toeplitz table (PLO 1) and the head-0 / NonlinAttention scoring off
//    the Toeplitz MFMA form (TPNA 0): 481.9 ms with both, 464.3 / 467.3 ms with one of them retired,
//    464.0 ms with both; the attention-score projection as a fully split product (linear<3>)
//    instead of the weight-split one (every arm of that record ran attn_in_wsplit, below)
#pragma once
#include "zv_gemm.inc"
#include "zv_gemm256.inc"
#include "zv_weights.inc"

// K-ring depth of the fp16 parity mode's weight-split value projection (A/B builds; 3: 25.3 ->
// 21.6 ms per C2 step against 2, 4 stages at one block per CU 22.3, profiles/r06_wsplit_ab.txt)
#ifndef ZV_WSPLIT_T_STAGES
#define ZV_WSPLIT_T_STAGES 3
#endif

namespace {

struct Act {           // GEMM operand in HBM: bf16 hi (+ lo in fp32-accurate mode)
  bf16* h = nullptr;
  bf16* l = nullptr;
  long ld = 0;
  // fp8 mode: the MX-fp8 copy (values (rows, ldq), scales (rows, ldq / 32)) or null
  uint8_t* q = nullptr;
  uint8_t* qs = nullptr;
  long ldq = 0;
};

struct Out {              // epilogue of a linear
  float* C = nullptr; long ldc = 0;
  Act act;               // bf16 hi/lo copy (act.h null = none)
  int act_fn = 0;
  const float* resid = nullptr;
  const float* rowvec = nullptr; long rowvec_ld = 0; int rows_per_group = 1;
  const float* orig = nullptr; const float* byp = nullptr;
  // pair-residual form (bf16 mode): residual / bypass original as bf16 hi/lo pairs
  const bf16* residh = nullptr; const bf16* residl = nullptr;
  const bf16* origh = nullptr; const bf16* origl = nullptr;
};

// one linear's launch: 2 x 2 waves, one tile per block; the template parameters that vary
template <int BM, int BN, int SPLIT, int EPI, int STAGES = 2, int OCC = 2, int ROLE = 0, int MXO = 0,
          int BK = GEMM_BK, int UTT = 0>
void gemm_tile(const GemmParams& p, hipStream_t s, const char* tag) {
  launch_gemm<BM, BN, 2, 2, SPLIT, EPI, STAGES, OCC, BK, 0, 0, ROLE, MXO, UTT>(p, 1, s, tag, true, -1);
}
// the counted NA / transposed linears: utterance-aligned M tiles (zv_gemm.inc UTT) or row tiles
template <int BM, int BN, int SPLIT, int EPI, int STAGES, int OCC>
void gemm_tile_t(const GemmParams& p, bool utt, hipStream_t s, const char* tag) {
  if (utt) gemm_tile<BM, BN, SPLIT, EPI, STAGES, OCC, 3, 0, GEMM_BK, 1>(p, s, tag);
  else gemm_tile<BM, BN, SPLIT, EPI, STAGES, OCC, 3>(p, s, tag);
}

struct LinearPolicy {
  int res_counted = 31;            // ZV_RES_COUNTED: the counted epilogues (bit mask: 1 residual,
                                   // 2 plain, 4 NA, 8 GLU, 16 transposed; 1 = all, 0 = the general
                                   // epilogue, zv_gemm.inc gemm_epilogue: bitwise A/B tests;
                                   // 32 + mask: that mask)
  // ZV_GEMM256: the 256x256 phased kernel (zv_gemm256.inc) for the bias (+ SwooshL) and GLU
  // linears with at least gemm256_min_tiles tiles (1 persistent, 2 one tile per block, 0 off)
  int gemm256 = 2;
  static constexpr int gemm256_min_tiles = 256;
  // ZV_TRANS_ALIGNED: utterance-aligned tiles with 16-B transposed stores (zv_gemm.inc UTT /
  // store_trans8) for the counted NA in-projection and value projection where gemm_utt_ok holds
  // (1 both, 0 neither: the row tiles and per-element stores; 2 the NA in-projection alone, 3 the
  // value projection alone).  Bitwise equal; profiles/trans_aligned_ab.txt
  bool utt_na = true, utt_t = true;

  LinearPolicy() {
    auto envi = [](const char* k, int d) { const char* v = getenv(k); return v ? atoi(v) : d; };
    res_counted = envi("ZV_RES_COUNTED", 31);
    if (res_counted == 1) res_counted = 31;            // 1: all (0 / 1 are the A/B tests' arms)
    else if (res_counted >= 32) res_counted &= 31;     // 32 + mask: exactly that mask (bisection)
    gemm256 = envi("ZV_GEMM256", 2);
    const int ta = envi("ZV_TRANS_ALIGNED", 1);
    utt_na = ta == 1 || ta == 2;
    utt_t = ta == 1 || ta == 3;
  }

  // The tile regimes, by how many 128 x 128 tiles the launch has.  The residual and small plain
  // linears are HBM-bound in the epilogue; a grid of fewer tiles than ~1.5 per CU leaves CUs idle
  // or single-block, and smaller tiles with more blocks per CU overlap one block's residual traffic
  // with the others' K loops.  Bitwise equal (every accumulator sees the same MFMA sequence).
  static long tiles128(const GemmParams& p) { return (long)cdiv(p.M, 128) * cdiv(p.N, 128); }
  static bool under_half_tile_per_cu(const GemmParams& p) { return tiles128(p) < zv_num_cus() / 2; }
  static bool under_3half_tiles_per_cu(const GemmParams& p) { return tiles128(p) < zv_num_cus() * 3 / 2; }
  // the 256x256 kernel's preconditions (16-bit operands: the lo halves the fp32-accurate mode
  // keeps beside them are not read; padded K rows, the direct
  // epilogues' activations) and enough tiles to fill the chip
  bool use_gemm256(const GemmParams& p) const {
    return gemm256 != 0 && !p.Cl && !p.As && p.N % 8 == 0 && (p.act == 0 || p.act == 1) &&
           p.lda % 8 == 0 && p.ldb % 8 == 0 && p.lda >= round_up(p.K, GEMM_BK) &&
           p.ldb >= round_up(p.K, GEMM_BK) && p.Brows >= p.N &&
           (long)cdiv(p.M, 256) * cdiv(p.N, 256) >= gemm256_min_tiles;
  }

  static GemmParams gp_linear(const Linear& Lw, const Act& A, long M) {
    GemmParams p{};
    p.M = (int)M; p.N = Lw.N; p.K = Lw.K; p.nz2 = 1; p.Brows = Lw.Npad;
    p.Ah = A.h; p.Al = A.l; p.lda = A.ld;
    p.Bh = Lw.hi; p.Bl = Lw.lo; p.ldb = Lw.Kpad;
    p.bias = Lw.b; p.rows_per_group = 1; p.rpb = 1;
    return p;
  }
  static GemmParams gp_linear8(const Linear& Lw, const Act& A, long M) {
    GemmParams p = gp_linear(Lw, A, M);
    p.Ah = reinterpret_cast<const bf16*>(A.q); p.Al = nullptr; p.lda = A.ldq;
    p.As = A.qs; p.ldas = A.ldq / MX8_BLOCK;
    p.Bh = reinterpret_cast<const bf16*>(Lw.q8); p.Bl = nullptr; p.ldb = Lw.Kq;
    p.Bs = Lw.s8; p.ldbs = Lw.Kq / MX8_BLOCK;
    return p;
  }

  // the MX-fp8 copy of a bf16 operand, for producers that do not write one themselves
  void pack8(const Act& A, long M, int K, hipStream_t s) {
    ZV_REQUIRE(A.h && A.q && K % MX8_BLOCK == 0 && A.ldq >= K && A.ld % 8 == 0, "fp8 pack: operand layout");
    hipLaunchKernelGGL(zv_mx8_pack_kernel, grid1d(M * (K / 8)), dim3(256), 0, s, A.h, A.ld, M, K, A.q,
                       A.ldq, A.qs);
    ZV_LAUNCH_CHECK();
  }

  // a linear on block-scaled fp8 MFMA (A and W MX-fp8): the counted epilogues, writing the
  // output's fp8 copy where the next fp8 linear reads it (MXO 1: with the bf16 copy, 2: only)
  void linear8(const Linear& Lw, const Act& A, long M, const Out& o, hipStream_t s) {
    GemmParams p = gp_linear8(Lw, A, M);
    p.act = o.act_fn;
    p.C = o.C; p.ldc = o.ldc;
    p.Ch = o.act.h; p.Cl = nullptr; p.ldch = o.act.ld;
    p.resid = o.resid; p.orig = o.orig; p.byp = o.byp;
    p.rowvec = o.rowvec; p.rowvec_ld = o.rowvec_ld; p.rows_per_group = o.rows_per_group;
    p.Cq = o.act.q; p.Cs = o.act.qs; p.ldcq = o.act.ldq;
    ZV_REQUIRE(p.bias && !o.residh && Lw.N % 8 == 0 && (!o.rowvec || (o.resid && !o.orig && o.act.q)),
               "fp8 linear: bias; a row vector only on a residual linear with the fp8 copy");
    const int mxo = o.act.q ? (o.act.h ? 1 : 2) : 0;
    if (o.resid) {
      ZV_REQUIRE(mxo != 2 && !o.act_fn, "fp8 residual linear: fp32 stream out");
      const char* tag = "gemm_fp8_resid";
      if (o.rowvec) {
        gemm_tile<128, 128, 8, EPI_STD, 2, 2, 4, 1, MX8_KSTEP>(p, s, tag);
      } else if (o.orig) {
        if (mxo) gemm_tile<128, 128, 8, EPI_STD, 2, 2, 2, 1, MX8_KSTEP>(p, s, tag);
        else gemm_tile<128, 128, 8, EPI_STD, 2, 2, 2, 0, MX8_KSTEP>(p, s, tag);
      } else {
        if (mxo) gemm_tile<128, 128, 8, EPI_STD, 2, 2, 1, 1, MX8_KSTEP>(p, s, tag);
        else gemm_tile<128, 128, 8, EPI_STD, 2, 2, 1, 0, MX8_KSTEP>(p, s, tag);
      }
      return;
    }
    ZV_REQUIRE(!o.C && mxo, "fp8 plain linear: bias (+ activation) -> fp8 (+ bf16) copy");
    if (mxo == 2) gemm_tile<128, 128, 8, EPI_STD, 2, 2, 3, 2, MX8_KSTEP>(p, s, "gemm_fp8");
    else gemm_tile<128, 128, 8, EPI_STD, 2, 2, 3, 1, MX8_KSTEP>(p, s, "gemm_fp8");
  }

  template <int SPLIT>
  void linear(const Linear& Lw, const Act& A, long M, const Out& o, hipStream_t s) {
    if constexpr (SPLIT == 1)
      if (Lw.q8 && A.q) { linear8(Lw, A, M, o, s); return; }
    // a 16-bit linear whose output also feeds an fp8 linear: its kernel writes the fp8 copy
    // (the row-vector residual epilogue) or the pack kernel does
    if (!linear16<SPLIT>(Lw, A, M, o, s) && o.act.q) pack8(o.act, M, Lw.N, s);
  }

  // Residual linears (counted ROLE 1 / 2 / 4 / 5 epilogues): the tile by the launch's regime.
  // Lab, K = 560 ROLE 4 (profiles/r05_resid_tiles_ab.txt): M = 6502 14.1 -> 12.4 us (128 x 64),
  // 1625 11.1 -> 6.8 us (64 x 64); 13003 and up: 128 x 128 (128 x 64 or 64 x 64 at every size lost
  // in the C2 step, round 6: profiles/r06_resid_tile_ab.txt)
  template <int SPLIT, int ROLE>
  void launch_resid(const GemmParams& p, hipStream_t s, const char* tag) {
    if constexpr (SPLIT == 1) {
      if (under_half_tile_per_cu(p)) return gemm_tile<64, 64, 1, EPI_STD, 4, 2, ROLE>(p, s, tag);
      if (under_3half_tiles_per_cu(p)) return gemm_tile<128, 64, 1, EPI_STD, 2, 3, ROLE>(p, s, tag);
    }
    gemm_tile<128, 128, SPLIT, EPI_STD, 2, 2, ROLE>(p, s, tag);
  }

  // returns whether the kernel wrote the output's fp8 copy (o.act.q)
  template <int SPLIT>
  bool linear16(const Linear& Lw, const Act& A, long M, const Out& o, hipStream_t s) {
    constexpr bool split = SPLIT == 3;
    GemmParams p = gp_linear(Lw, A, M);
    p.act = o.act_fn;
    p.C = o.C; p.ldc = o.ldc;
    p.Ch = o.act.h; p.Cl = o.act.l; p.ldch = o.act.ld;
    p.resid = o.resid; p.rowvec = o.rowvec; p.rowvec_ld = o.rowvec_ld;
    p.rows_per_group = o.rows_per_group; p.orig = o.orig; p.byp = o.byp;
    p.residh = o.residh; p.residl = o.residl; p.origh = o.origh; p.origl = o.origl;
    if constexpr (SPLIT == 1) {
      if (o.residh) {   // pair-residual linear: own instantiation (RP 1), the residual policy
        launch_gemm<128, 128, 2, 2, 1, EPI_STD, 2, 2, GEMM_BK, 1>(p, 1, s, "gemm_bf16", true, -1);
        return false;
      }
    }
    ZV_REQUIRE(!o.residh, "pair residual needs the bf16 mode");
    const char* tag = split ? "gemm_fp32" : "gemm_bf16";
    if (Lw.N <= 64) {   // own tag: the roofline's gemm_bf16 is the 128x128 instantiation alone
      launch_gemm<128, 64, 2, 2, SPLIT, EPI_STD>(p, 1, s, split ? "gemm_fp32_n64" : "gemm_bf16_n64");
      return false;
    }
    if (o.resid) return linear16_resid<SPLIT>(p, o, s);
    // bias (+ activation) -> bf16 copy: the counted epilogue (ROLE 3)
    const bool counted = (res_counted & 2) && p.bias && p.Ch && !p.C && !p.rowvec && Lw.N % 8 == 0 &&
                         p.ldch % 8 == 0 && (p.Cl != nullptr) == split;
    // 96-wide tiles where they waste fewer columns than 128-wide ones (the attention-score
    // projection, N = 272: 288 computed columns instead of 384)
    if ((Lw.N + 95) / 96 * 96 < (Lw.N + 127) / 128 * 128) {
      const char* t96 = split ? "gemm_fp32_n96" : "gemm_bf16_n96";
      if (!counted || p.act) {
        gemm_tile<128, 96, SPLIT, EPI_STD>(p, s, t96);
      } else if constexpr (SPLIT == 1) {
        // 128 x 64 tiles at 3 blocks per CU (320 columns computed), at every size: 15.2 -> 13.9 ms per
        // C2 step against 128 x 128 for the large launches (round 6, profiles/r06_n96_ab.txt; 64 x 64
        // with a 4-deep ring 15.3); bitwise equal
        gemm_tile<128, 64, 1, EPI_STD, 2, 3, 3>(p, s, t96);
      } else {
        // counted 128 x 128 tiles (384 columns computed): 9.1 ms per step against 12.9 for the 96-wide
        // general epilogue (profiles/r02_n96_counted_ab.txt)
        gemm_tile<128, 128, SPLIT, EPI_STD, 2, 2, 3>(p, s, t96);
      }
      return false;
    }
    if (!counted) {
      gemm_tile<128, 128, SPLIT, EPI_STD>(p, s, tag);
      return false;
    }
    if constexpr (SPLIT == 1) {
      if (!o.act.q && use_gemm256(p)) {
        launch_gemm256<EPI_STD, 3>(p, s, tag, gemm256 == 1);
        return false;
      }
      // (fewer than 1.5 128 x 128 tiles per CU: 128 x 64 tiles, 3 blocks per CU; bitwise equal;
      // lab 3660 x 1536 x 512 13.7 -> 12.9 us, 1830 rows 10.5 -> 9.0, r05_resid_tiles_ab.txt)
      if (under_3half_tiles_per_cu(p)) {
        gemm_tile<128, 64, 1, EPI_STD, 2, 3, 3>(p, s, tag);
        return false;
      }
    }
    gemm_tile<128, 128, SPLIT, EPI_STD, 2, 2, 3>(p, s, tag);
    return false;
  }

  // linear16's residual-stream linears: their own symbols / tags (HBM roofline; one tag per ROLE:
  // the roofline's bytes and PMC traffic per symbol)
  template <int SPLIT>
  bool linear16_resid(GemmParams& p, const Out& o, hipStream_t s) {
    constexpr bool split = SPLIT == 3;
    if constexpr (SPLIT == 1) {
      // the copy-only form (no fp32 output) on the counted epilogue (ROLE 5;
      // profiles/r02_sa_copy_ab.txt)
      if (!p.C && p.rowvec && !p.orig && !o.act.l && !o.act.q && p.Ch && p.bias && p.N % 8 == 0 &&
          p.ldch % 8 == 0) {
        launch_resid<1, 5>(p, s, "gemm_bf16_resid_copy");
        return false;
      }
    }
    // the counted residual epilogue (zv_gemm.inc gemm_epilogue_res; ROLE 2 = with the
    // bypass original) where its preconditions hold, else the general epilogue
    const bool counted = (res_counted & 1) && p.bias && !(p.rowvec && p.orig) && !p.act && p.C &&
                         p.N % 8 == 0 && p.ldc % 4 == 0 && (!p.Ch || p.ldch % 8 == 0) &&
                         (!p.orig || p.byp) && (p.Cl != nullptr) == (split && p.Ch != nullptr);
    if (!counted) {
      gemm_tile<128, 128, SPLIT, EPI_STD>(p, s, split ? "gemm_fp32_resid" : "gemm_bf16_resid");
    } else if (p.orig) {
      launch_resid<SPLIT, 2>(p, s, split ? "gemm_fp32_resid_byp" : "gemm_bf16_resid_byp");
    } else if (p.rowvec) {         // + the row-group vector (ROLE 4)
      const char* tag = split ? "gemm_fp32_resid_rv" : "gemm_bf16_resid_rv";
      if constexpr (SPLIT == 1)
        if (o.act.q && o.act.h && p.Ch) {   // fp8 mode: + the stream's fp8 copy (MXO 1)
          p.Cq = o.act.q; p.Cs = o.act.qs; p.ldcq = o.act.ldq;
          gemm_tile<128, 128, 1, EPI_STD, 2, 2, 4, 1>(p, s, tag);
          return true;
        }
      launch_resid<SPLIT, 4>(p, s, tag);
    } else {
      launch_resid<SPLIT, 1>(p, s, split ? "gemm_fp32_resid" : "gemm_bf16_resid");
    }
    return false;
  }

  // mixed mode's attention-score projection: the weight-split product a.(wh + wl) (SPLIT 2:
  // the 16-bit layer input against the weight's hi/lo pair, 2 MFMAs per product instead of
  // the bf16x3 form's 3).  tools/precision_study.py --r03: mean |err| 5.4e-4 / 8.8e-4 / 9.3e-4
  // on the C1 / dialog / stereo fixtures vs 5.2e-4 / 8.6e-4 / 8.9e-4 fully split
  // (profiles/r03_precision_study_r03_*.txt); 128x64 tiles (the hi/lo weight stage fits two
  // blocks per CU)
  void attn_in_wsplit(const Linear& Lw, const Act& A, long M, const Out& o, hipStream_t s) {
    GemmParams p = gp_linear(Lw, A, M);
    p.Al = nullptr;
    p.Ch = o.act.h; p.Cl = nullptr; p.ldch = o.act.ld;
    ZV_REQUIRE(p.bias && p.Ch && !o.act.l && !o.C && !o.resid && !o.act_fn && Lw.lo && Lw.N % 8 == 0 &&
                   p.ldch % 8 == 0,
               "weight-split projection: bias -> 16-bit copy");
    gemm_tile<128, 64, 2, EPI_STD, 2, 2, 3>(p, s, "gemm_wsplit_n96");
  }

  // The layer's fused-epilogue launch choices on a prepared GemmParams (shared with zv_linear_check).
  // NonlinAttention in-projection (EPI_NA: rows permuted by perm_na)
  template <int SPLIT>
  void launch_na_in(const GemmParams& p, hipStream_t s) {
    // counted NA epilogue: 16-bit modes (in the split mode it differs from the general one
    // by up to 1.1e-4 in the decoder output, tools/counted_bisect.py; not bitwise: kept off)
    if constexpr (SPLIT == 1) {
      // (64-row tiles at 3 blocks per CU at every size: 32.5 -> 31.4 ms per C2 step against 128-row
      // tiles for the large launches, round 6, profiles/r06_ffn_rows_na_tile_ab.txt; bitwise equal)
      if ((res_counted & 4) && p.bias && p.N % 48 == 0 && p.ldch % 4 == 0)
        return gemm_tile_t<64, 96, 1, EPI_NA, 2, 3>(p, utt_na && gemm_utt_ok(p), s, "gemm_bf16_na");
    }
    gemm_tile<128, 96, SPLIT, EPI_NA>(p, s, SPLIT == 3 ? "gemm_fp32_na" : "gemm_bf16_na");
  }
  // SelfAttention value projection (EPI_TRANS); sa_split: the fp16 parity mode's a . (w_hi + w_lo)
  // N = 48 (64 padded): 64-row tiles give 2x the blocks of a 128-row grid (one tile column;
  // profiles/r01_skinny_ab.txt)
  template <int SPLIT>
  void launch_value_t(const GemmParams& p, bool sa_split, bool has_lo, hipStream_t s) {
    const char* tag = SPLIT == 3 ? "gemm_fp32_t" : "gemm_bf16_t";
    const bool utt = utt_t && gemm_utt_ok(p);
    if (sa_split) {                    // fp16 parity mode: a . (w_hi + w_lo)
      ZV_REQUIRE(has_lo && (res_counted & 16), "weight-split value projection");
      gemm_tile_t<64, 64, 2, EPI_TRANS, ZV_WSPLIT_T_STAGES, ZV_WSPLIT_T_STAGES < 4 ? 2 : 1>(p, utt, s, "gemm_wsplit_t");
    } else if (res_counted & 16) {
      // (a 4-deep K ring: one 64-row tile per block has 8 K steps and little else in flight;
      // 2 -> 4 stages: 24.0 -> 18.9 ms per C2 step, profiles/r05_vt_stages_ab.txt)
      gemm_tile_t<64, 64, SPLIT, EPI_TRANS, 4, 2>(p, utt, s, tag);
    } else {
      gemm_tile<64, 64, SPLIT, EPI_TRANS>(p, s, tag);
    }
  }
  // ConvolutionModule in-projection (EPI_GLU: rows permuted by perm_glu); g8: MX-fp8 operands
  template <int SPLIT>
  void launch_glu_in(const GemmParams& p, bool g8, hipStream_t s) {
    if (g8) {
      ZV_REQUIRE(p.bias && p.N % 32 == 0 && p.ldch % 8 == 0, "fp8 GLU linear layout");
      return gemm_tile<128, 128, 8, EPI_GLU, 2, 2, 3, 0, MX8_KSTEP>(p, s, "gemm_fp8_glu");
    }
    const char* tag = SPLIT == 3 ? "gemm_fp32_glu" : "gemm_bf16_glu";
    if (!((res_counted & 8) && p.bias && p.N % 32 == 0 && p.ldch % 8 == 0))
      return gemm_tile<128, 128, SPLIT, EPI_GLU>(p, s, tag);
    if constexpr (SPLIT == 1) {
      if (use_gemm256(p)) return launch_gemm256<EPI_GLU, 3>(p, s, tag, gemm256 == 1);
      // (fewer than 1.5 128 x 128 tiles per CU: 64 x 128, 3 blocks per CU, as launch_resid)
      if (under_3half_tiles_per_cu(p)) return gemm_tile<64, 128, 1, EPI_GLU, 2, 3, 3>(p, s, tag);
    }
    gemm_tile<128, 128, SPLIT, EPI_GLU, 2, 2, 3>(p, s, tag);
  }
  // The in-projection with the depthwise conv (+ SwooshR) in its epilogue (zv_gemm256.inc
  // g256_epi_glu_dw; p.dw_* set, dw_out == Ch): the counted GLU epilogue at D = 512 channels, a
  // kernel size with an instantiation, the 256x256 kernel's 16-bit operand layout
  bool glu_dw_fits(const GemmParams& p, int D, int ks) const {
    return (res_counted & 8) && D == 512 && p.N == 2 * D && (ks == 7 || ks == 15 || ks == 31) && p.bias &&
           !p.Cl && !p.As && p.lda % 8 == 0 && p.ldb % 8 == 0 && p.lda >= round_up(p.K, GEMM_BK) &&
           p.ldb >= round_up(p.K, GEMM_BK) && p.Brows >= p.N && p.ld_dw % 8 == 0;
  }
  void launch_glu_dw(const GemmParams& p, int ks, hipStream_t s, const char* tag) {
    if (ks == 31) launch_gemm256<EPI_GLU, 3, 0, 0, 1, 1, 31>(p, s, tag, false);
    else if (ks == 15) launch_gemm256<EPI_GLU, 3, 0, 0, 1, 1, 15>(p, s, tag, false);
    else launch_gemm256<EPI_GLU, 3, 0, 0, 1, 1, 7>(p, s, tag, false);
  }
};

}  // namespace
