// Fused (flash-style) relative-position attention for the three consumers of a
// Zipformer layer's attention weights.
//
// The reference computes W = softmax(q.k^T + pos) once per layer
// (RelPositionMultiheadAttentionWeights, zipformer.py:1149-1306) and multiplies
// it into three different value tensors at three points of the layer:
// NonlinAttention (head 0, 384-wide values, zipformer.py:1534), SelfAttention1
// and SelfAttention2 (4 heads x 12, :1383).  Materialising W costs
// H*B*L^2 elements of HBM traffic per write/read (0.8 GB per layer at the
// benchmark shape).  Here W never exists in memory:
//
//  * zv_attn_stats_kernel: head 0's per-row max m and 1/sum r of exp(s - m)
//    (the NonlinAttention consumer needs them up front, see below).
//  * zv_attn_na_kernel: NonlinAttention.  Per block of QTILES x 16 queries and
//    2 x QTILES waves: each wave scores a 16-query x 16-key quarter of a 32-key
//    step on MFMA (q.k^T, K = 32, + the rank-4 positional term), turns it into
//    p = exp(s - m) r and drops the bf16 P^T fragment into LDS; after one barrier
//    every wave multiplies 4 query tiles' P into its own slice of the 384 value
//    channels (12 MFMAs per step), V^T double-buffered in LDS.
//  * zv_attn_sa_kernel: SelfAttention (12-wide heads).  One head per block,
//    online softmax (running max per query, accumulator rescaled only when the
//    max grows by more than 2^8), and the softmax denominator comes out of the
//    same MFMA: V^T row 12 of the 16-row value tile is all ones, so the
//    accumulator row 12 is sum_j p_j.
//
// Scores are computed transposed, S^T = K . Q^T (keys on the MFMA rows, queries
// on the lanes), so the fp32 score accumulator of two 16-key tiles IS the bf16 B
// operand of the P^T . V product with no lane movement: k-slot e of lane group g
// is key 4g+e (tile a, e<4) or 16+4g+e-4 (tile b); the V^T operand is read with
// the same key permutation (two 8-byte LDS reads per lane).  All exponentials
// are v_exp_f32 (base 2) with log2(e) folded into the positional projection
// and the row constants; in the 8-keys-per-lane kernels the positional term is
// evaluated two keys at a time with packed fp32 FMAs from a pair-interleaved
// LDS copy of the head's slice of the projected table.
#pragma once
#include "zv_common.h"
#include "zv_gemm.inc"
#include "zv_attn.inc"

struct FlashParams {
  const bf16* qh; const bf16* ql; long ldq;   // (B, L, ldq) [q | k | p], hi/lo
  const float* P;                             // (2L-1, H*pd) positional projection
  const uint8_t* key_pad;                     // (B, L) or null
  float2* stats;                              // (B, L): head 0 (base-2 max, 1/sum)
  int B, L, H;
  // consumers
  const bf16* vh; const bf16* vl; long ldv;   // V^T rows (B, vrows, ldv)
  long sv_b; int vrows_per_head;              // batch stride; head offset = h * vrows_per_head rows
  int nv;                                     // value channels per head (12 SA, hid NA)
  const bf16* mulh; const bf16* mull; long ldmul;   // NA: y (B*L, ldmul), multiplied in
  bf16* oh; bf16* ol; long ldo; int ocol_per_head;  // out (B*L, ldo), col = h*ocol_per_head + d
  // SelfAttention (Toeplitz form) in the fp16 parity mode: ol = the output's lo half, oh2 a second
  // hi copy (the K-concatenated conv + SelfAttention out-projection's [o_hi | o_lo | o_hi] blocks)
  bf16* oh2;
  // second-generation consumers (zv_flash2.inc): force_exact sends every wave / block through the
  // exact path (test infrastructure: ZV_ATTN2_EXACT); fallback (or null) counts exact-path runs:
  // [0] a query's denominator under 2^-60, [1] over 2^100 or a non-finite accumulator, [2] all runs
  int force_exact;
  unsigned* fallback;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr float FA_LOG2E = 1.4426950408889634f;
constexpr float FA_MASKED = -1000.f * FA_LOG2E;   // the reference's masked_fill(-1000), base 2
constexpr int FA_KB = 32;       // keys per step
constexpr int FA_VROW = 40;     // bf16 per staged V^T row, SA (16-B aligned rows)
constexpr int NA_VROW = 36;     // bf16 per staged V^T row, NA (72-B rows: 8-B aligned, 2-way max)

// ---------------------------------------------------------------------------
// block staging of the head's positional slice, n = L-1-(qt0+QT-1) + t,
// t in [0, L+QT+32) (zero outside [0, 2L-2]), scaled by log2(e):
//   PAIR: Ps[2t], Ps[2t+1] = {P[n][0], P[n+1][0], P[n][1], P[n+1][1]},
//                            {P[n][2], P[n+1][2], P[n][3], P[n+1][3]}
//   else: Ps[t] = P[n]
// plus the key mask Ms[j] (0 keep, 1 masked, 2 beyond L) and one flag per
// 32-key step (any key of the step not plain).
// ---------------------------------------------------------------------------
template <int KS>
__device__ __forceinline__ void stage_mask(const FlashParams& p, int b, uint8_t* Ms, uint8_t* Fs,
                                           int tid, int nt);

template <bool PAIR, int KS = FA_KB>
__device__ __forceinline__ void stage_pos_mask(const FlashParams& p, int h, int b, int qt0, int QT,
                                               f32x4* Ps, uint8_t* Ms, uint8_t* Fs, int tid,
                                               int nt) {
  const int L = p.L;
  const int nlo = L - 1 - (qt0 + QT - 1);
  const int nkb = (L + KS - 1) / KS;
  for (int kb = tid; kb < nkb; kb += nt) Fs[kb] = 0;
  auto prow = [&](int n) -> f32x4 {
    if (n < 0 || n > 2 * L - 2) return f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 v = *reinterpret_cast<const f32x4*>(p.P + (long)n * p.H * ATT_PD + h * ATT_PD);
    return v * FA_LOG2E;
  };
  // batches of 4 entries per thread: all loads in flight before the first store
  const int N = L + QT + KS;
  for (int t0 = tid; t0 < N; t0 += 4 * nt) {
    f32x4 a[4], c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + i * nt;
      a[i] = prow(t < N ? nlo + t : -1);
      if constexpr (PAIR) c[i] = prow(t < N ? nlo + t + 1 : -1);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + i * nt;
      if (t >= N) break;
      if constexpr (PAIR) {
        Ps[2 * t] = f32x4{a[i][0], c[i][0], a[i][1], c[i][1]};
        Ps[2 * t + 1] = f32x4{a[i][2], c[i][2], a[i][3], c[i][3]};
      } else {
        Ps[t] = a[i];
      }
    }
  }
  stage_mask<KS>(p, b, Ms, Fs, tid, nt);
}

// key mask Ms[j] (0 keep, 1 masked, 2 beyond L) and one flag per KS-key step; the caller
// zeroed Fs (barrier inside)
template <int KS>
__device__ __forceinline__ void stage_mask(const FlashParams& p, int b, uint8_t* Ms, uint8_t* Fs,
                                           int tid, int nt) {
  const int L = p.L;
  const int nkb = (L + KS - 1) / KS;
  __syncthreads();   // Fs zeroed before the mask pass flags steps
  const uint8_t* kp = p.key_pad ? p.key_pad + (long)b * L : nullptr;
  const int NM = nkb * KS;
  for (int t0 = tid; t0 < NM; t0 += 4 * nt) {
    uint8_t m[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + i * nt;
      m[i] = (t >= L) ? 2 : (kp ? kp[t] : 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + i * nt;
      if (t >= NM) break;
      Ms[t] = m[i];
      if (m[i]) Fs[t / KS] = 1;
    }
  }
}

// LDS bytes of stage_pos_mask's image (Ps: (L+QT+KS) entries, Ms: nkb*KS, Fs: nkb)
__host__ __device__ inline size_t pos_mask_bytes(int L, int QT, bool pair, int KS = FA_KB) {
  const int nkb = (L + KS - 1) / KS;
  return (size_t)(L + QT + KS) * (pair ? 32 : 16) + (size_t)nkb * KS + round_up(nkb, 16);
}

// base-2 scores u = log2(e) (q.k + pos) of 4 consecutive keys jq..jq+3 for this
// lane's query, from the S^T accumulator s (rows 4g..4g+3) and the slice entry t
template <bool PAIR>
__device__ __forceinline__ void pos4(const f32x4& s, const f32x4* Ps, int t, const f32x2 (&pq)[4],
                                     float (&u)[4]) {
  if constexpr (PAIR) {
    const f32x4 a0 = Ps[2 * t], a1 = Ps[2 * t + 1];          // keys jq, jq+1
    const f32x4 b0 = Ps[2 * t + 4], b1 = Ps[2 * t + 5];      // keys jq+2, jq+3
    f32x2 x = f32x2{s[0], s[1]} * FA_LOG2E;
    f32x2 y = f32x2{s[2], s[3]} * FA_LOG2E;
    x = f32x2{a0[0], a0[1]} * pq[0] + x;
    y = f32x2{b0[0], b0[1]} * pq[0] + y;
    x = f32x2{a0[2], a0[3]} * pq[1] + x;
    y = f32x2{b0[2], b0[3]} * pq[1] + y;
    x = f32x2{a1[0], a1[1]} * pq[2] + x;
    y = f32x2{b1[0], b1[1]} * pq[2] + y;
    x = f32x2{a1[2], a1[3]} * pq[3] + x;
    y = f32x2{b1[2], b1[3]} * pq[3] + y;
    u[0] = x[0]; u[1] = x[1]; u[2] = y[0]; u[3] = y[1];
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x4 a = Ps[t + r];
      float v = s[r] * FA_LOG2E;
      v = fmaf(a[0], pq[0][0], v);
      v = fmaf(a[1], pq[1][0], v);
      v = fmaf(a[2], pq[2][0], v);
      u[r] = fmaf(a[3], pq[3][0], v);
    }
  }
}

__device__ __forceinline__ void mask4(const uint8_t* Ms, int jq, float (&u)[4]) {
  const unsigned mk = *reinterpret_cast<const unsigned*>(Ms + jq);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned m8 = (mk >> (8 * r)) & 0xff;
    u[r] = m8 ? (m8 == 1 ? FA_MASKED : -INFINITY) : u[r];
  }
}

// max over the four lanes {l, l^16, l^32, l^48} holding one query's keys (S^T
// layout): two VALU half-swaps (v_permlane16/32_swap) instead of two LDS-routed
// ds_bpermute shuffles on the softmax's serial chain
__device__ __forceinline__ float qmax4(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  const float a = __uint_as_float(r[0]), b = __uint_as_float(r[1]);
  const float m = a > b ? a : b;
  const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  const float c = __uint_as_float(r2[0]), d = __uint_as_float(r2[1]);
  return c > d ? c : d;
}

// Toeplitz table PP[t] = {P[n], P[n-1]} (n = L-1-(qt0+QT-1) + t, t < NT; zero outside
// [0, 2L-2]) in the operand format, natural units; PLO: the lo halves at PPl
template <int PLO>
__device__ __forceinline__ void stage_tp(const FlashParams& p, int h, int qt0, int QT, int NT,
                                         bf16x8* PPh, bf16x8* PPl, int tid, int nt) {
  const int L = p.L;
  const int nlo = L - 1 - (qt0 + QT - 1);
  auto prow = [&](int n) -> f32x4 {
    if (n < 0 || n > 2 * L - 2) return f32x4{0.f, 0.f, 0.f, 0.f};
    return *reinterpret_cast<const f32x4*>(p.P + (long)n * p.H * ATT_PD + h * ATT_PD);
  };
  for (int t0 = tid; t0 < NT; t0 += 2 * nt) {
    f32x4 a[2], c[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = t0 + i * nt;
      a[i] = prow(t < NT ? nlo + t : -1);
      c[i] = prow(t < NT ? nlo + t - 1 : -1);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = t0 + i * nt;
      if (t >= NT) break;
      bf16x8 hv, lv;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        hv[d] = (bf16)a[i][d];
        hv[4 + d] = (bf16)c[i][d];
        lv[d] = (bf16)(a[i][d] - (float)hv[d]);
        lv[4 + d] = (bf16)(c[i][d] - (float)hv[4 + d]);
      }
      PPh[t] = hv;
      if constexpr (PLO) PPl[t] = lv;
    }
  }
}

// the lane's query operands for a 16-query tile at i0 (query c16 = lane & 15): the Q^T
// fragment, the two positional B operands (shift halves), and the table offset of A row
// m = c16, shift slot 2g at key tile 0 for a block whose table starts at qt0 (QT queries)
__device__ __forceinline__ void tp_query(const FlashParams& p, long qrow, int h, int c16, int g,
                                         int i0, int qt0, int QT, bf16x8& qf, bf16x8 (&pb)[2],
                                         int& tbl) {
  qf = *reinterpret_cast<const bf16x8*>(p.qh + qrow + h * ATT_QD + g * 8);
  const bf16x4 pq = *reinterpret_cast<const bf16x4*>(p.qh + qrow + 2 * p.H * ATT_QD + h * ATT_PD);
  const bf16 zero = (bf16)0.f;
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const int dl = c16 - 8 * hf - 2 * g;          // this lane's k-slots hold shifts 2g, 2g+1
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      pb[hf][d] = dl == 0 ? pq[d] : zero;
      pb[hf][4 + d] = dl == 1 ? pq[d] : zero;
    }
  }
  tbl = QT - 1 - (i0 - qt0) + c16 - 2 * g;
}

// S^T tile (16 keys x 16 queries, natural units) = K.Q^T + the positional term;
// ta = key tile base + tbl
template <int PLO>
__device__ __forceinline__ f32x4 tp_score(const bf16x8* PPh, const bf16x8* PPl, int ta,
                                          const bf16x8 (&pb)[2], const bf16x8& kf,
                                          const bf16x8& qf) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if constexpr (PLO) {
    s = ZV_MFMA_16x16x32(PPl[ta], pb[0], s, 0, 0, 0);
    s = ZV_MFMA_16x16x32(PPl[ta - 8], pb[1], s, 0, 0, 0);
  }
  s = ZV_MFMA_16x16x32(PPh[ta], pb[0], s, 0, 0, 0);
  s = ZV_MFMA_16x16x32(PPh[ta - 8], pb[1], s, 0, 0, 0);
  return ZV_MFMA_16x16x32(kf, qf, s, 0, 0, 0);
}

// mask 4 natural-unit scores of keys jq..jq+3 (the reference's masked_fill(-1000); keys
// beyond L drop out)
__device__ __forceinline__ void mask4n(const uint8_t* Ms, int jq, f32x4& s) {
  const unsigned mk = *reinterpret_cast<const unsigned*>(Ms + jq);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned m8 = (mk >> (8 * r)) & 0xff;
    s[r] = m8 ? (m8 == 1 ? -1000.f : -INFINITY) : s[r];
  }
}

// S^T tile for 16 keys x 16 queries: K fragment (hi, lo) against the lane's Q^T
template <int SPLIT>
__device__ __forceinline__ f32x4 score_tile(const bf16x8& kh, const bf16x8& kl, const bf16x8& qh,
                                            const bf16x8& ql) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if constexpr (SPLIT == 3) {
    s = ZV_MFMA_16x16x32(kl, qh, s, 0, 0, 0);
    s = ZV_MFMA_16x16x32(kh, ql, s, 0, 0, 0);
  }
  return ZV_MFMA_16x16x32(kh, qh, s, 0, 0, 0);
}

// the lane's query: Q^T fragment and its positional projection (paired)
template <int SPLIT>
__device__ __forceinline__ void load_query(const FlashParams& p, long qbase, int qc, int h, int g,
                                           bf16x8& qfh, bf16x8& qfl, f32x2 (&pq)[4]) {
  const int HQ = p.H * ATT_QD;
  load_qk_frag<SPLIT>(p.qh, p.ql, qbase + (long)qc * p.ldq + h * ATT_QD + g * 8, true, qfh, qfl);
  const long po = qbase + (long)qc * p.ldq + 2 * HQ + h * ATT_PD;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const float v = ld_split(p.qh, p.ql, po + d);
    pq[d] = f32x2{v, v};
  }
}

template <int SPLIT>
__device__ __forceinline__ void load_kfrag(const FlashParams& p, long qbase, int h, int j,
                                           int g, bf16x8& kh, bf16x8& kl) {
  const long off = qbase + (long)min(j, p.L - 1) * p.ldq + p.H * ATT_QD + h * ATT_QD + g * 8;
  kh = *reinterpret_cast<const bf16x8*>(p.qh + off);
  if constexpr (SPLIT == 3) kl = *reinterpret_cast<const bf16x8*>(p.ql + off);
}

// ---------------------------------------------------------------------------
// head-0 row statistics (pass 1 of the two-pass softmax, zipformer.py:1295) for
// the NonlinAttention consumer.  Lane = query, 8 keys per lane per 32-key step;
// online max with one rescale of the running sum per step.
// ---------------------------------------------------------------------------
// TPM (16-bit modes): 0 = positional term on VALU FMAs from the paired fp32 table,
// 1 / 2 = Toeplitz MFMA form (tp_score; 2 adds the table's lo half)
template <int SPLIT, int TPM = 0>
__global__ __launch_bounds__(256) void zv_attn_stats_kernel(FlashParams p) {
  constexpr int QT = 64;
  constexpr int PLO = TPM == 2 ? 1 : 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char ssm[];
  const int L = p.L;
  const int NT = L + QT + 32;
  f32x4* Ps2 = reinterpret_cast<f32x4*>(ssm);
  bf16x8* PPh = reinterpret_cast<bf16x8*>(ssm);
  bf16x8* PPl = PPh + NT;
  uint8_t* Ms = ssm + (size_t)NT * (TPM ? 16 * (1 + PLO) : 32);
  const int nkb = (L + FA_KB - 1) / FA_KB;
  uint8_t* Fs = Ms + nkb * FA_KB;
  const int qt0 = blockIdx.x * QT;
  const int h = 0, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const long qbase = (long)b * L * p.ldq;
  const int qi = qt0 + wave * 16 + (lane & 15);
  const int qc = min(qi, L - 1);
  bf16x8 qfh, qfl, pb[2];
  f32x2 pq[4];
  int tbl = 0;
  if constexpr (TPM) {
    for (int kb = tid; kb < nkb; kb += 256) Fs[kb] = 0;
    stage_tp<PLO>(p, h, qt0, QT, NT, PPh, PPl, tid, 256);
    stage_mask<FA_KB>(p, b, Ms, Fs, tid, 256);
    tp_query(p, qbase + (long)qc * p.ldq, h, lane & 15, g, qt0 + wave * 16, qt0, QT, qfh, pb, tbl);
  } else {
    stage_pos_mask<true>(p, h, b, qt0, QT, Ps2, Ms, Fs, tid, 256);
    load_query<SPLIT>(p, qbase, qc, h, g, qfh, qfl, pq);
  }
  const int nbase = qt0 + QT - 1 - qc;
  __syncthreads();
  float mx = -1e30f, sm = 0.f;     // finite: a lane group may see only keys >= L
  bf16x8 kh[2], kl[2], nh[2], nl[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) load_kfrag<SPLIT>(p, qbase, h, t * 16 + (lane & 15), g, kh[t], kl[t]);
  for (int kb = 0; kb < nkb; ++kb) {
    const int j0 = kb * FA_KB;
    if (kb + 1 < nkb) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
        load_kfrag<SPLIT>(p, qbase, h, j0 + FA_KB + t * 16 + (lane & 15), g, nh[t], nl[t]);
    }
    float u[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float v4[4];
      if constexpr (TPM) {
        f32x4 s = tp_score<PLO>(PPh, PPl, j0 + t * 16 + tbl, pb, kh[t], qfh);
        if (Fs[kb]) mask4n(Ms, j0 + t * 16 + g * 4, s);
#pragma unroll
        for (int r = 0; r < 4; ++r) v4[r] = s[r] * FA_LOG2E;
      } else {
        const f32x4 s = score_tile<SPLIT>(kh[t], kl[t], qfh, qfl);
        pos4<true>(s, Ps2, nbase + j0 + t * 16 + g * 4, pq, v4);
        if (Fs[kb]) mask4(Ms, j0 + t * 16 + g * 4, v4);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) u[t * 4 + r] = v4[r];
    }
    const float ml = fmaxf(fmaxf(fmaxf(u[0], u[1]), fmaxf(u[2], u[3])),
                           fmaxf(fmaxf(u[4], u[5]), fmaxf(u[6], u[7])));
    if (ml > mx) { sm *= __builtin_amdgcn_exp2f(mx - ml); mx = ml; }
#pragma unroll
    for (int e = 0; e < 8; ++e) sm += __builtin_amdgcn_exp2f(u[e] - mx);
#pragma unroll
    for (int t = 0; t < 2; ++t) { kh[t] = nh[t]; kl[t] = nl[t]; }
  }
  // combine the 4 lane groups holding this query's keys
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float mo = __shfl_xor(mx, o, 64), so = __shfl_xor(sm, o, 64);
    const float mn = fmaxf(mx, mo);
    sm = sm * __builtin_amdgcn_exp2f(mx - mn) + so * __builtin_amdgcn_exp2f(mo - mn);
    mx = mn;
  }
  if (g == 0 && qi < L) p.stats[(long)b * L + qi] = make_float2(mx, 1.f / sm);
}

// ---------------------------------------------------------------------------
// NonlinAttention consumer: out[q][d] = y[q][d] * sum_j p[q][j] xt[d][j]
// QTILES query tiles per block (2 x QTILES waves); wave w scores query tile
// w >> 1, key half w & 1, and accumulates query tiles 4 (w >> 3) .. +3 times
// value tiles (w & 7) * DTW .. +DTW-1.
// ---------------------------------------------------------------------------
template <int SPLIT, int DTW, int QTILES, int TPM = 0>
__host__ __device__ inline size_t na_lds_bytes(int L) {
  constexpr int NS = SPLIT == 3 ? 2 : 1;
  return (size_t)2 * NS * (8 * DTW * 16) * NA_VROW * 2 +   // V^T double buffer
         (size_t)2 * NS * QTILES * 64 * 16 +               // P^T fragments double buffer
         pos_mask_bytes(L, QTILES * 16, false) +           // table (16 B per entry) + mask
         (TPM == 2 ? (size_t)(L + QTILES * 16 + 32) * 16 : 0);   // the table's lo half
}

// TPM as zv_attn_stats_kernel (the two must score alike: this kernel normalises with the
// statistics that one wrote)
template <int SPLIT, int DTW, int QTILES, int TPM = 0>
__global__ __launch_bounds__(128 * QTILES) void zv_attn_na_kernel(FlashParams p) {
  constexpr int PLO = TPM == 2 ? 1 : 0;
  constexpr int NT = 128 * QTILES;
  constexpr int QT = 16 * QTILES;
  constexpr int NS = SPLIT == 3 ? 2 : 1;
  constexpr int VROWS = 8 * DTW * 16;                 // staged value channels
  constexpr int VTILE = VROWS * NA_VROW;              // bf16 per staged V^T tile (one half)
  constexpr int VCH = VROWS * (FA_KB / 8);            // 16-B chunks per tile
  constexpr int VPT = (VCH + NT - 1) / NT;
  constexpr int PFR = QTILES * 64 * 8;                // bf16 per P^T fragment set
  static_assert(QTILES % 4 == 0, "4 query tiles per accumulating wave");
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  const int L = p.L;
  bf16* Vs = reinterpret_cast<bf16*>(fsm);                        // [2][NS][VROWS][NA_VROW]
  bf16* Pf = Vs + (size_t)2 * NS * VTILE;                         // [2][NS][QTILES][64][8]
  const int NTB = L + QT + 32;                       // table entries
  f32x4* Ps = reinterpret_cast<f32x4*>(Pf + (size_t)2 * NS * PFR);
  bf16x8* PPh = reinterpret_cast<bf16x8*>(Ps);
  bf16x8* PPl = PPh + NTB;
  uint8_t* Ms = reinterpret_cast<uint8_t*>(Ps + NTB * (1 + PLO));
  const int nkb = (L + FA_KB - 1) / FA_KB;
  uint8_t* Fs = Ms + nkb * FA_KB;

  const int qt0 = blockIdx.x * QT, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const long qbase = (long)b * L * p.ldq;

  // scoring role
  const int sq = wave >> 1, hh = wave & 1;
  const int qi = qt0 + sq * 16 + (lane & 15);
  const int qc = min(qi, L - 1);
  bf16x8 qfh, qfl, pb[2];
  f32x2 pq[4];
  int tbl = 0;
  if constexpr (TPM) {
    for (int kb = tid; kb < nkb; kb += NT) Fs[kb] = 0;
    stage_tp<PLO>(p, 0, qt0, QT, NTB, PPh, PPl, tid, NT);
    stage_mask<FA_KB>(p, b, Ms, Fs, tid, NT);
    tp_query(p, qbase + (long)qc * p.ldq, 0, lane & 15, g, qt0 + sq * 16, qt0, QT, qfh, pb, tbl);
  } else {
    stage_pos_mask<false>(p, 0, b, qt0, QT, Ps, Ms, Fs, tid, NT);
    load_query<SPLIT>(p, qbase, qc, 0, g, qfh, qfl, pq);
  }
  const float2 st = p.stats[(long)b * L + qc];
  const float cst = -st.x + __builtin_amdgcn_logf(st.y);   // base 2: p = 2^(u - m) / sum
  const int nbase = qt0 + QT - 1 - qc;
  // accumulating role
  const int aq0 = (wave >> 3) * 4, ad0 = (wave & 7) * DTW;

  const bf16* vh = p.vh + (long)b * p.sv_b;
  const bf16* vl = (SPLIT == 3) ? p.vl + (long)b * p.sv_b : nullptr;
  const int nv = p.nv;
  bf16x8 vreg[NS][VPT];
  auto load_v = [&](int j0) {
#pragma unroll
    for (int c = 0; c < VPT; ++c) {
      const int idx = tid + c * NT;
      if (VCH % NT == 0 || idx < VCH) {
        const int row = idx / (FA_KB / 8), ch = idx % (FA_KB / 8);
        const int vr = row < nv ? row : nv - 1;       // pad rows: finite duplicates
        const long off = (long)vr * p.ldv + j0 + ch * 8;
        vreg[0][c] = *reinterpret_cast<const bf16x8*>(vh + off);
        if constexpr (SPLIT == 3) vreg[1][c] = *reinterpret_cast<const bf16x8*>(vl + off);
      }
    }
  };
  auto store_v = [&](int buf) {
#pragma unroll
    for (int c = 0; c < VPT; ++c) {
      const int idx = tid + c * NT;
      if (VCH % NT == 0 || idx < VCH) {
        const int row = idx / (FA_KB / 8), ch = idx % (FA_KB / 8);
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) {
          bf16* d = Vs + ((buf * NS + s2) * VROWS + row) * NA_VROW + ch * 8;
          const bf16x8 v = vreg[s2][c];
          *reinterpret_cast<bf16x4*>(d) = bf16x4{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<bf16x4*>(d + 4) = bf16x4{v[4], v[5], v[6], v[7]};
        }
      }
    }
  };

  f32x4 acc[4][DTW];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int t = 0; t < DTW; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // score this wave's 16 x 16 quarter of key step ks -> P^T fragment slots 4hh..4hh+3
  auto score_step = [&](int ks, const bf16x8& kfh, const bf16x8& kfl) {
    const int j0 = ks * FA_KB;
    float u[4];
    const int jq = j0 + hh * 16 + g * 4;
    if constexpr (TPM) {
      f32x4 s = tp_score<PLO>(PPh, PPl, j0 + hh * 16 + tbl, pb, kfh, qfh);
      if (Fs[ks]) mask4n(Ms, jq, s);
#pragma unroll
      for (int r = 0; r < 4; ++r) u[r] = s[r] * FA_LOG2E;
    } else {
      const f32x4 s = score_tile<SPLIT>(kfh, kfl, qfh, qfl);
      pos4<false>(s, Ps, nbase + jq, pq, u);
      if (Fs[ks]) mask4(Ms, jq, u);
    }
    bf16x4 ph, pl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pr = __builtin_amdgcn_exp2f(u[r] + cst);
      ph[r] = (bf16)pr;
      if constexpr (SPLIT == 3) pl[r] = (bf16)(pr - (float)ph[r]);
    }
    bf16* pdst = Pf + (size_t)((ks & 1) * NS) * PFR + (sq * 64 + lane) * 8 + hh * 4;
    *reinterpret_cast<bf16x4*>(pdst) = ph;
    if constexpr (SPLIT == 3) *reinterpret_cast<bf16x4*>(pdst + PFR) = pl;
  };
  // P^T(ks) . V^T(ks) into this wave's 4 query tiles x DTW value tiles
  auto accumulate_step = [&](int ks) {
    const int buf = ks & 1;
    const bf16* vb = Vs + (size_t)(buf * NS) * VTILE;
    bf16x8 va[NS][DTW];
#pragma unroll
    for (int t = 0; t < DTW; ++t) {
      const bf16* row = vb + ((ad0 + t) * 16 + (lane & 15)) * NA_VROW;
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) {
        const bf16x4 lo4 = *reinterpret_cast<const bf16x4*>(row + s2 * VTILE + g * 4);
        const bf16x4 hi4 = *reinterpret_cast<const bf16x4*>(row + s2 * VTILE + 16 + g * 4);
        va[s2][t] = bf16x8{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
      }
    }
    const bf16* pbuf = Pf + (size_t)(buf * NS) * PFR;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bf16x8 pbh = *reinterpret_cast<const bf16x8*>(pbuf + ((aq0 + q) * 64 + lane) * 8);
      bf16x8 pbl;
      if constexpr (SPLIT == 3)
        pbl = *reinterpret_cast<const bf16x8*>(pbuf + PFR + ((aq0 + q) * 64 + lane) * 8);
#pragma unroll
      for (int t = 0; t < DTW; ++t) {
        if constexpr (SPLIT == 3) {
          acc[q][t] = ZV_MFMA_16x16x32(va[1][t], pbh, acc[q][t], 0, 0, 0);
          acc[q][t] = ZV_MFMA_16x16x32(va[0][t], pbl, acc[q][t], 0, 0, 0);
        }
        acc[q][t] = ZV_MFMA_16x16x32(va[0][t], pbh, acc[q][t], 0, 0, 0);
      }
    }
  };

  // Software-pipelined key loop: iteration ks scores step ks+1 (its K fragment loaded one
  // iteration ahead) and stages V^T(ks+1) while it accumulates step ks, so the scoring's
  // exp / VALU work and the P.V MFMAs of the same wave are independent and interleave;
  // one barrier per iteration makes P^T(ks+1) / V^T(ks+1) visible and frees the step-ks
  // buffers for iteration ks+1's writes.
  bf16x8 kh, kl, nh, nl;
  load_kfrag<SPLIT>(p, qbase, 0, hh * 16 + (lane & 15), g, kh, kl);
  load_v(0);
  store_v(0);
  __syncthreads();   // staged slice / mask visible to the scoring
  score_step(0, kh, kl);
  if (nkb > 1) {
    load_kfrag<SPLIT>(p, qbase, 0, FA_KB + hh * 16 + (lane & 15), g, kh, kl);
    load_v(FA_KB);
  }
  __syncthreads();   // P^T(0), V^T(0) visible
  for (int kb = 0; kb < nkb; ++kb) {
    if (kb + 1 < nkb) {
      score_step(kb + 1, kh, kl);
      store_v((kb + 1) & 1);       // that slot was last read in iteration kb-1 (before its barrier)
      if (kb + 2 < nkb) {
        load_kfrag<SPLIT>(p, qbase, 0, (kb + 2) * FA_KB + hh * 16 + (lane & 15), g, nh, nl);
        load_v((kb + 2) * FA_KB);
        kh = nh; kl = nl;
      }
    }
    accumulate_step(kb);
    __syncthreads();
  }

  // ---- epilogue: lane holds out[query qt0 + 16 (aq0+q) + (lane&15)][d = 16 (ad0+t) + 4g + r]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int qo = qt0 + (aq0 + q) * 16 + (lane & 15);
    if (qo >= L) continue;
    const long orow = (long)b * L + qo;
#pragma unroll
    for (int t = 0; t < DTW; ++t) {
      const int d0 = (ad0 + t) * 16 + g * 4;
      if (d0 >= nv) continue;
      float v[4] = {acc[q][t][0], acc[q][t][1], acc[q][t][2], acc[q][t][3]};
      float y[4];
      load_split4(p.mulh, p.mull, orow * p.ldmul + d0, y);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= y[e];
      store_split4(p.oh, SPLIT == 3 ? p.ol : nullptr, orow * p.ldo + d0, v);
    }
  }
}

// ---------------------------------------------------------------------------
// SelfAttention consumer (online softmax, one head per block, 4 waves x QPW
// query tiles, 64 keys per step).  Nothing but the positional slice goes
// through LDS: each wave reads its K and V^T fragments straight from L2 one step
// ahead (shared by its QPW query tiles), so the key loop has no barriers.
// ---------------------------------------------------------------------------
constexpr int SA_QPW = 2;            // query tiles per wave (4: same time, more registers)
constexpr int SA_QT = 64 * SA_QPW;   // queries per block
constexpr int SA_KS = 64;            // keys per step (two 32-key P^T.V products)
constexpr float SA_RESCALE = 8.f;    // rescale when the running max grows by > 2^8

__host__ __device__ inline size_t sa_lds_bytes(int L) {
  return pos_mask_bytes(L, SA_QT, true, SA_KS);
}

template <int SPLIT>
__global__ __launch_bounds__(256) void zv_attn_sa_kernel(FlashParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  const int L = p.L;
  const int nks = (L + SA_KS - 1) / SA_KS;
  f32x4* Ps2 = reinterpret_cast<f32x4*>(fsm);
  uint8_t* Ms = reinterpret_cast<uint8_t*>(Ps2 + 2 * (L + SA_QT + SA_KS));
  uint8_t* Fs = Ms + nks * SA_KS;

  const int qt0 = blockIdx.x * SA_QT;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const long qbase = (long)b * L * p.ldq;
  const int nv = p.nv;                                  // <= 12: row 12 is the ones row
  stage_pos_mask<true, SA_KS>(p, h, b, qt0, SA_QT, Ps2, Ms, Fs, tid, 256);

  int qi[SA_QPW], nbase[SA_QPW];
  bf16x8 qfh[SA_QPW], qfl[SA_QPW];
  f32x2 pq[SA_QPW][4];
#pragma unroll
  for (int qq = 0; qq < SA_QPW; ++qq) {
    qi[qq] = qt0 + (wave * SA_QPW + qq) * 16 + (lane & 15);
    const int qc = min(qi[qq], L - 1);
    load_query<SPLIT>(p, qbase, qc, h, g, qfh[qq], qfl[qq], pq[qq]);
    nbase[qq] = qt0 + SA_QT - 1 - qc;
  }

  // K fragment rows (32-bit element offsets within the item)
  const bf16* kbh = p.qh + qbase + p.H * ATT_QD + h * ATT_QD + g * 8;
  const bf16* kbl = (SPLIT == 3) ? p.ql + qbase + p.H * ATT_QD + h * ATT_QD + g * 8 : nullptr;
  const int ldq = (int)p.ldq;
  auto load_k = [&](int j, bf16x8& kh, bf16x8& kl) {
    const int off = min(j, L - 1) * ldq;
    kh = *reinterpret_cast<const bf16x8*>(kbh + off);
    if constexpr (SPLIT == 3) kl = *reinterpret_cast<const bf16x8*>(kbl + off);
  };
  // V^T fragment rows: d = lane & 15 (< nv: loaded; 12: ones; else zero)
  const int vrow = lane & 15;
  const bool vload = vrow < nv;
  const long voff = (long)b * p.sv_b + (long)(h * p.vrows_per_head + (vload ? vrow : 0)) * p.ldv;
  const bf16* vbh = p.vh + voff + g * 4;
  const bf16* vbl = (SPLIT == 3) ? p.vl + voff + g * 4 : nullptr;
  const bf16 vconst = (bf16)(vrow == 12 ? 1.f : 0.f);
  auto load_v = [&](int j, bf16x8& ah, bf16x8& al) {   // keys j + 4g.. and j + 16 + 4g..
    if (vload) {
      const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(vbh + j);
      const bf16x4 a1 = *reinterpret_cast<const bf16x4*>(vbh + j + 16);
      ah = bf16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      if constexpr (SPLIT == 3) {
        const bf16x4 b0 = *reinterpret_cast<const bf16x4*>(vbl + j);
        const bf16x4 b1 = *reinterpret_cast<const bf16x4*>(vbl + j + 16);
        al = bf16x8{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
      }
    } else {
      ah = bf16x8{vconst, vconst, vconst, vconst, vconst, vconst, vconst, vconst};
      const bf16 z = (bf16)0.f;
      al = bf16x8{z, z, z, z, z, z, z, z};
    }
  };

  f32x4 acc[SA_QPW];
  float mref[SA_QPW];
#pragma unroll
  for (int qq = 0; qq < SA_QPW; ++qq) { acc[qq] = f32x4{0.f, 0.f, 0.f, 0.f}; mref[qq] = -1e30f; }
  bf16x8 kh[4], kl[4], nkh[4], nkl[4];
  bf16x8 vah[2], val[2], nvah[2], nval[2];
#pragma unroll
  for (int t = 0; t < 4; ++t) load_k(t * 16 + (lane & 15), kh[t], kl[t]);
#pragma unroll
  for (int t = 0; t < 2; ++t) load_v(t * 32, vah[t], val[t]);
  __syncthreads();   // staged slice / mask
  for (int ks = 0; ks < nks; ++ks) {
    const int j0 = ks * SA_KS;
    const bool more = ks + 1 < nks;
    if (more) {
#pragma unroll
      for (int t = 0; t < 4; ++t) load_k(j0 + SA_KS + t * 16 + (lane & 15), nkh[t], nkl[t]);
#pragma unroll
      for (int t = 0; t < 2; ++t) load_v(j0 + SA_KS + t * 32, nvah[t], nval[t]);
    }
    const bool mpath = Fs[ks];
#pragma unroll
    for (int qq = 0; qq < SA_QPW; ++qq) {
      float u[16];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 s = score_tile<SPLIT>(kh[t], kl[t], qfh[qq], qfl[qq]);
        float v4[4];
        pos4<true>(s, Ps2, nbase[qq] + j0 + t * 16 + g * 4, pq[qq], v4);
        if (mpath) mask4(Ms, j0 + t * 16 + g * 4, v4);
#pragma unroll
        for (int r = 0; r < 4; ++r) u[t * 4 + r] = v4[r];
      }
      float ml = u[0];
#pragma unroll
      for (int e = 1; e < 16; ++e) ml = fmaxf(ml, u[e]);
      ml = qmax4(ml);
      if (ml > mref[qq] + SA_RESCALE) {    // per query (uniform across its 4 lane groups)
        acc[qq] = acc[qq] * __builtin_amdgcn_exp2f(mref[qq] - ml);
        mref[qq] = ml;
      }
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {     // keys j0 + 32 hf: tiles 2hf (slots 0-3), 2hf+1 (4-7)
        bf16x8 pbh, pbl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float pr = __builtin_amdgcn_exp2f(u[hf * 8 + e] - mref[qq]);
          const bf16 ph = (bf16)pr;
          pbh[e] = ph;
          if constexpr (SPLIT == 3) pbl[e] = (bf16)(pr - (float)ph);
        }
        if constexpr (SPLIT == 3) {
          acc[qq] = ZV_MFMA_16x16x32(val[hf], pbh, acc[qq], 0, 0, 0);
          acc[qq] = ZV_MFMA_16x16x32(vah[hf], pbl, acc[qq], 0, 0, 0);
        }
        acc[qq] = ZV_MFMA_16x16x32(vah[hf], pbh, acc[qq], 0, 0, 0);
      }
    }
    if (more) {
#pragma unroll
      for (int t = 0; t < 4; ++t) { kh[t] = nkh[t]; kl[t] = nkl[t]; }
#pragma unroll
      for (int t = 0; t < 2; ++t) { vah[t] = nvah[t]; val[t] = nval[t]; }
    }
  }
  // acc rows: d = 4g + r; the denominator is row 12 (lane group 3, r = 0)
#pragma unroll
  for (int qq = 0; qq < SA_QPW; ++qq) {
    const float den = __shfl(acc[qq][0], 48 + (lane & 15), 64);
    const int d0 = g * 4;
    if (qi[qq] >= L || d0 >= nv) continue;
    const float rden = 1.f / den;
    float v[4] = {acc[qq][0] * rden, acc[qq][1] * rden, acc[qq][2] * rden, acc[qq][3] * rden};
    const long o = ((long)b * L + qi[qq]) * p.ldo + (long)h * p.ocol_per_head + d0;
    if (d0 + 3 < nv) {
      store_split4(p.oh, SPLIT == 3 ? p.ol : nullptr, o, v);
    } else {
      for (int e = 0; d0 + e < nv; ++e) split_store(p.oh, SPLIT == 3 ? p.ol : nullptr, o + e, v[e]);
    }
  }
}

// ---------------------------------------------------------------------------
// SelfAttention consumer with the rank-4 positional term folded into the score MFMA
// chain as a Toeplitz product (16-bit operand modes).  For a 16-key x 16-query S^T tile
// (keys j = jt + m, queries i = i0 + c) the term is pos[m][c] = sum_d pq_c[d] P[n][d],
// n = L-1-i+j, i.e. the table row depends on m - c only.  With K = 32 = 8 shifts x 4 dims:
//   A[m][(s, d)] = P[n0 + m - 8hf - s][d]      (table rows, one 16-B LDS read per lane)
//   B[(s, d)][c] = pq_c[d] if c == 8hf + s else 0   (built once per query tile)
// two MFMAs (hf = 0, 1: shifts 0-7 and 8-15) add the exact positional term for all 16
// queries into the q.k accumulator, so the loop's VALU work is the softmax alone:
// one fma + v_exp_f32 per score, the row max and the bf16 P conversion.  The table is
// staged as PP[t] = {P[n], P[n-1]} (n = nlo + t) in the operand format; PLO = 1 adds
// the table's lo half (a second pair of MFMAs) for the mixed-precision mode.
// ---------------------------------------------------------------------------
template <int PLO>
__host__ __device__ inline size_t sa_tp_lds_bytes(int L) {
  const int nks = (L + SA_KS - 1) / SA_KS;
  return (size_t)(L + SA_QT + SA_KS) * 16 * (1 + PLO) + (size_t)nks * SA_KS * 4 + round_up(nks, 16);
}

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// key mask as fp16 pairs Mh[j] = {mul, add}, applied as s = fma(s, mul, add) (one
// v_fma_mix_f32 per score): keep {1, 0} (exact), masked {0, -1000} (the reference's
// masked_fill(-1000)), beyond L {0, -inf}; one flag per KS-key step.  The caller zeroed Fs.
template <int KS>
__device__ __forceinline__ void stage_mask_h(const FlashParams& p, int b, unsigned* Mh, uint8_t* Fs,
                                             int tid, int nt) {
  const int L = p.L;
  const int NM = ((L + KS - 1) / KS) * KS;
  __syncthreads();   // Fs zeroed before the mask pass flags steps
  const uint8_t* kp = p.key_pad ? p.key_pad + (long)b * L : nullptr;
  for (int t = tid; t < NM; t += nt) {
    const int m = (t >= L) ? 2 : (kp ? kp[t] : 0);
    const h16x2 v = m == 0 ? h16x2{(_Float16)1.f, (_Float16)0.f}
                           : h16x2{(_Float16)0.f, m == 1 ? (_Float16)-1000.f : (_Float16)-INFINITY};
    Mh[t] = __builtin_bit_cast(unsigned, v);
    if (m) Fs[t / KS] = 1;
  }
}

// mask the 4 natural-unit scores of keys jq..jq+3 (jq a multiple of 4: one 16-B read).
// Read as 8 halves: hipcc (ROCm 7.2) miscompiles the same read as 4 dwords each
// bit_cast to a half pair, keeping only the first dword for all four keys.
__device__ __forceinline__ void mask4h(const unsigned* Mh, int jq, f32x4& s) {
  const h16x8 m = *reinterpret_cast<const h16x8*>(Mh + jq);
#pragma unroll
  for (int r = 0; r < 4; ++r) s[r] = fmaf(s[r], (float)m[2 * r], (float)m[2 * r + 1]);
}

// MINW 2: the compiler's register budget for 2 waves per SIMD keeps every score in VGPRs
// (MINW 1 parks them in AGPRs and copies them back for the softmax); both land at 3
// waves per SIMD.  The key loop is unrolled by two steps so the next step's K/V operands
// land in the other register set (no copies) and every global load of a step is
// unconditional (exact vmcnt accounting): the softmax VALU is what bounds this loop.
template <int PLO, int MINW = 2>
__global__ __launch_bounds__(256, MINW) void zv_attn_sa_tp_kernel(FlashParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  const int L = p.L;
  const int nks = (L + SA_KS - 1) / SA_KS;
  const int NT = L + SA_QT + SA_KS;
  bf16x8* PPh = reinterpret_cast<bf16x8*>(fsm);
  bf16x8* PPl = PPh + NT;
  unsigned* Mh = reinterpret_cast<unsigned*>(PPh + (1 + PLO) * NT);
  uint8_t* Fs = reinterpret_cast<uint8_t*>(Mh + nks * SA_KS);

  const int qt0 = blockIdx.x * SA_QT;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const long qbase = (long)b * L * p.ldq;
  const int nv = p.nv;

  for (int kb = tid; kb < nks; kb += 256) Fs[kb] = 0;
  stage_tp<PLO>(p, h, qt0, SA_QT, NT, PPh, PPl, tid, 256);
  stage_mask_h<SA_KS>(p, b, Mh, Fs, tid, 256);

  int qi[SA_QPW], tbl[SA_QPW];
  bf16x8 qf[SA_QPW], pb[SA_QPW][2];
#pragma unroll
  for (int qq = 0; qq < SA_QPW; ++qq) {
    const int i0 = qt0 + (wave * SA_QPW + qq) * 16;
    qi[qq] = i0 + c16;
    const long qrow = qbase + (long)min(qi[qq], L - 1) * p.ldq;
    tp_query(p, qrow, h, c16, g, i0, qt0, SA_QT, qf[qq], pb[qq], tbl[qq]);
  }

  const bf16* kb_ = p.qh + qbase + p.H * ATT_QD + h * ATT_QD + g * 8;
  const int ldq = (int)p.ldq;
  // this lane's key row within a 16-key tile; rows clamp to L - 1 (masked keys) with one
  // min and a full-rate 24-bit multiply, branch-free: a fast/slow path split here loses the
  // compiler's count of outstanding loads at the join and it over-waits on the prefetch
  const bf16* krow = kb_ + (long)c16 * ldq;
  const int klast = L - 1 - c16;
  auto load_k = [&](int j) { return *reinterpret_cast<const bf16x8*>(kb_ + min(j, L - 1) * ldq); };
  const int vrow = c16;
  const bool vload = vrow < nv;
  const long voff = (long)b * p.sv_b + (long)(h * p.vrows_per_head + (vload ? vrow : 0)) * p.ldv;
  const bf16* vb_ = p.vh + voff + g * 4;
  // keys j + 4g.. and j + 16 + 4g..  Every lane loads (rows past nv read row 0) and
  // rows >= nv then take their constant (row 12 ones: the softmax denominator) through
  // (w & vmask) | vbits with a mask the compiler cannot see through: it would otherwise
  // turn the select into a branch around the load, lose count of the step's loads and
  // make the first MFMA of every step wait for the next step's prefetch.
  const bf16x2 vc2 = {(bf16)(vrow == 12 ? 1.f : 0.f), (bf16)(vrow == 12 ? 1.f : 0.f)};
  const unsigned vbits = vload ? 0u : __builtin_bit_cast(unsigned, vc2);
  unsigned vmask;
  asm volatile("v_mov_b32 %0, %1" : "=v"(vmask) : "v"(vload ? ~0u : 0u));
  auto load_v = [&](int j) -> bf16x8 {
    const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(vb_ + j);
    const bf16x4 a1 = *reinterpret_cast<const bf16x4*>(vb_ + j + 16);
    return bf16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  };
  auto vfix = [&](const bf16x8& v) -> bf16x8 {   // applied at the use, one step later
    const u32x4 w = (__builtin_bit_cast(u32x4, v) & vmask) | vbits;
    return __builtin_bit_cast(bf16x8, w);
  };

  f32x4 acc[SA_QPW];
  float mref[SA_QPW];
#pragma unroll
  for (int qq = 0; qq < SA_QPW; ++qq) { acc[qq] = f32x4{0.f, 0.f, 0.f, 0.f}; mref[qq] = -1e30f; }
  bf16x8 kA[4], kB[4], vA[2], vB[2];
#pragma unroll
  for (int t = 0; t < 4; ++t) kA[t] = load_k(t * 16 + c16);
#pragma unroll
  for (int t = 0; t < 2; ++t) vA[t] = load_v(t * 32);
  __syncthreads();   // staged table / mask

  auto step = [&](int ks, const bf16x8 (&kf)[4], const bf16x8 (&vf)[2], bf16x8 (&nkf)[4],
                  bf16x8 (&nvf)[2]) {
    const int j0 = ks * SA_KS;
    {   // next step's operands, unconditionally (the last step re-reads itself)
      const int jn = min(j0 + SA_KS, (nks - 1) * SA_KS);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        nkf[t] = *reinterpret_cast<const bf16x8*>(krow + __mul24(min(jn + t * 16, klast), ldq));
#pragma unroll
      for (int t = 0; t < 2; ++t) nvf[t] = load_v(jn + t * 32);
    }
    const bool mpath = Fs[ks];
#pragma unroll
    for (int qq = 0; qq < SA_QPW; ++qq) {
      f32x4 st[4];
      bf16x8 ta[4][2], tl[4][2];     // all table operands of the step in flight at once
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ix = j0 + t * 16 + tbl[qq];
        ta[t][0] = PPh[ix];
        ta[t][1] = PPh[ix - 8];
        if constexpr (PLO) { tl[t][0] = PPl[ix]; tl[t][1] = PPl[ix - 8]; }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 sc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (PLO) {
          sc = ZV_MFMA_16x16x32(tl[t][0], pb[qq][0], sc, 0, 0, 0);
          sc = ZV_MFMA_16x16x32(tl[t][1], pb[qq][1], sc, 0, 0, 0);
        }
        st[t] = ZV_MFMA_16x16x32(kf[t], qf[qq], sc, 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) st[t] = ZV_MFMA_16x16x32(ta[t][0], pb[qq][0], st[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) st[t] = ZV_MFMA_16x16x32(ta[t][1], pb[qq][1], st[t], 0, 0, 0);
      if (mpath) {
#pragma unroll
        for (int t = 0; t < 4; ++t) mask4h(Mh, j0 + t * 16 + g * 4, st[t]);
      }
      float ml = st[0][0];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) ml = fmaxf(ml, st[t][r]);
      ml = qmax4(ml) * FA_LOG2E;
      if (ml > mref[qq] + SA_RESCALE) {    // per query (uniform across its 4 lane groups)
        acc[qq] = acc[qq] * __builtin_amdgcn_exp2f(mref[qq] - ml);
        mref[qq] = ml;
      }
      const float nm = -mref[qq];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {     // keys j0 + 32 hf: tiles 2hf (slots 0-3), 2hf+1 (4-7)
        bf16x8 pbv;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          pbv[e] = (bf16)__builtin_amdgcn_exp2f(fmaf(st[2 * hf + (e >> 2)][e & 3], FA_LOG2E, nm));
        acc[qq] = ZV_MFMA_16x16x32(vfix(vf[hf]), pbv, acc[qq], 0, 0, 0);
      }
    }
  };
  int ks = 0;
  for (; ks + 1 < nks; ks += 2) {
    step(ks, kA, vA, kB, vB);
    step(ks + 1, kB, vB, kA, vA);
  }
  if (ks < nks) step(ks, kA, vA, kB, vB);
#pragma unroll
  for (int qq = 0; qq < SA_QPW; ++qq) {
    const float den = __shfl(acc[qq][0], 48 + c16, 64);
    const int d0 = g * 4;
    if (qi[qq] >= L || d0 >= nv) continue;
    const float rden = 1.f / den;
    float v[4] = {acc[qq][0] * rden, acc[qq][1] * rden, acc[qq][2] * rden, acc[qq][3] * rden};
    const long o = ((long)b * L + qi[qq]) * p.ldo + (long)h * p.ocol_per_head + d0;
    if (d0 + 3 < nv) {
      store_split4(p.oh, p.ol, o, v);
      if (p.oh2) store_split4(p.oh2, nullptr, o, v);
    } else {
      for (int e = 0; d0 + e < nv; ++e) {
        split_store(p.oh, p.ol, o + e, v[e]);
        if (p.oh2) split_store(p.oh2, nullptr, o + e, v[e]);
      }
    }
  }
}


// ---------------------------------------------------------------------------
template <int SPLIT, int TPM = 0>
static void launch_attn_stats(const FlashParams& p, hipStream_t s) {
  static_assert(SPLIT == 1 || TPM == 0, "Toeplitz scoring is the 16-bit modes' form");
  dim3 grid(cdiv(p.L, 64), 1, p.B);
  const size_t lds = pos_mask_bytes(p.L, 64, true);
  ZV_REQUIRE(lds <= 160 * 1024, "sequence too long for the attention kernels");
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_attn_stats_kernel<SPLIT, TPM>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr |= 1ull << zv_cur_device();
  }
  ZvProfScope prof(SPLIT == 3 ? "attn_stats_fp32" : "attn_stats_bf16",
                   72.0 * p.B * (double)p.L * p.L, 0.0, s);
  g_zv_last_attn = {0, SPLIT, 0, 0, TPM, (int)grid.x, (int)grid.y, (int)grid.z};
  hipLaunchKernelGGL((zv_attn_stats_kernel<SPLIT, TPM>), grid, dim3(256), lds, s, p);
  ZV_LAUNCH_CHECK();
}

template <int SPLIT, int DTW, int QTILES, int TPM = 0>
static void launch_attn_na(const FlashParams& p, hipStream_t s) {
  static_assert(SPLIT == 1 || TPM == 0, "Toeplitz scoring is the 16-bit modes' form");
  const size_t lds = na_lds_bytes<SPLIT, DTW, QTILES, TPM>(p.L);
  ZV_REQUIRE(lds <= 160 * 1024, "sequence too long for the fused attention kernel");
  ZV_REQUIRE(p.nv <= 8 * DTW * 16, "value width exceeds the kernel's channel tiles");
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_attn_na_kernel<SPLIT, DTW, QTILES, TPM>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr |= 1ull << zv_cur_device();
  }
  dim3 grid(cdiv(p.L, 16 * QTILES), 1, p.B);
  // algorithmic work: scores (72 flop) + P.V (2 nv flop) per (query, key)
  ZvProfScope prof(SPLIT == 3 ? "attn_na_fp32" : "attn_na_bf16",
                   (72.0 + 2.0 * p.nv) * p.B * (double)p.L * p.L, 0.0, s);
  g_zv_last_attn = {1, SPLIT, DTW, QTILES, TPM, (int)grid.x, (int)grid.y, (int)grid.z};
  hipLaunchKernelGGL((zv_attn_na_kernel<SPLIT, DTW, QTILES, TPM>), grid, dim3(128 * QTILES), lds, s, p);
  ZV_LAUNCH_CHECK();
}

// the first-generation NonlinAttention consumer by the hidden width (the engine's layers and
// zv_attn_check launch it through here)
template <int SPLIT, int TPM>
static void attn_na_v1(const FlashParams& f, int hid, hipStream_t s) {
  constexpr int QTILES = SPLIT == 3 ? 4 : 8;
  if (hid <= 128) launch_attn_na<SPLIT, 1, QTILES, TPM>(f, s);
  else if (hid <= 256) launch_attn_na<SPLIT, 2, QTILES, TPM>(f, s);
  else launch_attn_na<SPLIT, 3, QTILES, TPM>(f, s);
}

template <int SPLIT>
static void launch_attn_sa(const FlashParams& p, hipStream_t s) {
  const size_t lds = sa_lds_bytes(p.L);
  ZV_REQUIRE(lds <= 160 * 1024, "sequence too long for the fused attention kernel");
  ZV_REQUIRE(p.nv <= 12, "value_head_dim > 12 unsupported by the fused kernel (row 12 = ones)");
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_attn_sa_kernel<SPLIT>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr |= 1ull << zv_cur_device();
  }
  dim3 grid(cdiv(p.L, SA_QT), p.H, p.B);
  ZvProfScope prof(SPLIT == 3 ? "attn_sa_fp32" : "attn_sa_bf16",
                   (72.0 + 2.0 * p.nv) * p.H * p.B * (double)p.L * p.L, 0.0, s);
  g_zv_last_attn = {2, SPLIT, 0, 0, 0, (int)grid.x, (int)grid.y, (int)grid.z};
  hipLaunchKernelGGL((zv_attn_sa_kernel<SPLIT>), grid, dim3(256), lds, s, p);
  ZV_LAUNCH_CHECK();
}

template <int PLO, int MINW = 2>
static void launch_attn_sa_tp(const FlashParams& p, hipStream_t s) {
  const size_t lds = sa_tp_lds_bytes<PLO>(p.L);
  ZV_REQUIRE(lds <= 160 * 1024, "sequence too long for the fused attention kernel");
  ZV_REQUIRE(p.nv <= 12, "value_head_dim > 12 unsupported by the fused kernel (row 12 = ones)");
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_attn_sa_tp_kernel<PLO, MINW>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr |= 1ull << zv_cur_device();
  }
  dim3 grid(cdiv(p.L, SA_QT), p.H, p.B);
  ZvProfScope prof("attn_sa_bf16", (72.0 + 2.0 * p.nv) * p.H * p.B * (double)p.L * p.L, 0.0, s);
  g_zv_last_attn = {3, 1, PLO, MINW, 1, (int)grid.x, (int)grid.y, (int)grid.z};
  hipLaunchKernelGGL((zv_attn_sa_tp_kernel<PLO, MINW>), grid, dim3(256), lds, s, p);
  ZV_LAUNCH_CHECK();
}


// Whether the fused consumers' LDS images (positional slice of length ~L + the
// staged V^T / P^T tiles) fit one workgroup for this sequence length; past that
// (fp32-accurate mode beyond L ~ 2.9k, bf16 beyond ~4.7k) a layer falls back to
// the W-materialising path (zv_attn.inc), which has no length limit but writes
// H x B x L x L_pad weights.  It sizes the kernels the layer will launch: the
// SelfAttention consumer (sa_plo < 0: zv_attn_sa_kernel, else zv_attn_sa_tp_kernel<sa_plo>),
// the NonlinAttention consumer with its scoring form (tpm) and the head-0 statistics.
template <int SPLIT>
static size_t na_lds_bytes_for(int L, int nv_na, int tpm) {
  constexpr int QT_NA = SPLIT == 3 ? 4 : 8;
  if (tpm == 2)
    return nv_na <= 128 ? na_lds_bytes<SPLIT, 1, QT_NA, 2>(L)
           : nv_na <= 256 ? na_lds_bytes<SPLIT, 2, QT_NA, 2>(L) : na_lds_bytes<SPLIT, 3, QT_NA, 2>(L);
  return nv_na <= 128 ? na_lds_bytes<SPLIT, 1, QT_NA>(L)
         : nv_na <= 256 ? na_lds_bytes<SPLIT, 2, QT_NA>(L) : na_lds_bytes<SPLIT, 3, QT_NA>(L);
}
template <int SPLIT>
static bool fused_attn_fits(int L, int nv_na, int sa_plo = -1, int tpm = 0) {
  const size_t lim = 160 * 1024;
  const size_t sa = sa_plo < 0 ? sa_lds_bytes(L) : (sa_plo ? sa_tp_lds_bytes<1>(L) : sa_tp_lds_bytes<0>(L));
  return pos_mask_bytes(L, 64, true) <= lim && sa <= lim && na_lds_bytes_for<SPLIT>(L, nv_na, tpm) <= lim;
}
