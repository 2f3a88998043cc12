// Attention consumers, second generation (16-bit operand modes): scores in base 2 and no
// running maximum.
//
// What the first generation (zv_flash.inc) spends per score besides the exponential: the
// log2(e) scaling fma, the running row maximum (a max3 chain, two lane swaps, compare), the
// conditional accumulator rescale and -- in NonlinAttention -- a whole statistics pre-pass
// (zv_attn_stats_kernel) for the head-0 maximum and sum.  Counters on the C2 per-stream shape
// (profiles/r05_attn_sq_before.txt): SelfAttention issues 114 VALU per 16x64 unit against
// 14 MFMAs, 44 % of its wave cycles issue-stalled.
//
// Here:
//  * log2(e) is folded into the attention-score projection's k and p weight rows at load time
//    (zv_engine: attn_b2), so the MFMA chain q.k + pos(q, k) already yields log2(e) x score;
//  * p = 2^s is taken without subtracting a maximum.  softmax is shift-invariant, and fp32 /
//    bf16 cover 2^-126 .. 2^127: as long as every query's largest score sits in [-60, 100]
//    (base 2; the reference's training caps |score| at 25 natural units, 36 in base 2,
//    zipformer.py:1257-1269), every weight within 2^66 of the largest is a normal number and
//    the sums cannot overflow.  Each query's denominator (SelfAttention: the ones row of the
//    value tile; NonlinAttention: a per-lane sum) is checked at the end; a query outside
//    [2^-60, 2^100], or any non-finite accumulator, sends its wave (SelfAttention) or block
//    (NonlinAttention) through an exact path with the row maximum subtracted, so results are
//    correct for every input and fast for every realistic one;
//  * masks are additive: the MFMA chain starts from a per-key bias (0 keep, -1000 log2(e)
//    padded, -inf beyond L) on the steps that have one; every other step starts from zero;
//  * NonlinAttention needs no statistics pass: it accumulates p . V and sum(p) and divides at
//    the end (the stats kernel and its launch are gone);
//  * the value operand of SelfAttention comes straight from memory with 16 rows per head: the
//    value projection's weight is laid out [12 values | a zero-weight row with bias 1 | 3 zero
//    rows] per head (zv_engine: sa_vpad), so row 12 of V^T is exactly 1 (the softmax
//    denominator comes out of the P.V MFMA) with no per-lane fix-up;
//  * K and V fragments are buffer loads: a lane-constant offset plus a scalar step offset, keys
//    past L read as zero through the buffer's range check (their bias is -inf).
#pragma once
#include "zv_flash.inc"

constexpr float FA2_MASKED = -1000.f * 1.4426950408889634f;   // masked_fill(-1000), base 2
constexpr float FA2_DEN_LO = 8.673617379884035e-19f;          // 2^-60
constexpr float FA2_DEN_HI = 1.2676506002282294e30f;          // 2^100
constexpr int SA2_KS = 64;                                    // keys per SelfAttention step
// fp16 operands (the parity-grade mode's library): fp16's largest finite value is 2^16, so P cannot
// be 2^s of a raw score.  Each query takes an integer offset o = ceil(max of its scores over the first
// key step and over the step holding its own query tile) and the kernels form p = 2^(s - o): the MFMA
// chain starts from -o (+ the key bias), so the loop costs nothing more (the prologue: one more step's
// scores).  p stays finite while the query's later scores rise less than 16 above o;
// one that rises further overflows to inf, fails the range check and sends its wave / block through
// the exact path, as an out-of-range denominator does in bf16.  In bf16 (8 exponent bits) o = 0
constexpr bool FA2_OFS = std::is_same<bf16, _Float16>::value;
// (A/B builds: -DZV_FA2_DIAG=0 takes the offsets from the first key step alone)
#ifndef ZV_FA2_DIAG
#define ZV_FA2_DIAG 1
#endif

// per-key additive bias Mb[j] (0 keep, -1000 log2(e) padded, -inf beyond L) for j < nks * KS,
// and one flag per KS-key step (any bias in it).  Ends with a barrier.
template <int KS>
__device__ __forceinline__ void stage_bias2(const FlashParams& p, int b, float* Mb, uint8_t* Fs, int tid,
                                            int nt) {
  const int L = p.L, nks = (L + KS - 1) / KS, NM = nks * KS;
  for (int k = tid; k < nks; k += nt) Fs[k] = 0;
  __syncthreads();
  const uint8_t* kp = p.key_pad ? p.key_pad + (long)b * L : nullptr;
  for (int t = tid; t < NM; t += nt) {
    const int m = t >= L ? 2 : (kp ? kp[t] : 0);
    Mb[t] = m == 0 ? 0.f : (m == 1 ? FA2_MASKED : -INFINITY);
    if (m) Fs[t / KS] = 1;
  }
  __syncthreads();
}

// Workgroups are dealt round-robin over the 8 XCDs (block i -> XCD i % 8; observed, used for
// speed only).  Renumber so that each XCD gets a contiguous run of the logical block order: the
// blocks of one (utterance, head) -- which read the same K / V rows -- then share one XCD's L2
// instead of every XCD fetching every utterance's keys (the first generation's grid did that).
__device__ __forceinline__ int fa2_xcd_block(int i, int n) {
  const int q = n >> 3, rem = n & 7, x = i & 7, k = i >> 3;
  return x * q + min(x, rem) + k;
}

// the range check of one query: lo = its denominator under 2^-60, hi = over 2^100 (or NaN) or a
// non-finite accumulator
__device__ __forceinline__ void fa2_range(float den, const f32x4& a, bool& lo, bool& hi) {
  lo |= den < FA2_DEN_LO;
  hi |= !(den <= FA2_DEN_HI);
#pragma unroll
  for (int r = 0; r < 4; ++r) hi |= !(fabsf(a[r]) <= 3.4e38f);
}

// FA2_OFS: a query's offset, the integer ceiling of its largest score in one 64-key step (the
// lane's 16 scores of query c16, then the query's four lane groups)
__device__ __forceinline__ float fa2_step_offset(const f32x4 (&st)[4]) {
  float ml = st[0][0];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) ml = fmaxf(ml, st[t][r]);
  return ceilf(qmax4(ml));
}

// FA2_OFS: the key step whose maxima join step 0's in a query tile's offsets -- the step holding the
// tile, or, where every key of that step is masked (the padded tail of a shorter utterance), the last
// step before it with a key left (wave-uniform; Mb[j] == 0 marks a kept key)
template <int KS>
__device__ __forceinline__ int fa2_diag_step(const float* Mb, int ks, int lane) {
  while (ks > 0 && __builtin_amdgcn_ballot_w64(Mb[ks * KS + (lane % KS)] == 0.f) == 0) --ks;
  return ks;
}

// exact-path bookkeeping (one lane of the wave / block that takes it; the path is rare)
__device__ __forceinline__ void fa2_count(const FlashParams& p, bool lo, bool hi) {
  if (!p.fallback) return;
  if (lo) atomicAdd(p.fallback + 0, 1u);
  if (hi) atomicAdd(p.fallback + 1, 1u);
  atomicAdd(p.fallback + 2, 1u);
}

// ---------------------------------------------------------------------------
// SelfAttention (4 x 12-wide heads; one head per block, 4 waves x QPW query tiles of 16)
// ---------------------------------------------------------------------------
template <int QPW>
__host__ __device__ inline size_t sa2_lds_bytes(int L) {
  const int nks = (L + SA2_KS - 1) / SA2_KS;
  return (size_t)(L + 64 * QPW + SA2_KS) * 16 + (size_t)nks * SA2_KS * 4 + round_up(nks, 16);
}

// ABL (lab ablations, 0 in the engine): 1 no exponentials (p = s), 2 no positional MFMAs,
// 3 no P.V MFMAs (p folded into the accumulator by one add per score), 4 K and V of the first
// step reused for every step (no loads in the loop), 5 V of the first step reused (K loaded)
// PIPE: the key loop software-pipelined by one step: iteration ks issues the score MFMAs of
// step ks+1 beside the exponentials and P.V MFMAs of step ks (independent work in one basic
// block; the step's key bias always comes from LDS, zero where nothing is masked)
template <int QPW, int MINW = 2, int ABL = 0, int PIPE = 0>
__global__ __launch_bounds__(256, MINW) void zv_attn_sa2_kernel(FlashParams p) {
  constexpr int QT = 64 * QPW, KS = SA2_KS, NU = QPW + 3;
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  const int L = p.L;
  const int nks = (L + KS - 1) / KS;
  const int NT = L + QT + KS;
  bf16x8* PP = reinterpret_cast<bf16x8*>(fsm);
  float* Mb = reinterpret_cast<float*>(PP + NT);
  uint8_t* Fs = reinterpret_cast<uint8_t*>(Mb + nks * KS);

  // 1-D grid over (query block, head, utterance), query blocks fastest, XCD-grouped
  const int nqb = (L + QT - 1) / QT;
  const int lb = fa2_xcd_block(blockIdx.x, gridDim.x);
  const int qt0 = (lb % nqb) * QT, h = (lb / nqb) % p.H, b = lb / nqb / p.H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const long qbase = (long)b * L * p.ldq;

  stage_tp<0>(p, h, qt0, QT, NT, PP, nullptr, tid, 256);
  stage_bias2<KS>(p, b, Mb, Fs, tid, 256);

  int qi[QPW], tbl0 = 0;
  bf16x8 qf[QPW], pb[QPW][2];
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) {
    const int i0 = qt0 + (wave * QPW + qq) * 16;
    qi[qq] = i0 + c16;
    int t;
    tp_query(p, qbase + (long)min(qi[qq], L - 1) * p.ldq, h, c16, g, i0, qt0, QT, qf[qq], pb[qq], t);
    if (qq == 0) tbl0 = t;   // query tile qq's table index is tbl0 - 16 qq
  }
  // K rows of this head: lane-constant offset (key row c16 of a 16-key tile, dims 8g..8g+7),
  // scalar step offset; rows >= L are past the range: zero
  const int ldqb = (int)p.ldq * 2;
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16*>(p.qh + qbase + p.H * ATT_QD + h * ATT_QD), 0, (L - 1) * ldqb + 2 * ATT_QD, 0x00020000);
  const int vk = c16 * ldqb + g * 16;
  auto ldk = [&](int j) -> bf16x8 {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsK, vk, j * ldqb, 0));
  };
  // V^T rows of this head (16: 12 values, the ones row, 3 zero rows): keys j + 4g.. and j + 16 + 4g..
  const int ldvb = (int)p.ldv * 2;
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16*>(p.vh + (long)b * p.sv_b + (long)h * 16 * p.ldv), 0, 16 * ldvb, 0x00020000);
  const int vv = c16 * ldvb + g * 8;
  auto ldv = [&](int j) -> bf16x8 {
    const bf16x4 a0 = __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(rsV, vv, j * 2, 0));
    const bf16x4 a1 = __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(rsV, vv, j * 2 + 32, 0));
    return bf16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  };

  // scores of one 64-key step for every query tile (base 2, + the step's key bias if BIAS)
  // per-query offsets as the chains' initial value (-o, zero in bf16; FA2_OFS)
  f32x4 ofs[QPW], zofs[QPW];
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) { ofs[qq] = f32x4{0.f, 0.f, 0.f, 0.f}; zofs[qq] = ofs[qq]; }
  auto scores = [&](auto BIAS_, int j0, const bf16x8 (&kf)[4], f32x4 (&st)[QPW][4], const f32x4 (&of)[QPW]) {
    constexpr bool BIAS = decltype(BIAS_)::value;
    bf16x8 TA[NU], TB[NU];     // table operands shared by the query tiles (tile qq reads u = t - qq)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int ix = j0 + 16 * (u - (QPW - 1)) + tbl0;
      TA[u] = PP[ix];
      TB[u] = PP[ix - 8];
    }
    f32x4 c0[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      c0[t] = BIAS ? *reinterpret_cast<const f32x4*>(Mb + j0 + t * 16 + g * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 ci = FA2_OFS ? (BIAS ? c0[t] + of[qq] : of[qq]) : c0[t];
        f32x4 c = ZV_MFMA_16x16x32(kf[t], qf[qq], ci, 0, 0, 0);
        if constexpr (ABL != 2) {
          c = ZV_MFMA_16x16x32(TA[t - qq + QPW - 1], pb[qq][0], c, 0, 0, 0);
          c = ZV_MFMA_16x16x32(TB[t - qq + QPW - 1], pb[qq][1], c, 0, 0, 0);
        }
        st[qq][t] = c;
      }
  };
  auto pv = [&](const f32x4 (&st)[4], const bf16x8 (&vf)[2], float sub, f32x4& acc) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {     // keys j0 + 32 hf: tiles 2hf (slots 0-3), 2hf+1 (4-7)
      bf16x8 pbv;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        pbv[e] = (bf16)(ABL == 1 ? st[2 * hf + (e >> 2)][e & 3] - sub
                                 : __builtin_amdgcn_exp2f(st[2 * hf + (e >> 2)][e & 3] - sub));
      if constexpr (ABL == 3) {
        const f32x4 w = __builtin_bit_cast(f32x4, pbv);
        acc += w;
      } else {
        acc = ZV_MFMA_16x16x32(vf[hf], pbv, acc, 0, 0, 0);
      }
    }
  };

  // FA2_OFS: the per-query maxima of the step holding the wave's first query tile (taken with
  // step 0's for the offsets, as in sa3 below)
  float od[QPW];
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) od[qq] = -1e30f;
  if constexpr (FA2_OFS && !PIPE && ZV_FA2_DIAG) {
    const int jd = fa2_diag_step<KS>(Mb, min((qt0 + wave * QPW * 16) / KS, nks - 1), lane) * KS;
    bf16x8 kd[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) kd[t] = ldk(jd + t * 16);
    f32x4 sd[QPW][4];
    scores(std::true_type{}, jd, kd, sd, zofs);
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq) od[qq] = fa2_step_offset(sd[qq]);
  }
  f32x4 acc[QPW];
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) acc[qq] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 kA[4], kB[4], vA[2], vB[2];
#pragma unroll
  for (int t = 0; t < 4; ++t) kA[t] = ldk(t * 16);
#pragma unroll
  for (int t = 0; t < 2; ++t) vA[t] = ldv(t * 32);
  if constexpr (PIPE) {
    // registers: K(ks+1) in kf, K(ks+2) loading into nkf; V(ks) in vf, V(ks+1) loading into nvf;
    // scores of step ks in sc, of step ks+1 produced into sn
    const int last = (nks - 1) * KS;
#pragma unroll
    for (int t = 0; t < 4; ++t) kB[t] = ldk(min(KS, last) + t * 16);
    static_assert(!(PIPE && FA2_OFS), "the pipelined loop has no per-query offsets");
    f32x4 sA[QPW][4], sB[QPW][4];
    scores(std::true_type{}, 0, kA, sA, zofs);
    auto body = [&](int ks, const f32x4 (&sc)[QPW][4], f32x4 (&sn)[QPW][4], const bf16x8 (&kf)[4],
                    bf16x8 (&nkf)[4], const bf16x8 (&vf)[2], bf16x8 (&nvf)[2]) {
      const int j1 = min((ks + 1) * KS, last), j2 = min((ks + 2) * KS, last);
#pragma unroll
      for (int t = 0; t < 4; ++t) nkf[t] = ldk(j2 + t * 16);
#pragma unroll
      for (int t = 0; t < 2; ++t) nvf[t] = ldv(j1 + t * 32);
      scores(std::true_type{}, j1, kf, sn, zofs);
#pragma unroll
      for (int qq = 0; qq < QPW; ++qq) pv(sc[qq], vf, 0.f, acc[qq]);
    };
    int k2 = 0;
    for (; k2 + 1 < nks; k2 += 2) {
      body(k2, sA, sB, kB, kA, vA, vB);
      body(k2 + 1, sB, sA, kA, kB, vB, vA);
    }
    if (k2 < nks) body(k2, sA, sB, kB, kA, vA, vB);
  } else {

  auto step = [&](auto BIAS_, auto FIRST_, int ks, const bf16x8 (&kf)[4], const bf16x8 (&vf)[2],
                  bf16x8 (&nkf)[4], bf16x8 (&nvf)[2]) {
    const int j0 = ks * KS;
    const int jn = min(j0 + KS, (nks - 1) * KS);    // next step's operands (the last re-reads itself)
    if constexpr (ABL == 4 || ABL == 5) {
#pragma unroll
      for (int t = 0; t < 4; ++t) nkf[t] = ABL == 4 ? kf[t] : ldk(jn + t * 16);
#pragma unroll
      for (int t = 0; t < 2; ++t) nvf[t] = vf[t];
    } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) nkf[t] = ldk(jn + t * 16);
#pragma unroll
    for (int t = 0; t < 2; ++t) nvf[t] = ldv(jn + t * 32);
    }
    f32x4 st[QPW][4];
    scores(BIAS_, j0, kf, st, ofs);
    if constexpr (decltype(FIRST_)::value) {   // FA2_OFS, step 0 (offsets still zero): the offsets
#pragma unroll
      for (int qq = 0; qq < QPW; ++qq) {
        const float o = fmaxf(fa2_step_offset(st[qq]), od[qq]);
        ofs[qq] = f32x4{-o, -o, -o, -o};
        pv(st[qq], vf, o, acc[qq]);
      }
    } else {
#pragma unroll
      for (int qq = 0; qq < QPW; ++qq) pv(st[qq], vf, 0.f, acc[qq]);
    }
  };
  auto run = [&](int ks, const bf16x8 (&kf)[4], const bf16x8 (&vf)[2], bf16x8 (&nkf)[4], bf16x8 (&nvf)[2]) {
    if (__builtin_amdgcn_readfirstlane(Fs[ks])) step(std::true_type{}, std::false_type{}, ks, kf, vf, nkf, nvf);
    else step(std::false_type{}, std::false_type{}, ks, kf, vf, nkf, nvf);
  };
  if constexpr (FA2_OFS) {
    // step 0 peeled (it sets the offsets), then the same loop with the register sets swapped
    step(std::true_type{}, std::true_type{}, 0, kA, vA, kB, vB);
    int ks = 1;
    for (; ks + 1 < nks; ks += 2) {
      run(ks, kB, vB, kA, vA);
      run(ks + 1, kA, vA, kB, vB);
    }
    if (ks < nks) run(ks, kB, vB, kA, vA);
  } else {
    int ks = 0;
    for (; ks + 1 < nks; ks += 2) {
      run(ks, kA, vA, kB, vB);
      run(ks + 1, kB, vB, kA, vA);
    }
    if (ks < nks) run(ks, kA, vA, kB, vB);
  }
  }

  // the denominator is row 12 of the accumulator (lane group 3, r = 0)
  float den[QPW];
  bool lo = false, hi = false;
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) {
    den[qq] = __shfl(acc[qq][0], 48 + c16, 64);
    fa2_range(den[qq], acc[qq], lo, hi);
  }
  const bool any_lo = __builtin_amdgcn_ballot_w64(lo) != 0, any_hi = __builtin_amdgcn_ballot_w64(hi) != 0;
  if (any_lo || any_hi || p.force_exact) {
    if (lane == 0) fa2_count(p, any_lo, any_hi);
    // exact path (rare): online softmax with the row maximum subtracted, one step at a time
    float mref[QPW];
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq) { acc[qq] = f32x4{0.f, 0.f, 0.f, 0.f}; mref[qq] = -1e30f; }
    for (int k2 = 0; k2 < nks; ++k2) {
      const int j0 = k2 * KS;
      bf16x8 kf[4], vf[2];
#pragma unroll
      for (int t = 0; t < 4; ++t) kf[t] = ldk(j0 + t * 16);
#pragma unroll
      for (int t = 0; t < 2; ++t) vf[t] = ldv(j0 + t * 32);
      f32x4 st[QPW][4];
      scores(std::true_type{}, j0, kf, st, zofs);
#pragma unroll
      for (int qq = 0; qq < QPW; ++qq) {
        float ml = st[qq][0][0];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) ml = fmaxf(ml, st[qq][t][r]);
        // an integer maximum: rescaling the accumulator by 2^(mref - mn) is exact, and the
        // maximum's own p lies in (1/2, 1]
        const float mn = fmaxf(mref[qq], ceilf(qmax4(ml)));
        acc[qq] = acc[qq] * __builtin_amdgcn_exp2f(mref[qq] - mn);
        mref[qq] = mn;
        pv(st[qq], vf, mn, acc[qq]);
      }
    }
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq) den[qq] = __shfl(acc[qq][0], 48 + c16, 64);
  }

#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) {
    const int d0 = g * 4;
    if (qi[qq] >= L || d0 >= p.nv) continue;
    const float rden = 1.f / den[qq];
    float v[4] = {acc[qq][0] * rden, acc[qq][1] * rden, acc[qq][2] * rden, acc[qq][3] * rden};
    const long o = ((long)b * L + qi[qq]) * p.ldo + (long)h * p.ocol_per_head + d0;
    if (d0 + 3 < p.nv) {
      store_split4(p.oh, p.ol, o, v);
      if (p.oh2) store_split4(p.oh2, nullptr, o, v);
    } else {
      for (int e = 0; d0 + e < p.nv; ++e) {
        split_store(p.oh, p.ol, o + e, v[e]);
        if (p.oh2) split_store(p.oh2, nullptr, o + e, v[e]);
      }
    }
  }
}

template <int QPW = 2, int MINW = 2, int ABL = 0, int PIPE = 0>
static void launch_attn_sa2(const FlashParams& p, hipStream_t s) {
  const size_t lds = sa2_lds_bytes<QPW>(p.L);
  ZV_REQUIRE(lds <= 160 * 1024, "sequence too long for the fused attention kernel");
  ZV_REQUIRE(p.nv <= 12 && p.vrows_per_head == 16 && p.ldq % 8 == 0 && p.ldv % 4 == 0,
             "SelfAttention v2: 16-row value heads (row 12 = ones)");
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_attn_sa2_kernel<QPW, MINW, ABL, PIPE>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr |= 1ull << zv_cur_device();
  }
  const long nblk = (long)cdiv(p.L, 64 * QPW) * p.H * p.B;
  ZV_REQUIRE(nblk < (1L << 31), "SelfAttention v2 grid");
  ZvProfScope prof("attn_sa_bf16", (72.0 + 2.0 * p.nv) * p.H * p.B * (double)p.L * p.L, 0.0, s);
  hipLaunchKernelGGL((zv_attn_sa2_kernel<QPW, MINW, ABL, PIPE>), dim3((unsigned)nblk), dim3(256), lds, s, p);
  ZV_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------
// NonlinAttention (head 0, 384-wide values) without a statistics pass:
// out[q][d] = y[q][d] * sum_j 2^s[q][j] xt[d][j] / sum_j 2^s[q][j]
// QTILES query tiles per block (2 x QTILES waves); wave w scores query tile w >> 1, key half
// w & 1 of each 32-key step and keeps its lanes' running sum of p; it accumulates query tiles
// 4 (w >> 3) .. +3 times value tiles (w & 7) * DTW .. +DTW-1 from the P^T fragments the
// scoring waves left in LDS.
// ---------------------------------------------------------------------------
template <int DTW, int QTILES>
__host__ __device__ inline size_t na2_lds_bytes(int L) {
  return (size_t)2 * (8 * DTW * 16) * NA_VROW * 2 +   // V^T double buffer
         (size_t)2 * QTILES * 64 * 16 +                // P^T fragments double buffer
         (size_t)(L + QTILES * 16 + 32) * 16 +         // Toeplitz table
         (size_t)round_up(L, FA_KB) * 4 +              // key bias
         round_up((L + FA_KB - 1) / FA_KB, 16) +       // step flags
         (size_t)2 * QTILES * 16 * 4 + 16;             // per-query half sums / maxima, block flag
}

template <int DTW, int QTILES>
__global__ __launch_bounds__(128 * QTILES) void zv_attn_na2_kernel(FlashParams p) {
  constexpr int NT = 128 * QTILES;
  constexpr int QT = 16 * QTILES;
  constexpr int VROWS = 8 * DTW * 16;                 // staged value channels
  constexpr int VTILE = VROWS * NA_VROW;              // bf16 per staged V^T tile
  constexpr int VCH = VROWS * (FA_KB / 8);            // 16-B chunks per tile
  constexpr int VPT = (VCH + NT - 1) / NT;
  constexpr int PFR = QTILES * 64 * 8;                // bf16 per P^T fragment set
  static_assert(QTILES % 4 == 0, "4 query tiles per accumulating wave");
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  const int L = p.L;
  const int nkb = (L + FA_KB - 1) / FA_KB;
  const int NTB = L + QT + 32;                         // table entries
  bf16* Vs = reinterpret_cast<bf16*>(fsm);                              // [2][VROWS][NA_VROW]
  bf16* Pf = Vs + (size_t)2 * VTILE;                                     // [2][QTILES][64][8]
  bf16x8* PP = reinterpret_cast<bf16x8*>(Pf + (size_t)2 * PFR);          // [NTB]
  float* Mb = reinterpret_cast<float*>(PP + NTB);                       // [nkb * 32]
  uint8_t* Fs = reinterpret_cast<uint8_t*>(Mb + nkb * FA_KB);            // [nkb]
  float* Qs = reinterpret_cast<float*>(Fs + round_up(nkb, 16));         // [2][QT] half sums / maxima
  int* bflag = reinterpret_cast<int*>(Qs + 2 * QT);

  const int nqb = (L + QT - 1) / QT;
  const int lb = fa2_xcd_block(blockIdx.x, gridDim.x);   // query blocks fastest, XCD-grouped
  const int qt0 = (lb % nqb) * QT, b = lb / nqb;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const long qbase = (long)b * L * p.ldq;

  // scoring role
  const int sq = wave >> 1, hh = wave & 1;
  const int qi = qt0 + sq * 16 + c16;
  const int qc = min(qi, L - 1);
  bf16x8 qf, pb[2];
  int tbl = 0;
  if (tid == 0) *bflag = 0;
  stage_tp<0>(p, 0, qt0, QT, NTB, PP, nullptr, tid, NT);
  stage_bias2<FA_KB>(p, b, Mb, Fs, tid, NT);            // (barrier inside)
  tp_query(p, qbase + (long)qc * p.ldq, 0, c16, g, qt0 + sq * 16, qt0, QT, qf, pb, tbl);
  const int ldqb = (int)p.ldq * 2;
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16*>(p.qh + qbase + p.H * ATT_QD), 0, (L - 1) * ldqb + 2 * ATT_QD, 0x00020000);
  const int vk = (hh * 16 + c16) * ldqb + g * 16;
  auto ldk = [&](int j0) -> bf16x8 {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsK, vk, j0 * ldqb, 0));
  };
  // accumulating role
  const int aq0 = (wave >> 3) * 4, ad0 = (wave & 7) * DTW;
  const bf16* vh = p.vh + (long)b * p.sv_b;
  const int nv = p.nv;
  bf16x8 vreg[VPT];
  auto load_v = [&](int j0) {
#pragma unroll
    for (int c = 0; c < VPT; ++c) {
      const int idx = tid + c * NT;
      if (VCH % NT == 0 || idx < VCH) {
        const int row = idx / (FA_KB / 8), ch = idx % (FA_KB / 8);
        const int vr = row < nv ? row : nv - 1;       // pad rows: finite duplicates
        vreg[c] = *reinterpret_cast<const bf16x8*>(vh + (long)vr * p.ldv + j0 + ch * 8);
      }
    }
  };
  auto store_v = [&](int buf) {
#pragma unroll
    for (int c = 0; c < VPT; ++c) {
      const int idx = tid + c * NT;
      if (VCH % NT == 0 || idx < VCH) {
        const int row = idx / (FA_KB / 8), ch = idx % (FA_KB / 8);
        bf16* d = Vs + ((size_t)buf * VROWS + row) * NA_VROW + ch * 8;
        const bf16x8 v = vreg[c];
        *reinterpret_cast<bf16x4*>(d) = bf16x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<bf16x4*>(d + 4) = bf16x4{v[4], v[5], v[6], v[7]};
      }
    }
  };

  f32x4 acc[4][DTW];
  float psum = 0.f;
  f32x4 cofs = {0.f, 0.f, 0.f, 0.f};    // FA2_OFS fast path: -o of the lane's query, the chains' start
  // score this wave's 16 x 16 quarter of key step ks -> P^T fragment slots 4hh..4hh+3
  auto score_step = [&](int ks, const bf16x8& kf, float sub) {
    const int j0 = ks * FA_KB;
    const int jb = j0 + hh * 16;
    f32x4 c = __builtin_amdgcn_readfirstlane(Fs[ks]) ? *reinterpret_cast<const f32x4*>(Mb + jb + g * 4) + cofs
                                                     : cofs;
    c = ZV_MFMA_16x16x32(kf, qf, c, 0, 0, 0);
    c = ZV_MFMA_16x16x32(PP[jb + tbl], pb[0], c, 0, 0, 0);
    c = ZV_MFMA_16x16x32(PP[jb + tbl - 8], pb[1], c, 0, 0, 0);
    bf16x4 ph;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pr = __builtin_amdgcn_exp2f(c[r] - sub);
      psum += pr;
      ph[r] = (bf16)pr;
    }
    *reinterpret_cast<bf16x4*>(Pf + (size_t)(ks & 1) * PFR + (sq * 64 + lane) * 8 + hh * 4) = ph;
  };
  // P^T(ks) . V^T(ks) into this wave's 4 query tiles x DTW value tiles
  auto accumulate_step = [&](int ks) {
    const int buf = ks & 1;
    const bf16* vb = Vs + (size_t)buf * VTILE;
    bf16x8 va[DTW];
#pragma unroll
    for (int t = 0; t < DTW; ++t) {
      const bf16* row = vb + ((ad0 + t) * 16 + c16) * NA_VROW;
      const bf16x4 lo4 = *reinterpret_cast<const bf16x4*>(row + g * 4);
      const bf16x4 hi4 = *reinterpret_cast<const bf16x4*>(row + 16 + g * 4);
      va[t] = bf16x8{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
    }
    const bf16* pbuf = Pf + (size_t)buf * PFR;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bf16x8 pbh = *reinterpret_cast<const bf16x8*>(pbuf + ((aq0 + q) * 64 + lane) * 8);
#pragma unroll
      for (int t = 0; t < DTW; ++t) acc[q][t] = ZV_MFMA_16x16x32(va[t], pbh, acc[q][t], 0, 0, 0);
    }
  };
  // the whole key loop with p = 2^(s - sub) (sub: 0, or the row maximum on the exact path);
  // software-pipelined as the first generation: iteration ks scores step ks+1 and stages V^T(ks+1)
  // while it accumulates step ks; one barrier per iteration
  auto key_loop = [&](float sub) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int t = 0; t < DTW; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    psum = 0.f;
    bf16x8 kf = ldk(0), nk;
    load_v(0);
    store_v(0);
    score_step(0, kf, sub);
    if (nkb > 1) {
      kf = ldk(FA_KB);
      load_v(FA_KB);
    }
    __syncthreads();   // P^T(0), V^T(0) visible
    for (int kb = 0; kb < nkb; ++kb) {
      if (kb + 1 < nkb) {
        score_step(kb + 1, kf, sub);
        store_v((kb + 1) & 1);       // that slot was last read in iteration kb-1 (before its barrier)
        if (kb + 2 < nkb) {
          nk = ldk((kb + 2) * FA_KB);
          load_v((kb + 2) * FA_KB);
          kf = nk;
        }
      }
      accumulate_step(kb);
      __syncthreads();
    }
  };
  // per-query total over the two scoring waves of the query tile (lane groups first)
  auto half_sums = [&](float x, bool is_max) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float y = __shfl_xor(x, o, 64);
      x = is_max ? fmaxf(x, y) : x + y;
    }
    if (g == 0) Qs[hh * QT + sq * 16 + c16] = x;
    __syncthreads();
  };

  // FA2_OFS: the query's offset from key step 0 and the step holding the query tile itself (both
  // key halves; zero in bf16).  Step 0 alone left 4 of 204 blocks per utterance above fp16's range
  // at the C2 shape (a later score 16 over the offset), each an exact-path block on its CU; with the
  // diagonal step none (tools/offset_study.py, profiles/r06_offset_study.txt)
  float off = 0.f;
  if constexpr (FA2_OFS) {
    const int ksd = fa2_diag_step<FA_KB>(Mb, min((qt0 + sq * 16) / FA_KB, nkb - 1), lane);
    const bf16x8 k0 = ldk(0), kd = ldk(ksd * FA_KB);
    float ml = -1e30f;
#pragma unroll
    for (int e = 0; e < (ZV_FA2_DIAG ? 2 : 1); ++e) {
      const int jb = (e ? ksd * FA_KB : 0) + hh * 16;
      f32x4 c = *reinterpret_cast<const f32x4*>(Mb + jb + g * 4);
      c = ZV_MFMA_16x16x32(e ? kd : k0, qf, c, 0, 0, 0);
      c = ZV_MFMA_16x16x32(PP[jb + tbl], pb[0], c, 0, 0, 0);
      c = ZV_MFMA_16x16x32(PP[jb + tbl - 8], pb[1], c, 0, 0, 0);
      ml = fmaxf(ml, fmaxf(fmaxf(c[0], c[1]), fmaxf(c[2], c[3])));
    }
    half_sums(ml, true);
    off = ceilf(fmaxf(Qs[sq * 16 + c16], Qs[QT + sq * 16 + c16]));
    cofs = f32x4{-off, -off, -off, -off};
  }
  key_loop(0.f);
  half_sums(psum, false);
  // range check over the block's queries (both halves summed)
  // (bflag bit 0: a denominator under 2^-60, bit 1: over 2^100 or a non-finite accumulator)
  if (tid < QT) {
    const float den = Qs[tid] + Qs[QT + tid];
    if (qt0 + tid < L) {
      if (den < FA2_DEN_LO) atomicOr(bflag, 1);
      if (!(den <= FA2_DEN_HI)) atomicOr(bflag, 2);
    }
  }
  __syncthreads();
  bool nonfinite = false;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int t = 0; t < DTW; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) nonfinite |= !(fabsf(acc[q][t][r]) <= 3.4e38f);
  if (__builtin_amdgcn_ballot_w64(nonfinite) != 0 && lane == 0) atomicOr(bflag, 2);
  __syncthreads();
  const int bf = *bflag;
  if (bf || p.force_exact) {
    if (tid == 0) fa2_count(p, bf & 1, bf & 2);
    // exact path (rare): the head-0 row maximum first (scores only), then the loop again with
    // p = 2^(s - max)
    float mx = -1e30f;
    for (int ks = 0; ks < nkb; ++ks) {
      const int jb = ks * FA_KB + hh * 16;
      f32x4 c = *reinterpret_cast<const f32x4*>(Mb + jb + g * 4);
      c = ZV_MFMA_16x16x32(ldk(ks * FA_KB), qf, c, 0, 0, 0);
      c = ZV_MFMA_16x16x32(PP[jb + tbl], pb[0], c, 0, 0, 0);
      c = ZV_MFMA_16x16x32(PP[jb + tbl - 8], pb[1], c, 0, 0, 0);
      mx = fmaxf(mx, fmaxf(fmaxf(c[0], c[1]), fmaxf(c[2], c[3])));
    }
    half_sums(mx, true);
    // (an integer, as in SelfAttention)
    const float rowmax = ceilf(fmaxf(Qs[sq * 16 + c16], Qs[QT + sq * 16 + c16]));
    cofs = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    key_loop(rowmax);
    half_sums(psum, false);
  }

  // ---- epilogue: lane holds out[query qt0 + 16 (aq0+q) + c16][d = 16 (ad0+t) + 4g + r]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ql = (aq0 + q) * 16 + c16;
    const int qo = qt0 + ql;
    if (qo >= L) continue;
    const float rden = 1.f / (Qs[ql] + Qs[QT + ql]);
    const long orow = (long)b * L + qo;
#pragma unroll
    for (int t = 0; t < DTW; ++t) {
      const int d0 = (ad0 + t) * 16 + g * 4;
      if (d0 >= nv) continue;
      float v[4] = {acc[q][t][0], acc[q][t][1], acc[q][t][2], acc[q][t][3]};
      float y[4];
      load_split4(p.mulh, (const bf16*)nullptr, orow * p.ldmul + d0, y);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= y[e] * rden;
      store_split4(p.oh, nullptr, orow * p.ldo + d0, v);
    }
  }
}

// query tiles per NonlinAttention block: 4 up to 900 frames (more blocks where the 8-tile grid
// leaves CUs idle: lab 21 x 610 37.0 -> 27.4 us, 21 x 305 25.6 -> 17.8, 11 x 844 42.6 -> 30.7; past
// that the 8-tile form wins, 21 x 1219 60.2 vs 80.1; r05_attn_lab_na2q.txt).  By length only: the
// choice never depends on the batch
inline int na2_qtiles(int L) { return L <= 900 ? 4 : 8; }

template <int DTW, int QTILES = 8>
static void launch_attn_na2(const FlashParams& p, hipStream_t s) {
  const size_t lds = na2_lds_bytes<DTW, QTILES>(p.L);
  ZV_REQUIRE(lds <= 160 * 1024, "sequence too long for the fused attention kernel");
  ZV_REQUIRE(p.nv <= 8 * DTW * 16 && !p.ol && p.ldq % 8 == 0, "NonlinAttention v2 operands");
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_attn_na2_kernel<DTW, QTILES>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr |= 1ull << zv_cur_device();
  }
  const long nblk = (long)cdiv(p.L, 16 * QTILES) * p.B;
  ZvProfScope prof("attn_na_bf16", (72.0 + 2.0 * p.nv) * p.B * (double)p.L * p.L, 0.0, s);
  hipLaunchKernelGGL((zv_attn_na2_kernel<DTW, QTILES>), dim3((unsigned)nblk), dim3(128 * QTILES), lds, s, p);
  ZV_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------
// SelfAttention with the K / V tiles staged through LDS by DMA (global_load_lds_dwordx4), one
// copy per block instead of one per wave.  Measured on the register-fed form (attn_lab, B = 21,
// L = 1219): without the per-wave V loads the launch took 43 instead of 62 us, without K and V
// loads 39 us -- each wave re-fetching the same 16 rows x 64 keys through its own 16-line
// vector-memory requests was the cost, not the MFMAs or the exponentials.
//   K tile of a 64-key step: 4 fragment-major 1 KiB pieces (piece t = keys 16t..16t+15; lane l
//   of the piece holds key 16t + (l & 15), dims 8 (l >> 4)..+7: exactly the MFMA A operand, read
//   back lane-linear, conflict-free);
//   V tile: the head's 16 V^T rows x 64 keys row-major (128 B rows), 16-B chunks XOR-swizzled by
//   (row >> 1) & 7 so that the P.V operand's two 8-byte reads per lane are conflict-free.
// Ring of 3 step slots: iteration ks waits for its own pieces of step ks (counted vmcnt), one
// barrier, issues step ks+2 into the slot step ks-1 used, computes step ks.  Wave w issues K
// piece w; waves 0 and 1 also V half w.
// ---------------------------------------------------------------------------
constexpr int SA3_SLOT = 6144;   // bytes per ring slot: K 4 KiB + V 2 KiB
template <int QPW>
__host__ __device__ inline size_t sa3_lds_bytes(int L) {
  const int nks = (L + SA2_KS - 1) / SA2_KS;
  return (size_t)3 * SA3_SLOT + (size_t)(L + 64 * QPW + SA2_KS) * 16 + (size_t)nks * SA2_KS * 4 + round_up(nks, 16);
}

// the SelfAttention form of a length: the DMA-ring kernel where two blocks fit a CU and the
// sequence is long enough for the ring to pay (lab at 21 utterances: L = 305 sa2 9.4 vs sa3
// 10.4 us, L = 610 20.9 vs 17.4, L = 3376 (one block per CU) 189 vs 231; profiles/r05_attn_lab_sa3.txt,
// r05_attn_lab_long.txt)
// and its query tiles per wave: 4 from 1000 frames, 3 from 1500 (lab, 21 x 1219: 47.8 -> 43.6 us;
// 11 x 1688: 53.7 -> 48.1 us; 21 x 610 stays at 2: 17.4 vs 18.6; r05_attn_lab_sa3q.txt); 0 = sa2
inline int sa3_qpw(int L) {
  if (L <= 400) return 0;
  if (L >= 1500 && sa3_lds_bytes<3>(L) <= 80 * 1024) return 3;
  if (L >= 1000 && L < 1500 && sa3_lds_bytes<4>(L) <= 80 * 1024) return 4;
  return sa3_lds_bytes<2>(L) <= 80 * 1024 ? 2 : 0;
}
// the register-fed form past that (sequences whose ring and tables do not fit two blocks per CU):
// 3 query tiles per wave at one block per CU (lab at 3376 frames: 11 utterances 184.9 -> 160.4 us,
// 32: 499 -> 363 us; r05_attn_lab_sa2q.txt); 2 below 400 frames
inline int sa2_qpw(int L) { return L > 400 && sa2_lds_bytes<3>(L) <= 160 * 1024 ? 3 : 2; }
inline size_t sa3_plan_lds(int L) {
  const int q = sa3_qpw(L);
  return q == 4 ? sa3_lds_bytes<4>(L) : q == 3 ? sa3_lds_bytes<3>(L) : q == 2 ? sa3_lds_bytes<2>(L) : 0;
}

template <int QPW, int MINW = 2>
__global__ __launch_bounds__(256, MINW) void zv_attn_sa3_kernel(FlashParams p) {
  constexpr int QT = 64 * QPW, KS = SA2_KS, NU = QPW + 3;
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  const int L = p.L;
  const int nks = (L + KS - 1) / KS;
  const int NT = L + QT + KS;
  unsigned char* ring = fsm;
  bf16x8* PP = reinterpret_cast<bf16x8*>(fsm + 3 * SA3_SLOT);
  float* Mb = reinterpret_cast<float*>(PP + NT);
  uint8_t* Fs = reinterpret_cast<uint8_t*>(Mb + nks * KS);

  const int nqb = (L + QT - 1) / QT;
  const int lb = fa2_xcd_block(blockIdx.x, gridDim.x);
  const int qt0 = (lb % nqb) * QT, h = (lb / nqb) % p.H, b = lb / nqb / p.H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const long qbase = (long)b * L * p.ldq;

  // DMA sources: K rows of head h (byte offsets from kbase), V^T rows of head h (from vbase)
  const int ldqb = (int)p.ldq * 2, ldvb = (int)p.ldv * 2;
  const char* kbase = reinterpret_cast<const char*>(p.qh + qbase + p.H * ATT_QD + h * ATT_QD);
  const char* vbase = reinterpret_cast<const char*>(p.vh + (long)b * p.sv_b + (long)h * 16 * p.ldv);
  const unsigned k_lane = (unsigned)(c16 * ldqb + g * 16);        // piece `wave`: key 16 wave + c16
  const int vrow = 8 * (wave & 1) + (lane >> 3);                   // V half `wave` (waves 0, 1)
  const unsigned v_lane = (unsigned)(vrow * ldvb + (((lane & 7) ^ ((vrow >> 1) & 7)) * 16));
  auto issue = [&](int ks) {                                       // this wave's pieces of step ks
    unsigned char* slot = ring + (ks % 3) * SA3_SLOT;
    const int j0 = ks * KS, jk = j0 + 16 * wave;
    if (jk + 16 <= L) {
      glds16s(kbase + (long)jk * ldqb, k_lane, slot + wave * 1024);
    } else {                                                       // keys past L: row L - 1 (bias -inf)
      const unsigned kc = (unsigned)(min(jk + c16, L - 1) * ldqb + g * 16);
      glds16s(kbase, kc, slot + wave * 1024);
    }
    if (wave < 2) glds16s(vbase + (long)j0 * 2, v_lane, slot + 4096 + wave * 1024);
  };
  // (pieces per step: 2 for waves 0-1, 1 for waves 2-3; the wait leaves exactly the next step's in
  // flight, and the barrier sits in the same asm statement: no LDS read can be scheduled between
  // the two, and no fence makes the compiler drain the prefetch -- it does not see the DMAs)
  auto wait_step = [&](bool next_in_flight) {
    if (next_in_flight) {
      if (wave < 2) asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(1)\n\ts_barrier" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
  };

  issue(0);
  if (nks > 1) issue(1);
  stage_tp<0>(p, h, qt0, QT, NT, PP, nullptr, tid, 256);
  stage_bias2<KS>(p, b, Mb, Fs, tid, 256);

  int qi[QPW], tbl0 = 0;
  bf16x8 qf[QPW], pb[QPW][2];
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) {
    const int i0 = qt0 + (wave * QPW + qq) * 16;
    qi[qq] = i0 + c16;
    int t;
    tp_query(p, qbase + (long)min(qi[qq], L - 1) * p.ldq, h, c16, g, i0, qt0, QT, qf[qq], pb[qq], t);
    if (qq == 0) tbl0 = t;
  }
  // FA2_OFS: K of the step holding the wave's first query tile (its offsets take that step's
  // maximum too, see below), loaded beside tp_query's operands
  const int ksd = FA2_OFS ? fa2_diag_step<KS>(Mb, min((qt0 + wave * QPW * 16) / KS, nks - 1), lane) : 0;
  bf16x8 kd[4];
  if constexpr (FA2_OFS && ZV_FA2_DIAG) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      kd[t] = *reinterpret_cast<const bf16x8*>(kbase + (long)min(ksd * KS + 16 * t + c16, L - 1) * ldqb + g * 16);
  }
  // (tp_query's loads are vector-memory operations too: drain them before the counted ring waits)
  wait_vmcnt<0>();

  f32x4 ofs[QPW];                  // per-query offsets (FA2_OFS; zero in bf16)
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) ofs[qq] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto scores = [&](auto BIAS_, int j0, const unsigned char* slot, f32x4 (&st)[QPW][4]) {
    constexpr bool BIAS = decltype(BIAS_)::value;
    bf16x8 TA[NU], TB[NU], kf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) kf[t] = *reinterpret_cast<const bf16x8*>(slot + t * 1024 + lane * 16);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int ix = j0 + 16 * (u - (QPW - 1)) + tbl0;
      TA[u] = PP[ix];
      TB[u] = PP[ix - 8];
    }
    f32x4 c0[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      c0[t] = BIAS ? *reinterpret_cast<const f32x4*>(Mb + j0 + t * 16 + g * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 ci = FA2_OFS ? (BIAS ? c0[t] + ofs[qq] : ofs[qq]) : c0[t];
        f32x4 c = ZV_MFMA_16x16x32(kf[t], qf[qq], ci, 0, 0, 0);
        c = ZV_MFMA_16x16x32(TA[t - qq + QPW - 1], pb[qq][0], c, 0, 0, 0);
        st[qq][t] = ZV_MFMA_16x16x32(TB[t - qq + QPW - 1], pb[qq][1], c, 0, 0, 0);
      }
  };
  // scores of the step at j0 from K fragments in registers, key bias always applied (the exact
  // path and the offset prologue)
  auto scores_k = [&](int j0, const bf16x8 (&kf)[4], f32x4 (&st)[QPW][4]) {
    bf16x8 TA[NU], TB[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int ix = j0 + 16 * (u - (QPW - 1)) + tbl0;
      TA[u] = PP[ix];
      TB[u] = PP[ix - 8];
    }
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 c = ZV_MFMA_16x16x32(kf[t], qf[qq], *reinterpret_cast<const f32x4*>(Mb + j0 + t * 16 + g * 4), 0, 0, 0);
        c = ZV_MFMA_16x16x32(TA[t - qq + QPW - 1], pb[qq][0], c, 0, 0, 0);
        st[qq][t] = ZV_MFMA_16x16x32(TB[t - qq + QPW - 1], pb[qq][1], c, 0, 0, 0);
      }
  };
  // FA2_OFS: the diagonal step's per-query maxima.  Step 0 alone left 4 of 1600 waves per
  // utterance above fp16's range at the C2 shape (a later score 16 over the offset), each an
  // exact-path wave; with the diagonal step none (tools/offset_study.py, r06_offset_study.txt)
  float od[QPW];
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) od[qq] = -1e30f;
  if constexpr (FA2_OFS && ZV_FA2_DIAG) {
    f32x4 sd[QPW][4];
    scores_k(ksd * KS, kd, sd);
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq) od[qq] = fa2_step_offset(sd[qq]);
  }
  const int vsw = (c16 >> 1) & 7;
  auto vfrag = [&](const unsigned char* slot, int hf) -> bf16x8 {
    const unsigned char* row = slot + 4096 + c16 * 128 + (g & 1) * 8;
    const int c0 = 4 * hf + (g >> 1), c1 = c0 + 2;
    const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(row + ((c0 ^ vsw) * 16));
    const bf16x4 a1 = *reinterpret_cast<const bf16x4*>(row + ((c1 ^ vsw) * 16));
    return bf16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  };
  auto pv = [&](const f32x4 (&st)[4], const bf16x8 (&vf)[2], float sub, f32x4& acc) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      bf16x8 pbv;
#pragma unroll
      for (int e = 0; e < 8; ++e) pbv[e] = (bf16)__builtin_amdgcn_exp2f(st[2 * hf + (e >> 2)][e & 3] - sub);
      acc = ZV_MFMA_16x16x32(vf[hf], pbv, acc, 0, 0, 0);
    }
  };

  f32x4 acc[QPW];
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) acc[qq] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step = [&](auto BIAS_, auto FIRST_, int ks) {
    const unsigned char* slot = ring + (ks % 3) * SA3_SLOT;
    f32x4 st[QPW][4];
    scores(BIAS_, ks * KS, slot, st);
    const bf16x8 vf[2] = {vfrag(slot, 0), vfrag(slot, 1)};
    if constexpr (decltype(FIRST_)::value) {   // FA2_OFS, step 0 (offsets still zero): the offsets
#pragma unroll
      for (int qq = 0; qq < QPW; ++qq) {
        const float o = fmaxf(fa2_step_offset(st[qq]), od[qq]);
        ofs[qq] = f32x4{-o, -o, -o, -o};
        pv(st[qq], vf, o, acc[qq]);
      }
    } else {
#pragma unroll
      for (int qq = 0; qq < QPW; ++qq) pv(st[qq], vf, 0.f, acc[qq]);
    }
  };
  int ks = 0;
  if constexpr (FA2_OFS) {          // step 0 peeled: it sets the offsets
    wait_step(1 < nks);
    if (2 < nks) issue(2);
    step(std::true_type{}, std::true_type{}, 0);
    ks = 1;
  }
  for (; ks < nks; ++ks) {
    wait_step(ks + 1 < nks);       // step ks landed for every wave; slot (ks + 2) % 3 free
    if (ks + 2 < nks) issue(ks + 2);
    if (__builtin_amdgcn_readfirstlane(Fs[ks])) step(std::true_type{}, std::false_type{}, ks);
    else step(std::false_type{}, std::false_type{}, ks);
  }

  float den[QPW];
  bool lo = false, hi = false;
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) {
    den[qq] = __shfl(acc[qq][0], 48 + c16, 64);
    fa2_range(den[qq], acc[qq], lo, hi);
  }
  const bool any_lo = __builtin_amdgcn_ballot_w64(lo) != 0, any_hi = __builtin_amdgcn_ballot_w64(hi) != 0;
  if (any_lo || any_hi || p.force_exact) {
    if (lane == 0) fa2_count(p, any_lo, any_hi);
    // exact path (rare): online softmax with the row maximum subtracted, K / V straight from
    // memory (the ring is the block's; this wave alone goes back over the keys)
    const int vv = c16 * ldvb + g * 8;
    const __amdgpu_buffer_rsrc_t rsV =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(vbase), 0, 16 * ldvb, 0x00020000);
    float mref[QPW];
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq) { acc[qq] = f32x4{0.f, 0.f, 0.f, 0.f}; mref[qq] = -1e30f; }
    for (int k2 = 0; k2 < nks; ++k2) {
      const int j0 = k2 * KS;
      bf16x8 kf[4], vf[2];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        kf[t] = *reinterpret_cast<const bf16x8*>(kbase + (long)min(j0 + 16 * t + c16, L - 1) * ldqb + g * 16);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int j = j0 + 32 * hf;
        const bf16x4 a0 = __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(rsV, vv, j * 2, 0));
        const bf16x4 a1 = __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(rsV, vv, j * 2 + 32, 0));
        vf[hf] = bf16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      }
      // scores straight from the registers' K (the same chain as scores())
      f32x4 st[QPW][4];
      scores_k(j0, kf, st);
#pragma unroll
      for (int qq = 0; qq < QPW; ++qq) {
        float ml = st[qq][0][0];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) ml = fmaxf(ml, st[qq][t][r]);
        // an integer maximum: rescaling the accumulator by 2^(mref - mn) is exact, and the
        // maximum's own p lies in (1/2, 1]
        const float mn = fmaxf(mref[qq], ceilf(qmax4(ml)));
        acc[qq] = acc[qq] * __builtin_amdgcn_exp2f(mref[qq] - mn);
        mref[qq] = mn;
        pv(st[qq], vf, mn, acc[qq]);
      }
    }
#pragma unroll
    for (int qq = 0; qq < QPW; ++qq) den[qq] = __shfl(acc[qq][0], 48 + c16, 64);
  }

#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) {
    const int d0 = g * 4;
    if (qi[qq] >= L || d0 >= p.nv) continue;
    const float rden = 1.f / den[qq];
    float v[4] = {acc[qq][0] * rden, acc[qq][1] * rden, acc[qq][2] * rden, acc[qq][3] * rden};
    const long o = ((long)b * L + qi[qq]) * p.ldo + (long)h * p.ocol_per_head + d0;
    if (d0 + 3 < p.nv) {
      store_split4(p.oh, p.ol, o, v);
      if (p.oh2) store_split4(p.oh2, nullptr, o, v);
    } else {
      for (int e = 0; d0 + e < p.nv; ++e) {
        split_store(p.oh, p.ol, o + e, v[e]);
        if (p.oh2) split_store(p.oh2, nullptr, o + e, v[e]);
      }
    }
  }
}

template <int QPW = 2, int MINW = 2>
static void launch_attn_sa3(const FlashParams& p, hipStream_t s) {
  const size_t lds = sa3_lds_bytes<QPW>(p.L);
  ZV_REQUIRE(lds <= 160 * 1024, "sequence too long for the fused attention kernel");
  ZV_REQUIRE(p.nv <= 12 && p.vrows_per_head == 16 && p.ldq % 8 == 0 && p.ldv % 64 == 0,
             "SelfAttention v3: 16-row value heads (row 12 = ones), V^T rows padded to 64 keys");
  static unsigned long long attr = 0;   // per device (hipFuncSetAttribute is per device)
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_attn_sa3_kernel<QPW, MINW>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr |= 1ull << zv_cur_device();
  }
  const long nblk = (long)cdiv(p.L, 64 * QPW) * p.H * p.B;
  ZV_REQUIRE(nblk < (1L << 31), "SelfAttention v3 grid");
  ZvProfScope prof("attn_sa_bf16", (72.0 + 2.0 * p.nv) * p.H * p.B * (double)p.L * p.L, 0.0, s);
  hipLaunchKernelGGL((zv_attn_sa3_kernel<QPW, MINW>), dim3((unsigned)nblk), dim3(256), lds, s, p);
  ZV_LAUNCH_CHECK();
}

// The consumers' forms (the numbers of zv_attn2_check's ABI) and the form a length runs on.
// SelfAttention 1 / 2: sa2 with 2 / 3 query tiles per wave, 3 / 4 / 5: sa3 with 2 / 3 / 4: LDS-staged
// K / V (sa3) while two blocks fit a CU, the register-fed form past that
inline int sa_b2_form(int L) {
  const int q3 = sa3_qpw(L);
  return q3 ? q3 + 1 : sa2_qpw(L) == 3 ? 2 : 1;
}
static void launch_attn_sa_b2(const FlashParams& f, int form, hipStream_t s) {
  switch (form) {
    case 1: launch_attn_sa2<2>(f, s); break;
    case 2: launch_attn_sa2<3, 1>(f, s); break;
    case 3: launch_attn_sa3<2>(f, s); break;
    case 4: launch_attn_sa3<3>(f, s); break;
    default: launch_attn_sa3<4>(f, s); break;
  }
}
// NonlinAttention 1 / 2: 4 / 8 query tiles per block; the kernel by the hidden width
inline int na_b2_form(int L) { return na2_qtiles(L) == 4 ? 1 : 2; }
static void launch_attn_na_b2(const FlashParams& f, int hid, int form, hipStream_t s) {
  if (hid <= 128) { if (form == 1) launch_attn_na2<1, 4>(f, s); else launch_attn_na2<1>(f, s); }
  else if (hid <= 256) { if (form == 1) launch_attn_na2<2, 4>(f, s); else launch_attn_na2<2>(f, s); }
  else if (form == 1) launch_attn_na2<3, 4>(f, s);
  else launch_attn_na2<3>(f, s);
}

// the v2 consumers' LDS images fit one workgroup at this length (else: the materialising path)
static bool fused_attn2_fits(int L, int nv_na) {
  const size_t lim = 160 * 1024;
  const size_t na = nv_na <= 128 ? na2_lds_bytes<1, 8>(L) : nv_na <= 256 ? na2_lds_bytes<2, 8>(L) : na2_lds_bytes<3, 8>(L);
  return sa2_lds_bytes<2>(L) <= lim && na <= lim;
}
