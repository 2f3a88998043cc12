// Relative-position attention weights for one Zipformer layer.
//
// RelPositionMultiheadAttentionWeights.forward (zipformer.py:1149-1306):
//   s[h,b,i,j] = q[b,i,h,:] . k[b,j,h,:]            (no 1/sqrt(d) scale)
//              + p[b,i,h,:] . P[L-1-i+j, h, :]       (P = linear_pos(pe))
//   s = -1000 where key j is padded;  W = softmax_j(s)
//
// One workgroup = (64-query tile, head, batch item); 4 waves x 16 query rows.
// q.k^T runs on MFMA 16x16x32 (K = query_head_dim = 32: one MFMA, x3 in split
// mode); the rank-4 positional term is gathered from an LDS copy of the head's
// slice of P covering the tile's offset range.  Two passes over the keys
// (running max/sum, then normalised write), so no LxL scratch is needed beyond
// the output W itself.
#pragma once
#include "zv_common.h"
#include "zv_gemm.inc"

struct AttnParams {
  const bf16* qh;    // (B, L, ldq): [q (H*qd) | k (H*qd) | p (H*pd)], bf16 hi
  const bf16* ql;    // lo half (fp32-accurate mode) or null
  long ldq;
  const float* P;    // (2L-1, H*pd) positional projection
  const uint8_t* key_pad;  // (B, L) 1 = padded, or null
  bf16* Wh;          // (H, B, L, ldw) softmax weights, hi
  bf16* Wl;          // lo half or null
  long ldw;
  int B, L, H;
  int b2;            // scores arrive in base 2 (log2(e) folded into the k / p weights, zv_flash2.inc):
                     // exp2 and masked_fill(-1000 log2(e))
};

constexpr int ATT_QD = 32, ATT_PD = 4;

// What the last attention launch of this file or zv_flash.inc was, written by its launch function (test
// infrastructure: zv_attn_check reports it, so a test sees which instantiation ran): kernel 0 stats,
// 1 NonlinAttention, 2 SelfAttention, 3 SelfAttention Toeplitz, 4 materialising softmax; a = value tiles per
// wave (NonlinAttention) or PLO (Toeplitz SelfAttention), b = query tiles per block or MINW
struct AttnLaunchRec { int kernel, split, a, b, tpm, gx, gy, gz; };
static thread_local AttnLaunchRec g_zv_last_attn = {-1, 0, 0, 0, 0, 0, 0, 0};

template <int SPLIT>
__device__ __forceinline__ void load_qk_frag(const bf16* qh, const bf16* ql, long off, bool valid,
                                             bf16x8& hi, bf16x8& lo) {
  const bf16x8 z = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
  hi = valid ? *reinterpret_cast<const bf16x8*>(qh + off) : z;
  if constexpr (SPLIT == 3) lo = valid ? *reinterpret_cast<const bf16x8*>(ql + off) : z;
}

template <int SPLIT>
__global__ __launch_bounds__(256) void zv_attn_softmax_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) f32x4 Ps[];
  const int L = p.L;
  const int qt0 = blockIdx.x * 64;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long qbase = (long)b * L * p.ldq;
  const bf16* qh = p.qh;
  const bf16* ql = p.ql;
  const int HQ = p.H * ATT_QD;

  // offsets n = L-1-i+j for i in [qt0, qt0+63], j in [0, L)
  const int nlo = L - 1 - (qt0 + 63);     // may be negative (rows >= L never read it)
  const int nrange = L + 63;
  for (int t = tid; t < nrange; t += 256) {
    int n = nlo + t;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n >= 0 && n <= 2 * L - 2) v = *reinterpret_cast<const f32x4*>(p.P + (long)n * p.H * ATT_PD + h * ATT_PD);
    Ps[t] = v;
  }

  // Q fragment (A operand): rows i0 + (lane&15), k = 8*(lane>>4) .. +7
  const int i0 = qt0 + wave * 16;
  bf16x8 qfh, qfl;
  {
    const int r = i0 + (lane & 15);
    load_qk_frag<SPLIT>(qh, ql, qbase + (long)r * p.ldq + h * ATT_QD + (lane >> 4) * 8, r < L,
                        qfh, qfl);
  }
  // positional queries for the 4 accumulator rows of this lane
  f32x4 pq[4];
  int rows[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    rows[r] = i0 + (lane >> 4) * 4 + r;
    pq[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rows[r] < L) {
      const long po = qbase + (long)rows[r] * p.ldq + 2 * HQ + h * ATT_PD;
      pq[r] = f32x4{ld_split(qh, ql, po), ld_split(qh, ql, po + 1), ld_split(qh, ql, po + 2),
                    ld_split(qh, ql, po + 3)};
    }
  }
  __syncthreads();

  const uint8_t* kp = p.key_pad ? p.key_pad + (long)b * L : nullptr;
  const int nkt = (L + 15) / 16;
  const float mval = p.b2 ? -1000.f * 1.4426950408889634f : -1000.f;
  auto ex = [&](float x) { return p.b2 ? exp2f(x) : expf(x); };

  auto tile_scores = [&](int kt, float (&s)[4], int& j) {
    const int j0 = kt * 16;
    const int jr = j0 + (lane & 15);
    bf16x8 kh, kl;
    load_qk_frag<SPLIT>(qh, ql, qbase + (long)jr * p.ldq + HQ + h * ATT_QD + (lane >> 4) * 8,
                        jr < L, kh, kl);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SPLIT == 3) {
      acc = ZV_MFMA_16x16x32(qfl, kh, acc, 0, 0, 0);
      acc = ZV_MFMA_16x16x32(qfh, kl, acc, 0, 0, 0);
    }
    acc = ZV_MFMA_16x16x32(qfh, kh, acc, 0, 0, 0);
    j = jr;
    const bool masked = (jr < L) && kp && kp[jr];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int nl = (L - 1 - rows[r] + jr) - nlo;   // in [0, nrange) for valid rows
      const f32x4 pv = Ps[nl < 0 ? 0 : (nl >= nrange ? nrange - 1 : nl)];
      float v = acc[r] + (pq[r][0] * pv[0] + pq[r][1] * pv[1] + pq[r][2] * pv[2] + pq[r][3] * pv[3]);
      s[r] = masked ? mval : v;
    }
  };

  // pass 1: running max / sum per row (this lane's columns)
  float mx[4], sm[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { mx[r] = -INFINITY; sm[r] = 0.f; }
  for (int kt = 0; kt < nkt; ++kt) {
    float s[4]; int j;
    tile_scores(kt, s, j);
    if (j < L) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mn = fmaxf(mx[r], s[r]);
        sm[r] = sm[r] * ex(mx[r] - mn) + ex(s[r] - mn);
        mx[r] = mn;
      }
    }
  }
  // combine across the 16 lanes that share a row group
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float om = __shfl_xor(mx[r], off, 64);
      const float os = __shfl_xor(sm[r], off, 64);
      const float mn = fmaxf(mx[r], om);
      float a = (mx[r] == -INFINITY) ? 0.f : sm[r] * ex(mx[r] - mn);
      float c = (om == -INFINITY) ? 0.f : os * ex(om - mn);
      sm[r] = a + c;
      mx[r] = mn;
    }
  }
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) inv[r] = 1.f / sm[r];

  // pass 2: recompute and write normalised weights (pad columns [L, ldw) = 0)
  const long wbase = ((long)h * p.B + b) * L * p.ldw;
  bf16* Wl = (SPLIT == 3) ? p.Wl : nullptr;
  const int nkt_w = (int)(p.ldw / 16);
  for (int kt = 0; kt < nkt_w; ++kt) {
    float s[4]; int j;
    if (kt < nkt) tile_scores(kt, s, j);
    else j = kt * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (rows[r] < L) {
        const float w = (j < L) ? ex(s[r] - mx[r]) * inv[r] : 0.f;
        split_store(p.Wh, Wl, wbase + (long)rows[r] * p.ldw + j, w);
      }
    }
  }
}

template <int SPLIT>
static void launch_attn_softmax(const AttnParams& p, hipStream_t s) {
  dim3 grid(cdiv(p.L, 64), p.H, p.B);
  size_t lds = (size_t)(p.L + 63) * sizeof(f32x4);
  ZV_REQUIRE(lds <= 160 * 1024, "sequence too long for the attention kernel (L > 10176)");
  static unsigned long long attr_set = 0;   // per device
  if (lds > 64 * 1024 && !((attr_set >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_attn_softmax_kernel<SPLIT>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set |= 1ull << zv_cur_device();
  }
  // algorithmic work: q.k (2*32 flop) + positional term (2*4) per score, x H*B*L^2
  ZvProfScope prof(SPLIT == 3 ? "attn_softmax_fp32" : "attn_softmax_bf16",
                   72.0 * p.H * p.B * (double)p.L * p.L,
                   (double)p.H * p.B * p.L * (double)p.ldw * 2 * (SPLIT == 3 ? 2 : 1), s);
  g_zv_last_attn = {4, SPLIT, 0, 0, 0, (int)grid.x, (int)grid.y, (int)grid.z};
  hipLaunchKernelGGL((zv_attn_softmax_kernel<SPLIT>), grid, dim3(256), lds, s, p);
  ZV_LAUNCH_CHECK();
}
