// Test-infrastructure and microbenchmark entry points of the C ABI: zv_bench_gemm, zv_bench_fused_linear,
// zv_gemm_selftest, zv_attn_plan, zv_attn2_check, zv_attn2_check_stale, zv_attn_check, zv_mx8_quantize, zv_mx8_gemm_check, zv_linear_check, zv_ffn_check,
// zv_dwconv_check, zv_stackedge_check, zv_bigvgan_check, zv_solve_check (and the host-only zv_time_steps,
// zv_cfg_plan).
// None of them builds an engine: each runs one launch (or a timed loop of one launch) of a kernel the
// engine, the vocoder or BigVGAN dispatch also instantiates, on operands it makes itself, through the
// launch function they launch it through (the form choice, the grid and the argument order exist
// once, beside the kernel); the only kernels launched here directly are this file's own.  Included by
// zv_engine.hip after zv_engine (zv_linear_check uses its perm_na / perm_glu) and the ZV_API_* helpers.
// Every device buffer of a call belongs to its ChkDev, which frees them when the call returns or throws.
//
// GEMM instantiations that only the microbenchmark launched, measured and retired (their variant
// numbers answer "unknown variant"; tile experiments belong in tools/lab/gemm_lab.hip; us at
// 78016 x 1536 x 512 with the bf16 output against the 128x128 two-stage kernel, variant 0, in the
// same record unless noted):
//  -  1: 128x128, 3-stage ring (96 KiB, one block per CU): 257.2 against 198.3 us (r02_gemm_ring_depth.txt)
//  -  2: 256x128, 4x2 waves, 2 stages: 224.2 against 225.4 us, fp32 output 260.9 against 252.6
//        (r01_gemm_variants.txt)
//  -  3: 256x128, 4x2 waves, 3 stages: 203.8 against 219.8 us alone (r01_gemm_variants_v2.txt), one
//        guided C2 forward 34.503 / 34.345 against 34.242 ms on 128x128 everywhere (r01_gemm_tile_ab.txt)
//  -  4: 128x64, 3 stages: 251.5 against 225.4 us (r01_gemm_variants.txt)
//  -  5: 128x256, 2x4 waves: 208.2 against 225.4 us alone (r01_gemm_variants.txt); never adopted by the
//        launch policy, no in-model record kept
//  -  6: 128x128, 4-stage ring: no record kept
//  -  7: 256x128, 2x2 waves (128x64 wave tiles, one block per CU): 332.6 against 203.2 us
//        (r02_gemm_wave_tiles.txt)
//  -  8: 256x256, 2x4 waves; 9: 256x128, 2x4 waves; 10: 128x256, 1x4 waves: no record kept
//  - 30 / 31: 128x128 with a 32-deep K step, 4 / 3 stages: 205.1 / 203.1 against 198.3 us
//        (r02_gemm_ring_depth.txt)
//  - 32 / 33: 256x128, 2x2 waves, 32-deep K step, 2 / 3 stages: 214.8 / 227.4 against 203.2 us
//        (r02_gemm_wave_tiles.txt)
//  - 40: deferred epilogue stores on 128x128 (the form is gone from zv_gemm.inc with it): 208.4
//        against 217.4 us alone, one guided forward 35.66 against 35.34 ms (r01_gemm_defer_ab.txt)
#pragma once

namespace {

struct ChkDev {   // the device buffers of one check call, freed when it returns or throws
  std::vector<void*> ptrs;
  void* raw(size_t bytes) {
    void* p = nullptr;
    ZV_CHECK(ZV_BLOCKING(hipMalloc(&p, bytes + 256)));
    ptrs.push_back(p);
    return p;
  }
  template <typename T> T* make(size_t n) { return reinterpret_cast<T*>(raw(n * sizeof(T))); }
  template <typename T> T* zero(size_t n) {
    T* d = make<T>(n);
    ZV_CHECK(ZV_BLOCKING(hipMemset(d, 0, n * sizeof(T))));
    return d;
  }
  template <typename T> T* up(const T* host, size_t n) {
    T* d = make<T>(n);
    ZV_CHECK(ZV_BLOCKING(hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice)));
    return d;
  }
  template <typename T> void down(T* host, const T* dev, size_t n) {
    ZV_CHECK(ZV_BLOCKING(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost)));
  }
  ~ChkDev() { for (void* p : ptrs) (void)ZV_BLOCKING(hipFree(p)); }
};

struct ChkEvent {   // one timing event of a check call
  hipEvent_t e = nullptr;
  ChkEvent() { ZV_CHECK(ZV_BLOCKING(hipEventCreate(&e))); }
  ~ChkEvent() { (void)ZV_BLOCKING(hipEventDestroy(e)); }
};

// an activation as the engine's producers write it: (rows, ld) 16-bit hi (+ lo), zero beyond cols
void chk_act(const float* x, long rows, int cols, long ld, bool lo, std::vector<bf16>& h, std::vector<bf16>& l) {
  h.assign((size_t)rows * ld, (bf16)0.f);
  if (lo) l.assign((size_t)rows * ld, (bf16)0.f);
  for (long r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) {
      const float v = x[r * cols + c];
      const bf16 hv = (bf16)v;
      h[(size_t)r * ld + c] = hv;
      if (lo) l[(size_t)r * ld + c] = (bf16)(v - (float)hv);
    }
}
// a (rows, cols) fp32 host array re-laid with row stride ld (zero padding)
std::vector<float> chk_pad(const float* x, long rows, int cols, long ld) {
  std::vector<float> v((size_t)rows * ld, 0.f);
  for (long r = 0; r < rows; ++r) memcpy(&v[(size_t)r * ld], x + r * cols, (size_t)cols * sizeof(float));
  return v;
}
void chk_record(int* launch, int* num_cus) {
  const ZvLaunchRec& r = g_zv_last_launch;
  const int v[8] = {r.BM, r.BN, r.SPLIT, r.EPI, r.ROLE, r.k256, r.grid, r.aux};
  memcpy(launch, v, sizeof(v));
  *num_cus = zv_num_cus();
}
}  // namespace

// GEMM microbenchmark on random operands: C(M,N) fp32 = A(M,K) . W(N,K)^T
static __global__ void zv_fill_rand_bf16(bf16* p, long n, unsigned seed) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    unsigned x = (unsigned)i * 2654435761u ^ seed;
    x ^= x >> 13; x *= 0x5bd1e995u; x ^= x >> 15;
    p[i] = (bf16)(((float)(x & 0xffff) / 65535.0f) * 2.0f - 1.0f);
  }
}

// the 128x128 two-stage tile (2 x 2 waves, two blocks per CU) on the general (ROLE 0) or a counted epilogue
template <int ROLE>
static float bench_variant(GemmParams p, int iters, bool persistent, hipStream_t s) {
  ChkEvent e0, e1;
  launch_gemm<128, 128, 2, 2, 1, EPI_STD, 2, 2, GEMM_BK, 0, 0, ROLE>(p, 1, s, "bench", persistent);
  ZV_CHECK(hipEventRecord(e0.e, s));
  for (int i = 0; i < iters; ++i)
    launch_gemm<128, 128, 2, 2, 1, EPI_STD, 2, 2, GEMM_BK, 0, 0, ROLE>(p, 1, s, "bench", persistent);
  ZV_CHECK(hipEventRecord(e1.e, s));
  ZV_CHECK(ZV_BLOCKING(hipEventSynchronize(e1.e)));
  float ms = 0.f;
  ZV_CHECK(hipEventElapsedTime(&ms, e0.e, e1.e));
  return ms / iters;
}

// GEMM self-check helpers
static __global__ void zv_zero_kpad_kernel(bf16* p, long rows, int ld, int K) {
  const long n = rows * (long)(ld - K);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    p[(i / (ld - K)) * ld + K + i % (ld - K)] = (bf16)0.f;
}
static __global__ void zv_bf16_to_f32_kernel(const bf16* a, float* b, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    b[i] = (float)a[i];
}
static __global__ void zv_maxdiff_kernel(const float* a, const float* b, long n, float* out) {
  float d = 0.f, r = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    d = fmaxf(d, fabsf(a[i] - b[i]));
    r = fmaxf(r, fabsf(b[i]));
  }
  atomicMax(reinterpret_cast<int*>(out), __float_as_int(d));
  atomicMax(reinterpret_cast<int*>(out + 1), __float_as_int(r));
}

extern "C" {

int zv_bench_gemm(int M, int N, int K, int variant, int iters, int out_mode, float* ms_out) {
  ZV_API_BEGIN
  const bool persistent = variant < 100;
  variant %= 100;
  ZV_REQUIRE(variant == 0 || variant == 70 || variant == 72, "unknown variant");
  ZV_REQUIRE(variant != 72 || out_mode == 7, "variant 72: mode 7 only");
  ZV_REQUIRE(variant != 70 || out_mode == 5 || out_mode == 6, "variant 70: modes 5 / 6 only");
  ChkDev dev;
  hipStream_t s = nullptr;
  const long Kp = round_up(K, 64), Np = round_up(N, 256);
  const size_t mn = (size_t)M * N;
  bf16* A = dev.make<bf16>((size_t)M * Kp);
  bf16* W = dev.make<bf16>((size_t)Np * Kp);
  bf16* Ch = out_mode != 0 ? dev.make<bf16>(mn) : nullptr;
  float* C = out_mode == 0 || out_mode == 2 || out_mode == 5 || out_mode == 6 ? dev.zero<float>(mn) : nullptr;
  hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(4096), dim3(256), 0, s, A, (long)M * Kp, 1u);
  hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(4096), dim3(256), 0, s, W, (long)Np * Kp, 2u);
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.nz2 = 1; p.Brows = (int)Np;
  p.Ah = A; p.lda = Kp; p.Bh = W; p.ldb = Kp;
  p.C = C; p.ldc = N; p.Ch = Ch; p.ldch = N; p.rows_per_group = 1; p.rpb = 1;
  if (out_mode == 2) p.resid = C;
  if (out_mode == 3) p.act = 1;
  if (out_mode == 4) { p.C = nullptr; p.Ch = nullptr; }
  if (out_mode == 7) {             // a plain linear's: bias + SwooshL -> bf16 copy
    p.C = nullptr; p.bias = dev.zero<float>((size_t)N); p.act = 1;
  }
  if (out_mode == 5 || out_mode == 6) {   // a residual linear's epilogue operands
    float* extra = dev.zero<float>(2 * (size_t)N + (out_mode == 6 ? mn : 0));
    p.resid = C; p.bias = extra;
    if (out_mode == 6) { p.byp = extra + N; p.orig = extra + 2 * N; }
  }
  switch (variant) {
    case 0: *ms_out = bench_variant<0>(p, iters, persistent, s); break;
    case 72: *ms_out = bench_variant<3>(p, iters, persistent, s); break;   // counted plain epilogue
    default:                                                               // 70: counted residual epilogue
      *ms_out = out_mode == 5 ? bench_variant<1>(p, iters, persistent, s) : bench_variant<2>(p, iters, persistent, s);
  }
  ZV_API_END
}

// The NonlinAttention in-projection (ZV_LIN_NA) or the value projection (ZV_LIN_TRANS) alone, 16-bit
// product, through LinearPolicy's launch choice (ZV_TRANS_ALIGNED read as the engine reads it), on
// random operands in the engine's layout: utterances of rpb rows, V^T rows of round_up(rpb, 64) frames
int zv_bench_fused_linear(int form, int M, int N, int K, int rpb, int iters, float* ms_out) {
  ZV_API_BEGIN
  ZV_REQUIRE((form == ZV_LIN_NA || form == ZV_LIN_TRANS) && M > 0 && N > 0 && K > 0 && rpb > 0 && iters > 0 &&
                 ms_out && (form != ZV_LIN_NA || N % 48 == 0),
             "zv_bench_fused_linear: form NA (N % 48 == 0) or TRANS, positive sizes");
  ChkDev dev;
  hipStream_t s = nullptr;
  const long Kp = round_up(K, 64), Np = round_up(N, 128), Lpad = round_up(rpb, 64);
  const int rows_t = form == ZV_LIN_NA ? N / 3 : N, nutt = cdiv(M, rpb);
  bf16* A = dev.make<bf16>((size_t)M * Kp);
  bf16* W = dev.make<bf16>((size_t)Np * Kp);
  hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(4096), dim3(256), 0, s, A, (long)M * Kp, 1u);
  hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(4096), dim3(256), 0, s, W, (long)Np * Kp, 2u);
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.nz2 = 1; p.Brows = (int)Np;
  p.Ah = A; p.lda = Kp; p.Bh = W; p.ldb = Kp;
  p.bias = dev.zero<float>((size_t)N); p.rows_per_group = 1;
  p.Cth = dev.zero<bf16>((size_t)nutt * rows_t * Lpad);
  p.ldct = Lpad; p.rpb = rpb; p.sCt = (long)rows_t * Lpad;
  if (form == ZV_LIN_NA) { p.ldch = round_up(rows_t, 8); p.Ch = dev.make<bf16>((size_t)M * p.ldch); }
  LinearPolicy policy;
  auto launch = [&]() {
    if (form == ZV_LIN_NA) policy.launch_na_in<1>(p, s);
    else policy.launch_value_t<1>(p, false, false, s);
  };
  ChkEvent e0, e1;
  launch();
  ZV_CHECK(hipEventRecord(e0.e, s));
  for (int i = 0; i < iters; ++i) launch();
  ZV_CHECK(hipEventRecord(e1.e, s));
  ZV_CHECK(ZV_BLOCKING(hipEventSynchronize(e1.e)));
  float ms = 0.f;
  ZV_CHECK(hipEventElapsedTime(&ms, e0.e, e1.e));
  *ms_out = ms / iters;
  ZV_API_END
}

// GEMM self-check: a counted epilogue of the 128x128 kernel (70 residual, 71 residual + bypass: mode 2;
// 72 plain -> bf16: modes 0 / 1) against its general epilogue on the same random operands.  Writes the
// max |diff| and the max |ref|.
int zv_gemm_selftest(int M, int N, int K, int variant, int mode, float* maxdiff, float* maxref) {
  ZV_API_BEGIN
  ZV_REQUIRE(variant == 70 || variant == 71 || variant == 72, "selftest: unknown variant");
  ZV_REQUIRE(variant == 72 || mode == 2, "selftest: residual-only variant");
  // variant 72 writes bf16 only (the string predates it: the retired variant 40 shared the path)
  ZV_REQUIRE(variant != 72 || mode != 2, "selftest: variant 40 has no residual form");
  ChkDev dev;
  hipStream_t s = nullptr;
  const long Kp = round_up(K, 64), Np = round_up(N, 256);
  const size_t mn = (size_t)M * N;
  bf16* A = dev.make<bf16>((size_t)M * Kp);
  bf16* W = dev.make<bf16>((size_t)Np * Kp);
  float* outs[2] = {dev.make<float>(mn), dev.make<float>(mn)};
  float* R = dev.make<float>(mn);
  float* res = dev.make<float>(2);
  hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(4096), dim3(256), 0, s, A, (long)M * Kp, 1u);
  hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(4096), dim3(256), 0, s, W, (long)Np * Kp, 2u);
  hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(4096), dim3(256), 0, s, reinterpret_cast<bf16*>(R),
                     (long)M * N * 2, 3u);   // finite garbage as the residual
  if (Kp > K) {   // the engine's operands are zero beyond K (padded to the K step)
    hipLaunchKernelGGL(zv_zero_kpad_kernel, dim3(1024), dim3(256), 0, s, A, (long)M, (int)Kp, K);
    hipLaunchKernelGGL(zv_zero_kpad_kernel, dim3(1024), dim3(256), 0, s, W, (long)Np, (int)Kp, K);
  }
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.nz2 = 1; p.Brows = (int)Np;
  p.Ah = A; p.lda = Kp; p.Bh = W; p.ldb = Kp; p.ldc = N; p.rows_per_group = 1; p.rpb = 1;
  if (mode == 1) p.act = 1;
  const bool bf16_out = variant == 72;   // counted plain epilogue: bias (+ SwooshL) -> bf16
  if (bf16_out) {
    float* bias = dev.make<float>((size_t)N);
    hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(64), dim3(256), 0, s, reinterpret_cast<bf16*>(bias),
                       (long)N * 2, 5u);
    p.bias = bias;
  } else {                               // bias, bypass scale / original
    float* extra = dev.make<float>(2 * (size_t)N + mn);
    hipLaunchKernelGGL(zv_fill_rand_bf16, dim3(4096), dim3(256), 0, s, reinterpret_cast<bf16*>(extra),
                       (long)(2 * N + (long)M * N) * 2, 4u);
    p.bias = extra;
    if (variant == 71) { p.byp = extra + N; p.orig = extra + 2 * N; }
  }
  for (int k = 0; k < 2; ++k) {
    p.C = outs[k];
    if (bf16_out) {   // both runs write bf16 (into the two halves of R), widened into outs[] below
      p.C = nullptr;
      p.Ch = reinterpret_cast<bf16*>(R) + (size_t)k * M * N;   // R (2 x M x N bf16) is free here
      p.ldch = N;
    }
    if (mode == 2) {
      ZV_CHECK(hipMemcpyAsync(outs[k], R, mn * 4, hipMemcpyDeviceToDevice, s));
      p.resid = outs[k];
    }
    if (k == 0) launch_gemm<128, 128, 2, 2, 1, EPI_STD, 2, 2>(p, 1, s, "ref", true, 0);
    // the counted epilogue (ROLE 1 / 2 / 3) against the general one
    else if (variant == 70) launch_gemm<128, 128, 2, 2, 1, EPI_STD, 2, 2, GEMM_BK, 0, 0, 1>(p, 1, s, "t", true, -1);
    else if (variant == 71) launch_gemm<128, 128, 2, 2, 1, EPI_STD, 2, 2, GEMM_BK, 0, 0, 2>(p, 1, s, "t", true, -1);
    else launch_gemm<128, 128, 2, 2, 1, EPI_STD, 2, 2, GEMM_BK, 0, 0, 3>(p, 1, s, "t", true, -1);
  }
  if (bf16_out)
    for (int k = 0; k < 2; ++k)
      hipLaunchKernelGGL(zv_bf16_to_f32_kernel, dim3(1024), dim3(256), 0, s,
                         reinterpret_cast<bf16*>(R) + (size_t)k * M * N, outs[k], (long)M * N);
  ZV_CHECK(hipMemsetAsync(res, 0, 8, s));
  hipLaunchKernelGGL(zv_maxdiff_kernel, dim3(1024), dim3(256), 0, s, outs[1], outs[0], (long)M * N, res);
  float h[2];
  dev.down(h, res, 2);
  *maxdiff = h[0]; *maxref = h[1];
  ZV_API_END
}

int zv_attn_plan(int split, int sa_plo, int tpm, int L, int nv_na, int64_t* lds_sa, int64_t* lds_na,
                 int64_t* lds_stats, int* fits) {
  ZV_API_BEGIN
  ZV_REQUIRE((split == 1 || split == 3) && L > 0 && nv_na > 0 && sa_plo >= -1 && sa_plo <= 1 &&
                 tpm >= 0 && tpm <= 3 && (split == 1 || (sa_plo < 0 && tpm == 0)) && lds_sa && lds_na &&
                 lds_stats && fits,
             "bad arguments");
  if (tpm == 3) {   // second-generation set (zv_flash2.inc): no statistics kernel
    *lds_sa = (int64_t)(sa3_qpw(L) ? sa3_plan_lds(L) : sa2_qpw(L) == 3 ? sa2_lds_bytes<3>(L) : sa2_lds_bytes<2>(L));
    *lds_na = (int64_t)(nv_na <= 128 ? na2_lds_bytes<1, 8>(L) : nv_na <= 256 ? na2_lds_bytes<2, 8>(L) : na2_lds_bytes<3, 8>(L));
    *lds_stats = 0;
    *fits = fused_attn2_fits(L, nv_na);
    return 0;
  }
  *lds_sa = (int64_t)(sa_plo < 0 ? sa_lds_bytes(L) : (sa_plo ? sa_tp_lds_bytes<1>(L) : sa_tp_lds_bytes<0>(L)));
  *lds_na = (int64_t)(split == 1 ? na_lds_bytes_for<1>(L, nv_na, tpm) : na_lds_bytes_for<3>(L, nv_na, tpm));
  *lds_stats = (int64_t)pos_mask_bytes(L, 64, true);
  *fits = split == 1 ? fused_attn_fits<1>(L, nv_na, sa_plo, tpm) : fused_attn_fits<3>(L, nv_na, sa_plo, tpm);
  ZV_API_END
}

// Second-generation attention consumers on the device, alone (test infrastructure; host pointers).
// Inputs are rounded to the library's 16-bit operand format here (bf16, or fp16 in
// libzipvoice_hip_f16.so, whose kernels add the per-query offsets), as the engine's producers round
// them: qkp (B, L, 2 H 32 + 4 H) fp32 = [q | k | p] per row in base-2 units (the engine folds
// log2(e) into the k / p weights), P (2L - 1, 4 H) the positional projection (also base 2), key_pad
// (B, L) or null.  kernel 0 SelfAttention: v (B, L, H * nv), nv <= 12, out (B, L, H * nv);
// kernel 1 NonlinAttention (head 0): v (B, L, nv), y (B, L, nv), out (B, L, nv) = y * (W0 . v).
// form 0: the engine's choice for L; SelfAttention 1 / 2: sa2 with 2 / 3 query tiles per wave,
// 3 / 4 / 5: sa3 with 2 / 3 / 4; NonlinAttention 1 / 2: 4 / 8 query tiles per block.
// force_exact: every wave / block on its exact path.  counts (or null): zv_attn_fallbacks's three.
// stale: V^T columns [L, Lpad) hold +-stale (zv_attn2_check_stale) instead of zeros
static void attn2_check_run(int kernel, int form, int B, int L, int H, int nv, const float* qkp, const float* P,
                            const uint8_t* key_pad, const float* v, const float* y, int force_exact, float stale,
                            float* out, int64_t* counts) {
  ZV_REQUIRE((kernel == 0 || kernel == 1) && B > 0 && L > 0 && H > 0 && qkp && P && v && out &&
                 (kernel == 0 ? (nv > 0 && nv <= 12) : (nv > 0 && nv <= 384 && y)),
             "zv_attn2_check: bad arguments");
  ZV_REQUIRE(kernel != 0 || (form >= 0 && form <= 5), "zv_attn2_check: SelfAttention form 0..5");
  ZV_REQUIRE(kernel != 1 || (form >= 0 && form <= 2), "zv_attn2_check: NonlinAttention form 0..2");
  const long ldq = 2L * H * ATT_QD + H * ATT_PD, M = (long)B * L, Lpad = round_up(L, 64);
  const long vrows = kernel == 0 ? 16L * H : nv;   // V^T rows per utterance
  std::vector<bf16> hq((size_t)M * ldq), hv((size_t)B * vrows * Lpad, (bf16)0.f);
  for (size_t i = 0; i < hq.size(); ++i) hq[i] = (bf16)qkp[i];
  for (int b = 0; b < B; ++b)
    for (long r = 0; r < vrows; ++r) {
      const int h = kernel == 0 ? (int)(r / 16) : 0, d = kernel == 0 ? (int)(r % 16) : (int)r;
      for (int j = 0; j < L; ++j) {
        float x = 0.f;
        if (kernel == 1) x = v[((long)b * L + j) * nv + d];
        else if (d < nv) x = v[((long)b * L + j) * H * nv + (long)h * nv + d];
        else if (d == 12) x = 1.f;                       // the ones row (softmax denominator)
        hv[((size_t)b * vrows + r) * Lpad + j] = (bf16)x;
      }
      if (stale != 0.f)
        for (long j = L; j < Lpad; ++j)
          hv[((size_t)b * vrows + r) * Lpad + j] = (bf16)(((r + j) & 1) ? -stale : stale);
    }
  std::vector<bf16> hy;
  if (kernel == 1) {
    hy.resize((size_t)M * nv);
    for (size_t i = 0; i < hy.size(); ++i) hy[i] = (bf16)y[i];
  }
  const long ocols = kernel == 0 ? (long)H * nv : nv, ldo = round_up(ocols, 8);
  ChkDev dev;
  bf16* dout = dev.zero<bf16>((size_t)M * ldo);
  unsigned* dcnt = dev.zero<unsigned>(4);
  FlashParams f{};
  f.qh = dev.up(hq.data(), hq.size()); f.ldq = ldq;
  f.P = dev.up(P, (size_t)(2 * L - 1) * H * ATT_PD);
  f.key_pad = key_pad ? dev.up(key_pad, (size_t)M) : nullptr;
  f.B = B; f.L = L; f.H = H;
  f.vh = dev.up(hv.data(), hv.size()); f.ldv = Lpad; f.sv_b = vrows * Lpad; f.nv = nv;
  f.oh = dout; f.ldo = ldo;
  f.force_exact = force_exact; f.fallback = dcnt;
  hipStream_t s = nullptr;
  if (kernel == 0) {
    f.vrows_per_head = 16; f.ocol_per_head = nv;
    launch_attn_sa_b2(f, form ? form : sa_b2_form(L), s);
  } else {
    f.vrows_per_head = 0; f.ocol_per_head = 0;
    f.mulh = dev.up(hy.data(), hy.size()); f.ldmul = nv;
    launch_attn_na_b2(f, nv, form ? form : na_b2_form(L), s);
  }
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  std::vector<bf16> ho((size_t)M * ldo);
  dev.down(ho.data(), dout, ho.size());
  for (long m = 0; m < M; ++m)
    for (long c = 0; c < ocols; ++c) out[m * ocols + c] = (float)ho[m * ldo + c];
  if (counts) {
    unsigned c[4];
    dev.down(c, dcnt, 4);
    for (int i = 0; i < 3; ++i) counts[i] = c[i];
  }
}

int zv_attn2_check(int kernel, int form, int B, int L, int H, int nv, const float* qkp, const float* P,
                   const uint8_t* key_pad, const float* v, const float* y, int force_exact, float* out,
                   int64_t* counts) {
  ZV_API_BEGIN
  attn2_check_run(kernel, form, B, L, H, nv, qkp, P, key_pad, v, y, force_exact, 0.f, out, counts);
  ZV_API_END
}

// zv_attn2_check with V^T columns [L, Lpad) filled with +-stale: finite values a reused workspace
// may hold there (the transposed stores write frames below L only)
int zv_attn2_check_stale(int kernel, int form, int B, int L, int H, int nv, const float* qkp, const float* P,
                         const uint8_t* key_pad, const float* v, const float* y, int force_exact, float stale,
                         float* out, int64_t* counts) {
  ZV_API_BEGIN
  ZV_REQUIRE(stale == stale && fabsf(stale) <= 60000.f, "zv_attn2_check_stale: a finite fill (within fp16's range)");
  attn2_check_run(kernel, form, B, L, H, nv, qkp, P, key_pad, v, y, force_exact, stale, out, counts);
  ZV_API_END
}

// ---------------------------------------------------------------------------
// zv_attn_check: one first-generation attention kernel (zv_flash.inc) or the materialising softmax
// (zv_attn.inc) alone, through its launch function, on host arrays with canary-guarded outputs
// ---------------------------------------------------------------------------
int zv_attn_check(zv_attn_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->kind >= ZV_ATTN_STATS && a->kind <= ZV_ATTN_SOFTMAX && a->B > 0 && a->L > 0 && a->H > 0 &&
                 (a->split == 1 || a->split == 3) && a->guard >= 0 && a->qkp && a->P,
             "zv_attn_check: bad arguments");
  const int kind = a->kind, B = a->B, L = a->L, H = a->H, nv = a->nv, G = a->guard;
  const bool split3 = a->split == 3;
  ZV_REQUIRE(kind == ZV_ATTN_SA ? (a->form >= 0 && a->form <= 2) : kind == ZV_ATTN_SOFTMAX ? a->form == 0
                                                                                           : (a->form == 0 || a->form == 1),
             "zv_attn_check: form (STATS / NA 0 VALU, 1 Toeplitz; SA 0 sa, 1 sa_tp<0, 2>, 2 sa_tp<0, 1>)");
  ZV_REQUIRE(a->form == 0 || !split3, "zv_attn_check: the Toeplitz forms are 16-bit forms");
  ZV_REQUIRE(kind == ZV_ATTN_SOFTMAX || a->b2 == 0, "zv_attn_check: b2 belongs to SOFTMAX");
  ZV_REQUIRE(a->stale == a->stale && fabsf(a->stale) <= 60000.f, "zv_attn_check: a finite fill (within fp16's range)");
  const long ldq = 2L * H * ATT_QD + H * ATT_PD, M = (long)B * L, Lpad = round_up(L, 64), rows = M + 2 * G;
  ChkDev dev;
  hipStream_t s = nullptr;
  std::vector<bf16> h, l;
  chk_act(a->qkp, M, (int)ldq, ldq, split3, h, l);
  const bf16* qh = dev.up(h.data(), h.size());
  const bf16* ql = split3 ? dev.up(l.data(), l.size()) : nullptr;
  const float* P = dev.up(a->P, (size_t)(2 * L - 1) * H * ATT_PD);
  const uint8_t* pad = a->key_pad ? dev.up(a->key_pad, (size_t)M) : nullptr;
  auto up16 = [&](uint16_t* p, long n, long ld) {
    return p ? reinterpret_cast<bf16*>(dev.up(p, (size_t)(n + 2 * G) * ld)) : nullptr;
  };
  auto down16 = [&](uint16_t* p, bf16* d, long n, long ld) {
    if (p) dev.down(p, reinterpret_cast<uint16_t*>(d), (size_t)(n + 2 * G) * ld);
  };
  if (kind == ZV_ATTN_SOFTMAX) {
    ZV_REQUIRE(a->Wh && (a->Wl != nullptr) == split3 && a->ldw == Lpad,
               "zv_attn_check: SOFTMAX writes Wh (Wl with split 3) in rows of L rounded up to 64");
    const long n = (long)H * M;
    bf16 *Wh = up16(a->Wh, n, Lpad), *Wl = up16(a->Wl, n, Lpad);
    AttnParams ap{qh, ql, ldq, P, pad, Wh + (size_t)G * Lpad, Wl ? Wl + (size_t)G * Lpad : nullptr, Lpad, B, L, H,
                  a->b2 ? 1 : 0};
    if (split3) launch_attn_softmax<3>(ap, s);
    else launch_attn_softmax<1>(ap, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    down16(a->Wh, Wh, n, Lpad); down16(a->Wl, Wl, n, Lpad);
  } else {
    FlashParams f{};
    f.qh = qh; f.ql = ql; f.ldq = ldq; f.P = P; f.key_pad = pad;
    f.B = B; f.L = L; f.H = H;
    float2* st = nullptr;
    float* stg = nullptr;
    if (kind == ZV_ATTN_STATS) {
      ZV_REQUIRE(a->stats, "zv_attn_check: STATS writes stats");
      stg = dev.up(a->stats, (size_t)rows * 2);
      st = reinterpret_cast<float2*>(stg) + G;
    } else if (kind == ZV_ATTN_NA) {
      st = dev.zero<float2>((size_t)M);
    }
    f.stats = st;
    if (kind != ZV_ATTN_SA) {   // head-0 statistics, in the form the NonlinAttention launch scores in
      if (split3) launch_attn_stats<3>(f, s);
      else if (a->form == 1) launch_attn_stats<1, 1>(f, s);
      else launch_attn_stats<1>(f, s);
    }
    if (kind == ZV_ATTN_STATS) {
      ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
      dev.down(a->stats, stg, (size_t)rows * 2);
    } else {
      const bool na = kind == ZV_ATTN_NA;
      ZV_REQUIRE(a->v && a->oh && nv > 0 && (na ? (nv <= 384 && nv % 4 == 0 && a->y && a->ldo % 4 == 0 && a->ldo >= nv)
                                                : (nv <= 12 && a->ldo >= (long)H * nv)),
                 "zv_attn_check: v, out and the value width (SA <= 12 per head; NA <= 384, a multiple of 4, with y)");
      ZV_REQUIRE(split3 ? (a->ol && !a->oh2) : (!na && a->form > 0) ? ((a->ol != nullptr) == (a->oh2 != nullptr))
                                                                     : (!a->ol && !a->oh2),
                 "zv_attn_check: ol with split 3; ol and oh2 together with the Toeplitz SelfAttention form only");
      // V^T as the engine's transposed linears leave it: rows of Lpad frames, frames below L written,
      // the rest whatever the workspace held (+-stale here).  SA: nv rows per head (the first-generation
      // kernels make their ones row in registers: vconst / vfix), NA: nv rows
      // (vrows = 16: the layout of a value projection built padded for the second generation, which the
      // engine's fallback / ZV_ATTN2=0 arms hand to these kernels with a 16-row head stride; rows nv..15 of
      // a head -- the ones row and zero rows there -- are not read: stale values here)
      ZV_REQUIRE(a->vrows == 0 || (!na && a->vrows >= nv && a->vrows <= 16),
                 "zv_attn_check: vrows (SA V^T rows per head): 0 = nv, or nv..16");
      const long vph = na ? nv : (a->vrows ? a->vrows : nv);
      const long vrows = na ? nv : (long)H * vph, vcols = na ? nv : (long)H * nv;
      std::vector<bf16> vh((size_t)B * vrows * Lpad), vl;
      if (split3) vl.resize(vh.size());
      for (int b = 0; b < B; ++b)
        for (long r = 0; r < vrows; ++r) {
          bf16* dh = &vh[((size_t)b * vrows + r) * Lpad];
          bf16* dl = split3 ? &vl[((size_t)b * vrows + r) * Lpad] : nullptr;
          for (long j = 0; j < Lpad; ++j) {
            const long hh = r / vph, d = r % vph;      // (NonlinAttention: hh = 0, d = r)
            const float x = j < L && d < nv ? a->v[((long)b * L + j) * vcols + hh * nv + d]
                                            : (((r + j) & 1) ? -a->stale : a->stale);
            dh[j] = (bf16)x;
            if (dl) dl[j] = j < L && d < nv ? (bf16)(x - (float)dh[j]) : (bf16)x;
          }
        }
      f.vh = dev.up(vh.data(), vh.size());
      f.vl = split3 ? dev.up(vl.data(), vl.size()) : nullptr;
      f.ldv = Lpad; f.sv_b = vrows * Lpad; f.nv = nv;
      bf16 *oh = up16(a->oh, M, a->ldo), *ol = up16(a->ol, M, a->ldo), *oh2 = up16(a->oh2, M, a->ldo);
      f.oh = oh + (size_t)G * a->ldo; f.ol = ol ? ol + (size_t)G * a->ldo : nullptr;
      f.oh2 = oh2 ? oh2 + (size_t)G * a->ldo : nullptr; f.ldo = a->ldo;
      if (na) {
        const long ldy = round_up(nv, 8);
        std::vector<bf16> yh, yl;
        chk_act(a->y, M, nv, ldy, split3, yh, yl);
        f.mulh = dev.up(yh.data(), yh.size());
        f.mull = split3 ? dev.up(yl.data(), yl.size()) : nullptr;
        f.ldmul = ldy; f.vrows_per_head = 0; f.ocol_per_head = 0;
        if (split3) attn_na_v1<3, 0>(f, nv, s);
        else if (a->form == 1) attn_na_v1<1, 1>(f, nv, s);
        else attn_na_v1<1, 0>(f, nv, s);
      } else {
        f.vrows_per_head = (int)vph; f.ocol_per_head = nv;
        if (split3) launch_attn_sa<3>(f, s);
        else if (a->form == 1) launch_attn_sa_tp<0>(f, s);
        else if (a->form == 2) launch_attn_sa_tp<0, 1>(f, s);
        else launch_attn_sa<1>(f, s);
      }
      ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
      down16(a->oh, oh, M, a->ldo); down16(a->ol, ol, M, a->ldo); down16(a->oh2, oh2, M, a->ldo);
    }
  }
  const AttnLaunchRec& r = g_zv_last_attn;       // the last launch: the kind's own kernel
  const int rec[8] = {r.kernel, r.split, r.a, r.b, r.tpm, r.gx, r.gy, r.gz};
  memcpy(a->launch, rec, sizeof(rec));
  ZV_API_END
}

int zv_mx8_quantize(const float* x, int rows, int K, uint8_t* q, uint8_t* s) {
  ZV_API_BEGIN
  ZV_REQUIRE(x && q && s && rows >= 0 && K > 0, "bad arguments");
  mx8_quantize_host(x, K, rows, K, q, round_up(K, MX8_KSTEP), s);
  ZV_API_END
}

int zv_mx8_gemm_check(int M, int N, int K, const float* A, const float* W, float* C, uint8_t* Aq,
                      uint8_t* As) {
  ZV_API_BEGIN
  ZV_REQUIRE(A && W && C && M > 0 && N > 0 && K > 0 && K % MX8_KSTEP == 0 && N % 8 == 0,
             "zv_mx8_gemm_check: K a multiple of 128, N of 8");
  hipStream_t s = nullptr;
  const long Np = round_up(N, 128);
  std::vector<bf16> ah((size_t)M * K);
  for (size_t i = 0; i < ah.size(); ++i) ah[i] = (bf16)A[i];
  std::vector<float> wp((size_t)Np * K, 0.f);
  memcpy(wp.data(), W, (size_t)N * K * 4);
  std::vector<uint8_t> wq((size_t)Np * K), ws((size_t)Np * K / MX8_BLOCK);
  mx8_quantize_host(wp.data(), K, (int)Np, K, wq.data(), K, ws.data());
  ChkDev dev;
  uint8_t* dAq = dev.make<uint8_t>((size_t)M * K);
  uint8_t* dAs = dev.make<uint8_t>((size_t)M * K / MX8_BLOCK);
  const uint8_t* dWq = dev.up(wq.data(), wq.size());
  const uint8_t* dWs = dev.up(ws.data(), ws.size());
  float* dC = dev.zero<float>((size_t)M * N);
  Act a16;                                 // the bf16 operand and where its MX-fp8 copy goes
  a16.h = dev.up(ah.data(), ah.size()); a16.ld = K;
  a16.q = dAq; a16.qs = dAs; a16.ldq = K;
  LinearPolicy().pack8(a16, M, K, s);
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.nz2 = 1; p.Brows = (int)Np;
  p.Ah = reinterpret_cast<const bf16*>(dAq); p.lda = K; p.As = dAs; p.ldas = K / MX8_BLOCK;
  p.Bh = reinterpret_cast<const bf16*>(dWq); p.ldb = K; p.Bs = dWs; p.ldbs = K / MX8_BLOCK;
  p.bias = dev.zero<float>((size_t)N); p.C = dC; p.ldc = N; p.resid = dC; p.rows_per_group = 1; p.rpb = 1;
  launch_gemm<128, 128, 2, 2, 8, EPI_STD, 2, 2, MX8_KSTEP, 0, 0, 1>(p, 1, s, "mx8_check", true, -1);
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  dev.down(C, dC, (size_t)M * N);
  if (Aq) dev.down(Aq, dAq, (size_t)M * K);
  if (As) dev.down(As, dAs, (size_t)M * K / MX8_BLOCK);
  ZV_API_END
}

// ---------------------------------------------------------------------------
// zv_linear_check / zv_ffn_check: one linear through the engine's dispatch, and the fused
// FeedForward alone, on host arrays with canary-guarded outputs
// ---------------------------------------------------------------------------
int zv_linear_check(zv_linear_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->M > 0 && a->N > 0 && a->K > 0 && a->A && a->W && a->bias && a->guard >= 0 &&
                 (a->split == 1 || a->split == 2 || a->split == 3) && a->form >= ZV_LIN_PLAIN &&
                 a->form <= ZV_LIN_GLU_DW,
             "zv_linear_check: bad arguments");
  const int M = a->M, N = a->N, K = a->K, form = a->form, G = a->guard;
  const bool split3 = a->split == 3;
  const bool fused = form >= ZV_LIN_TRANS;
  const bool resid = form >= ZV_LIN_RESID && form <= ZV_LIN_RESID_RV_COPY;
  const bool rv = form == ZV_LIN_RESID_RV || form == ZV_LIN_RESID_RV_COPY;
  const bool wantC = form == ZV_LIN_PLAIN_F32 || (resid && form != ZV_LIN_RESID_RV_COPY);
  const bool wantT = form == ZV_LIN_TRANS || form == ZV_LIN_NA;
  ZV_REQUIRE(a->split != 2 || (form == ZV_LIN_PLAIN && !a->act) || form == ZV_LIN_TRANS,
             "zv_linear_check: split 2 is the plain form without activation, or TRANS");
  ZV_REQUIRE(wantC == (a->C != nullptr) && (!a->C || a->ldc >= N) && (!resid || a->resid) &&
                 (form != ZV_LIN_RESID_BYP || (a->orig && a->byp)) &&
                 (!rv || (a->rowvec && a->rows_per_group > 0)) && (form != ZV_LIN_RESID_RV_COPY || a->ldc >= N),
             "zv_linear_check: the form's fp32 operands");
  const bool glu = form == ZV_LIN_GLU || form == ZV_LIN_GLU_DW;
  const int wch = form == ZV_LIN_NA ? N / 3 : glu ? N / 2 : N;   // width of Ch
  const bool needCh = form == ZV_LIN_PLAIN || form == ZV_LIN_RESID_RV_COPY || form == ZV_LIN_NA || glu;
  ZV_REQUIRE((!needCh || a->Ch) && (form != ZV_LIN_PLAIN_F32 || !a->Ch) && (form != ZV_LIN_TRANS || !a->Ch) &&
                 (!a->Ch || a->ldch >= wch) && (a->Cl != nullptr) == (split3 && a->Ch != nullptr),
             "zv_linear_check: the form's 16-bit outputs (Cl with split 3 only)");
  ZV_REQUIRE(wantT == (a->Cth != nullptr) && (!wantT || (a->rpb > 0 && a->ldct >= a->rpb)) &&
                 (a->Ctl != nullptr) == (split3 && wantT),
             "zv_linear_check: the transposed outputs");
  ZV_REQUIRE((form != ZV_LIN_NA || N % 48 == 0) && (!glu || N % 32 == 0), "zv_linear_check: NA / GLU widths");
  // the fused GLU + depthwise conv: its argument errors by name (LinearPolicy::glu_dw_fits decides below)
  const int dwk = a->dw_ks;
  ZV_REQUIRE(form != ZV_LIN_GLU_DW || (a->dw_w && a->dw_b && a->dw_L > 0 && M % a->dw_L == 0),
             "zv_linear_check: GLU_DW needs the taps, the conv bias and whole utterances of dw_L rows");
  ZV_REQUIRE(form != ZV_LIN_GLU_DW || (a->split == 1 && N == 2 * 512 && (dwk == 7 || dwk == 15 || dwk == 31)),
             "zv_linear_check: GLU_DW is the 16-bit product at 512 channels with kernel size 7, 15 or 31");
  ZV_REQUIRE(form != ZV_LIN_GLU_DW || a->ldch % 8 == 0, "zv_linear_check: GLU_DW output rows of a multiple of 8 elements");

  LinearPolicy policy;                     // the engine's dispatch policy (its run-time knobs)
  WeightStore store;
  std::vector<int> perm(N);               // the fused epilogues' row order (identity otherwise)
  for (int n = 0; n < N; ++n) perm[n] = n;
  if (form == ZV_LIN_NA) perm = zv_engine::perm_na(N / 3);
  if (glu) perm = zv_engine::perm_glu(N / 2);
  std::vector<float> wp((size_t)N * K), bp(N);
  for (int n = 0; n < N; ++n) {
    memcpy(&wp[(size_t)n * K], a->W + (size_t)perm[n] * K, (size_t)K * sizeof(float));
    bp[n] = a->bias[perm[n]];
  }
  const Linear Lw = store.make_linear(wp.data(), N, K, bp.data());

  ChkDev dev;
  hipStream_t s = nullptr;
  Act A;
  {
    std::vector<bf16> h, l;
    A.ld = round_up(K, 64);
    chk_act(a->A, M, K, A.ld, split3, h, l);
    A.h = dev.up(h.data(), h.size());
    if (split3) A.l = dev.up(l.data(), l.size());
  }
  const long rows = (long)M + 2 * G;
  float* dC = nullptr;
  bf16 *dCh = nullptr, *dCl = nullptr, *dCth = nullptr, *dCtl = nullptr;
  const int nutt = wantT ? cdiv(M, a->rpb) : 0, rows_t = form == ZV_LIN_NA ? N / 3 : N;
  const long trows = wantT ? (long)nutt * rows_t + 2 * G : 0;
  if (a->C) {
    std::vector<float> hc(a->C, a->C + (size_t)rows * a->ldc);
    if (resid)
      for (long m = 0; m < M; ++m)
        memcpy(&hc[(size_t)(G + m) * a->ldc], a->resid + m * N, (size_t)N * sizeof(float));
    dC = dev.up(hc.data(), hc.size());
  }
  if (a->Ch) dCh = reinterpret_cast<bf16*>(dev.up(a->Ch, (size_t)rows * a->ldch));
  if (a->Cl) dCl = reinterpret_cast<bf16*>(dev.up(a->Cl, (size_t)rows * a->ldch));
  if (a->Cth) dCth = reinterpret_cast<bf16*>(dev.up(a->Cth, (size_t)trows * a->ldct));
  if (a->Ctl) dCtl = reinterpret_cast<bf16*>(dev.up(a->Ctl, (size_t)trows * a->ldct));
  const uint8_t* dmask = a->rowmask ? dev.up(a->rowmask, (size_t)M) : nullptr;

  if (!fused) {
    Out o;
    o.act_fn = a->act;
    if (dC) { o.C = dC + (size_t)G * a->ldc; o.ldc = a->ldc; }
    if (dCh) { o.act.h = dCh + (size_t)G * a->ldch; o.act.ld = a->ldch; }
    if (dCl) o.act.l = dCl + (size_t)G * a->ldch;
    if (resid) {
      if (o.C) {
        o.resid = o.C;                     // in place, as the engine updates its stream
      } else {
        o.ldc = a->ldc;
        std::vector<float> r = chk_pad(a->resid, M, N, a->ldc);
        o.resid = dev.up(r.data(), r.size());
      }
    }
    if (form == ZV_LIN_RESID_BYP) {
      std::vector<float> og = chk_pad(a->orig, M, N, a->ldc);
      o.orig = dev.up(og.data(), og.size());
      o.byp = dev.up(a->byp, (size_t)N);
    }
    if (rv) {
      o.rowvec = dev.up(a->rowvec, (size_t)cdiv(M, a->rows_per_group) * N);
      o.rowvec_ld = N; o.rows_per_group = a->rows_per_group;
    }
    if (a->split == 2) policy.attn_in_wsplit(Lw, A, M, o, s);
    else if (split3) policy.linear16<3>(Lw, A, M, o, s);
    else policy.linear16<1>(Lw, A, M, o, s);
  } else {
    GemmParams p = LinearPolicy::gp_linear(Lw, A, M);
    if (a->split == 2) p.Al = nullptr;
    if (dCh) { p.Ch = dCh + (size_t)G * a->ldch; p.ldch = a->ldch; }
    if (dCl) p.Cl = dCl + (size_t)G * a->ldch;
    if (wantT) {
      p.Cth = dCth + (size_t)G * a->ldct;
      if (dCtl) p.Ctl = dCtl + (size_t)G * a->ldct;
      p.ldct = a->ldct; p.rpb = a->rpb; p.sCt = (long)rows_t * a->ldct;
    }
    if (glu) p.rowmask = dmask;
    if (form == ZV_LIN_GLU_DW) {
      p.dw_w = dev.up(a->dw_w, (size_t)(N / 2) * dwk); p.dw_b = dev.up(a->dw_b, (size_t)(N / 2));
      p.dw_out = p.Ch; p.ld_dw = p.ldch; p.dw_L = a->dw_L;
      ZV_REQUIRE(policy.glu_dw_fits(p, N / 2, dwk),
                 "zv_linear_check: GLU_DW operands (the engine would take the unfused pair)");
      policy.launch_glu_dw(p, dwk, s, "glu_dw_check");
    } else if (form == ZV_LIN_NA) {
      if (split3) policy.launch_na_in<3>(p, s); else policy.launch_na_in<1>(p, s);
    } else if (form == ZV_LIN_TRANS) {
      if (split3) policy.launch_value_t<3>(p, false, true, s);
      else policy.launch_value_t<1>(p, a->split == 2, Lw.lo != nullptr, s);
    } else {
      if (split3) policy.launch_glu_in<3>(p, false, s); else policy.launch_glu_in<1>(p, false, s);
    }
  }
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  chk_record(a->launch, &a->num_cus);
  if (a->C) dev.down(a->C, dC, (size_t)rows * a->ldc);
  if (a->Ch) dev.down(a->Ch, reinterpret_cast<uint16_t*>(dCh), (size_t)rows * a->ldch);
  if (a->Cl) dev.down(a->Cl, reinterpret_cast<uint16_t*>(dCl), (size_t)rows * a->ldch);
  if (a->Cth) dev.down(a->Cth, reinterpret_cast<uint16_t*>(dCth), (size_t)trows * a->ldct);
  if (a->Ctl) dev.down(a->Ctl, reinterpret_cast<uint16_t*>(dCtl), (size_t)trows * a->ldct);
  ZV_API_END
}

int zv_ffn_check(zv_ffn_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->M > 0 && a->H > 0 && a->H % (2 * FFN_HC) == 0 && a->form >= 0 && a->form <= 3 &&
                 a->guard >= 0 && a->part_slots >= 0 && (a->x || a->K > 0) && a->W1 && a->b1 && a->W2 && a->b2 &&
                 a->resid && a->C && a->ldc >= FFN_D && (!a->Ch || a->ldch >= FFN_D),
             "zv_ffn_check: bad arguments");
  const int M = a->M, H = a->H, form = a->form, G = a->guard, D = FFN_D;
  const bool norm = form == 3, byp = form == 2 || norm, rv = a->rowvec != nullptr;
  const bool pre = a->K > 0;
  ZV_REQUIRE(!pre || (byp && a->A && a->Wp && a->bp), "zv_ffn_check: the pre-projection belongs to forms 2 and 3");
  ZV_REQUIRE((form == 1) == (rv && !norm) || norm || pre, "zv_ffn_check: the row vector belongs to form 1 (or 3)");
  ZV_REQUIRE((!rv || a->rows_per_group > 0) && (!byp || (a->orig && a->byp)) && (!norm || a->nb) &&
                 (form == 0 || a->Ch) && (norm || (!a->Cl && !a->C2h && !a->C2l)) &&
                 (!a->C2l || a->C2h),
             "zv_ffn_check: the form's operands");
  ZV_REQUIRE(a->part_slots <= zv_num_cus(), "zv_ffn_check: more lines than CUs");
  WeightStore store;
  const Linear L1 = store.make_linear(a->W1, H, D, a->b1);
  const Linear L2 = store.make_linear(a->W2, D, H, a->b2);
  ChkDev dev;
  hipStream_t s = nullptr;
  const long n = (long)H * D;
  bf16* w1f = dev.make<bf16>((size_t)n);
  bf16* w2f = dev.make<bf16>((size_t)n);
  ffn_pack_weights(L1, L2, H, w1f, w2f, s);
  FfnParams q{};
  q.H = H; q.nseg = 1;
  FfnSeg& g = q.seg[0];
  g.M = M;
  if (pre) {
    // the pre-projection form: Wp (512, K) packed as the engine packs conv_sa_out, W1 in the tile's
    // register order; A in rows of lda = 32 ceil(K / 32) + 8 elements, zero past K
    const int K = a->K;
    const Linear Lp = store.make_linear(a->Wp, D, K, a->bp);
    const int nkp = ffn_pre_chunks(K);
    bf16* wpf = dev.make<bf16>((size_t)nkp * FFN_HC * D);
    ffn_pack_pre_weights(L1, H, w1f, Lp, wpf, s);
    q.Wpf = wpf; q.bp = Lp.b; q.nkp = nkp; q.lda = (long)nkp * FFN_HC + 8;
    std::vector<bf16> h, l;
    chk_act(a->A, M, K, q.lda, false, h, l);
    g.A = dev.up(h.data(), h.size());
  } else {
    std::vector<bf16> h, l;
    chk_act(a->x, M, D, D, false, h, l);
    g.X = dev.up(h.data(), h.size());
    q.ldx = D;
  }
  q.W1f = w1f; q.b1 = L1.b; q.W2f = w2f; q.b2 = L2.b;
  const long rows = (long)M + 2 * G;
  // C: resid in its interior (in place), or for the BiasNorm epilogue orig (C == orig, resid apart)
  std::vector<float> hc(a->C, a->C + (size_t)rows * a->ldc);
  for (long m = 0; m < M; ++m)
    memcpy(&hc[(size_t)(G + m) * a->ldc], (norm ? a->orig : a->resid) + m * D, (size_t)D * sizeof(float));
  float* dC = dev.up(hc.data(), hc.size());
  g.C = dC + (size_t)G * a->ldc; q.ldc = a->ldc;
  auto padded = [&](const float* x) {
    std::vector<float> v = chk_pad(x, M, D, a->ldc);
    return dev.up(v.data(), v.size());
  };
  if (norm) { g.resid = padded(a->resid); g.orig = g.C; }
  else { g.resid = g.C; if (byp) g.orig = padded(a->orig); }
  if (byp) q.byp = dev.up(a->byp, (size_t)D);
  if (norm) { q.nb = dev.up(a->nb, (size_t)D); q.log_scale = a->log_scale; }
  if (rv) {
    g.rowvec = dev.up(a->rowvec, (size_t)cdiv(M, a->rows_per_group) * D);
    q.rowvec_ld = D; q.rows_per_group = a->rows_per_group;
  }
  uint16_t* host16[4] = {a->Ch, a->Cl, a->C2h, a->C2l};
  bf16* dev16[4] = {};
  for (int i = 0; i < 4; ++i)
    if (host16[i]) dev16[i] = reinterpret_cast<bf16*>(dev.up(host16[i], (size_t)rows * a->ldch));
  q.ldch = a->Ch ? a->ldch : 0;
  auto inner = [&](bf16* p) { return p ? p + (size_t)G * a->ldch : nullptr; };
  g.Ch = inner(dev16[0]); g.Cl = inner(dev16[1]); g.C2h = inner(dev16[2]); g.C2l = inner(dev16[3]);
  if (a->part_slots > 0) {   // the persistent line schedule's scratch, zero-filled
    q.part_slots = a->part_slots;
    q.part = dev.zero<float>((size_t)a->part_slots * FFN_PART_FLOATS);
    q.flag = dev.zero<unsigned>((size_t)a->part_slots + 64);
  }
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  launch_ffn(q, s, norm ? "ffn_norm_check" : "ffn_check");
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  chk_record(a->launch, &a->num_cus);
  volatile unsigned* e = zv_dev_err_host();
  if (*e != 0) {
    *e = 0;
    throw std::runtime_error("zv_ffn_check: the device error word was set (a C item outwaited its producer)");
  }
  dev.down(a->C, dC, (size_t)rows * a->ldc);
  for (int i = 0; i < 4; ++i)
    if (host16[i]) dev.down(host16[i], reinterpret_cast<uint16_t*>(dev16[i]), (size_t)rows * a->ldch);
  ZV_API_END
}

// ---------------------------------------------------------------------------
// zv_dwconv_check / zv_stackedge_check: the ConvolutionModule's depthwise conv through
// launch_dwconv, and the kernels at the stack boundaries as zv_engine launches them, on host
// arrays with canary-guarded outputs
// ---------------------------------------------------------------------------
int zv_dwconv_check(zv_dwconv_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->B > 0 && a->L > 0 && a->C > 0 && a->ks > 0 && (a->split == 1 || a->split == 3) &&
                 a->guard >= 0 && a->g && a->w && a->bias && a->Oh && a->ldin >= a->C && a->ldout >= a->C,
             "zv_dwconv_check: bad arguments");
  ZV_REQUIRE((a->Ol != nullptr) == (a->split == 3), "zv_dwconv_check: Ol with split 3 only");
  ZV_REQUIRE(!a->q || (a->qs && a->ldq >= a->C && a->ldq % MX8_KSTEP == 0),
             "zv_dwconv_check: the fp8 copy needs its scales and a row stride that is a multiple of 128");
  const int B = a->B, L = a->L, C = a->C, G = a->guard;
  const long M = (long)B * L, rows = M + 2 * G;
  const bool split3 = a->split == 3;
  ChkDev dev;
  hipStream_t s = nullptr;
  std::vector<bf16> h, l;
  chk_act(a->g, M, C, a->ldin, split3, h, l);
  const bf16* ih = dev.up(h.data(), h.size());
  const bf16* il = split3 ? dev.up(l.data(), l.size()) : nullptr;
  const float* w = dev.up(a->w, (size_t)C * a->ks);
  const float* bias = dev.up(a->bias, (size_t)C);
  bf16* dOh = reinterpret_cast<bf16*>(dev.up(a->Oh, (size_t)rows * a->ldout));
  bf16* dOl = split3 ? reinterpret_cast<bf16*>(dev.up(a->Ol, (size_t)rows * a->ldout)) : nullptr;
  const long ldqs = a->ldq / MX8_BLOCK;
  uint8_t* dq = a->q ? dev.up(a->q, (size_t)rows * a->ldq) : nullptr;
  uint8_t* dqs = a->q ? dev.up(a->qs, (size_t)rows * ldqs) : nullptr;
  launch_dwconv(ih, il, a->ldin, w, bias, dOh + (size_t)G * a->ldout, dOl ? dOl + (size_t)G * a->ldout : nullptr,
                a->ldout, B, L, C, a->ks, s, dq ? dq + (size_t)G * a->ldq : nullptr,
                dqs ? dqs + (size_t)G * ldqs : nullptr, a->ldq);
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  chk_record(a->launch, &a->num_cus);
  dev.down(a->Oh, reinterpret_cast<uint16_t*>(dOh), (size_t)rows * a->ldout);
  if (dOl) dev.down(a->Ol, reinterpret_cast<uint16_t*>(dOl), (size_t)rows * a->ldout);
  if (dq) {
    dev.down(a->q, dq, (size_t)rows * a->ldq);
    dev.down(a->qs, dqs, (size_t)rows * ldqs);
  }
  ZV_API_END
}

int zv_stackedge_check(zv_stackedge_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->kind >= ZV_SE_DOWNSAMPLE && a->kind <= ZV_SE_BIASNORM && a->B > 0 && a->L > 0 &&
                 a->guard >= 0 && (a->kind == ZV_SE_MASK || (a->C > 0 && a->C % 4 == 0 && a->x)),
             "zv_stackedge_check: bad arguments");
  const int kind = a->kind, B = a->B, L = a->L, C = a->C, ds = a->ds, G = a->guard;
  const bool resample = kind <= ZV_SE_MASK;
  ZV_REQUIRE(!resample || ds >= 1, "zv_stackedge_check: the downsampling factor");
  const int dL = resample ? (L + ds - 1) / ds : 0;
  const long M = (long)B * L, Md = (long)B * dL;
  ChkDev dev;
  hipStream_t s = nullptr;
  EdgeLaunch ran{};                                  // kernel form, grid blocks, block threads
  // a canary-guarded fp32 output of `n` rows of C, with `fill` (or nothing) in its interior
  auto up32 = [&](long n, const float* fill) {
    std::vector<float> hc(a->out, a->out + (size_t)(n + 2 * G) * C);
    if (fill) memcpy(&hc[(size_t)G * C], fill, (size_t)n * C * sizeof(float));
    return dev.up(hc.data(), hc.size());
  };
  auto up16 = [&](uint16_t* p, long n) {
    return p ? reinterpret_cast<bf16*>(dev.up(p, (size_t)(n + 2 * G) * a->ldact)) : nullptr;
  };
  auto in16 = [&](bf16* p) { return p ? p + (size_t)G * a->ldact : nullptr; };
  auto down16 = [&](uint16_t* p, bf16* d, long n) {
    if (p) dev.down(p, reinterpret_cast<uint16_t*>(d), (size_t)(n + 2 * G) * a->ldact);
  };
  if (kind == ZV_SE_DOWNSAMPLE) {
    ZV_REQUIRE(a->w && a->out, "zv_stackedge_check: downsample needs the weights and out");
    const float* in = dev.up(a->x, (size_t)M * C);
    const float* w = dev.up(a->w, (size_t)ds);
    float* d = up32(Md, nullptr);
    ran = launch_downsample(in, d + (size_t)G * C, B, L, dL, C, ds, w, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    dev.down(a->out, d, (size_t)(Md + 2 * G) * C);
  } else if (kind == ZV_SE_UPSAMPLE) {
    ZV_REQUIRE(a->w && a->orig && a->out, "zv_stackedge_check: upsample needs the scale, orig and out");
    const float* d = dev.up(a->x, (size_t)Md * C);
    const float* sc = dev.up(a->w, (size_t)C);
    float* o = up32(M, a->orig);                     // in place over orig, as the engine's stream
    float* main = o + (size_t)G * C;
    ran = launch_upsample_combine(main, d, sc, main, B, L, dL, C, ds, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    dev.down(a->out, o, (size_t)(M + 2 * G) * C);
  } else if (kind == ZV_SE_MASK) {
    ZV_REQUIRE(a->mask && a->mout, "zv_stackedge_check: the mask and its output");
    const uint8_t* in = dev.up(a->mask, (size_t)M);
    uint8_t* o = dev.up(a->mout, (size_t)(Md + 2 * G));
    ran = launch_mask_downsample(in, o + G, B, L, dL, ds, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    dev.down(a->mout, o, (size_t)(Md + 2 * G));
  } else if (kind == ZV_SE_ENTRY) {
    ZV_REQUIRE(a->h && a->h2 && a->ldact >= C && a->ldact % 4 == 0 && (!a->rowvec || a->rows_per_group > 0),
               "zv_stackedge_check: stack entry writes h (src) and h2 (cur), rows of a multiple of 4");
    const float* src = dev.up(a->x, (size_t)M * C);
    const float* rv = a->rowvec ? dev.up(a->rowvec, (size_t)cdiv(M, a->rows_per_group) * C) : nullptr;
    float* cur = a->out ? up32(M, nullptr) : nullptr;
    bf16 *h = up16(a->h, M), *l = up16(a->l, M), *h2 = up16(a->h2, M), *l2 = up16(a->l2, M);
    ran = launch_stack_entry(src, rv, cur ? cur + (size_t)G * C : nullptr, in16(h), in16(l), in16(h2), in16(l2),
                             a->ldact, M, C, rv ? a->rows_per_group : 1, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    if (cur) dev.down(a->out, cur, (size_t)(M + 2 * G) * C);
    down16(a->h, h, M); down16(a->l, l, M); down16(a->h2, h2, M); down16(a->l2, l2, M);
  } else {   // BiasNorm + bypass, in place over orig
    ZV_REQUIRE(a->nb && a->w && a->orig && a->out && a->h && a->ldact >= C && a->ldact % 4 == 0 &&
                   (!a->l2 || a->h2) && (!a->rowvec || a->rows_per_group > 0),
               "zv_stackedge_check: BiasNorm needs nb, the bypass scale, orig, out and h");
    ZV_REQUIRE(!a->q2 || (a->h2 && a->qs2 && C % 256 == 0 && a->ldq >= C && a->ldq % MX8_KSTEP == 0),
               "zv_stackedge_check: the fp8 copy belongs to h2, channels a multiple of 256");
    const float* x = dev.up(a->x, (size_t)M * C);
    const float* nb = dev.up(a->nb, (size_t)C);
    const float* byp = dev.up(a->w, (size_t)C);
    const float* rv = a->rowvec ? dev.up(a->rowvec, (size_t)cdiv(M, a->rows_per_group) * C) : nullptr;
    float* o = up32(M, a->orig);
    float* src = o + (size_t)G * C;
    bf16 *h = up16(a->h, M), *l = up16(a->l, M), *h2 = up16(a->h2, M), *l2 = up16(a->l2, M);
    const long ldqs = a->ldq / MX8_BLOCK;
    uint8_t* q2 = a->q2 ? dev.up(a->q2, (size_t)(M + 2 * G) * a->ldq) : nullptr;
    uint8_t* qs2 = a->q2 ? dev.up(a->qs2, (size_t)(M + 2 * G) * ldqs) : nullptr;
    uint8_t* q2i = q2 ? q2 + (size_t)G * a->ldq : nullptr;
    uint8_t* qs2i = qs2 ? qs2 + (size_t)G * ldqs : nullptr;
    ran = launch_biasnorm_bypass(x, src, nb, a->log_scale, byp, src, in16(h), in16(l), in16(h2), in16(l2), a->ldact,
                                 rv, rv ? a->rows_per_group : 1, M, C, q2i, qs2i, a->ldq, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    dev.down(a->out, o, (size_t)(M + 2 * G) * C);
    down16(a->h, h, M); down16(a->l, l, M); down16(a->h2, h2, M); down16(a->l2, l2, M);
    if (q2) {
      dev.down(a->q2, q2, (size_t)(M + 2 * G) * a->ldq);
      dev.down(a->qs2, qs2, (size_t)(M + 2 * G) * ldqs);
    }
  }
  const int rec[8] = {kind, ran.form, ran.blocks, ran.threads, 0, 0, 0, 0};
  memcpy(a->launch, rec, sizeof(rec));
  a->num_cus = zv_num_cus();
  ZV_API_END
}

// zv_padrow_check: the row padding mode's two kernels through the engine's launches: the lengths of
// a host mask, then the downsample of x clamped at them, both between canary guards
int zv_padrow_check(zv_padrow_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->B > 0 && a->L > 0 && a->C > 0 && a->C % 4 == 0 && a->ds >= 1 && a->guard >= 0 && a->mask &&
                 a->x && a->w && a->lens && a->out,
             "zv_padrow_check: bad arguments");
  const int B = a->B, L = a->L, C = a->C, ds = a->ds, G = a->guard;
  const int dL = (L + ds - 1) / ds;
  const long M = (long)B * L, Md = (long)B * dL;
  ChkDev dev;
  hipStream_t s = nullptr;
  const uint8_t* mask = dev.up(a->mask, (size_t)M);
  const float* in = dev.up(a->x, (size_t)M * C);
  const float* w = dev.up(a->w, (size_t)ds);
  int32_t* n = dev.up(a->lens, (size_t)B + 2 * G);
  float* d = dev.up(a->out, (size_t)(Md + 2 * G) * C);
  const EdgeLaunch r0 = launch_row_len(mask, n + G, B, L, s);
  const EdgeLaunch r1 = launch_downsample_row(in, d + (size_t)G * C, n + G, B, L, dL, C, ds, w, s);
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  dev.down(a->lens, n, (size_t)B + 2 * G);
  dev.down(a->out, d, (size_t)(Md + 2 * G) * C);
  const int rec[8] = {0, r0.blocks, r0.threads, r1.blocks, r1.threads, 0, 0, 0};
  memcpy(a->launch, rec, sizeof(rec));
  a->num_cus = zv_num_cus();
  ZV_API_END
}

// ---------------------------------------------------------------------------
// zv_solve_check: the kernels around the decoder (operand build, Euler / CFG, mask copy, fill, timestep
// embedding, the small fp32 linear, the positional projection, the text-side lookups) through the
// launch functions zv_engine calls (zv_elem.inc), on host arrays with canary-guarded outputs; and the
// solve's two host decisions, zv_time_steps and zv_cfg_plan (no GPU).
// ---------------------------------------------------------------------------
int zv_solve_check(zv_solve_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->kind >= ZV_SV_BUILD_INPUT && a->kind <= ZV_SV_SPEECH_COND && a->guard >= 0,
             "zv_solve_check: bad arguments");
  const int kind = a->kind;
  const size_t G = (size_t)a->guard;
  ChkDev dev;
  hipStream_t s = nullptr;
  EdgeLaunch ran{};
  // a canary-guarded output of `rows` rows of stride ld (guard rows at both ends), as the caller filled it
  auto up32 = [&](size_t rows, size_t ld) { return dev.up(a->out, (rows + 2 * G) * ld); };
  auto down32 = [&](float* d, size_t rows, size_t ld) { dev.down(a->out, d, (rows + 2 * G) * ld); };
  auto sync = [&] { ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize())); };
  if (kind == ZV_SV_BUILD_INPUT) {
    const int B = a->B, T = a->T, Fx = a->Fx, Ft = a->Ft, Fs = a->Fs, Fin = Fx + Ft + Fs;
    ZV_REQUIRE(B > 0 && T > 0 && Fx > 0 && Ft > 0 && Fs > 0 && (a->copies == 1 || a->copies == 2) && a->ld >= Fin &&
                   a->x && a->tc && a->sc && a->oh,
               "zv_solve_check: BUILD_INPUT needs x, tc, sc, oh, copies 1 / 2, ld >= Fx + Ft + Fs");
    const size_t bt = (size_t)B * T, rows = (size_t)a->copies * bt, n16 = (rows + 2 * G) * a->ld;
    const float* x = dev.up(a->x, bt * Fx);
    const float* tc = dev.up(a->tc, bt * Ft);
    const float* sc = dev.up(a->sc, bt * Fs);
    uint16_t* oh = dev.up(a->oh, n16);
    uint16_t* ol = a->ol ? dev.up(a->ol, n16) : nullptr;
    ran = launch_build_input(x, tc, sc, reinterpret_cast<bf16*>(oh) + G * a->ld,
                             ol ? reinterpret_cast<bf16*>(ol) + G * a->ld : nullptr, a->ld, B, T, Fx, Ft, Fs,
                             a->copies, a->zero_speech, s);
    sync();
    dev.down(a->oh, oh, n16);
    if (ol) dev.down(a->ol, ol, n16);
  } else if (kind == ZV_SV_EULER || kind == ZV_SV_CFG_COMBINE) {
    const bool euler = kind == ZV_SV_EULER;
    const int cfg = euler ? a->cfg : 1;
    const long n = a->n;
    ZV_REQUIRE(n > 0 && a->v && a->out && (cfg == 0 || cfg == 1) && (!euler || a->x), "zv_solve_check: EULER / CFG_COMBINE need v and out (EULER: x)");
    ZV_REQUIRE(!a->grows || (a->B > 0 && a->per_row > 0 && (long)a->B * a->per_row == n),
               "zv_solve_check: per-row scales need n = B * per_row");
    const float* v = dev.up(a->v, (size_t)(cfg ? 2 * n : n));
    const float* gr = a->grows ? dev.up(a->grows, (size_t)a->B) : nullptr;
    std::vector<float> ho(a->out, a->out + (size_t)n + 2 * G);
    if (euler) memcpy(&ho[G], a->x, (size_t)n * sizeof(float));   // in place over x, as the engine's solve
    float* o = dev.up(ho.data(), ho.size());
    ran = euler ? launch_euler_update(o + G, v, n, cfg, a->g, a->dt, gr, a->gmul, a->per_row > 0 ? a->per_row : n, s)
                : launch_cfg_combine(o + G, v, n, a->g, gr, a->gmul, a->per_row > 0 ? a->per_row : n, s);
    sync();
    dev.down(a->out, o, (size_t)n + 2 * G);
  } else if (kind == ZV_SV_MASK_COPY) {
    ZV_REQUIRE(a->n > 0 && a->copies >= 1 && a->mask && a->mout, "zv_solve_check: MASK_COPY needs the mask and mout");
    const uint8_t* in = dev.up(a->mask, (size_t)a->n);
    uint8_t* o = dev.up(a->mout, (size_t)a->n * a->copies + 2 * G);
    ran = launch_copy_u8(in, o + G, a->n, a->copies, s);
    sync();
    dev.down(a->mout, o, (size_t)a->n * a->copies + 2 * G);
  } else if (kind == ZV_SV_FILL) {
    ZV_REQUIRE(a->n > 0 && a->n < (1L << 30) && a->out, "zv_solve_check: FILL needs out");
    float* o = up32((size_t)a->n, 1);
    ran = launch_fill(o + G, a->value, (int)a->n, s);
    sync();
    down32(o, (size_t)a->n, 1);
  } else if (kind == ZV_SV_TEMB) {
    const int M = a->M, dim = a->N;
    ZV_REQUIRE(M > 0 && dim > 1 && a->x && a->W && a->out, "zv_solve_check: TEMB needs t (x), freqs (W), out");
    const float* t = dev.up(a->x, (size_t)M);
    const float* fr = dev.up(a->W, (size_t)(dim / 2));
    float* o = up32((size_t)M, (size_t)dim);
    ran = launch_timestep_embed(t, fr, o + G * dim, M, dim, s);
    sync();
    down32(o, (size_t)M, (size_t)dim);
  } else if (kind == ZV_SV_SMALL_LINEAR) {
    const int M = a->M, N = a->N, K = a->K;
    ZV_REQUIRE(M > 0 && N > 0 && K > 0 && a->ldin >= K && a->ldw >= K && a->ld >= N && a->x && a->W && a->out &&
                   (a->pre == 0 || a->pre == 1) && a->form >= -1 && a->form <= 1 && (!a->inplace || a->add),
               "zv_solve_check: SMALL_LINEAR needs x (M, ldin), W (N, ldw), out, pre 0 / 1, form -1 / 0 / 1");
    const float* in = dev.up(a->x, (size_t)M * a->ldin);
    const float* W = dev.up(a->W, (size_t)N * a->ldw);
    const float* b = a->bias ? dev.up(a->bias, (size_t)N) : nullptr;
    std::vector<float> ho(a->out, a->out + ((size_t)M + 2 * G) * a->ld);
    std::vector<float> hadd;
    if (a->add) hadd = chk_pad(a->add, M, N, a->ld);
    if (a->inplace)                                          // add == out, as the engine's e0 += guid(e1)
      for (int m = 0; m < M; ++m) memcpy(&ho[(G + m) * a->ld], a->add + (size_t)m * N, (size_t)N * sizeof(float));
    float* o = dev.up(ho.data(), ho.size());
    float* oi = o + G * a->ld;
    const float* add = a->inplace ? oi : (a->add ? dev.up(hadd.data(), hadd.size()) : nullptr);
    ran = launch_small_linear(in, (int)a->ldin, W, (int)a->ldw, b, add, oi, (int)a->ld, M, N, K, a->pre, a->form, s);
    sync();
    down32(o, (size_t)M, (size_t)a->ld);
  } else if (kind == ZV_SV_POSP) {
    const int L = a->T, nl = a->M, HPD = a->N, D = a->K;
    ZV_REQUIRE(L > 0 && nl > 0 && HPD > 0 && D > 0 && a->W && a->out, "zv_solve_check: POSP needs W (nl * HPD, D) and out");
    const size_t rows = (size_t)nl * (2 * (size_t)L - 1);
    const float* W = dev.up(a->W, (size_t)nl * HPD * D);
    float* o = up32(rows, (size_t)HPD);
    ran = launch_posp(W, o + G * HPD, L, nl, HPD, D, s);
    sync();
    down32(o, rows, (size_t)HPD);
  } else if (kind == ZV_SV_EMBED) {
    const int C = a->C, V = a->N;
    const long n = a->n;
    ZV_REQUIRE(n > 0 && C > 0 && V > 0 && a->ld >= C && a->tok && a->W && a->oh, "zv_solve_check: EMBED needs tok (n), W (N, C), oh");
    for (long i = 0; i < n; ++i) ZV_REQUIRE(a->tok[i] >= 0 && a->tok[i] < V, "zv_solve_check: token outside the table");
    const int64_t* tok = dev.up(a->tok, (size_t)n);
    const float* tab = dev.up(a->W, (size_t)V * C);
    const size_t n16 = ((size_t)n + 2 * G) * a->ld;
    uint16_t* oh = dev.up(a->oh, n16);
    uint16_t* ol = a->ol ? dev.up(a->ol, n16) : nullptr;
    ran = launch_embed(tok, tab, reinterpret_cast<bf16*>(oh) + G * a->ld, ol ? reinterpret_cast<bf16*>(ol) + G * a->ld : nullptr,
                       a->ld, n, C, s);
    sync();
    dev.down(a->oh, oh, n16);
    if (ol) dev.down(a->ol, ol, n16);
  } else if (kind == ZV_SV_SPK_ADD) {
    const int C = a->C;
    const long n = a->n;
    ZV_REQUIRE(n > 0 && C > 0 && a->x && a->spk && a->W && a->out, "zv_solve_check: SPK_ADD needs x (n, C), spk (n), W (2, C), out");
    for (long i = 0; i < n; ++i) ZV_REQUIRE(a->spk[i] >= -1 && a->spk[i] <= 1, "zv_solve_check: speaker code outside {-1, 0, 1}");
    const int8_t* spk = dev.up(a->spk, (size_t)n);
    const float* tab = dev.up(a->W, (size_t)2 * C);
    std::vector<float> ho(a->out, a->out + ((size_t)n + 2 * G) * C);
    memcpy(&ho[G * C], a->x, (size_t)n * C * sizeof(float));    // in place, as text_encode's output
    float* o = dev.up(ho.data(), ho.size());
    ran = launch_spk_add(o + G * C, spk, tab, n, C, s);
    sync();
    down32(o, (size_t)n, (size_t)C);
  } else if (kind == ZV_SV_TEXT_COND) {
    const int B = a->B, T = a->T, S = a->S, C = a->C;
    ZV_REQUIRE(B > 0 && T > 0 && S > 1 && C > 0 && a->x && a->lens && a->lens2 && a->out,
               "zv_solve_check: TEXT_COND needs x (B, S, C), lens (tokens), lens2 (frames), out");
    for (int b = 0; b < B; ++b)
      ZV_REQUIRE(a->lens[b] > 0 && a->lens[b] < S && a->lens2[b] >= 0, "zv_solve_check: 0 < tok_lens < S, feat_lens >= 0");
    const float* emb = dev.up(a->x, (size_t)B * S * C);
    const int* tl = dev.up(a->lens, (size_t)B);
    const int* fl = dev.up(a->lens2, (size_t)B);
    float* o = up32((size_t)B * T, (size_t)C);
    ran = launch_text_cond(emb, S, C, tl, fl, o + G * C, B, T, s);
    sync();
    down32(o, (size_t)B * T, (size_t)C);
  } else {   // ZV_SV_SPEECH_COND
    const int B = a->B, T = a->T, Tp = a->S, F = a->C;
    ZV_REQUIRE(B > 0 && T > 0 && Tp > 0 && F > 0 && a->x && a->lens && a->out,
               "zv_solve_check: SPEECH_COND needs x (B, S = Tp, C), lens (prompt lengths), out");
    const float* pf = dev.up(a->x, (size_t)B * Tp * F);
    const int* pl = dev.up(a->lens, (size_t)B);
    float* o = up32((size_t)B * T, (size_t)F);
    ran = launch_speech_cond(pf, Tp, pl, o + G * F, B, T, F, s);
    sync();
    down32(o, (size_t)B * T, (size_t)F);
  }
  const int rec[8] = {kind, ran.form, ran.blocks, ran.threads, 0, 0, 0, 0};
  memcpy(a->launch, rec, sizeof(rec));
  a->num_cus = zv_num_cus();
  ZV_API_END
}

int zv_time_steps(float t_start, float t_end, int num_step, float t_shift, float* out) {
  ZV_API_BEGIN
  ZV_REQUIRE(num_step >= 0 && out, "zv_time_steps: num_step >= 0 and out (num_step + 1 floats)");
  const std::vector<float> ts = solve_time_steps(t_start, t_end, num_step, t_shift);
  memcpy(out, ts.data(), ts.size() * sizeof(float));
  ZV_API_END
}

int zv_cfg_plan(float t, float guidance_scale, int has_rows, int rows_nonzero, int distill, int* copies,
                int* zero_speech, float* g, float* gmul) {
  ZV_API_BEGIN
  ZV_REQUIRE(copies && zero_speech && g && gmul, "zv_cfg_plan: null output");
  const CfgPlan p = cfg_plan(t, guidance_scale, has_rows != 0, rows_nonzero != 0, distill != 0);
  *copies = p.copies; *zero_speech = p.zero_speech; *g = p.g; *gmul = p.gmul;
  ZV_API_END
}

// the scheduled solve's host plan (sched_plan, zv_elem.inc: the function zv_engine::euler_sample_sched runs)
int zv_sched_plan(const zv_row_sched* rows, int B, int distill, int step, zv_sched_plan_out* out) {
  ZV_API_BEGIN
  ZV_REQUIRE(out != nullptr, "zv_sched_plan: null output");
  const SchedPlan p = sched_plan(reinterpret_cast<const SchedRow*>(rows), B, distill != 0);
  ZV_REQUIRE(step >= 0 && step < p.K, "zv_sched_plan: step outside [0, max num_step)");
  const SchedStep& st = p.steps[step];
  out->steps = p.K;
  out->total_rows = p.total_rows;
  out->active = st.A;
  out->copies = st.U;
  for (int j = 0; j < st.U + st.A; ++j) {
    if (out->dec_src) out->dec_src[j] = st.src[j];
    if (out->dec_zero_text) out->dec_zero_text[j] = st.zt[j];
    if (out->dec_zero_speech) out->dec_zero_speech[j] = st.zs[j];
    if (out->dec_t) out->dec_t[j] = st.t[j];
  }
  for (int i = 0; i < st.A; ++i) {
    if (out->act_row) out->act_row[i] = st.upd[i].row;
    if (out->act_dt) out->act_dt[i] = st.upd[i].dt;
    if (out->act_scale) out->act_scale[i] = distill ? st.gdec[i] : (st.upd[i].vu < 0 ? 0.0f : st.upd[i].g);
    if (out->act_cond) out->act_cond[i] = st.upd[i].vc;
    if (out->act_uncond) out->act_uncond[i] = st.upd[i].vu;
  }
  ZV_API_END
}

// ---------------------------------------------------------------------------
// zv_sched_check: the scheduled solve's kernels (operand build through the row map, mask gather, the
// scattered Euler update) through the launch functions zv_engine::euler_sample_sched calls, on host
// arrays with canary-guarded outputs.  Every index is checked here before a launch.
// ---------------------------------------------------------------------------
int zv_sched_check(zv_sched_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->kind >= ZV_SC_BUILD_INPUT && a->kind <= ZV_SC_EULER && a->guard >= 0, "zv_sched_check: bad arguments");
  const int kind = a->kind, B = a->B, T = a->T, N = a->N;
  const size_t G = (size_t)a->guard;
  ZV_REQUIRE(B > 0 && B <= 32767, "zv_sched_check: B must be in [1, 32767]");
  ChkDev dev;
  hipStream_t s = nullptr;
  EdgeLaunch ran{};
  int gy = 0;
  auto sync = [&] { ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize())); };
  auto row_map = [&](bool flags) {
    ZV_REQUIRE(N > 0 && N <= 65535 && a->src && (!flags || (a->zero_text && a->zero_speech)),
               "zv_sched_check: src (and the zero flags) of N decoder rows");
    std::vector<int> m(N);
    for (int j = 0; j < N; ++j) {
      ZV_REQUIRE(a->src[j] >= 0 && a->src[j] < B, "zv_sched_check: a source row outside [0, B)");
      m[j] = sched_map_entry(a->src[j], flags && a->zero_text[j] != 0, flags && a->zero_speech[j] != 0);
    }
    return dev.up(m.data(), (size_t)N);
  };
  if (kind == ZV_SC_BUILD_INPUT) {
    const int Fx = a->Fx, Ft = a->Ft, Fs = a->Fs, Fin = Fx + Ft + Fs;
    ZV_REQUIRE(T > 0 && Fx > 0 && Ft > 0 && Fs > 0 && a->ld >= Fin && a->x && a->tc && a->sc && a->oh,
               "zv_sched_check: BUILD_INPUT needs x, tc, sc, oh, ld >= Fx + Ft + Fs");
    const int* map = row_map(true);
    const size_t bt = (size_t)B * T, n16 = ((size_t)N * T + 2 * G) * a->ld;
    const float* x = dev.up(a->x, bt * Fx);
    const float* tc = dev.up(a->tc, bt * Ft);
    const float* sc = dev.up(a->sc, bt * Fs);
    uint16_t* oh = dev.up(a->oh, n16);
    uint16_t* ol = a->ol ? dev.up(a->ol, n16) : nullptr;
    ran = launch_build_input_map(x, tc, sc, reinterpret_cast<bf16*>(oh) + G * a->ld,
                                 ol ? reinterpret_cast<bf16*>(ol) + G * a->ld : nullptr, a->ld, map, N, T, Fx, Ft, Fs, s);
    gy = N;
    sync();
    dev.down(a->oh, oh, n16);
    if (ol) dev.down(a->ol, ol, n16);
  } else if (kind == ZV_SC_MASK_GATHER) {
    ZV_REQUIRE(T > 0 && a->mask && a->mout, "zv_sched_check: MASK_GATHER needs the mask and mout");
    const int* map = row_map(false);
    const uint8_t* in = dev.up(a->mask, (size_t)B * T);
    uint8_t* o = dev.up(a->mout, (size_t)N * T + 2 * G);
    ran = launch_gather_u8(in, o + G, map, N, T, s);
    gy = N;
    sync();
    dev.down(a->mout, o, (size_t)N * T + 2 * G);
  } else {
    const int A = a->A;
    const long per_row = a->per_row;
    ZV_REQUIRE(N > 0 && A > 0 && A <= B && per_row > 0 && a->x && a->v && a->out && a->row && a->dt && a->scale &&
                   a->cond && a->uncond,
               "zv_sched_check: EULER needs x, v, out and row / dt / scale / cond / uncond of A <= B active rows");
    std::vector<SchedUpd> upd(A);
    std::vector<char> seen(B, 0);
    for (int i = 0; i < A; ++i) {
      ZV_REQUIRE(a->row[i] >= 0 && a->row[i] < B && !seen[a->row[i]], "zv_sched_check: active rows distinct and inside [0, B)");
      ZV_REQUIRE(a->cond[i] >= 0 && a->cond[i] < N && a->uncond[i] >= -1 && a->uncond[i] < N,
                 "zv_sched_check: a velocity row outside [0, N)");
      seen[a->row[i]] = 1;
      upd[i] = SchedUpd{a->row[i], a->dt[i], a->scale[i], a->cond[i], a->uncond[i]};
    }
    const size_t n = (size_t)B * per_row;
    const float* v = dev.up(a->v, (size_t)N * per_row);
    const SchedUpd* du = dev.up(upd.data(), (size_t)A);
    std::vector<float> ho(a->out, a->out + n + 2 * G);
    memcpy(&ho[G], a->x, n * sizeof(float));              // in place over x, as the engine's solve
    float* o = dev.up(ho.data(), ho.size());
    ran = launch_euler_update_sched(o + G, v, du, A, per_row, s);
    gy = A;
    sync();
    dev.down(a->out, o, n + 2 * G);
  }
  const int rec[8] = {kind, ran.form, ran.blocks, ran.threads, gy, 0, 0, 0};
  memcpy(a->launch, rec, sizeof(rec));
  a->num_cus = zv_num_cus();
  ZV_API_END
}

// a session tick's host plan (session_tick, zv_session.inc: the function zv_engine::session_step runs)
int zv_session_plan(const zv_row_sched* rows_, const int32_t* done, const int32_t* lens, int slots, int distill,
                    zv_sched_plan_out* out, int32_t* T_k) {
  ZV_API_BEGIN
  ZV_REQUIRE(rows_ && done && lens && out && T_k, "zv_session_plan: null argument");
  ZV_REQUIRE(slots >= 1 && slots <= SESSION_MAX_SLOTS, "session: slots must be in [1, 32767]");
  const SchedRow* rows = reinterpret_cast<const SchedRow*>(rows_);
  std::vector<std::vector<float>> ts(slots);
  int left = 0;
  for (int b = 0; b < slots; ++b) {
    if (rows[b].num_step == 0) continue;
    const std::string at = "session: slot " + std::to_string(b) + ": ";
    sched_check_row(rows[b], at);
    ZV_REQUIRE(done[b] >= 0 && done[b] <= rows[b].num_step, at + "done outside [0, num_step]");
    ZV_REQUIRE(lens[b] >= 1 && lens[b] < (1 << 30), at + "length outside [1, 2^30)");
    ts[b] = solve_time_steps(rows[b].t_start, rows[b].t_end, rows[b].num_step, rows[b].t_shift);
    left = std::max(left, rows[b].num_step - done[b]);
  }
  const SessTick tk = session_tick(rows, done, lens, ts, slots, distill != 0);
  const SchedStep& st = tk.st;
  out->steps = left;
  out->total_rows = 0;
  std::vector<int> d(done, done + slots);
  for (int j = 0; j < left; ++j) {             // the ticks to come, if nothing is admitted
    const SessTick nx = session_tick(rows, d.data(), lens, ts, slots, distill != 0);
    out->total_rows += nx.st.U + nx.st.A;
    for (const SchedUpd& u : nx.st.upd) d[u.row] += 1;
  }
  out->active = st.A;
  out->copies = st.U;
  *T_k = tk.Tk;
  for (int j = 0; j < st.U + st.A; ++j) {
    if (out->dec_src) out->dec_src[j] = st.src[j];
    if (out->dec_zero_text) out->dec_zero_text[j] = st.zt[j];
    if (out->dec_zero_speech) out->dec_zero_speech[j] = st.zs[j];
    if (out->dec_t) out->dec_t[j] = st.t[j];
  }
  for (int i = 0; i < st.A; ++i) {
    if (out->act_row) out->act_row[i] = st.upd[i].row;
    if (out->act_dt) out->act_dt[i] = st.upd[i].dt;
    if (out->act_scale) out->act_scale[i] = distill ? st.gdec[i] : (st.upd[i].vu < 0 ? 0.0f : st.upd[i].g);
    if (out->act_cond) out->act_cond[i] = st.upd[i].vc;
    if (out->act_uncond) out->act_uncond[i] = st.upd[i].vu;
  }
  ZV_API_END
}

// ---------------------------------------------------------------------------
// zv_session_check: the solve session's kernels (admit, retire, and the strided operand build, mask
// gather and Euler update) through the launch functions zv_engine::session_* calls, on host arrays
// with canary-guarded outputs.  Every index is checked here before a launch.
// ---------------------------------------------------------------------------
int zv_session_check(zv_session_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->kind >= ZV_SS_ADMIT && a->kind <= ZV_SS_EULER && a->guard >= 0, "zv_session_check: bad arguments");
  const int kind = a->kind, S = a->slots, maxT = a->max_frames, Tk = a->T_k, N = a->N;
  const int Fx = a->Fx, Ft = a->Ft, Fs = a->Fs;
  const size_t G = (size_t)a->guard;
  ZV_REQUIRE(S > 0 && S <= SESSION_MAX_SLOTS && maxT > 0, "zv_session_check: slots in [1, 32767], max_frames > 0");
  ZV_REQUIRE(kind == ZV_SS_MASK_GATHER || Fx > 0, "zv_session_check: Fx > 0");
  ZV_REQUIRE((long)S * maxT * std::max(1, std::max(Fx, std::max(Ft, Fs))) < (1L << 30),
             "zv_session_check: slot buffers under 2^30 values");
  const size_t st = (size_t)S * maxT;
  ChkDev dev;
  hipStream_t s = nullptr;
  EdgeLaunch ran{};
  int gy = 0;
  auto sync = [&] { ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize())); };
  auto rows_tab = [&](int lim) {               // slot / len (n) -> device SessRow table
    const int n = a->n;
    ZV_REQUIRE(n > 0 && n <= S && a->slot && a->len, "zv_session_check: slot and len of 1 to `slots` rows");
    std::vector<SessRow> t(n);
    std::vector<char> seen(S, 0);
    for (int i = 0; i < n; ++i) {
      ZV_REQUIRE(a->slot[i] >= 0 && a->slot[i] < S && !seen[a->slot[i]], "zv_session_check: slots distinct and inside [0, slots)");
      ZV_REQUIRE(a->len[i] >= 1 && a->len[i] <= lim && a->len[i] <= maxT, "zv_session_check: a length outside [1, min(T_io, max_frames)]");
      seen[a->slot[i]] = 1;
      t[i] = SessRow{a->slot[i], a->len[i]};
    }
    return dev.up(t.data(), (size_t)n);
  };
  auto row_map = [&](bool flags) {
    ZV_REQUIRE(N > 0 && N <= 65535 && a->src && (!flags || (a->zero_text && a->zero_speech)),
               "zv_session_check: src (and the zero flags) of N decoder rows");
    ZV_REQUIRE(Tk > 0 && Tk <= maxT, "zv_session_check: T_k must be in [1, max_frames]");
    std::vector<int> m(N);
    for (int j = 0; j < N; ++j) {
      ZV_REQUIRE(a->src[j] >= 0 && a->src[j] < S, "zv_session_check: a source slot outside [0, slots)");
      m[j] = sched_map_entry(a->src[j], flags && a->zero_text[j] != 0, flags && a->zero_speech[j] != 0);
    }
    return dev.up(m.data(), (size_t)N);
  };
  if (kind == ZV_SS_ADMIT) {
    const int n = a->n, Tin = a->T_io;
    ZV_REQUIRE(Tin > 0 && Ft > 0 && Fs == Fx && a->x && a->tc && a->sc && a->out && a->out_tc && a->out_sc && a->mout,
               "zv_session_check: ADMIT needs x, tc, sc, out, out_tc, out_sc, mout and Fs = Fx");
    const SessRow* tab = rows_tab(Tin);
    const float* x0 = dev.up(a->x, (size_t)n * Tin * Fx);
    const float* tc0 = dev.up(a->tc, (size_t)n * Tin * Ft);
    const float* sc0 = dev.up(a->sc, (size_t)n * Tin * Fx);
    // (the guards are rounded up to 4 values on the device so a 16-byte aligned base stays one)
    const size_t Gd = (G + 3) / 4 * 4;
    std::vector<float> hx(Gd - G + st * Fx + 2 * G), ht(Gd - G + st * Ft + 2 * G);
    std::vector<float> hs(hx.size());
    memcpy(&hx[Gd - G], a->out, (st * Fx + 2 * G) * sizeof(float));
    memcpy(&ht[Gd - G], a->out_tc, (st * Ft + 2 * G) * sizeof(float));
    memcpy(&hs[Gd - G], a->out_sc, (st * Fx + 2 * G) * sizeof(float));
    float* ox = dev.up(hx.data(), hx.size());
    float* ot = dev.up(ht.data(), ht.size());
    float* os = dev.up(hs.data(), hs.size());
    uint8_t* om = dev.up(a->mout, st + 2 * G);
    ran = launch_session_admit(x0, tc0, sc0, n, Tin, ox + Gd, ot + Gd, os + Gd, om + G, tab, maxT, Fx, Ft, s);
    gy = n;
    sync();
    dev.down(a->out, ox + (Gd - G), st * Fx + 2 * G);
    dev.down(a->out_tc, ot + (Gd - G), st * Ft + 2 * G);
    dev.down(a->out_sc, os + (Gd - G), st * Fx + 2 * G);
    dev.down(a->mout, om, st + 2 * G);
  } else if (kind == ZV_SS_RETIRE) {
    const int n = a->n, Tout = a->T_io;
    ZV_REQUIRE(Tout > 0 && a->x && a->out, "zv_session_check: RETIRE needs x and out");
    const SessRow* tab = rows_tab(Tout);
    const float* x = dev.up(a->x, st * Fx);
    const size_t Gd = (G + 3) / 4 * 4, no = (size_t)n * Tout * Fx + 2 * G;
    std::vector<float> ho(Gd - G + no);
    memcpy(&ho[Gd - G], a->out, no * sizeof(float));
    float* o = dev.up(ho.data(), ho.size());
    ran = launch_session_retire(x, o + Gd, n, Tout, tab, maxT, Fx, s);
    gy = n;
    sync();
    dev.down(a->out, o + (Gd - G), no);
  } else if (kind == ZV_SS_BUILD_INPUT) {
    const int Fin = Fx + Ft + Fs;
    ZV_REQUIRE(Ft > 0 && Fs > 0 && a->ld >= Fin && a->x && a->tc && a->sc && a->oh,
               "zv_session_check: BUILD_INPUT needs x, tc, sc, oh, ld >= Fx + Ft + Fs");
    const int* map = row_map(true);
    const size_t n16 = ((size_t)N * Tk + 2 * G) * a->ld;
    const float* x = dev.up(a->x, st * Fx);
    const float* tc = dev.up(a->tc, st * Ft);
    const float* sc = dev.up(a->sc, st * Fs);
    uint16_t* oh = dev.up(a->oh, n16);
    uint16_t* ol = a->ol ? dev.up(a->ol, n16) : nullptr;
    ran = launch_session_build_input(x, tc, sc, reinterpret_cast<bf16*>(oh) + G * a->ld,
                                     ol ? reinterpret_cast<bf16*>(ol) + G * a->ld : nullptr, a->ld, map, N, Tk, maxT,
                                     Fx, Ft, Fs, s);
    gy = N;
    sync();
    dev.down(a->oh, oh, n16);
    if (ol) dev.down(a->ol, ol, n16);
  } else if (kind == ZV_SS_MASK_GATHER) {
    ZV_REQUIRE(a->mask && a->mout, "zv_session_check: MASK_GATHER needs the mask and mout");
    const int* map = row_map(false);
    const uint8_t* in = dev.up(a->mask, st);
    uint8_t* o = dev.up(a->mout, (size_t)N * Tk + 2 * G);
    ran = launch_session_gather_u8(in, o + G, map, N, Tk, maxT, s);
    gy = N;
    sync();
    dev.down(a->mout, o, (size_t)N * Tk + 2 * G);
  } else {
    const int A = a->A;
    ZV_REQUIRE(N > 0 && A > 0 && A <= S && Tk > 0 && Tk <= maxT && a->x && a->v && a->out && a->row && a->dt &&
                   a->scale && a->cond && a->uncond,
               "zv_session_check: EULER needs x, v, out and row / dt / scale / cond / uncond of A <= slots active rows");
    std::vector<SchedUpd> upd(A);
    std::vector<char> seen(S, 0);
    for (int i = 0; i < A; ++i) {
      ZV_REQUIRE(a->row[i] >= 0 && a->row[i] < S && !seen[a->row[i]], "zv_session_check: active slots distinct and inside [0, slots)");
      ZV_REQUIRE(a->cond[i] >= 0 && a->cond[i] < N && a->uncond[i] >= -1 && a->uncond[i] < N,
                 "zv_session_check: a velocity row outside [0, N)");
      seen[a->row[i]] = 1;
      upd[i] = SchedUpd{a->row[i], a->dt[i], a->scale[i], a->cond[i], a->uncond[i]};
    }
    const size_t n = st * Fx;
    const float* v = dev.up(a->v, (size_t)N * Tk * Fx);
    const SchedUpd* du = dev.up(upd.data(), (size_t)A);
    std::vector<float> ho(a->out, a->out + n + 2 * G);
    memcpy(&ho[G], a->x, n * sizeof(float));              // in place over x, as the engine's tick
    float* o = dev.up(ho.data(), ho.size());
    ran = launch_session_euler_update(o + G, v, du, A, (long)Tk * Fx, (long)maxT * Fx, s);
    gy = A;
    sync();
    dev.down(a->out, o, n + 2 * G);
  }
  const int rec[8] = {kind, ran.form, ran.blocks, ran.threads, gy, 0, 0, 0};
  memcpy(a->launch, rec, sizeof(rec));
  a->num_cus = zv_num_cus();
  ZV_API_END
}

// ---------------------------------------------------------------------------
// zv_session_edit_check: the edit rows' two kernels through the rules, the table and the launch functions
// zv_engine::session_admit_edit / session_retire_edit run, on host arrays with canary-guarded outputs and
// the session's host state (state_left / state_len) given and updated by the caller's arrays.
// ---------------------------------------------------------------------------
int zv_session_edit_check(zv_session_edit_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && (a->kind == ZV_SE_ADMIT || a->kind == ZV_SE_RETIRE) && a->guard >= 0,
             "zv_session_edit_check: bad arguments");
  const int kind = a->kind, S = a->slots, maxT = a->max_frames, Fx = a->Fx, Ft = a->Ft, n = a->n, Tio = a->T_io;
  const size_t G = (size_t)a->guard, Gd = (G + 3) / 4 * 4;   // (device guards: a multiple of 4 values, as zv_session_check)
  ZV_REQUIRE(S > 0 && S <= SESSION_MAX_SLOTS && maxT > 0 && Fx > 0 && (kind == ZV_SE_RETIRE || Ft > 0),
             "zv_session_edit_check: slots in [1, 32767], max_frames, Fx (and Ft) > 0");
  ZV_REQUIRE((long)S * maxT * std::max(Fx, std::max(Ft, 1)) < (1L << 30), "zv_session_edit_check: slot buffers under 2^30 values");
  ZV_REQUIRE(a->pool_rows > 0 && (long)a->pool_rows * Fx < (1L << 30) && a->pool && a->state_left && a->state_len && a->x &&
                 a->out,
             "zv_session_edit_check: needs the pool (under 2^30 values), state_left, state_len, x and out");
  for (int b = 0; b < S; ++b)
    ZV_REQUIRE(a->state_left[b] >= -1 && a->state_len[b] >= 0 && a->state_len[b] <= maxT,
               "zv_session_edit_check: state_left >= -1 and state_len in [0, max_frames]");
  const size_t st = (size_t)S * maxT;
  const SessView view{S, maxT, a->state_left, a->state_len};
  const SessEditReq e{n, a->slot, a->offsets, a->lens, a->table, a->row_ptr, a->pool_rows};
  std::vector<int> T;
  hipStream_t s = nullptr;
  EdgeLaunch ran{};
  if (kind == ZV_SE_ADMIT) {
    ZV_REQUIRE(a->tc && a->out_tc && a->out_sc && a->mout, "zv_session_edit_check: ADMIT needs tc, out_tc, out_sc and mout");
    sess_edit_check_admit(view, e, reinterpret_cast<const SchedRow*>(a->rows), Tio, T);
  } else {
    sess_edit_check_retire(view, e, Tio, T);
  }
  ZV_REQUIRE((long)n * Tio * std::max(Fx, Ft) < (1L << 30), "zv_session_edit_check: request rows under 2^30 values");
  ChkDev dev;
  std::vector<unsigned> words(sess_edit_words(e));
  sess_edit_fill(words.data(), e, T);
  const unsigned* dtab = dev.up(words.data(), words.size());
  const float* pool = dev.up(a->pool, (size_t)a->pool_rows * Fx);
  auto sync = [&] { ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize())); };
  auto guarded = [&](const float* host, size_t count) {   // host (guard + count + guard) -> device, interior 16-byte aligned
    std::vector<float> h(Gd - G + count + 2 * G);
    memcpy(&h[Gd - G], host, (count + 2 * G) * sizeof(float));
    return dev.up(h.data(), h.size());
  };
  if (kind == ZV_SE_ADMIT) {
    const float* x0 = dev.up(a->x, (size_t)n * Tio * Fx);
    const float* tc0 = dev.up(a->tc, (size_t)n * Tio * Ft);
    float* ox = guarded(a->out, st * Fx);
    float* ot = guarded(a->out_tc, st * Ft);
    float* os = guarded(a->out_sc, st * Fx);
    uint8_t* om = dev.up(a->mout, st + 2 * G);
    ran = launch_session_admit_edit(x0, tc0, n, Tio, pool, ox + Gd, ot + Gd, os + Gd, om + G, dtab, maxT, Fx, Ft, s);
    sync();
    dev.down(a->out, ox + (Gd - G), st * Fx + 2 * G);
    dev.down(a->out_tc, ot + (Gd - G), st * Ft + 2 * G);
    dev.down(a->out_sc, os + (Gd - G), st * Fx + 2 * G);
    dev.down(a->mout, om, st + 2 * G);
    for (int i = 0; i < n; ++i) {
      a->state_left[a->slot[i]] = a->rows[i].num_step;
      a->state_len[a->slot[i]] = T[i];
    }
  } else {
    const float* x = dev.up(a->x, st * Fx);
    const size_t no = (size_t)n * Tio * Fx, nm = (size_t)n * Tio;
    float* o = guarded(a->out, no);
    uint8_t* om = a->mout ? dev.up(a->mout, nm + 2 * G) : nullptr;
    ran = launch_session_retire_edit(x, pool, o + Gd, om ? om + G : nullptr, n, Tio, dtab, maxT, Fx,
                                     a->keep_original != 0, s);
    sync();
    dev.down(a->out, o + (Gd - G), no + 2 * G);
    if (om) dev.down(a->mout, om, nm + 2 * G);
    for (int i = 0; i < n; ++i) {
      a->state_left[a->slot[i]] = -1;
      a->state_len[a->slot[i]] = 0;
    }
  }
  const int rec[8] = {kind, ran.form, ran.blocks, ran.threads, n, 0, 0, 0};
  memcpy(a->launch, rec, sizeof(rec));
  a->num_cus = zv_num_cus();
  ZV_API_END
}

}  // extern "C"

// ---------------------------------------------------------------------------
// zv_bigvgan_check: the BigVGAN kernels one at a time (and one AMP step), through the launches
// and relayouts zv_bigvgan::finalize / decode use (BvHost), on host arrays with canary-guarded
// outputs.  Everything the call allocates besides its inputs -- 16-bit operands, their padding
// columns and halo rows, fp32 scratch -- starts from a finite, non-zero pattern seeded by
// `stale`: a result that depends on unwritten memory changes with the seed.  (Non-finite stale
// data is outside the kernels' contract: 0 * inf in a padding column would be NaN.)
// ---------------------------------------------------------------------------
namespace {
inline unsigned chk_hash(size_t i, unsigned seed) {
  unsigned x = (unsigned)i * 2654435761u ^ (seed * 0x9E3779B9u + 0x7F4A7C15u);
  x ^= x >> 13; x *= 0x5bd1e995u; x ^= x >> 15;
  return x;
}
// 16-bit patterns that are finite and non-zero as bf16 and as fp16, of either sign
inline uint16_t chk_stale16(size_t i, unsigned seed) {
  const unsigned x = chk_hash(i, seed);
  return (uint16_t)(0x3C00u | (x & 0x3FFu) | ((x >> 16 & 1u) << 15));
}
inline float chk_stale32(size_t i, unsigned seed) {
  const unsigned x = chk_hash(i, seed);
  return ((x >> 20 & 1u) ? -1.f : 1.f) * (1.f + (float)(x & 0xFFFFu) / 16384.f);
}
bf16* chk_stale_dev16(ChkDev& dev, size_t n, unsigned seed) {
  std::vector<uint16_t> h(n);
  for (size_t i = 0; i < n; ++i) h[i] = chk_stale16(i, seed);
  return reinterpret_cast<bf16*>(dev.up(h.data(), n));
}
float* chk_stale_dev32(ChkDev& dev, size_t n, unsigned seed) {
  std::vector<float> h(n);
  for (size_t i = 0; i < n; ++i) h[i] = chk_stale32(i, seed);
  return dev.up(h.data(), n);
}
// chk_act with the stale pattern in the padding columns [cols, ld)
Act chk_act_stale(ChkDev& dev, const float* x, long rows, int cols, long ld, bool lo, unsigned seed) {
  std::vector<bf16> h, l;
  chk_act(x, rows, cols, ld, lo, h, l);
  uint16_t* hu = reinterpret_cast<uint16_t*>(h.data());
  uint16_t* lu = lo ? reinterpret_cast<uint16_t*>(l.data()) : nullptr;
  for (long r = 0; r < rows; ++r)
    for (long c = cols; c < ld; ++c) {
      hu[r * ld + c] = chk_stale16((size_t)(r * ld + c), seed);
      if (lu) lu[r * ld + c] = chk_stale16((size_t)(r * ld + c), seed + 1);
    }
  Act a;
  a.ld = ld;
  a.h = dev.up(h.data(), h.size());
  if (lo) a.l = dev.up(l.data(), l.size());
  return a;
}
template <int SPLIT>
void bv_check_run(zv_bigvgan_check_args* a) {
  const int kind = a->kind, B = a->B, L = a->Lmax, C = a->C, G = a->guard, halo = a->halo;
  const bool split = SPLIT == 3;
  const unsigned seed = a->stale;
  ChkDev dev;
  WeightStore store;
  hipStream_t s = nullptr;
  const int* lens = a->lens ? dev.up(a->lens, (size_t)B) : nullptr;
  const BvFilter filt = a->taps ? BvHost::filter_of(a->taps) : BvHost::make_filter();
  auto snake = [&](const float* al, const float* ib) {
    return BvAct{dev.up(al, (size_t)C), dev.up(ib, (size_t)C)};
  };
  auto out32 = [&](long rows, int cols) { return dev.up(a->out, (size_t)(rows + 2 * G) * cols); };
  auto down32 = [&](float* d, long rows, int cols) { dev.down(a->out, d, (size_t)(rows + 2 * G) * cols); };
  // the implicit-conv operand as decode allocates it: M + 2 * halo rows, base advanced by halo
  auto operand = [&](long M, int Cp, unsigned sd) {
    Act o;
    o.ld = Cp;
    o.h = chk_stale_dev16(dev, (size_t)(M + 2 * halo) * Cp, sd) + (long)halo * Cp;
    if (split) o.l = chk_stale_dev16(dev, (size_t)(M + 2 * halo) * Cp, sd + 1) + (long)halo * Cp;
    return o;
  };
  int rec5 = 0;
  if (kind == ZV_BV_ACT) {
    const int Lp = BvHost::stage_rows(L, halo);
    const long M = (long)B * Lp;
    const float* x = dev.up(a->x, (size_t)M * C);
    const BvAct sn = snake(a->alpha, a->ibeta);
    if (a->mode == 0) {
      float* o = out32(M, C);
      BvHost::act<0>(sn, filt, halo, x, lens, a->scale, B, L, Lp, C, o + (size_t)G * C, Act{}, s);
      ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
      down32(o, M, C);
    } else {
      const int Cp = (int)round_up(C, 32);
      const size_t n = (size_t)(M + 2 * halo + 2 * G) * Cp;
      uint16_t* oh = dev.up(a->oh, n);
      uint16_t* ol = split ? dev.up(a->ol, n) : nullptr;
      Act o;
      o.ld = Cp;
      o.h = reinterpret_cast<bf16*>(oh) + (size_t)(G + halo) * Cp;
      if (ol) o.l = reinterpret_cast<bf16*>(ol) + (size_t)(G + halo) * Cp;
      BvHost::act<2>(sn, filt, halo, x, lens, a->scale, B, L, Lp, C, nullptr, o, s);
      ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
      dev.down(a->oh, oh, n);
      if (ol) dev.down(a->ol, ol, n);
    }
  } else if (kind == ZV_BV_CONV) {
    const int Lp = BvHost::stage_rows(L, halo), Cp = (int)round_up(C, 32), Co = a->Cout;
    const long M = (long)B * Lp;
    const std::vector<float> w2 = BvHost::conv_rows(a->w, Co, C, a->ks, Cp);
    const Linear W = store.make_linear(w2.data(), Co, Cp * a->ks, a->bias);
    const size_t n = (size_t)(M + 2 * halo) * Cp;
    Act A;
    A.ld = Cp;
    A.h = reinterpret_cast<bf16*>(dev.up(a->ah, n)) + (long)halo * Cp;
    if (split) A.l = reinterpret_cast<bf16*>(dev.up(a->al, n)) + (long)halo * Cp;
    std::vector<float> hc(a->out, a->out + (size_t)(M + 2 * G) * Co);
    if (a->resid) memcpy(&hc[(size_t)G * Co], a->resid, (size_t)M * Co * sizeof(float));
    float* o = dev.up(hc.data(), hc.size());
    float* oi = o + (size_t)G * Co;                   // the residual in place, as decode's blocks 1, 2
    rec5 = BvHost::gemm<SPLIT, 1>(W, A, M, oi, Co, Act{}, a->resid ? oi : nullptr, s, "bigvgan_check", Cp, a->d,
                                  a->d * (a->ks - 1) / 2);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    down32(o, M, Co);
  } else if (kind == ZV_BV_CONVT) {
    const int Co = a->Cout, k = a->ks, u = a->u, Ls = a->Ls;
    const int Lo_s = BvHost::stage_rows(L * u, halo);
    const long Min = (long)B * Ls, M = (long)B * Lo_s, ldp = (long)k * Co;
    const float* bias = dev.up(a->bias, (size_t)Co);
    const float* Pb;
    if (a->flag) {
      const std::vector<float> w2 = BvHost::convt_rows(a->w, C, Co, k);
      const Linear W = store.make_linear(w2.data(), k * Co, C, nullptr);
      const Act A = chk_act_stale(dev, a->x, Min, C, round_up(C, W_KPAD), split, seed);
      float* P = chk_stale_dev32(dev, (size_t)(Min + 1) * ldp, seed + 2);   // (one spare row, as below)
      rec5 = BvHost::gemm<SPLIT>(W, A, Min, P, ldp, Act{}, nullptr, s, "bigvgan_check");
      Pb = P;
    } else {
      // one spare stale row behind P: a gather that reads frame len_in of the last utterance stays
      // inside the buffer, and the test sees a wrong value
      float* P = chk_stale_dev32(dev, (size_t)(Min + 1) * ldp, seed + 2);
      ZV_CHECK(ZV_BLOCKING(hipMemcpy(P, a->x, (size_t)Min * ldp * sizeof(float), hipMemcpyHostToDevice)));
      Pb = P;
    }
    float* o = out32(M, Co);
    BvHost::convt_gather(Pb, bias, lens, a->scale, B, L, Ls, u, k, Co, Lo_s, o + (size_t)G * Co, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    down32(o, M, Co);
  } else if (kind == ZV_BV_AVG) {
    const long M = (long)B * L;
    const float* y0 = dev.up(a->x, (size_t)M * C);
    const float* y1 = a->n > 1 ? dev.up(a->x1, (size_t)M * C) : nullptr;
    const float* y2 = a->n > 2 ? dev.up(a->x2, (size_t)M * C) : nullptr;
    float* o = out32(M, C);
    const size_t n16 = (size_t)(M + 2 * G) * a->ld;
    uint16_t* oh = a->oh ? dev.up(a->oh, n16) : nullptr;
    uint16_t* ol = a->ol ? dev.up(a->ol, n16) : nullptr;
    Act xo;
    xo.ld = a->ld;
    if (oh) xo.h = reinterpret_cast<bf16*>(oh) + (size_t)G * a->ld;
    if (ol) xo.l = reinterpret_cast<bf16*>(ol) + (size_t)G * a->ld;
    BvHost::avg(y0, y1, y2, a->n, M, C, o + (size_t)G * C, xo, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    down32(o, M, C);
    if (oh) dev.down(a->oh, oh, n16);
    if (ol) dev.down(a->ol, ol, n16);
  } else if (kind == ZV_BV_POST) {
    const float* x = dev.up(a->x, (size_t)B * a->Ls * C);
    const float* w = dev.up(a->w, (size_t)C * 7);
    float* o = out32((long)B * L, 1);
    BvHost::post(x, lens, a->scale, B, L, a->Ls, C, w, a->bias0, a->flag, o + G, s);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    down32(o, (long)B * L, 1);
  } else if (kind == ZV_BV_IM2COL) {
    const long M = (long)B * L;
    const int K = C * a->ks;
    const long ld = round_up((long)K, W_KPAD);
    const float* in = dev.up(a->x, (size_t)M * C);
    const size_t n16 = (size_t)(M + 2 * G) * ld;
    uint16_t* oh = dev.up(a->oh, n16);
    uint16_t* ol = split ? dev.up(a->ol, n16) : nullptr;
    Act A;
    A.ld = ld;
    A.h = reinterpret_cast<bf16*>(oh) + (size_t)G * ld;
    if (ol) A.l = reinterpret_cast<bf16*>(ol) + (size_t)G * ld;
    launch_voc_im2col(in, a->layout, a->div, a->sub, lens, B, L, C, a->ks, A, s);
    float* o = nullptr;
    if (a->flag) {
      const std::vector<float> w2 = BvHost::conv_rows(a->w, a->Cout, C, a->ks, C);
      const Linear W = store.make_linear(w2.data(), a->Cout, K, a->bias);
      o = out32(M, a->Cout);
      rec5 = BvHost::gemm<SPLIT>(W, A, M, o + (size_t)G * a->Cout, a->Cout, Act{}, nullptr, s, "bigvgan_check");
    }
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    dev.down(a->oh, oh, n16);
    if (ol) dev.down(a->ol, ol, n16);
    if (o) down32(o, M, a->Cout);
  } else {   // ZV_BV_STEP: x += conv2(act2(conv1_d(act1(x)))) of one AMP block, as decode runs it
    const int Lp = BvHost::stage_rows(L, halo), Cp = (int)round_up(C, 32), ks = a->ks;
    const long M = (long)B * Lp;
    const float* x = dev.up(a->x, (size_t)M * C);
    const BvAct s1 = snake(a->alpha, a->ibeta), s2 = snake(a->alpha2, a->ibeta2);
    const std::vector<float> wa = BvHost::conv_rows(a->w, C, C, ks, Cp), wb = BvHost::conv_rows(a->w2, C, C, ks, Cp);
    const Linear W1 = store.make_linear(wa.data(), C, Cp * ks, a->bias);
    const Linear W2 = store.make_linear(wb.data(), C, Cp * ks, a->bias2);
    const Act ca = operand(M, Cp, seed);
    float* t1 = chk_stale_dev32(dev, (size_t)M * C, seed + 2);
    float* o = out32(M, C);
    float* y = o + (size_t)G * C;
    BvHost::act<2>(s1, filt, halo, x, lens, a->scale, B, L, Lp, C, nullptr, ca, s);
    BvHost::gemm<SPLIT, 1>(W1, ca, M, t1, C, Act{}, nullptr, s, "bigvgan_check", Cp, a->d, a->d * (ks - 1) / 2);
    BvHost::act<2>(s2, filt, halo, t1, lens, a->scale, B, L, Lp, C, nullptr, ca, s);
    rec5 = BvHost::gemm<SPLIT, 1>(W2, ca, M, y, C, Act{}, x, s, "bigvgan_check", Cp, 1, (ks - 1) / 2);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    down32(o, M, C);
  }
  chk_record(a->launch, &a->num_cus);
  a->launch[5] = rec5;                                 // the K step of the last GEMM (0: none ran)
}
}  // namespace

extern "C" {

int zv_bigvgan_check(zv_bigvgan_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && a->kind >= ZV_BV_FILTER && a->kind <= ZV_BV_STEP, "zv_bigvgan_check: unknown kind");
  const int kind = a->kind;
  if (kind == ZV_BV_FILTER) {
    ZV_REQUIRE(a->out, "zv_bigvgan_check: FILTER writes 24 floats to out");
    const BvFilter f = a->taps ? BvHost::filter_of(a->taps) : BvHost::make_filter();
    memcpy(a->out, &f, sizeof(f));
    return 0;
  }
  ZV_REQUIRE((a->split == 1 || a->split == 3) && a->guard >= 0 && a->B > 0 && a->Lmax > 0 && a->C > 0 &&
                 (a->x || kind == ZV_BV_CONV),
             "zv_bigvgan_check: bad arguments");
  ZV_REQUIRE(a->out || (kind == ZV_BV_ACT && a->mode == 2) || (kind == ZV_BV_IM2COL && !a->flag),
             "zv_bigvgan_check: the fp32 output");
  const bool needs_halo = kind == ZV_BV_ACT || kind == ZV_BV_CONV || kind == ZV_BV_CONVT || kind == ZV_BV_STEP;
  ZV_REQUIRE(!needs_halo || (a->halo >= 8 && a->halo % 8 == 0), "zv_bigvgan_check: halo a positive multiple of 8");
  const bool scaled = kind == ZV_BV_ACT || kind == ZV_BV_CONVT || kind == ZV_BV_POST || kind == ZV_BV_STEP;
  ZV_REQUIRE(!scaled || a->scale >= 1, "zv_bigvgan_check: scale >= 1");
  if (a->lens && kind != ZV_BV_AVG && kind != ZV_BV_CONV)
    for (int b = 0; b < a->B; ++b) ZV_REQUIRE(a->lens[b] >= 0, "zv_bigvgan_check: negative length");
  switch (kind) {
    case ZV_BV_ACT:
      ZV_REQUIRE((a->mode == 0 || a->mode == 2) && a->alpha && a->ibeta, "zv_bigvgan_check: ACT mode 0 / 2, alpha, ibeta");
      ZV_REQUIRE(a->mode == 0 || (a->oh && (a->ol != nullptr) == (a->split == 3)),
                 "zv_bigvgan_check: ACT mode 2 writes oh (ol with split 3 only)");
      break;
    case ZV_BV_CONV:
    case ZV_BV_STEP:
      ZV_REQUIRE(a->Cout > 0 && a->Cout % 4 == 0 && a->ks >= 1 && a->ks % 2 == 1 && a->d >= 1 && a->w && a->bias,
                 "zv_bigvgan_check: the conv's weight, bias, odd kernel size, dilation, Cout a multiple of 4");
      ZV_REQUIRE(a->d * (a->ks - 1) / 2 <= a->halo, "zv_bigvgan_check: halo below the conv's padding");
      if (kind == ZV_BV_CONV)
        ZV_REQUIRE(a->ah && (a->al != nullptr) == (a->split == 3), "zv_bigvgan_check: CONV operand (al with split 3 only)");
      else
        ZV_REQUIRE(a->Cout == a->C && a->w2 && a->bias2 && a->alpha && a->ibeta && a->alpha2 && a->ibeta2,
                   "zv_bigvgan_check: STEP needs both convs and both activations");
      break;
    case ZV_BV_CONVT:
      ZV_REQUIRE(a->Cout > 0 && a->Cout % 4 == 0 && a->u >= 1 && a->ks >= a->u && (a->ks - a->u) % 2 == 0 && a->Ls >= a->Lmax && a->bias &&
                     (!a->flag || a->w),
                 "zv_bigvgan_check: CONVT needs k >= u, k - u even, Ls >= Lmax, bias (and the weight with the GEMM)");
      break;
    case ZV_BV_AVG:
      ZV_REQUIRE(a->n >= 1 && a->n <= 3 && (a->n < 2 || a->x1) && (a->n < 3 || a->x2) && (!a->ol || a->oh) &&
                     (!a->oh || a->ld >= a->C),
                 "zv_bigvgan_check: AVG of 1..3 streams, ld >= C");
      break;
    case ZV_BV_POST:
      ZV_REQUIRE(a->w && a->Ls >= a->Lmax, "zv_bigvgan_check: POST needs the weight and Ls >= Lmax");
      (void)BvHost::post_lds(a->C);
      break;
    default:   // ZV_BV_IM2COL
      ZV_REQUIRE(a->ks >= 1 && (a->layout == 0 || a->layout == 1) && a->div != 0.f && a->oh &&
                     (a->ol != nullptr) == (a->split == 3) && (!a->flag || (a->w && a->bias && a->Cout > 0 && a->Cout % 4 == 0)),
                 "zv_bigvgan_check: IM2COL layout 0 / 1, div != 0, oh (ol with split 3 only)");
  }
  if (a->split == 3) bv_check_run<3>(a); else bv_check_run<1>(a);
  ZV_API_END
}

}  // extern "C"
