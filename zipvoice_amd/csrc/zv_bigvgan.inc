// BigVGAN-v2 vocoder (bigvgan_v2_24khz_100band_256x) for gfx950: mel (B, 100, T) -> wav (B, 256 T).
//
// The reference loads the third-party `bigvgan` package for feature.type "bigvgan_v2"
// (zipvoice/bin/infer_zipvoice.py:261-269: BigVGAN.from_pretrained(...,
// use_cuda_kernel=False), remove_weight_norm(), decode = forward).  Published algorithm
// (NVIDIA BigVGAN v2, bigvgan.py / activations.py / alias_free_activation/torch):
//   conv_pre Conv1d(n_mels, C0, 7, pad 3)
//   per stage i: ConvTranspose1d(C, C/2, k_i, u_i, pad (k_i-u_i)/2) ->
//                mean_j AMPBlock1_j(C/2, ks_j, dilations (1,3,5))
//   AMPBlock1: for d: x += conv2(act2(conv1_d(act1(x))))
//   act = Activation1d(SnakeBeta): 2x kaiser-sinc upsample (replicate pad) -> SnakeBeta
//         x + 1/(e^beta + 1e-9) sin^2(x e^alpha) -> 12-tap low-pass 2x downsample
//   activation_post -> conv_post Conv1d(C_last, 1, 7, pad 3) -> clamp(-1, 1) (or tanh)
// MI355X mapping (channel-last (B*L, C) fp32 streams, rows = time):
//   * every AMP Conv1d = implicit-GEMM on MFMA: the anti-aliased activation kernel writes
//     the (rows, Cpad) bf16 operand once (channels zero-padded to a 32-multiple K step, zero
//     halo rows around each utterance), and the GEMM's A loader shifts the rows of each
//     K step by tap*d - pad (zv_gemm.inc CONV mode), so no k-times im2col copy exists;
//     conv_pre (100 mel channels, once per call) uses an explicit im2col;
//   * ConvTranspose1d = GEMM P[s][j*Cout + o] = sum_c x[s][c] W[c][o][j] (N = k*Cout, K = Cin)
//     + a gather kernel y[t][o] = b[o] + sum_{j = (t+pad) mod u, +u} P[(t+pad-j)/u][j][o];
//   * the conv2 GEMM epilogue adds the AMP residual (resid = block input);
//   * a row kernel averages the 3 AMP blocks and emits the next stage's bf16 operand;
//   * conv_post (C_last -> 1, 7 taps) + clamp is one small gather kernel.
// Per-utterance lengths: utterance b occupies rows [b*Lmax, b*Lmax + len_b) of each stage;
// every kernel reads only inside [0, len_b) (zero / replicate padding at len_b, as a
// separate single-utterance forward would see) and zeroes rows beyond.
#pragma once

struct BvFilter { float up_even[6], up_odd[6], down[12]; };

// Anti-aliased SnakeBeta over a stage stream (utterance b = rows b*Lp + [0, Lmax), rows
// [Lmax, Lp) halo), TT consecutive frames of one channel per thread.  Output:
//   MODE 0: fp32 (rows, C);
//   MODE 2: the (rows, ld) bf16 hi/lo operand of an implicit-conv GEMM: rows outside
//           [0, len_b) and channels [C, ld) zeroed, including the H rows before
//           utterance 0 (the GEMM's negative tap shifts read them).
template <int MODE, int TT = 8>
__global__ __launch_bounds__(256) void zv_bv_act_kernel(
    const float* __restrict__ x, const int* lens, int scale, int B, int Lmax, int Lp, int H, int C,
    const float* __restrict__ alpha, const float* __restrict__ ibeta, BvFilter f, float* out,
    bf16* oh, bf16* ol, long ld) {
  static_assert(MODE == 0 || MODE == 2, "output mode");
  const int tbeg = MODE == 2 ? -H : 0;
  const int ngrp = (Lp - tbeg + TT - 1) / TT;
  const long total = (long)B * ngrp * C;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const long r = idx / C;
    const int g = (int)(r % ngrp), b = (int)(r / ngrp);
    const int t0 = tbeg + g * TT;
    const int len = lens ? min(lens[b] * scale, Lmax) : Lmax;
    const long rowb = (long)b * Lp;
    float z[TT];
    if (t0 >= 0 && t0 < len) {
      // x[t0-6 .. t0+TT+5], replicate-clamped to [0, len)
      constexpr int NX = TT + 12, NY = 2 * TT + 10;
      float xr[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) xr[i] = x[(rowb + min(max(t0 - 6 + i, 0), len - 1)) * C + c];
      // 2x upsample, y[s] for s = 2 t0 - 5 + j (polyphase: 6 taps per phase)
      float yv[NY];
#pragma unroll
      for (int j = 0; j < NY; ++j) {
        float acc = 0.f;
        if (j & 1) {          // s even: x[t' + m], m = -3..2, t' = t0 + (j - 5) / 2
#pragma unroll
          for (int m = 0; m < 6; ++m) acc = fmaf(f.up_even[m], xr[(j - 5) / 2 + m + 3], acc);
        } else {              // s odd: x[t' + m], m = -2..3, t' = t0 + (j - 6) / 2
#pragma unroll
          for (int m = 0; m < 6; ++m) acc = fmaf(f.up_odd[m], xr[(j - 6) / 2 + m + 4], acc);
        }
        yv[j] = acc;
      }
      // replicate padding of the upsampled signal at [0, 2 len): s < 0 -> y[0], s >= 2len -> y[2len-1]
      const int s0 = 2 * t0 - 5;
      if (s0 < 0 || s0 + NY > 2 * len) {
        float y0 = 0.f, ye = 0.f;
#pragma unroll
        for (int m = 0; m < 6; ++m) {     // y[0] (even, t' = 0), y[2len-1] (odd, t' = len-1)
          y0 = fmaf(f.up_even[m], x[(rowb + min(max(m - 3, 0), len - 1)) * C + c], y0);
          ye = fmaf(f.up_odd[m], x[(rowb + min(max(len - 1 + m - 2, 0), len - 1)) * C + c], ye);
        }
#pragma unroll
        for (int j = 0; j < NY; ++j) {
          const int s = s0 + j;
          yv[j] = s < 0 ? y0 : (s >= 2 * len ? ye : yv[j]);
        }
      }
      const float a = alpha[c], ib = ibeta[c];
#pragma unroll
      for (int j = 0; j < NY; ++j) {
        const float sn = __sinf(yv[j] * a);   // v_sin_f32 (|arg| << 256 turns here)
        yv[j] = yv[j] + ib * (sn * sn);
      }
#pragma unroll
      for (int i = 0; i < TT; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int jj = 0; jj < 12; ++jj) acc = fmaf(f.down[jj], yv[2 * i + jj], acc);
        z[i] = acc;
      }
    }
#pragma unroll
    for (int i = 0; i < TT; ++i) {
      const int t = t0 + i;
      if (t >= Lp) break;
      const bool valid = t >= 0 && t < len;
      if (MODE == 0) {
        out[(rowb + t) * C + c] = valid ? z[i] : 0.f;
      } else {
        split_store(oh, ol, (rowb + t) * ld + c, valid ? z[i] : 0.f);
        for (int cc = C + c; cc < ld; cc += C) split_store(oh, ol, (rowb + t) * ld + cc, 0.f);
      }
    }
  }
}

// ConvTranspose1d col2im: y[b, t, o] = bias[o] + sum_{j = (t+pad) mod u, j < k, step u}
// P[b*Lin + (t+pad-j)/u][j*Cout + o] over source frames inside [0, len_in).
// Input utterance b = P rows b*Lin_s + [0, Lin); output rows b*Lout_s + [0, Lout_s).
__global__ void zv_bv_convt_gather_kernel(const float* __restrict__ P, long ldp, const float* bias,
                                          const int* lens, int scale_in, int B, int Lin, int Lin_s,
                                          int u, int k, int pad, int Cout, int Lout_s, float* y) {
  const long total = (long)B * Lout_s * Cout;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int o = (int)(idx % Cout);
    const long r = idx / Cout;
    const int t = (int)(r % Lout_s), b = (int)(r / Lout_s);
    const int len_in = lens ? min(lens[b] * scale_in, Lin) : Lin;
    float v = 0.f;
    if (t < len_in * u) {
      float acc = 0.f;
      for (int j = (t + pad) % u; j < k; j += u) {
        const int q = t + pad - j;
        if (q < 0) break;
        const int s = q / u;
        if (s < len_in) acc += P[((long)b * Lin_s + s) * ldp + (long)j * Cout + o];
      }
      v = bias[o] + acc;
    }
    y[idx] = v;
  }
}

// x = (y0 + y1 + ... ) / n over the AMP blocks (bigvgan.py: xs += block(x); x = xs / n),
// optionally also as the next ConvTranspose's bf16 operand (ld columns).
__global__ void zv_bv_avg_kernel(const float* y0, const float* y1, const float* y2, int n, long M,
                                 int C, float* x, bf16* oh, bf16* ol, long ld) {
  const long total = M * C;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    float s = y0[idx];
    if (n > 1) s += y1[idx];
    if (n > 2) s += y2[idx];
    const float v = s / (float)n;
    x[idx] = v;
    if (oh) {
      const long m = idx / C;
      const int c = (int)(idx % C);
      split_store(oh, ol, m * ld + c, v);
    }
  }
}

// conv_post (C -> 1, 7 taps, zero "same" padding inside [0, len)) + clamp / tanh.
// A block covers 256 consecutive samples of one utterance: the (256 + 6) x C input
// window is staged in LDS with coalesced row loads, then each lane reduces its 7 x C taps.
constexpr int BV_POST_T = 256;
__global__ __launch_bounds__(BV_POST_T) void zv_bv_post_kernel(
    const float* __restrict__ a, const int* lens, int scale, int B, int Lmax, int Lp, int C,
    const float* __restrict__ w, float bias, int use_tanh, float* wav) {
  extern __shared__ float win[];                   // (BV_POST_T + 6) x C
  const int nblk = (Lmax + BV_POST_T - 1) / BV_POST_T;
  const int b = blockIdx.x / nblk, t0 = (blockIdx.x % nblk) * BV_POST_T;
  const int len = lens ? min(lens[b] * scale, Lmax) : Lmax;
  const int nwin = (BV_POST_T + 6) * C;
  for (int i = threadIdx.x; i < nwin; i += BV_POST_T) {
    const int ts = t0 - 3 + i / C;
    win[i] = (ts >= 0 && ts < len) ? a[((long)b * Lp + ts) * C + i % C] : 0.f;
  }
  __syncthreads();
  const int t = t0 + threadIdx.x;
  if (t >= Lmax) return;
  float v = 0.f;
  if (t < len) {
    float acc = 0.f;
    const float* row = win + threadIdx.x * C;
    for (int tap = 0; tap < 7; ++tap)
      for (int c = 0; c < C; ++c) acc = fmaf(w[c * 7 + tap], row[tap * C + c], acc);
    v = acc + bias;
    v = use_tanh ? tanhf(v) : fminf(fmaxf(v, -1.0f), 1.0f);
  }
  wav[(long)b * Lmax + t] = v;
}

// ===========================================================================
// host side
// ===========================================================================
struct BvAct { float* alpha = nullptr; float* ibeta = nullptr; };

// The host pieces zv_bigvgan (finalize / decode) and zv_bigvgan_check share: the weight
// relayouts, the alias-free filter, the halo rule and the launches with a choice in them.
struct BvHost {
  // zero rows around each utterance of an implicit-conv operand: >= the conv's padding, whole
  // 8-frame groups of the activation kernel; a stage stream's rows per utterance
  static int halo_for(int halo, int ks, int d) { return std::max(halo, (int)round_up(d * (ks - 1) / 2, 8)); }
  static int stage_rows(int L, int halo) { return (int)round_up(L + halo, 8); }

  // Conv1d weight (Cout, Cin, k) -> GEMM rows [o][tap * Cp + c]
  // (input channels zero-padded to Cp: the implicit-conv operand's row width)
  static std::vector<float> conv_rows(const float* w, int Cout, int Cin, int k, int Cp) {
    std::vector<float> w2((size_t)Cout * Cp * k, 0.f);
    for (int o = 0; o < Cout; ++o)
      for (int c = 0; c < Cin; ++c)
        for (int t = 0; t < k; ++t) w2[(size_t)o * Cp * k + (size_t)t * Cp + c] = w[((size_t)o * Cin + c) * k + t];
    return w2;
  }
  // ConvTranspose1d weight (Cin, Cout, k) -> GEMM rows [j * Cout + o][c]
  static std::vector<float> convt_rows(const float* w, int Cin, int Cout, int k) {
    std::vector<float> w2((size_t)k * Cout * Cin);
    for (int c = 0; c < Cin; ++c)
      for (int o = 0; o < Cout; ++o)
        for (int j = 0; j < k; ++j) w2[((size_t)j * Cout + o) * Cin + c] = w[((size_t)c * Cout + o) * k + j];
    return w2;
  }

  // the kernel's filter arguments from the 12 low-pass taps
  // upsample: y[2t] = 2 sum_m f[5-2m] x[t+m] (m=-3..2), y[2t+1] = 2 sum_m f[6-2m] x[t+m] (m=-2..3)
  static BvFilter filter_of(const float* f32) {
    BvFilter filt{};
    for (int m = 0; m < 6; ++m) {
      filt.up_even[m] = 2.0f * f32[5 - 2 * (m - 3)];
      filt.up_odd[m] = 2.0f * f32[6 - 2 * (m - 2)];
    }
    for (int n = 0; n < 12; ++n) filt.down[n] = f32[n];
    return filt;
  }
  // alias_free_activation filter.py: kaiser-windowed sinc, cutoff 0.25, half width 0.3,
  // 12 taps, normalised to unit DC gain (double, rounded once to fp32 like the buffer)
  static BvFilter make_filter() {
    const int ks = 12, half = 6;
    const double cutoff = 0.25, delta_f = 4 * 0.3;
    const double A = 2.285 * (half - 1) * M_PI * delta_f + 7.95;
    const double beta = A > 50.0 ? 0.1102 * (A - 8.7)
                        : (A >= 21.0 ? 0.5842 * pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
    double fd[12], sum = 0.0;
    for (int n = 0; n < ks; ++n) {
      const double r = 2.0 * n / (ks - 1) - 1.0;
      const double win = std::cyl_bessel_i(0.0, beta * sqrt(1.0 - r * r)) / std::cyl_bessel_i(0.0, beta);
      const double tm = (n - half) + 0.5;
      const double arg = 2.0 * cutoff * tm;
      const double sinc = arg == 0.0 ? 1.0 : sin(M_PI * arg) / (M_PI * arg);
      fd[n] = 2.0 * cutoff * win * sinc;
      sum += fd[n];
    }
    float f32[12];
    for (int n = 0; n < ks; ++n) f32[n] = (float)(fd[n] / sum);
    return filter_of(f32);
  }

  // W . A (+ bias, + resid) -> C and / or the 16-bit copy `out`; CONV: the implicit-conv A loader
  // over the (rows, conv_c) operand.  Returns the K step of the instantiation it launched.
  template <int SPLIT, int CONV = 0>
  static int gemm(const Linear& W, const Act& A, long M, float* C, long ldc, Act out, const float* resid,
                  hipStream_t s, const char* tag, int conv_c = 0, int conv_d = 1, int conv_pad = 0) {
    GemmParams p{};
    p.M = (int)M; p.N = W.N; p.K = W.K; p.nz2 = 1; p.Brows = W.Npad;
    p.Ah = A.h; p.Al = A.l; p.lda = A.ld;
    p.Bh = W.hi; p.Bl = W.lo; p.ldb = W.Kpad;
    p.bias = W.b; p.rows_per_group = 1; p.rpb = 1;
    p.resid = resid;
    p.C = C; p.ldc = ldc;
    p.Ch = out.h; p.Cl = out.l; p.ldch = out.ld;
    p.conv_c = conv_c; p.conv_d = conv_d; p.conv_pad = conv_pad;
    if constexpr (CONV) {
      // tile width matched to the narrow late stages (N = C), K step to the padded
      // channel count (Cp = round_up(C, 32): 64-deep steps when Cp % 64 == 0)
      if (conv_c % 64 == 0) {
        if (W.N <= 48)
          launch_gemm<256, 48, 4, 1, SPLIT, EPI_STD, 2, 2, 64, 0, 1>(p, 1, s, tag, true, -1);
        else if (W.N <= 64)
          launch_gemm<64, 64, 2, 2, SPLIT, EPI_STD, 2, 2, 64, 0, 1>(p, 1, s, tag, true, -1);
        else
          launch_gemm<128, 128, 2, 2, SPLIT, EPI_STD, 2, 2, 64, 0, 1>(p, 1, s, tag);
        return 64;
      }
      if (W.N <= 32)
        launch_gemm<256, 32, 4, 1, SPLIT, EPI_STD, 2, 2, 32, 0, 1>(p, 1, s, tag, true, -1);
      else if (W.N <= 96)
        launch_gemm<128, 96, 2, 2, SPLIT, EPI_STD, 2, 2, 32, 0, 1>(p, 1, s, tag, true, -1);
      else
        launch_gemm<128, 128, 2, 2, SPLIT, EPI_STD, 2, 2, 32, 0, 1>(p, 1, s, tag);
      return 32;
    } else {
      launch_gemm<128, 128, 2, 2, SPLIT, EPI_STD>(p, 1, s, tag);
      return GEMM_BK;
    }
  }

  template <int MODE>
  static void act(const BvAct& a, const BvFilter& filt, int halo, const float* in, const int* lens, int scale,
                  int B, int Lmax, int Lp, int C, float* out, Act o, hipStream_t s) {
    constexpr int TT = 8;
    const int rows = Lp + (MODE == 2 ? halo : 0);
    const long n = (long)B * cdiv(rows, TT) * C;
    hipLaunchKernelGGL((zv_bv_act_kernel<MODE, TT>), grid1d(n), dim3(256), 0, s, in, lens, scale,
                       B, Lmax, Lp, halo, C, a.alpha, a.ibeta, filt, out, o.h, o.l, o.ld);
    ZV_LAUNCH_CHECK();
  }

  // ConvTranspose1d's col2im gather (+ bias) of P (B * Ls rows of k * Co) into the stage stream
  static void convt_gather(const float* P, const float* bias, const int* lens, int scale, int B, int L, int Ls,
                           int u, int k, int Co, int Lp, float* out, hipStream_t s) {
    hipLaunchKernelGGL(zv_bv_convt_gather_kernel, grid1d((long)B * Lp * Co), dim3(256), 0, s, P, (long)k * Co, bias,
                       lens, scale, B, L, Ls, u, k, (k - u) / 2, Co, Lp, out);
    ZV_LAUNCH_CHECK();
  }
  // mean of the n AMP blocks' streams (+ the next stage's operand o)
  static void avg(const float* y0, const float* y1, const float* y2, int n, long M, int C, float* out, Act o,
                  hipStream_t s) {
    hipLaunchKernelGGL(zv_bv_avg_kernel, grid1d(M * C), dim3(256), 0, s, y0, y1, y2, n, M, C, out, o.h, o.l, o.ld);
    ZV_LAUNCH_CHECK();
  }
  // conv_post's LDS window must fit; returns its bytes
  static size_t post_lds(int C) {
    const size_t b = (size_t)(BV_POST_T + 6) * C * sizeof(float);
    ZV_REQUIRE(b <= 64 * 1024, "conv_post input channels too wide for the LDS window");
    return b;
  }
  static void post(const float* x, const int* lens, int scale, int B, int L, int Ls, int C, const float* w,
                   float bias, int use_tanh, float* wav, hipStream_t s) {
    hipLaunchKernelGGL(zv_bv_post_kernel, dim3(B * cdiv(L, BV_POST_T)), dim3(BV_POST_T), post_lds(C), s, x, lens,
                       scale, B, L, Ls, C, w, bias, use_tanh, wav);
    ZV_LAUNCH_CHECK();
  }
};

struct zv_bigvgan {
  zv_bigvgan_config cfg;
  WeightStore store;
  BvFilter filt{};
  int halo = 8;                                  // zero rows around each utterance (>= max conv pad)
  Linear conv_pre;
  std::vector<Linear> ups;
  std::vector<float*> ups_b;
  std::vector<int> chans;                        // channels after each upsampling stage
  // resblocks[i * nk + j]: convs1/convs2 [n], acts [2n], [2n+1]
  std::vector<std::vector<Linear>> c1, c2;
  std::vector<std::vector<BvAct>> acts;
  BvAct act_post;
  float* post_w = nullptr;
  float post_b = 0.f;
  DBuf x, y[3], t1[3], P, post;
  ActBuf col[3], xa;
  // the AMP blocks of a stage are independent until their average: block j runs on
  // side stream j (fork after the ConvTranspose gather, join before the average), so
  // the three GEMM chains share the CUs when one alone does not fill them
  hipStream_t side[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};

  explicit zv_bigvgan(const zv_bigvgan_config& c) : cfg(c) {}
  ~zv_bigvgan() {
    for (int j = 0; j < 3; ++j) {
      if (side[j]) (void)ZV_BLOCKING(hipStreamDestroy(side[j]));
      if (ev_join[j]) (void)ZV_BLOCKING(hipEventDestroy(ev_join[j]));
    }
    if (ev_fork) (void)ZV_BLOCKING(hipEventDestroy(ev_fork));
  }

  Linear conv_linear(const std::string& p, int Cout, int Cin, int k, bool bias, int Cp = 0) {
    if (Cp < Cin) Cp = Cin;
    const std::vector<float> w2 = BvHost::conv_rows(store.take(p + ".weight", (size_t)Cout * Cin * k).data(), Cout, Cin, k, Cp);
    return store.make_linear(w2.data(), Cout, Cp * k, bias ? store.take(p + ".bias", Cout).data() : nullptr);
  }
  BvAct snake(const std::string& p, int C) {
    const auto& a = store.take(p + "alpha", C);
    const auto& b = store.take(p + "beta", C);
    std::vector<float> ea(C), ib(C);
    for (int c = 0; c < C; ++c) {
      ea[c] = cfg.snake_logscale ? expf(a[c]) : a[c];
      const float eb = cfg.snake_logscale ? expf(b[c]) : b[c];
      ib[c] = 1.0f / (eb + 1e-9f);
    }
    return BvAct{store.upload(ea), store.upload(ib)};
  }

  void finalize() {
    const int nu = cfg.num_upsamples, nk = cfg.num_kernels;
    ZV_REQUIRE(nu >= 1 && nu <= 8 && nk >= 1 && nk <= 3, "bad num_upsamples / num_kernels");
    filt = BvHost::make_filter();
    const int C0 = cfg.upsample_initial_channel, nm = cfg.num_mels;
    conv_pre = conv_linear("conv_pre", C0, nm, 7, true);
    int C = C0;
    size_t expected = 2;
    for (int i = 0; i < nu; ++i) {
      const int u = cfg.upsample_rates[i], k = cfg.upsample_kernel_sizes[i], Co = C / 2;
      ZV_REQUIRE(u >= 1 && k >= u && (k - u) % 2 == 0, "upsample kernel / rate must satisfy k >= u, k - u even");
      ZV_REQUIRE(C % 2 == 0, "channel count must halve per stage");
      const std::string p = "ups." + std::to_string(i) + ".0.";
      const std::vector<float> w2 = BvHost::convt_rows(store.take(p + "weight", (size_t)C * Co * k).data(), C, Co, k);
      ups.push_back(store.make_linear(w2.data(), k * Co, C, nullptr));
      ups_b.push_back(store.upload_key(p + "bias", Co));
      expected += 2;
      C = Co;
      chans.push_back(C);
      for (int j = 0; j < nk; ++j) {
        const int ks = cfg.resblock_kernel_sizes[j];
        ZV_REQUIRE(ks % 2 == 1, "resblock kernel sizes must be odd");
        const std::string rp = "resblocks." + std::to_string(i * nk + j) + ".";
        std::vector<Linear> a1, a2;
        std::vector<BvAct> ac;
        for (int n = 0; n < 3; ++n) {
          const int d = cfg.resblock_dilation_sizes[j][n];
          ZV_REQUIRE(d >= 1, "bad dilation");
          halo = BvHost::halo_for(halo, ks, d);
          const int Cp = (int)round_up(C, 32);
          a1.push_back(conv_linear(rp + "convs1." + std::to_string(n), C, C, ks, true, Cp));
          a2.push_back(conv_linear(rp + "convs2." + std::to_string(n), C, C, ks, true, Cp));
          ac.push_back(snake(rp + "activations." + std::to_string(2 * n) + ".act.", C));
          ac.push_back(snake(rp + "activations." + std::to_string(2 * n + 1) + ".act.", C));
          expected += 8;
        }
        c1.push_back(std::move(a1));
        c2.push_back(std::move(a2));
        acts.push_back(std::move(ac));
      }
    }
    act_post = snake("activation_post.act.", C);
    post_w = store.upload_key("conv_post.weight", (size_t)C * 7);
    expected += 3;
    if (cfg.use_bias_at_final) {
      post_b = store.take("conv_post.bias", 1)[0];
      expected += 1;
    }
    // alias-free filter buffers (".upsample.filter", ".downsample.lowpass.filter") are
    // recomputed above; they must match it when present
    size_t filters = 0;
    for (auto& kv : store.staged) {
      const std::string& k = kv.first;
      const bool up = k.size() > 16 && k.compare(k.size() - 16, 16, ".upsample.filter") == 0;
      const bool dn = k.size() > 26 && k.compare(k.size() - 26, 26, ".downsample.lowpass.filter") == 0;
      if (!up && !dn) continue;
      ++filters;
      ZV_REQUIRE(kv.second.size() == 12, "alias-free filter " + k + " must have 12 taps");
      for (int n = 0; n < 12; ++n)
        ZV_REQUIRE(fabsf(kv.second[n] - filt.down[n]) <= 1e-6f,
                   "alias-free filter " + k + " differs from kaiser_sinc_filter1d(0.25, 0.3, 12)");
    }
    if (store.staged.size() - filters != expected)
      throw std::invalid_argument("bigvgan state dict has " + std::to_string(store.staged.size() - filters) +
                                  " tensors, config expects " + std::to_string(expected) +
                                  " (unexpected keys present)");
    store.staged.clear();
    ZV_CHECK(ZV_BLOCKING(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming)));
    for (int j = 0; j < nk; ++j) {
      ZV_CHECK(ZV_BLOCKING(hipStreamCreateWithFlags(&side[j], hipStreamNonBlocking)));
      ZV_CHECK(ZV_BLOCKING(hipEventCreateWithFlags(&ev_join[j], hipEventDisableTiming)));
    }
    store.ready = true;
  }

  template <int SPLIT, int CONV = 0>
  void gemm(const Linear& W, const Act& A, long M, float* C, long ldc, Act out, const float* resid,
            hipStream_t s, const char* tag, int conv_c = 0, int conv_d = 1, int conv_pad = 0) {
    BvHost::gemm<SPLIT, CONV>(W, A, M, C, ldc, out, resid, s, tag, conv_c, conv_d, conv_pad);
  }
  template <int MODE>
  void act(const BvAct& a, const float* in, const int* lens, int scale, int B, int Lmax, int Lp,
           int C, float* out, Act o, hipStream_t s) {
    BvHost::act<MODE>(a, filt, halo, in, lens, scale, B, Lmax, Lp, C, out, o, s);
  }

  // Stage streams: utterance b at rows b*Lp + [0, Lmax), Lp = round_up(Lmax + halo, 8);
  // every AMP Conv1d is an implicit GEMM over the (rows, Cp) activation operand (MODE 2:
  // channels zero-padded to Cp = round_up(C, 32), `halo` zero rows around each utterance
  // absorb the tap shifts).
  template <int SPLIT>
  void decode(const float* in, int layout, float div, float sub, const int* lens, int B, int T,
              float* wav, hipStream_t s) {
    const bool split = SPLIT == 3;
    const char* tg = split ? "bigvgan_gemm_fp32" : "bigvgan_gemm_bf16";
    const char* tgc = split ? "bigvgan_conv_fp32" : "bigvgan_conv_bf16";
    const int nm = cfg.num_mels, nk = cfg.num_kernels;
    // conv_pre: im2col of the mel input -> GEMM -> bf16 operand of ups[0] (rows b*T + t)
    int C = cfg.upsample_initial_channel, L = T, Ls = T, scale = 1;
    Act xcur;
    {
      Act a0 = col[0].get((long)B * T, round_up((long)nm * 7, W_KPAD), split);
      launch_voc_im2col(in, layout, div, sub, lens, B, T, nm, 7, a0, s);
      xcur = xa.get((long)B * T, round_up(C, W_KPAD), split);
      gemm<SPLIT>(conv_pre, a0, (long)B * T, nullptr, 0, xcur, nullptr, s, tg);
    }
    float* xs = nullptr;
    for (int i = 0; i < cfg.num_upsamples; ++i) {
      const int u = cfg.upsample_rates[i], k = cfg.upsample_kernel_sizes[i], Co = chans[i];
      // ConvTranspose1d: P = x W^T (N = k * Co), col2im gather (+ bias)
      const long Min = (long)B * Ls;
      float* Pb = P.get<float>((size_t)Min * k * Co);
      gemm<SPLIT>(ups[i], xcur, Min, Pb, (long)k * Co, Act{}, nullptr, s, tg);
      const int Lo = L * u, Lp = BvHost::stage_rows(Lo, halo);
      const long M = (long)B * Lp;
      xs = x.get<float>((size_t)M * Co);
      BvHost::convt_gather(Pb, ups_b[i], lens, scale, B, L, Ls, u, k, Co, Lp, xs, s);
      C = Co; L = Lo; Ls = Lp; scale *= u;
      const int Cp = (int)round_up(C, 32);
      // AMP blocks, block j on side stream j
      float* yb[3] = {nullptr, nullptr, nullptr};
      float* tb[3] = {nullptr, nullptr, nullptr};
      Act ca[3];
      for (int j = 0; j < nk; ++j) {      // (allocation may synchronise: before the fork)
        yb[j] = y[j].get<float>((size_t)M * C);
        tb[j] = t1[j].get<float>((size_t)M * C);
        ca[j] = col[j].get(M + 2 * halo, Cp, split);
        ca[j].h += (long)halo * Cp;
        if (ca[j].l) ca[j].l += (long)halo * Cp;
      }
      ZV_CHECK(hipEventRecord(ev_fork, s));
      for (int j = 0; j < nk; ++j) {
        hipStream_t sj = side[j];
        ZV_CHECK(hipStreamWaitEvent(sj, ev_fork, 0));
        const int ks = cfg.resblock_kernel_sizes[j];
        const int r = i * nk + j;
        for (int n = 0; n < 3; ++n) {
          const float* yin = n == 0 ? xs : yb[j];
          const int d = cfg.resblock_dilation_sizes[j][n];
          act<2>(acts[r][2 * n], yin, lens, scale, B, L, Lp, C, nullptr, ca[j], sj);
          gemm<SPLIT, 1>(c1[r][n], ca[j], M, tb[j], C, Act{}, nullptr, sj, tgc, Cp, d, d * (ks - 1) / 2);
          act<2>(acts[r][2 * n + 1], tb[j], lens, scale, B, L, Lp, C, nullptr, ca[j], sj);
          gemm<SPLIT, 1>(c2[r][n], ca[j], M, yb[j], C, Act{}, yin, sj, tgc, Cp, 1, (ks - 1) / 2);
        }
        ZV_CHECK(hipEventRecord(ev_join[j], sj));
        ZV_CHECK(hipStreamWaitEvent(s, ev_join[j], 0));
      }
      const bool last = i + 1 == cfg.num_upsamples;
      Act xo = last ? Act{} : xa.get(M, round_up(C, W_KPAD), split);
      BvHost::avg(yb[0], yb[1], yb[2], nk, M, C, xs, xo, s);
      xcur = xo;
    }
    const long M = (long)B * Ls;
    float* ab = post.get<float>((size_t)M * C);
    act<0>(act_post, xs, lens, scale, B, L, Ls, C, ab, Act{}, s);
    BvHost::post(ab, lens, scale, B, L, Ls, C, post_w, post_b, cfg.use_tanh_at_final, wav, s);
  }

  size_t device_bytes() const {
    size_t b = store.weight_bytes + x.bytes + P.bytes + post.bytes + xa.bytes();
    for (int j = 0; j < 3; ++j) b += y[j].bytes + t1[j].bytes + col[j].bytes();
    return b;
  }
};
