// Vocos vocoder (mel-24khz configuration) for gfx950: mel (B, n_mels, T) -> wav (B, T*hop).
//
// The reference calls the third-party `vocos` package after sampling
// (zipvoice/bin/infer_zipvoice.py:249-260, :374-378; dialog stereo
// infer_zipvoice_dialog.py:483-488).  Published algorithm (vocos 0.1.0):
//   VocosBackbone: embed Conv1d(n_mels, dim, 7, pad 3) -> LayerNorm(1e-6) ->
//                  num_layers x ConvNeXtBlock -> final LayerNorm
//   ConvNeXtBlock: dwconv k7 -> LayerNorm -> Linear(dim, inter) -> GELU ->
//                  Linear(inter, dim) -> x + gamma * y
//   ISTFTHead:     Linear(dim, n_fft + 2) -> mag = min(exp, 1e2), S = mag e^{i phase} ->
//                  irfft(n_fft) * window -> overlap-add (hop) -> trim (n_fft-hop)/2 per side ->
//                  / sum of squared windows
// MI355X mapping: every contraction is the engine's MFMA GEMM (zv_gemm.inc):
//   * embed conv = GEMM over an im2col operand (K = 7 * n_mels; the A23 post-processing
//     `pred.permute(0,2,1) / feat_scale - feat_bias` is folded into the im2col read);
//   * pwconv1 with the GELU epilogue, pwconv2 with the layer-scale + residual epilogue;
//   * the head Linear with the SPEC epilogue (exp/clip/sincos -> re/im operand);
//   * irfft * window = one GEMM against a precomputed real basis
//     C[n][k] = w[n] c_k cos(2 pi k n / N) / N, S[n][k] = -w[n] c_k sin(2 pi k n / N) / N
//     (c_0 = c_{N/2} = 1, else 2; the DC / Nyquist imaginary parts drop out as in C2R);
//   * overlap-add + envelope division + clamp in one gather kernel (each output sample
//     sums its <= n_fft/hop frames; no atomics).
// Row-local kernels (LayerNorm, dwconv+LayerNorm) run one wave per frame.
#pragma once

// ---- im2col of the embed conv input (+ A23 feature post-processing) --------
// in: layout 0 = (B, C, T) (Vocos.decode input), 1 = (B, T, C) (model output);
// v = in / div - sub; A[b*T + t][tap*C + c] = v[b, c, t + tap - ks/2] (0 outside [0, len_b)).
__global__ void zv_voc_im2col_kernel(const float* in, int layout, float div, float sub,
                                     const int* lens, int B, int T, int C, int ks, bf16* oh,
                                     bf16* ol, long ld) {
  const int K = ks * C;
  const long total = (long)B * T * K;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int j = (int)(idx % K);
    const long row = idx / K;
    const int t = (int)(row % T), b = (int)(row / T);
    const int tap = j / C, c = j % C;
    const int ts = t + tap - ks / 2;
    const int len = lens ? lens[b] : T;
    float v = 0.f;
    if (ts >= 0 && ts < len) {
      const float x = layout == 0 ? in[((long)b * C + c) * T + ts] : in[((long)b * T + ts) * C + c];
      v = x / div - sub;
    }
    split_store(oh, ol, row * ld + j, v);
  }
}
static void launch_voc_im2col(const float* in, int layout, float div, float sub, const int* lens, int B, int T,
                              int C, int ks, const Act& out, hipStream_t s) {
  hipLaunchKernelGGL(zv_voc_im2col_kernel, grid1d((long)B * T * C * ks), dim3(256), 0, s, in, layout, div, sub,
                     lens, B, T, C, ks, out.h, out.l, out.ld);
  ZV_LAUNCH_CHECK();
}

// ---- LayerNorm over C channels, one wave per row (C % 4 == 0, C <= 1024) ----
// y = (x - mean) / sqrt(var + eps) * w + b  (biased variance, two-pass in registers)
constexpr int LN_MAXCH = 4;   // 4 chunks of 256 channels
__device__ __forceinline__ void ln_row(f32x4 (&v)[LN_MAXCH], int C, int lane, const float* w,
                                       const float* b, float eps) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i)
    if (i * 256 + lane * 4 < C) s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  const float mean = s / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i)
    if (i * 256 + lane * 4 < C) {
      const f32x4 d = v[i] - mean;
      ss += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  const float rstd = 1.0f / sqrtf(ss / (float)C + eps);
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    const int k = i * 256 + lane * 4;
    if (k < C) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(b + k);
      v[i] = (v[i] - mean) * rstd * wv + bv;
    }
  }
}

__device__ __forceinline__ void ln_store(const f32x4 (&v)[LN_MAXCH], int C, int lane, long m,
                                         float* out, bf16* oh, bf16* ol, long ld) {
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    const int k = i * 256 + lane * 4;
    if (k < C) {
      if (out) *reinterpret_cast<f32x4*>(out + m * C + k) = v[i];
      if (oh) {
        float a[4] = {v[i][0], v[i][1], v[i][2], v[i][3]};
        store_split4(oh, ol, m * ld + k, a);
      }
    }
  }
}

__global__ __launch_bounds__(256) void zv_layernorm_kernel(const float* x, const float* w,
                                                           const float* b, float eps, float* out,
                                                           bf16* oh, bf16* ol, long ld, long M,
                                                           int C) {
  const long m = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  f32x4 v[LN_MAXCH];
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    const int k = i * 256 + lane * 4;
    v[i] = k < C ? *reinterpret_cast<const f32x4*>(x + m * C + k) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  ln_row(v, C, lane, w, b, eps);
  ln_store(v, C, lane, m, out, oh, ol, ld);
}

// ---- ConvNeXt dwconv (k taps, "same", bias) + LayerNorm -> GEMM operand ------
// x: (B*T, C) fp32; frames >= len_b read as zero (per-utterance conv padding).
template <int KS>
__global__ __launch_bounds__(256) void zv_voc_dwconv_ln_kernel(
    const float* x, const int* lens, int T, const float* w, const float* bias, const float* lw,
    const float* lb, float eps, bf16* oh, bf16* ol, long ld, long M, int C) {
  const long m = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const int t = (int)(m % T), b = (int)(m / T);
  const int len = lens ? lens[b] : T;
  f32x4 v[LN_MAXCH];
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    const int k = i * 256 + lane * 4;
    if (k >= C) { v[i] = f32x4{0.f, 0.f, 0.f, 0.f}; continue; }
    float a[4] = {bias[k], bias[k + 1], bias[k + 2], bias[k + 3]};
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < KS; ++tap) {
      const int ts = t + tap - KS / 2;
      if (ts < 0 || ts >= len) continue;
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + ((long)b * T + ts) * C + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(xv[e], w[(k + e) * KS + tap], acc[e]);
    }
    v[i] = f32x4{acc[0] + a[0], acc[1] + a[1], acc[2] + a[2], acc[3] + a[3]};
  }
  ln_row(v, C, lane, lw, lb, eps);
  ln_store(v, C, lane, m, nullptr, oh, ol, ld);
}

// ---- overlap-add + window-envelope normalisation (+ clamp) -----------------
// wav[b, i] (i < len_b * hop) = sum_f frames[b*T + f][p - f*hop] / sum_f window[p - f*hop]^2,
// p = i + (n_fft - hop)/2, f over this utterance's frames covering p; 0 beyond len_b * hop.
__global__ void zv_voc_ola_kernel(const float* frames, const float* window, const int* lens,
                                  int B, int T, int hop, int n_fft, float* wav, int clamp) {
  const long total = (long)B * T * hop;
  const int pad = (n_fft - hop) / 2;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int b = (int)(idx / ((long)T * hop));
    const int i = (int)(idx % ((long)T * hop));
    const int len = lens ? lens[b] : T;
    float y = 0.f;
    if (i < len * hop) {
      const int p = i + pad;
      int f0 = (p - n_fft) / hop + 1;
      if (p - n_fft < 0) f0 = 0;
      const int f1 = min(p / hop, len - 1);
      float acc = 0.f, env = 0.f;
      for (int f = f0; f <= f1; ++f) {
        const int n = p - f * hop;
        const float wn = window[n];
        acc += frames[((long)b * T + f) * n_fft + n];
        env += wn * wn;
      }
      y = acc / env;
      if (clamp) y = fminf(fmaxf(y, -1.0f), 1.0f);
    }
    wav[idx] = y;
  }
}

// ===========================================================================
// host side
// ===========================================================================
struct zv_vocoder {
  zv_vocoder_config cfg;
  WeightStore store;
  int nbins = 0, nbins_pad = 0, spec_ld = 0;
  Linear embed, head, basis;
  std::vector<Linear> pw1, pw2;
  std::vector<float*> dw_w, dw_b, ln_w, ln_b, gamma;
  float *norm0_w = nullptr, *norm0_b = nullptr, *normf_w = nullptr, *normf_b = nullptr;
  float* window = nullptr;
  DBuf x, frames, lens_d;
  ActBuf col, h, hid, spec;

  explicit zv_vocoder(const zv_vocoder_config& c) : cfg(c) {}

  // host matrix w (N x K, row-major, computed in double) -> the padded hi/lo device weight
  Linear make_linear(const std::vector<double>& w, int N, int K, const std::vector<float>* b) {
    const std::vector<float> wf(w.begin(), w.end());
    return store.make_linear(wf.data(), N, K, b ? b->data() : nullptr);
  }

  void finalize() {
    const int C = cfg.dim, I = cfg.intermediate_dim, nm = cfg.n_mels, ke = cfg.embed_kernel;
    ZV_REQUIRE(C % 64 == 0 && C <= 256 * LN_MAXCH, "vocoder dim must be a multiple of 64, <= 1024");
    ZV_REQUIRE(cfg.dw_kernel == 7, "vocoder ConvNeXt kernel must be 7");
    ZV_REQUIRE(cfg.n_fft % 32 == 0 && cfg.hop > 0 && cfg.n_fft > cfg.hop && (cfg.n_fft - cfg.hop) % 2 == 0,
               "bad n_fft / hop");
    // embed conv (C, n_mels, ke) -> [o][tap * n_mels + c]
    {
      const auto& w = store.take("backbone.embed.weight", (size_t)C * nm * ke);
      std::vector<double> w2((size_t)C * nm * ke);
      for (int o = 0; o < C; ++o)
        for (int c = 0; c < nm; ++c)
          for (int t = 0; t < ke; ++t) w2[(size_t)o * nm * ke + t * nm + c] = w[((size_t)o * nm + c) * ke + t];
      embed = make_linear(w2, C, nm * ke, &store.take("backbone.embed.bias", C));
    }
    norm0_w = store.upload_key("backbone.norm.weight", C);
    norm0_b = store.upload_key("backbone.norm.bias", C);
    for (int i = 0; i < cfg.num_layers; ++i) {
      const std::string p = "backbone.convnext." + std::to_string(i) + ".";
      dw_w.push_back(store.upload_key(p + "dwconv.weight", (size_t)C * 7));
      dw_b.push_back(store.upload_key(p + "dwconv.bias", C));
      ln_w.push_back(store.upload_key(p + "norm.weight", C));
      ln_b.push_back(store.upload_key(p + "norm.bias", C));
      pw1.push_back(store.make_linear(store.take(p + "pwconv1.weight", (size_t)I * C).data(), I, C,
                                      store.take(p + "pwconv1.bias", I).data()));
      pw2.push_back(store.make_linear(store.take(p + "pwconv2.weight", (size_t)C * I).data(), C, I,
                                      store.take(p + "pwconv2.bias", C).data()));
      gamma.push_back(store.upload_key(p + "gamma", C));
    }
    normf_w = store.upload_key("backbone.final_layer_norm.weight", C);
    normf_b = store.upload_key("backbone.final_layer_norm.bias", C);
    // head Linear (n_fft+2, C): rows [mag | phase] -> groups of 32 = [mag16 | phase16],
    // bins padded to a multiple of 16 with zero rows
    const int N = cfg.n_fft;
    nbins = N / 2 + 1;
    nbins_pad = (int)round_up(nbins, 16);
    spec_ld = (int)round_up(2 * nbins_pad, W_KPAD);
    {
      const auto& w = store.take("head.out.weight", (size_t)2 * nbins * C);
      const auto& b = store.take("head.out.bias", (size_t)2 * nbins);
      std::vector<double> w2((size_t)2 * nbins_pad * C, 0.0);
      std::vector<float> b2((size_t)2 * nbins_pad, 0.f);
      for (int g = 0; g < nbins_pad / 16; ++g)
        for (int i = 0; i < 16; ++i) {
          const int k = g * 16 + i;
          if (k >= nbins) continue;
          for (int half = 0; half < 2; ++half) {
            const int dst = g * 32 + half * 16 + i, src = half * nbins + k;
            for (int c = 0; c < C; ++c) w2[(size_t)dst * C + c] = w[(size_t)src * C + c];
            b2[dst] = b[src];
          }
        }
      head = make_linear(w2, 2 * nbins_pad, C, &b2);
    }
    // irfft * window basis: frame[n] = sum_k re_k C[n][k] + im_k S[n][k];
    // A operand columns [re (nbins_pad) | im (nbins_pad)]
    const auto& win = store.take("head.istft.window", N);
    window = store.upload(win);
    {
      std::vector<double> w2((size_t)N * 2 * nbins_pad, 0.0);
      for (int n = 0; n < N; ++n)
        for (int k = 0; k < nbins; ++k) {
          const double ck = (k == 0 || 2 * k == N) ? 1.0 : 2.0;
          const long r = ((long)k * n) % N;           // exact angle reduction
          const double ang = 2.0 * M_PI * (double)r / (double)N;
          w2[(size_t)n * 2 * nbins_pad + k] = win[n] * ck * cos(ang) / N;
          if (k != 0 && 2 * k != N)
            w2[(size_t)n * 2 * nbins_pad + nbins_pad + k] = -win[n] * ck * sin(ang) / N;
        }
      basis = make_linear(w2, N, 2 * nbins_pad, nullptr);
    }
    size_t expected = 6 + 9 * (size_t)cfg.num_layers + 3;
    size_t ignored = 0;
    for (auto& kv : store.staged)
      if (kv.first.rfind("feature_extractor.", 0) == 0) ++ignored;   // mel front-end buffers
    if (store.staged.size() - ignored != expected)
      throw std::invalid_argument("vocoder state dict has " + std::to_string(store.staged.size() - ignored) +
                                  " tensors, config expects " + std::to_string(expected) +
                                  " (unexpected keys present)");
    store.staged.clear();
    store.ready = true;
  }

  template <int SPLIT, int EPI>
  void gemm(const Linear& W, const Act& A, long M, float* C, long ldc, Act out, int act,
            const float* colscale, const float* resid, hipStream_t s, const char* tag) {
    GemmParams p{};
    p.M = (int)M; p.N = W.N; p.K = W.K; p.nz2 = 1; p.Brows = W.Npad;
    p.Ah = A.h; p.Al = A.l; p.lda = A.ld;
    p.Bh = W.hi; p.Bl = W.lo; p.ldb = W.Kpad;
    p.bias = W.b; p.rows_per_group = 1; p.rpb = 1;
    p.act = act; p.colscale = colscale; p.resid = resid;
    p.C = C; p.ldc = ldc;
    p.Ch = out.h; p.Cl = out.l; p.ldch = out.ld;
    p.spec_im_off = nbins_pad;
    launch_gemm<128, 128, 2, 2, SPLIT, EPI>(p, 1, s, tag);
  }

  template <int SPLIT>
  void decode(const float* in, int layout, float div, float sub, const int* lens, int B, int T,
              float* wav, int clamp, hipStream_t s) {
    const bool split = SPLIT == 3;
    const long M = (long)B * T;
    const int C = cfg.dim, nm = cfg.n_mels, ke = cfg.embed_kernel;
    const char* tg = split ? "vocos_gemm_fp32" : "vocos_gemm_bf16";
    Act a0 = col.get(M, round_up((long)nm * ke, W_KPAD), split);
    launch_voc_im2col(in, layout, div, sub, lens, B, T, nm, ke, a0, s);
    float* xs = x.get<float>((size_t)M * C);
    gemm<SPLIT, EPI_STD>(embed, a0, M, xs, C, Act{}, 0, nullptr, nullptr, s, tg);
    hipLaunchKernelGGL(zv_layernorm_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, xs, norm0_w, norm0_b,
                       1e-6f, xs, (bf16*)nullptr, (bf16*)nullptr, 0L, M, C);
    ZV_LAUNCH_CHECK();
    Act ha = h.get(M, C, split);
    Act hh = hid.get(M, round_up(cfg.intermediate_dim, W_KPAD), split);
    for (int i = 0; i < cfg.num_layers; ++i) {
      hipLaunchKernelGGL(zv_voc_dwconv_ln_kernel<7>, dim3(cdiv(M, 4)), dim3(256), 0, s, xs, lens, T,
                         dw_w[i], dw_b[i], ln_w[i], ln_b[i], 1e-6f, ha.h, ha.l, ha.ld, M, C);
      ZV_LAUNCH_CHECK();
      gemm<SPLIT, EPI_STD>(pw1[i], ha, M, nullptr, 0, hh, 2, nullptr, nullptr, s, tg);
      gemm<SPLIT, EPI_STD>(pw2[i], hh, M, xs, C, Act{}, 0, gamma[i], xs, s, tg);
    }
    hipLaunchKernelGGL(zv_layernorm_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, xs, normf_w, normf_b,
                       1e-6f, (float*)nullptr, ha.h, ha.l, ha.ld, M, C);
    ZV_LAUNCH_CHECK();
    Act sp = spec.get(M, spec_ld, split);
    gemm<SPLIT, EPI_SPEC>(head, ha, M, nullptr, 0, sp, 0, nullptr, nullptr, s,
                          split ? "vocos_head_fp32" : "vocos_head_bf16");
    float* fr = frames.get<float>((size_t)M * cfg.n_fft);
    gemm<SPLIT, EPI_STD>(basis, sp, M, fr, cfg.n_fft, Act{}, 0, nullptr, nullptr, s,
                         split ? "vocos_istft_fp32" : "vocos_istft_bf16");
    hipLaunchKernelGGL(zv_voc_ola_kernel, grid1d(M * cfg.hop), dim3(256), 0, s, fr, window, lens, B,
                       T, cfg.hop, cfg.n_fft, wav, clamp);
    ZV_LAUNCH_CHECK();
  }
};
