// Prompt resampler for gfx950: torchaudio.transforms.Resample (sinc_interp_hann,
// lowpass_filter_width 6, rolloff 0.99), the step the reference runs on a loaded prompt
// whose rate differs from the model's.
//
// Reference: zipvoice/bin/infer_zipvoice.py:332-338 and infer_zipvoice_dialog.py:270-277,
// :417-422.  With g = gcd(orig, new), o = orig / g, n = new / g torchaudio convolves the
// zero-padded input with a dense [n, 2 width + o] table at stride o: output i*n + j is
// sum_k K[j, k] xpad[i*o + k].  Only the taps with |t| < lowpass_filter_width are nonzero in
// fp32, so the host plan (zipvoice_amd/feature.py resample_plan) hands over the compact
// form: per phase j a first-tap offset start[j] (relative to sample i*o) and S taps
// table[j, 0..S).  The dense table (4.5 GB for 48001 -> 24000) is never built.
//
// One kernel per batch: a workgroup owns RS_THREADS * 8 (or fewer, see plan()) consecutive
// outputs y of one row.  pos(y) = (y / n) * o + start[y % n] is non-decreasing in y, so
// these outputs read one contiguous input span; the workgroup stages it in LDS once
// (samples before 0 or at / past lens[r] are 0: torchaudio's zero padding, and what makes
// a row of a ragged batch equal that row alone), then every lane accumulates its outputs
// with fp32 FMAs, taps ascending, one accumulator per output, and stores lane-contiguously.
// The table is kept transposed ([S, n]: lanes with consecutive phases read consecutive
// words, in LDS and in global memory alike); it is copied into LDS when it fits beside the
// span and read through L2 otherwise.
#pragma once

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_FLOATS = 16384;      // 64 KiB: input span (+ table when it fits)
constexpr int RS_MAX_S = 512;             // taps per output (o / n up to ~42 at width 6)
constexpr long RS_MAX_TABLE = 16L << 20;  // n * S entries (64 MiB)

template <bool TABLE_LDS>
__global__ __launch_bounds__(RS_THREADS) void zv_resample_kernel(
    const float* wav, long wav_ld, const int* lens, int o, int n, int S, int E, int span_max,
    const int* start, const float* table_t, float* out, long out_ld, long out_cols) {
  extern __shared__ float rs_lds[];
  float* xs = rs_lds;                      // [span_max]
  float* ts = rs_lds + span_max;           // [S, n] when TABLE_LDS
  const int r = blockIdx.y, tid = threadIdx.x;
  const long y0 = (long)blockIdx.x * E;
  const long y1 = min(y0 + (long)E, out_cols);          // this workgroup's outputs [y0, y1)
  const long len = lens[r];
  const long olen = min(((long)n * len + o - 1) / o, out_cols);
  float* orow = out + (long)r * out_ld;
  if (y0 >= olen) {                        // past the row's end: zeros only
    for (long y = y0 + tid; y < y1; y += RS_THREADS) orow[y] = 0.f;
    return;
  }
  // local output e = y - y0 has phase (j0 + e) % n and input offset
  // ((j0 + e) / n) * o + start[phase] - start[j0] from the span's first sample pos0
  const int j0 = (int)(y0 % n), s0 = start[j0];
  const long pos0 = (y0 / n) * o + s0;
  const int ne = (int)(y1 - y0);                        // outputs stored (<= E)
  const int nc = (int)(min(y1, olen) - y0);             // of which computed (>= 1)
  const int jl = j0 + nc - 1;
  const int span = min((jl / n) * o + start[jl % n] - s0 + S, span_max);
  const float* x = wav + (long)r * wav_ld;
  for (int s = tid; s < span; s += RS_THREADS) {
    const long g = pos0 + s;
    xs[s] = (g >= 0 && g < len) ? x[g] : 0.f;
  }
  if (TABLE_LDS)
    for (int i = tid; i < S * n; i += RS_THREADS) ts[i] = table_t[i];
  __syncthreads();
  const float* tab = TABLE_LDS ? ts : table_t;
  for (int e = tid; e < ne; e += RS_THREADS) {
    float acc = 0.f;
    if (e < nc) {
      const int jj = j0 + e, j = jj % n;
      const int p = (jj / n) * o + start[j] - s0;       // p + S <= span
      for (int k = 0; k < S; ++k) acc = fmaf(tab[k * n + j], xs[p + k], acc);
    }
    orow[y0 + e] = acc;
  }
}

struct zv_resample {
  int o = 0, n = 0, S = 0;
  int E = 0, span_max = 0;                 // outputs per workgroup, LDS span in samples
  bool table_lds = false;
  int* start = nullptr;                    // [n]
  float* table_t = nullptr;                // [S, n]
  size_t bytes = 0;
  ~zv_resample() {
    if (start) (void)ZV_BLOCKING(hipFree(start));
    if (table_t) (void)ZV_BLOCKING(hipFree(table_t));
  }
  // the longest input span of E consecutive outputs: max over the first phase of
  // pos(j0 + E - 1) - pos(j0) + S
  static long span_of(const int32_t* st, int o, int n, int S, int E) {
    long m = 0;
    for (int j0 = 0; j0 < n; ++j0) {
      const long y = (long)j0 + E - 1;
      m = std::max(m, (y / n) * o + st[y % n] - st[j0] + S);
    }
    return m;
  }
  void init(int o_, int n_, int S_, const int32_t* st, const float* tab) {
    ZV_REQUIRE(o_ > 0 && n_ > 0, "o and n must be positive");
    ZV_REQUIRE(o_ != n_, "o == n: equal rates need no resampling (return the input)");
    ZV_REQUIRE(S_ > 0 && S_ <= RS_MAX_S, "S must be in [1, 512]");
    ZV_REQUIRE((long)n_ * S_ <= RS_MAX_TABLE, "n * S exceeds 16 Mi table entries");
    for (int j = 1; j < n_; ++j)
      ZV_REQUIRE(st[j] >= st[j - 1], "host_start must be non-decreasing");
    ZV_REQUIRE((long)st[n_ - 1] - st[0] <= o_, "host_start spans more than o samples");
    ZV_REQUIRE(st[0] >= -(1 << 24) && st[n_ - 1] <= (1 << 24), "host_start out of range");
    o = o_; n = n_; S = S_;
    // the largest workgroup tile whose span (and, preferably, the table) fits the LDS budget
    for (int pass = 0; pass < 2 && !E; ++pass)
      for (int e = RS_THREADS * 8; e >= RS_THREADS && !E; e /= 2) {
        const long sp = span_of(st, o, n, S, e);
        const long tb = pass == 0 ? (long)n * S : 0;
        if (sp + tb <= RS_LDS_FLOATS) { E = e; span_max = (int)sp; table_lds = pass == 0; }
      }
    ZV_REQUIRE(E > 0, "o / n too large: the input span of 256 outputs exceeds 64 KiB of LDS");
    std::vector<float> tt((size_t)n * S);
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < S; ++k) tt[(size_t)k * n + j] = tab[(size_t)j * S + k];
    ZV_CHECK(ZV_BLOCKING(hipMalloc(&start, (size_t)n * sizeof(int))));
    ZV_CHECK(ZV_BLOCKING(hipMemcpy(start, st, (size_t)n * sizeof(int), hipMemcpyHostToDevice)));
    ZV_CHECK(ZV_BLOCKING(hipMalloc(&table_t, tt.size() * sizeof(float))));
    ZV_CHECK(ZV_BLOCKING(hipMemcpy(table_t, tt.data(), tt.size() * sizeof(float),
                                   hipMemcpyHostToDevice)));
    bytes = (size_t)n * sizeof(int) + tt.size() * sizeof(float);
  }
  void apply(const float* wav, long wav_ld, const int* lens, int R, float* out, long out_ld,
             long out_cols, hipStream_t s) {
    dim3 grid(cdiv(out_cols, E), R);
    const size_t lds = ((size_t)span_max + (table_lds ? (size_t)n * S : 0)) * sizeof(float);
    if (table_lds)
      hipLaunchKernelGGL(zv_resample_kernel<true>, grid, dim3(RS_THREADS), lds, s, wav, wav_ld,
                         lens, o, n, S, E, span_max, start, table_t, out, out_ld, out_cols);
    else
      hipLaunchKernelGGL(zv_resample_kernel<false>, grid, dim3(RS_THREADS), lds, s, wav, wav_ld,
                         lens, o, n, S, E, span_max, start, table_t, out, out_ld, out_cols);
    ZV_LAUNCH_CHECK();
  }
};
