// Voice store for gfx950: the prompt front kept on the device (zipvoice_amd/voices.py VoiceStore).
// No reference counterpart: the reference normalises a prompt on the host, once per sentence
// (zipvoice/bin/infer_zipvoice.py:340-342, :399-400).  The behaviour is defined in
// include/zipvoice_hip.h and restated in numpy by tests/voice_ref.py.
//   rms      one workgroup of 256 per row.  Lane j adds the float64 squares of elements j, j + 256, ...
//            of the row in rising order; the 256 partial sums are folded in LDS, at widths 128, 64,
//            ... 1 (s[j] += s[j + w] for j < w); lane 0 divides by the length, takes the float64 root
//            and rounds it once to fp32.  The order is a function of the row's length alone, so the
//            result does not depend on B, ld or the launch.  len * 4 bytes read, 12 written per row.
//   scale    y = (x * target) / rms (fp32, IEEE division) on the rows below the target, a copy on the
//            others, zeros on columns [len, ld).  Four samples per thread as 16-byte loads and stores
//            when ld % 4 == 0 and both bases are 16-byte aligned, one sample otherwise.  ld * 4 bytes
//            written per row, len * 4 read.
//   gather   one admitted row per blockIdx.y: the voice's frames * F values as one flat copy from the
//            pool, then one flat zero fill up to T * F (sess_copy_zero, zv_session.inc: f32x4 when
//            F % 4 == 0 and the bases are 16-byte aligned); the row's gain is copied by one thread.
//            The {offset, frames} table is a host array, checked completely before anything is
//            queued, and travels through the pinned staging of a zv_edit (zv_edit.inc).
// No atomics; every output element is written once, by one thread.
#pragma once

constexpr int VOICE_THREADS = 256;

// a row's length as the kernels use it: never outside [0, ld], whatever the device array holds
__device__ __forceinline__ long voice_len(int len, long ld) { return len < 0 ? 0 : (len > ld ? ld : (long)len); }

__global__ __launch_bounds__(VOICE_THREADS) void zv_prompt_rms_kernel(const float* wav, long ld, const int* lens,
                                                                     float target, float* rms, float* gain_in,
                                                                     float* gain_out) {
  __shared__ double s[VOICE_THREADS];
  const int b = blockIdx.x, j = threadIdx.x;
  const long n = voice_len(lens[b], ld);
  const float* x = wav + (long)b * ld;
  double acc = 0.0;
  for (long i = j; i < n; i += VOICE_THREADS) {
    const double v = (double)x[i];
    acc += v * v;                                  // (v * v is exact in float64: fused or not, the same sum)
  }
  s[j] = acc;
  __syncthreads();
  for (int w = VOICE_THREADS / 2; w > 0; w >>= 1) {
    if (j < w) s[j] += s[j + w];
    __syncthreads();
  }
  if (j == 0) {
    const float r = (float)sqrt(s[0] / (double)n);
    const bool quiet = r < target;
    rms[b] = r;
    gain_in[b] = quiet ? __fdiv_rn(target, r) : 1.f;
    gain_out[b] = quiet ? __fdiv_rn(r, target) : 1.f;
  }
}

__device__ __forceinline__ float voice_scale1(float x, bool quiet, float target, float r) {
  return quiet ? __fdiv_rn(x * target, r) : x;
}

template <bool QUAD>
__global__ __launch_bounds__(VOICE_THREADS) void zv_prompt_scale_kernel(const float* wav, long ld, const int* lens,
                                                                       const float* rms, float target, float* out) {
  const int b = blockIdx.y;
  const long n = voice_len(lens[b], ld);
  const float r = rms[b];
  const bool quiet = r < target;
  const float* x = wav + (long)b * ld;
  float* y = out + (long)b * ld;
  const long stride = (long)gridDim.x * blockDim.x;
  if (QUAD) {
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < ld / 4; q += stride) {
      const long i = q * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i + 4 <= n) {
        v = *reinterpret_cast<const f32x4*>(x + i);
        for (int k = 0; k < 4; ++k) v[k] = voice_scale1(v[k], quiet, target, r);
      } else {
        for (int k = 0; k < 4; ++k)
          if (i + k < n) v[k] = voice_scale1(x[i + k], quiet, target, r);
      }
      *reinterpret_cast<f32x4*>(y + i) = v;
    }
  } else {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < ld; i += stride)
      y[i] = i < n ? voice_scale1(x[i], quiet, target, r) : 0.f;
  }
}

struct VoiceRow { int off, frames; };   // one row of a gather table: first pool row, frames

template <bool QUAD>
__global__ __launch_bounds__(VOICE_THREADS) void zv_voice_gather_kernel(const float* pool, const VoiceRow* tab, int T,
                                                                       int F, float* out, const float* gains_pool,
                                                                       float* gains_out) {
  const VoiceRow r = tab[blockIdx.y];
  sess_copy_zero<QUAD>(out + (long)blockIdx.y * T * F, pool + (long)r.off * F, r.frames * F, T * F);
  if (gains_out && blockIdx.x == 0 && threadIdx.x == 0) gains_out[blockIdx.y] = gains_pool[r.off];
}

// ---- launches (the C ABI below them in zv_engine.hip) ----
static void voice_check_lens(const int* host_lens, int B, long ld, const char* who) {
  for (int b = 0; b < B; ++b)
    ZV_REQUIRE(host_lens[b] >= 1 && host_lens[b] <= ld,
               std::string(who) + ": every length must be in [1, ld] (row " + std::to_string(b) + ")");
}
static void launch_prompt_rms(const float* wav, long ld, const int* lens, int B, float target, float* rms,
                              float* gain_in, float* gain_out, hipStream_t s) {
  hipLaunchKernelGGL(zv_prompt_rms_kernel, dim3((unsigned)B), dim3(VOICE_THREADS), 0, s, wav, ld, lens, target, rms,
                     gain_in, gain_out);
  ZV_LAUNCH_CHECK();
}
// form 1: the quad kernel
static EdgeLaunch launch_prompt_scale(const float* wav, long ld, const int* lens, const float* rms, int B,
                                      float target, float* out, hipStream_t s) {
  const bool quad = ld % 4 == 0 && sess_aligned16(wav, out);
  const dim3 grid = sched_grid(quad ? ld / 4 : ld, B);
  if (quad)
    hipLaunchKernelGGL(zv_prompt_scale_kernel<true>, grid, dim3(VOICE_THREADS), 0, s, wav, ld, lens, rms, target, out);
  else
    hipLaunchKernelGGL(zv_prompt_scale_kernel<false>, grid, dim3(VOICE_THREADS), 0, s, wav, ld, lens, rms, target, out);
  ZV_LAUNCH_CHECK();
  return {quad ? 1 : 0, (int)grid.x, VOICE_THREADS};
}

struct zv_voice {
  zv_edit stage;   // the pinned staging ring and the device table (zv_edit::upload)

  EdgeLaunch gather(const float* pool, int pool_rows, int F, const int* table, int n, int T, float* out,
                    const float* gains_pool, float* gains_out, hipStream_t s) {
    static_assert(sizeof(VoiceRow) == 2 * sizeof(int), "VoiceRow is two 4-byte words");
    for (int r = 0; r < n; ++r) {
      const long off = table[2 * r], fr = table[2 * r + 1];
      const std::string at = " (row " + std::to_string(r) + ")";
      ZV_REQUIRE(off >= 0 && fr >= 1 && off + fr <= pool_rows, "voice table: range outside the pool" + at);
      ZV_REQUIRE(fr <= T, "voice table: more frames than T" + at);
    }
    stage.words.assign(table, table + 2L * n);
    const VoiceRow* d = reinterpret_cast<const VoiceRow*>(stage.upload(s));
    const bool quad = F % 4 == 0 && sess_aligned16(pool, out);
    const long per = (long)T * F;
    const dim3 grid = sched_grid(quad ? per / 4 : per, n);
    if (quad)
      hipLaunchKernelGGL(zv_voice_gather_kernel<true>, grid, dim3(VOICE_THREADS), 0, s, pool, d, T, F, out, gains_pool,
                         gains_out);
    else
      hipLaunchKernelGGL(zv_voice_gather_kernel<false>, grid, dim3(VOICE_THREADS), 0, s, pool, d, T, F, out, gains_pool,
                         gains_out);
    ZV_LAUNCH_CHECK();
    return {quad ? 1 : 0, (int)grid.x, VOICE_THREADS};
  }
};
