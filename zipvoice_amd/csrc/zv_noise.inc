// Seeded initial noise for gfx950: standard normals that are a pure function of
// (seed, stream, element index), so a request's noise does not depend on the batch it was drawn in.
//
// No reference counterpart beyond --seed (zipvoice/bin/infer_zipvoice.py:240, fix_random_seed): the
// reference speaks one sentence per call and draws torch.randn(batch, frames, feat)
// (zipvoice/models/zipvoice.py:453-458).  The definition is this project's own and is written out in
// include/zipvoice_hip.h (tests/noise_ref.py restates it in numpy): element e of row b is lane e % 4
// of the Box-Muller pair outputs of Philox4x32-10 at counter (e / 4, stream_b, 0), key seed_b.
//
// philox4x32_10 and noise_box_muller are __host__ __device__ plain C++: the fill kernel, the one-off
// device kernels of zv_noise_check and its host mode run the same source.  The uint32 words are
// bit-exact everywhere; the normals are bitwise reproducible on the device (no atomics, nothing
// depends on the launch geometry, the stride, the alignment or the operand format of the build) and
// agree with a float64 evaluation within 16 * 2^-24 * (1 + r).
//
// zv_noise_normal_kernel: one thread owns whole Philox blocks (four consecutive outputs of one row),
// grid-stride over the row's blocks in x, the row in y, 64-bit indices.  The four values go out as
// one 16-byte store where the row's base is 16-byte aligned and the block lies inside the row; the
// row's tail (n % 4) and every block of a row whose base is not aligned go out one dword at a time,
// each under its own bound.  Write-bound: 16 bytes per about 150 integer and float operations.
//
// Included by zv_engine.hip after zv_checks.inc (ChkDev, the ZV_API_* helpers).
#pragma once

struct NoiseWords { uint32_t v[4]; };

__host__ __device__ static inline uint32_t noise_mulhi(uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Philox4x32 with ten rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11;
// the Random123 constants)
__host__ __device__ static inline NoiseWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                           uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = noise_mulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = noise_mulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return NoiseWords{{c0, c1, c2, c3}};
}

// u(x) = fl32(fl32(x) * 2^-32 + 2^-33), in (0, 1]: the product is exact, so a fused multiply-add
// rounds to the same value
__host__ __device__ static inline float noise_unit(uint32_t x) { return (float)x * 0x1p-32f + 0x1p-33f; }

// Two normals of one word pair: r(u(xa)) * (sin, cos)(2 pi u(xb)), r(u) = sqrt(-2 ln u); u = 1 gives
// a radius of 0.  On the device the angle goes through sincospi of 2 u (an exact argument, no
// reduction of 2 pi u); the host mode evaluates the same expression in double.
__host__ __device__ static inline void noise_box_muller(uint32_t xa, uint32_t xb, float* zs, float* zc) {
  const float ua = noise_unit(xa), ub = noise_unit(xb);
#ifdef __HIP_DEVICE_COMPILE__
  const float r = sqrtf(-2.0f * logf(ua));
  float s, c;
  sincospif(2.0f * ub, &s, &c);
  *zs = r * s;
  *zc = r * c;
#else
  const double r = sqrt(-2.0 * log((double)ua)), a = 6.283185307179586476925 * (double)ub;
  *zs = (float)(r * sin(a));
  *zc = (float)(r * cos(a));
#endif
}

// the four normals of one Philox block
__host__ __device__ static inline void noise_block(uint64_t seed, uint32_t stream, uint64_t j, float (&z)[4]) {
  const NoiseWords w = philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), stream, 0u, (uint32_t)seed,
                                     (uint32_t)(seed >> 32));
  noise_box_muller(w.v[0], w.v[1], &z[0], &z[1]);
  noise_box_muller(w.v[2], w.v[3], &z[2], &z[3]);
}

constexpr int NOISE_THREADS = 256;
constexpr long NOISE_MAX_GRID_X = 2048;   // blocks over one row; the rest of the row is grid-stride

__global__ __launch_bounds__(NOISE_THREADS) void zv_noise_normal_kernel(
    const int64_t* seeds, const int32_t* streams, long n, long ld, float* out) {
  const int b = blockIdx.y;
  const uint64_t seed = (uint64_t)seeds[b];
  const uint32_t stream = streams ? (uint32_t)streams[b] : 0u;
  float* row = out + (long)b * ld;
  const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const long nblk = (n + 3) / 4, step = (long)gridDim.x * NOISE_THREADS;
  for (long j = (long)blockIdx.x * NOISE_THREADS + threadIdx.x; j < nblk; j += step) {
    float z[4];
    noise_block(seed, stream, (uint64_t)j, z);
    const long e = 4 * j;
    if (aligned && e + 4 <= n) {
      store4(row + e, z);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (e + i < n) row[e + i] = z[i];
    }
  }
}

// out[b * ld + e] = normal(seeds[b], streams[b], e) for e < n; nothing else is written.  No
// allocation, no host-blocking call (graph-capturable).
static void launch_noise_normal(const int64_t* seeds, const int32_t* streams, int B, long n, long ld, float* out,
                                hipStream_t s) {
  const long nblk = (n + 3) / 4;
  const long gx = std::min((nblk + NOISE_THREADS - 1) / NOISE_THREADS, NOISE_MAX_GRID_X);
  hipLaunchKernelGGL(zv_noise_normal_kernel, dim3((unsigned)gx, (unsigned)B), dim3(NOISE_THREADS), 0, s, seeds,
                     streams, n, ld, out);
  ZV_LAUNCH_CHECK();
}

// zv_noise_check on the device: the same two functions, one thread per block / word quadruple
static __global__ void zv_noise_bits_kernel(NoiseWords ctr, uint32_t k0, uint32_t k1, long nblocks, uint32_t* out) {
  const uint64_t lo = (uint64_t)ctr.v[0] | ((uint64_t)ctr.v[1] << 32);
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < nblocks; j += (long)gridDim.x * blockDim.x) {
    const uint64_t c = lo + (uint64_t)j;
    const NoiseWords w = philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), ctr.v[2], ctr.v[3], k0, k1);
    for (int i = 0; i < 4; ++i) out[4 * j + i] = w.v[i];
  }
}
static __global__ void zv_noise_box_muller_kernel(const uint32_t* words, long m, float* out) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < m; j += (long)gridDim.x * blockDim.x) {
    noise_box_muller(words[4 * j], words[4 * j + 1], &out[4 * j], &out[4 * j + 1]);
    noise_box_muller(words[4 * j + 2], words[4 * j + 3], &out[4 * j + 2], &out[4 * j + 3]);
  }
}

extern "C" {

int zv_noise_normal(const int64_t* seeds, const int32_t* streams, int B, int64_t n, int64_t ld, float* out,
                    void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(B > 0 && B <= 65535, "zv_noise_normal: B must be in [1, 65535]");
  ZV_REQUIRE(n >= 0 && n <= (1LL << 40), "zv_noise_normal: n must be in [0, 2^40]");
  ZV_REQUIRE(ld >= n, "zv_noise_normal: ld < n");
  if (n == 0) return 0;
  ZV_REQUIRE(seeds && out, "zv_noise_normal: null seeds / out");
  launch_noise_normal(seeds, streams, B, (long)n, (long)ld, out, (hipStream_t)stream);
  ZV_API_END
}

int zv_noise_check(zv_noise_check_args* a) {
  ZV_API_BEGIN
  ZV_REQUIRE(a && (a->mode == ZV_NOISE_BITS || a->mode == ZV_NOISE_NORMALS) && (a->where == 0 || a->where == 1),
             "zv_noise_check: bad arguments");
  ZV_REQUIRE(a->count >= 0 && a->count <= (1LL << 26), "zv_noise_check: count must be in [0, 2^26]");
  const long m = (long)a->count;
  const bool bits = a->mode == ZV_NOISE_BITS;
  ZV_REQUIRE(m == 0 || (bits ? a->bits != nullptr : a->words && a->normals),
             "zv_noise_check: BITS needs bits, NORMALS needs words and normals");
  if (m == 0) return 0;
  if (a->where == 0) {
    const uint64_t lo = (uint64_t)a->counter[0] | ((uint64_t)a->counter[1] << 32);
    for (long j = 0; j < m; ++j) {
      if (bits) {
        const uint64_t c = lo + (uint64_t)j;
        const NoiseWords w = philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), a->counter[2], a->counter[3],
                                           a->key[0], a->key[1]);
        memcpy(a->bits + 4 * j, w.v, sizeof(w.v));
      } else {
        noise_box_muller(a->words[4 * j], a->words[4 * j + 1], &a->normals[4 * j], &a->normals[4 * j + 1]);
        noise_box_muller(a->words[4 * j + 2], a->words[4 * j + 3], &a->normals[4 * j + 2], &a->normals[4 * j + 3]);
      }
    }
    return 0;
  }
  ChkDev dev;
  hipStream_t s = nullptr;
  const dim3 grid = grid1d(m);
  if (bits) {
    uint32_t* o = dev.zero<uint32_t>((size_t)4 * m);
    const NoiseWords ctr{{a->counter[0], a->counter[1], a->counter[2], a->counter[3]}};
    hipLaunchKernelGGL(zv_noise_bits_kernel, grid, dim3(256), 0, s, ctr, a->key[0], a->key[1], m, o);
    ZV_LAUNCH_CHECK();
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    dev.down(a->bits, o, (size_t)4 * m);
  } else {
    const uint32_t* w = dev.up(a->words, (size_t)4 * m);
    float* o = dev.zero<float>((size_t)4 * m);
    hipLaunchKernelGGL(zv_noise_box_muller_kernel, grid, dim3(256), 0, s, w, m, o);
    ZV_LAUNCH_CHECK();
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    dev.down(a->normals, o, (size_t)4 * m);
  }
  ZV_API_END
}

}  // extern "C"
