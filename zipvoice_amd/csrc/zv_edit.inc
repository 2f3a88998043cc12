// Speech editing for gfx950: the two assembly passes around the solve of an edit
// (zipvoice_amd/edit.py, ZipVoice.sample_edit).  No reference counterpart: the reference's
// sample_intermediate takes a ready speech condition and returns features; the behaviour is
// defined in include/zipvoice_hip.h and restated in numpy by tests/edit_ref.py.
//
// Both passes are driven by a host table of segments per row, (dst, src, len) in frames for the
// gather and (out, src, len, kind) in samples for the splice, rows delimited by row_ptr [B + 1].
// The host validates a table completely before anything is queued (tiling, bounds against every
// buffer the kernels index), so the kernels trust it; the checked table is written into a pinned
// slot and copied to the handle's device table on the caller's stream.
//   gather   one workgroup per EG_TILE frames of a row.  The first EG_TILE threads find their
//            frame's segment by bisection in the row's table, once per frame, and leave the
//            source frame in LDS (>= 0 a frame of feat, EG_GEN generated, EG_PAD at or past
//            T_b); then every thread moves 4 features of a frame per item with 16-byte loads and
//            stores (F % 4 == 0 and 16-byte aligned buffers), or one feature (any F).
//            B * T * F * 4 bytes written, as many read (none for a generated frame without
//            fill), B * T mask bytes.
//   splice   a thread owns 4 consecutive output samples of a row, in every channel.  Away from
//            the junctions they are one dword-aligned 16-byte load and store (original samples
//            bitwise, generated ones times the row's gain); inside the window of a junction the
//            two sources are mixed sample by sample (wj_mix, zv_wavjoin.inc).  The half-window
//            of every junction is worked out on the host with the table (es_half) and travels in
//            it.  C * out_cols * 4 bytes written per row, the row's length read once plus the
//            windows twice.
// No atomics; every output element is written exactly once, by one thread, so results are
// bitwise reproducible and do not depend on the launch geometry.
#pragma once

constexpr int EG_THREADS = 256;
constexpr int EG_TILE = 16;               // frames per workgroup of the gather pass
constexpr int EG_GEN = -1, EG_PAD = -2;   // LDS marks: generated frame, frame at or past T_b
constexpr int ES_TILE = EG_THREADS * 4;   // output samples per workgroup of the splice pass

// one segment of a sample table on the device: h is the half-window of the junction with the
// next segment of the row (0 after the last)
struct es_seg { int out, src, len, kind, h; };

// the last segment i in [lo, hi) whose first word (dst / out) is <= pos; needs hi > lo
__device__ __forceinline__ int edit_find(const int* tab, int stride, int lo, int hi, int pos) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab[(long)mid * stride] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

template <bool VEC>
__global__ __launch_bounds__(EG_THREADS) void zv_edit_gather_kernel(
    const float* feat, int Lmax, const float* fill, const int* row_ptr, const int* tab, int T,
    int F, float* out, uint8_t* mask) {
  __shared__ int s_src[EG_TILE];
  const int b = blockIdx.y, t0 = blockIdx.x * EG_TILE;
  if (threadIdx.x < EG_TILE) {
    const int t = t0 + threadIdx.x;
    int v = EG_PAD;
    const int lo = row_ptr[b], hi = row_ptr[b + 1];
    if (t < T && hi > lo) {
      const int* last = tab + 3L * (hi - 1);
      if (t < last[0] + last[2]) {                       // t < T_b
        const int* sg = tab + 3L * edit_find(tab, 3, lo, hi, t);
        v = sg[1] < 0 ? EG_GEN : sg[1] + (t - sg[0]);
      }
    }
    s_src[threadIdx.x] = v;
    if (mask && t < T) mask[(long)b * T + t] = v == EG_GEN;
  }
  __syncthreads();
  const int per = VEC ? F / 4 : F;                       // items per frame
  const int W = VEC ? 4 : 1;
  feat += (long)b * Lmax * F;
  const long row = (long)b * T * F;
  for (int i = threadIdx.x; i < EG_TILE * per; i += EG_THREADS) {
    const int fr = i / per, c = (i - fr * per) * W;
    const int t = t0 + fr;
    if (t >= T) break;                                   // fr rises with i
    const int v = s_src[fr];
    const long o = row + (long)t * F + c;
    const float* src = v >= 0 ? feat + (long)v * F + c : (v == EG_GEN && fill ? fill + o : nullptr);
    if (VEC) {
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (src) x = *reinterpret_cast<const f32x4*>(src);
      *reinterpret_cast<f32x4*>(out + o) = x;
    } else {
      out[o] = src ? *src : 0.f;
    }
  }
}

// one sample of the splice at output position q of a row whose segments are sg[lo, hi), q inside
// segment i: a junction's window mixes the left segment continued forward with the right one
// continued backward, each under its own gain
__device__ __forceinline__ float es_sample(const es_seg* sg, int lo, int hi, int i, int q,
                                           const float* orig, const float* gen, float g) {
  const es_seg s = sg[i];
  int l = -1;                                            // the junction is between l and l + 1
  if (i > lo && q < s.out + sg[i - 1].h) l = i - 1;
  else if (i + 1 < hi && q >= s.out + s.len - s.h) l = i;
  if (l < 0) {
    const long k = (long)s.src + (q - s.out);
    return s.kind ? (g != 1.f ? g * gen[k] : gen[k]) : orig[k];
  }
  const es_seg a = sg[l], r = sg[l + 1];
  const int h = a.h;
  const float xa = (a.kind ? gen : orig)[(long)a.src + (q - a.out)];
  const float xb = (r.kind ? gen : orig)[(long)r.src + (q - r.out)];
  const float w = ((float)(q - (r.out - h)) + 0.5f) / (float)(2 * h);
  return wj_mix(a.kind ? g : 1.f, xa, r.kind ? g : 1.f, xb, w);
}

__global__ __launch_bounds__(EG_THREADS) void zv_edit_splice_kernel(
    const float* orig, long ld, const float* gen, long ldg, const int* row_ptr, const es_seg* sg,
    const float* gains, int C, int tiles, float* out, long out_ld, long out_cols) {
  const int b = blockIdx.x / tiles;
  const long q0 = ((long)(blockIdx.x % tiles) * EG_THREADS + threadIdx.x) * 4;
  if (q0 >= out_cols) return;
  const int lo = row_ptr[b], hi = row_ptr[b + 1];
  const long n = hi > lo ? (long)sg[hi - 1].out + sg[hi - 1].len : 0;   // the row's length
  const float g = gains[b];
  orig += (long)b * C * ld;
  gen += (long)b * C * ldg;
  out += (long)b * C * out_ld;
  const bool full = q0 + 4 <= out_cols;
  if (q0 >= n) {                                         // zero past the row's length
    for (int c = 0; c < C; ++c) {
      float* o = out + c * out_ld + q0;
      if (full) *reinterpret_cast<wj_f32x4*>(o) = wj_f32x4{0.f, 0.f, 0.f, 0.f};
      else for (long k = 0; q0 + k < out_cols; ++k) o[k] = 0.f;
    }
    return;
  }
  int i = edit_find(&sg[0].out, (int)(sizeof(es_seg) / sizeof(int)), lo, hi, (int)q0);
  {
    const es_seg s = sg[i];
    const int hl = i > lo ? sg[i - 1].h : 0, hr = i + 1 < hi ? s.h : 0;
    if (full && q0 >= s.out + hl && q0 + 4 <= (long)s.out + s.len - hr) {   // 4 plain samples
      const long k = (long)s.src + (q0 - s.out);
      for (int c = 0; c < C; ++c) {
        wj_f32x4 v = *reinterpret_cast<const wj_f32x4*>((s.kind ? gen + c * ldg : orig + c * ld) + k);
        if (s.kind && g != 1.f) v *= g;
        *reinterpret_cast<wj_f32x4*>(out + c * out_ld + q0) = v;
      }
      return;
    }
  }
  for (int k = 0; k < 4 && q0 + k < out_cols; ++k) {
    const long q = q0 + k;
    if (q < n)
      while (i + 1 < hi && q >= sg[i + 1].out) ++i;
    for (int c = 0; c < C; ++c)
      out[c * out_ld + q] = q < n ? es_sample(sg, lo, hi, i, (int)q, orig + c * ld, gen + c * ldg, g) : 0.f;
  }
}

// The half-window of the junction between consecutive segments a and b of a row: the fade, the
// len / 2 clamps that keep neighbouring windows apart, and the two reads past a segment's own
// samples kept inside their buffers (lim: the valid samples of a segment's source)
static inline long es_half(long fade, long a_src, long a_len, long a_lim, long b_src, long b_len) {
  long h = std::min(fade, std::min(a_len / 2, b_len / 2));
  h = std::min(h, a_lim - (a_src + a_len));              // a continued forward h samples
  h = std::min(h, b_src);                                // b continued backward h samples
  return std::max(h, 0L);
}

struct zv_edit {
  // Staging as the scheduled solve's (zv_engine.hip SchedSlot): a pinned slot per upload in
  // flight, taken again only when the one-thread kernel queued behind its copy has written the
  // upload's sequence number into the slot's host-mapped word.  A call that finds no idle slot
  // allocates one, so back-to-back calls never overwrite a table the GPU has yet to read.
  struct Slot {
    unsigned* base = nullptr;   // pinned + mapped: word 0 the completion mark, the table from byte 64
    unsigned* mark_dev = nullptr;
    size_t cap = 0;
    unsigned issued = 0;
    bool idle() const { return *reinterpret_cast<volatile unsigned*>(base) == issued; }
  };
  std::vector<Slot> slots;
  char* tab = nullptr;          // the device copy of the last call's table
  size_t tab_bytes = 0;
  std::vector<int> words;       // the table being assembled

  ~zv_edit() {
    if (!slots.empty()) (void)ZV_BLOCKING(hipDeviceSynchronize());
    for (Slot& sl : slots) (void)ZV_BLOCKING(hipHostFree(sl.base));
    if (tab) (void)ZV_BLOCKING(hipFree(tab));
  }
  size_t device_bytes() const { return tab_bytes; }

  Slot& slot(size_t bytes) {
    for (Slot& sl : slots)
      if (sl.cap >= bytes && sl.idle()) return sl;
    Slot sl;
    sl.cap = (size_t)round_up((long)std::max<size_t>(bytes, 16 * 1024), 4096);
    ZV_CHECK(ZV_BLOCKING(hipHostMalloc((void**)&sl.base, sl.cap + 64, hipHostMallocMapped | hipHostMallocPortable)));
    sl.base[0] = 0;
    ZV_CHECK(ZV_BLOCKING(hipHostGetDevicePointer((void**)&sl.mark_dev, (void*)sl.base, 0)));
    slots.push_back(sl);
    return slots.back();
  }
  // `words` to the device table, ordered on s behind the kernels of earlier calls that read it
  const int* upload(hipStream_t s) {
    const size_t bytes = words.size() * sizeof(int);
    if (bytes > tab_bytes) {
      if (tab) {
        ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
        ZV_CHECK(ZV_BLOCKING(hipFree(tab)));
        tab = nullptr; tab_bytes = 0;
      }
      const size_t need = (size_t)round_up((long)std::max<size_t>(bytes, 16 * 1024), 4096);
      ZV_CHECK(ZV_BLOCKING(hipMalloc((void**)&tab, need)));
      tab_bytes = need;
    }
    Slot& sl = slot(bytes);
    memcpy(sl.base + 16, words.data(), bytes);
    ZV_CHECK(hipMemcpyAsync(tab, sl.base + 16, bytes, hipMemcpyHostToDevice, s));
    sl.issued += 1;
    hipLaunchKernelGGL(zv_mark_kernel, dim3(1), dim3(1), 0, s, sl.mark_dev, sl.issued);
    ZV_LAUNCH_CHECK();
    return reinterpret_cast<const int*>(tab);
  }

  // row_ptr rises from 0; returns the number of segments
  static int check_row_ptr(const int* row_ptr, int B) {
    ZV_REQUIRE(row_ptr[0] == 0, "edit table: row_ptr[0] must be 0");
    for (int b = 0; b < B; ++b)
      ZV_REQUIRE(row_ptr[b + 1] >= row_ptr[b], "edit table: row_ptr must not fall (row " + std::to_string(b) + ")");
    return row_ptr[B];
  }

  void gather(const float* feat, int B, int Lmax, int F, const int* lens, const float* fill,
              const int* table, const int* row_ptr, int T, float* out, uint8_t* mask, hipStream_t s) {
    const int nseg = check_row_ptr(row_ptr, B);
    for (int b = 0; b < B; ++b) {
      const std::string at = " (row " + std::to_string(b) + ")";
      ZV_REQUIRE(lens[b] >= 0 && lens[b] <= Lmax, "edit table: lens must be in [0, Lmax]" + at);
      long pos = 0;
      for (int i = row_ptr[b]; i < row_ptr[b + 1]; ++i) {
        const long dst = table[3 * i], src = table[3 * i + 1], len = table[3 * i + 2];
        ZV_REQUIRE(len > 0, "edit table: segment lengths must be positive" + at);
        ZV_REQUIRE(dst == pos, "edit table: segments must tile [0, T_b) in order" + at);
        ZV_REQUIRE(src == -1 || (src >= 0 && src + len <= lens[b]),
                   "edit table: kept segment outside [0, L_b)" + at);
        pos += len;
        ZV_REQUIRE(pos <= T, "edit table: row longer than T" + at);
      }
    }
    words.assign(row_ptr, row_ptr + B + 1);
    words.insert(words.end(), table, table + 3L * nseg);
    const int* d = upload(s);
    const bool vec = F % 4 == 0 && (((uintptr_t)feat | (uintptr_t)fill | (uintptr_t)out) & 15) == 0;
    const dim3 grid((unsigned)cdiv(T, EG_TILE), (unsigned)B), blk(EG_THREADS);
    if (vec)
      hipLaunchKernelGGL(zv_edit_gather_kernel<true>, grid, blk, 0, s, feat, Lmax, fill, d, d + B + 1, T, F, out, mask);
    else
      hipLaunchKernelGGL(zv_edit_gather_kernel<false>, grid, blk, 0, s, feat, Lmax, fill, d, d + B + 1, T, F, out, mask);
    ZV_LAUNCH_CHECK();
  }

  void splice(const float* orig, long ld, const int* lens, const float* gen, long ldg, const int* gen_lens,
              int B, int C, const int* table, const int* row_ptr, const float* gains, int fade, float* out,
              long out_ld, long out_cols, hipStream_t s) {
    const int nseg = check_row_ptr(row_ptr, B);
    static_assert(sizeof(es_seg) == 20 && sizeof(float) == sizeof(int), "es_seg is five 4-byte words");
    // row_ptr [B + 1] | gains [B] | segments [nseg]
    words.assign(row_ptr, row_ptr + B + 1);
    words.resize((size_t)2 * B + 1 + 5L * nseg);
    memcpy(words.data() + B + 1, gains, (size_t)B * sizeof(float));
    es_seg* sg = reinterpret_cast<es_seg*>(words.data() + 2 * B + 1);
    for (int b = 0; b < B; ++b) {
      const std::string at = " (row " + std::to_string(b) + ")";
      ZV_REQUIRE(lens[b] >= 0 && lens[b] <= ld, "edit table: lens must be in [0, ld]" + at);
      ZV_REQUIRE(gen_lens[b] >= 0 && gen_lens[b] <= ldg, "edit table: gen_lens must be in [0, ldg]" + at);
      long pos = 0;
      for (int i = row_ptr[b]; i < row_ptr[b + 1]; ++i) {
        const long o = table[4 * i], src = table[4 * i + 1], len = table[4 * i + 2], kind = table[4 * i + 3];
        ZV_REQUIRE(len > 0, "edit table: segment lengths must be positive" + at);
        ZV_REQUIRE(o == pos, "edit table: segments must tile [0, N_b) in order" + at);
        ZV_REQUIRE(kind == 0 || kind == 1, "edit table: kind must be 0 (original) or 1 (generated)" + at);
        ZV_REQUIRE(src >= 0 && src + len <= (kind ? gen_lens[b] : lens[b]),
                   "edit table: segment outside its source" + at);
        pos += len;
        ZV_REQUIRE(pos <= out_cols, "edit table: row longer than out_cols" + at);
        sg[i] = es_seg{(int)o, (int)src, (int)len, (int)kind, 0};
      }
      for (int i = row_ptr[b]; i + 1 < row_ptr[b + 1]; ++i)
        sg[i].h = (int)es_half(fade, sg[i].src, sg[i].len, sg[i].kind ? gen_lens[b] : lens[b], sg[i + 1].src,
                               sg[i + 1].len);
    }
    const long tiles = (out_cols + ES_TILE - 1) / ES_TILE;
    ZV_REQUIRE(B * tiles <= 0x7fffffffL, "batch too large for one launch");
    const int* d = upload(s);
    hipLaunchKernelGGL(zv_edit_splice_kernel, dim3((unsigned)(B * tiles)), dim3(EG_THREADS), 0, s, orig, ld, gen,
                       ldg, d, reinterpret_cast<const es_seg*>(d + 2 * B + 1),
                       reinterpret_cast<const float*>(d + B + 1), C, (int)tiles, out, out_ld, out_cols);
    ZV_LAUNCH_CHECK();
  }
};
