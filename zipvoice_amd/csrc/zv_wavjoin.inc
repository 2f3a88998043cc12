// Long-form join for gfx950: trim the pauses of a batch of chunk waveforms and glue the
// trimmed chunks of every document (a run of consecutive chunks, doc_ptr) into that
// document's waveform with linear cross-fades (zipvoice_amd/longform.py WavJoiner).  No
// reference counterpart: the reference has no long-form path; the behaviour is defined in
// include/zipvoice_hip.h and restated in float64 by tests/wavjoin_ref.py.
//
// Four passes over wav [B, C, wav_ld], all memory-bound, no atomics, every result
// independent of the launch geometry (12 B per input sample: 4 read by the energy pass,
// 4 read + at most 4 written by the gather pass):
//   energy   one wavefront per frame: lane l adds x[l]^2, x[l + 64]^2, ... (channel 0, then
//            channel 1) into one fp32 accumulator, then a 6-step xor butterfly; the frame is
//            loud unless e < thr^2 * samples.  flags [B, nfmax] (bit 0).
//   plan     one workgroup per chunk: first / last loud frame, per quiet frame the loud
//            frames that bound its run, the keep decision (flags bit 1) and the exclusive
//            prefix sum of the kept frames' sample counts, pre [B, nfmax + 1]
//            (pre[b, nf] = m_b).  Every thread owns a contiguous segment of frames; the
//            segments' summaries meet in LDS.
//   offsets  one workgroup per document, over its chunks only, so the chain of non-empty
//            chunks never crosses a document boundary: F_b, off_b (in the document's row),
//            the previous non-empty chunk and the overlap with the next one, the chunk's
//            document; out_len[d] and spans.
//   gather   a thread owns 4 consecutive input samples; kept samples go to column
//            off_b + pre[b, f] + (s - f * frame) of the chunk's document row.  Owner rule
//            for an overlap: the chunk that fades in writes it (and finds the fading-out
//            sample of the previous chunk by a binary search in that chunk's pre); a chunk
//            skips the samples of its own tail that the next chunk owns.  Outside overlaps
//            4 samples of one frame move as one dwordx4 load and store (dword-aligned: row
//            starts and destinations are arbitrary), and a gain of exactly 1 copies the bits.
//   zero     columns [N_d, out_cap) of every document row.
// doc_ptr is read on the device only, so its contents cannot be rejected: every bound is
// clamped into [0, B] with hi >= lo, and the gather pass moves a chunk only if the document
// recorded for it is below D and owns it by those bounds, so no store leaves columns
// [0, out_cap) of a row < D or the scratch, whatever the array holds.
#pragma once

constexpr int WJ_THREADS = 256;
constexpr int WJ_TILE = WJ_THREADS * 4;   // input samples per workgroup of the gather pass
constexpr int WJ_OFF_BLOCK = 1024;        // chunks staged in LDS per round of the offsets pass
typedef float wj_f32x4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ long wj_len(const int* lens, int b, long wav_ld) {
  return min(max((long)lens[b], 0L), wav_ld);
}

// chunks [lo, hi) of document d; doc_ptr == nullptr: one document of all B chunks
__device__ __forceinline__ void wj_doc_range(const int* doc_ptr, int d, int B, int& lo, int& hi) {
  lo = 0; hi = B;
  if (doc_ptr) {
    lo = min(max(doc_ptr[d], 0), B);
    hi = min(max(doc_ptr[d + 1], lo), B);
  }
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_energy_kernel(
    const float* wav, long wav_ld, const int* lens, int C, int frame, float thr2, int nfmax,
    int tiles, uint8_t* flags) {
  const int b = blockIdx.x / tiles;
  const long f = (long)(blockIdx.x % tiles) * (WJ_THREADS / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const long len = wj_len(lens, b, wav_ld);
  const long s0 = f * frame;
  if (f >= nfmax || s0 >= len) return;                   // wave-uniform
  const int cnt = (int)min((long)frame, len - s0);
  float e = 0.f;
  for (int c = 0; c < C; ++c) {
    const float* x = wav + ((long)b * C + c) * wav_ld + s0;
#pragma unroll 4
    for (int i = lane; i < cnt; i += 64) e = fmaf(x[i], x[i], e);
  }
  for (int o = 32; o; o >>= 1) e += __shfl_xor(e, o);
  if (lane == 0) flags[(long)b * nfmax + f] = !(e < thr2 * (float)((long)cnt * C));
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_plan_kernel(
    const int* lens, long wav_ld, int frame, int keep_edge, int max_gap, int nfmax,
    uint8_t* flags, int* pre, int* m) {
  __shared__ int s_first[WJ_THREADS], s_last[WJ_THREADS], s_cnt[WJ_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const long len = wj_len(lens, b, wav_ld);
  const long nf = (len + frame - 1) / frame;             // <= nfmax
  uint8_t* fl = flags + (long)b * nfmax;
  int* pr = pre + (long)b * (nfmax + 1);
  const long seg = (nf + WJ_THREADS - 1) / WJ_THREADS;
  const long lo = min(t * seg, nf), hi = min(lo + seg, nf);
  int fi = INT_MAX, la = -1;
  for (long f = lo; f < hi; ++f)
    if (fl[f]) { if (fi == INT_MAX) fi = (int)f; la = (int)f; }
  s_first[t] = fi; s_last[t] = la;
  __syncthreads();
  // first / last loud frame of the chunk; the last loud frame before this thread's segment
  // and the first one after it
  int first = INT_MAX, last = -1, prev = -1, nxt_out = INT_MAX;
  for (int i = 0; i < WJ_THREADS; ++i) {
    const int a = s_first[i], z = s_last[i];
    first = min(first, a); last = max(last, z);
    if (i < t) prev = max(prev, z);
    if (i > t) nxt_out = min(nxt_out, a);
  }
  if (last < 0) {                                        // no loud frame: the chunk is empty
    if (t == 0) m[b] = 0;
    return;
  }
  const long klo = max(0L, (long)first - keep_edge), khi = min(nf - 1, (long)last + keep_edge);
  const int head = max_gap / 2 + (max_gap & 1), tail = max_gap / 2;
  int cnt = 0;
  long nxt = -1;                                         // the first loud frame at or after f
  for (long f = lo; f < hi; ++f) {
    const bool loud = fl[f] & 1;
    bool keep;
    if (f < klo || f > khi) keep = false;
    else if (loud || f < first || f > last) keep = true;
    else {                                               // quiet, strictly between first and last
      if (nxt < f) {
        nxt = f + 1;
        while (nxt < hi && !(fl[nxt] & 1)) ++nxt;
        if (nxt >= hi) nxt = nxt_out;
      }
      const long run = nxt - prev - 1;
      keep = run <= max_gap || f - prev - 1 < head || nxt - f - 1 < tail;
    }
    if (loud) prev = (int)f;
    if (keep) cnt += (int)min((long)frame, len - f * frame);
    fl[f] = (uint8_t)(loud | (keep << 1));
  }
  s_cnt[t] = cnt;
  __syncthreads();
  int base = 0, total = 0;
  for (int i = 0; i < WJ_THREADS; ++i) {
    const int c = s_cnt[i];
    if (i < t) base += c;
    total += c;
  }
  for (long f = lo; f < hi; ++f) {
    pr[f] = base;
    if (fl[f] & 2) base += (int)min((long)frame, len - f * frame);
  }
  if (t == 0) { pr[nf] = total; m[b] = total; }
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_offsets_kernel(
    const int* m, int B, const int* doc_ptr, int fade, long* off, int* F, int* Fn, int* prevc,
    int* doc, long* out_len, int* spans) {
  __shared__ long s_off[WJ_OFF_BLOCK];
  __shared__ int s_m[WJ_OFF_BLOCK], s_F[WJ_OFF_BLOCK], s_prev[WJ_OFF_BLOCK];
  const int d = blockIdx.x, t = threadIdx.x;
  int lo, hi;
  wj_doc_range(doc_ptr, d, B, lo, hi);
  int p = -1, mp = 0;                                    // thread 0: the last non-empty chunk
  long offp = 0;
  for (int b0 = lo; b0 < hi; b0 += WJ_OFF_BLOCK) {
    const int nb = min(WJ_OFF_BLOCK, hi - b0);
    for (int i = t; i < nb; i += WJ_THREADS) s_m[i] = m[b0 + i];
    __syncthreads();
    if (t == 0)
      for (int i = 0; i < nb; ++i) {
        const int mb = s_m[i];
        Fn[b0 + i] = 0;
        if (mb == 0) { s_off[i] = -1; s_F[i] = 0; s_prev[i] = -1; continue; }
        const int f = p < 0 ? 0 : min(fade, min(mp / 2, mb / 2));
        const long o = p < 0 ? 0 : offp + mp - f;
        s_off[i] = o; s_F[i] = f; s_prev[i] = p;
        if (p >= 0) Fn[p] = f;
        p = b0 + i; mp = mb; offp = o;
      }
    __syncthreads();
    for (int i = t; i < nb; i += WJ_THREADS) {
      off[b0 + i] = s_off[i]; F[b0 + i] = s_F[i]; prevc[b0 + i] = s_prev[i]; doc[b0 + i] = d;
      if (spans) {
        int* sp = spans + 3L * (b0 + i);
        sp[0] = s_m[i]; sp[1] = (int)s_off[i]; sp[2] = s_F[i];
      }
    }
    __syncthreads();
  }
  if (t == 0) out_len[d] = p < 0 ? 0 : offp + mp;
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_gather_kernel(
    const float* wav, long wav_ld, const int* lens, const float* gains, int C, int frame,
    int nfmax, int tiles, const int* pre, const int* m, const long* off, const int* F,
    const int* Fn, const int* prevc, const int* doc, const int* doc_ptr, int B, int D,
    float* out, long out_ld, long out_cap) {
  const int b = blockIdx.x / tiles;
  const int mb = m[b], d = doc[b];                       // d is stale if no document owns b
  if (mb == 0 || (unsigned)d >= (unsigned)D) return;
  int lo, hi;
  wj_doc_range(doc_ptr, d, B, lo, hi);
  if (b < lo || b >= hi) return;
  out += (long)d * C * out_ld;
  const long len = wj_len(lens, b, wav_ld);
  const long s0 = ((long)(blockIdx.x % tiles) * WJ_THREADS + threadIdx.x) * 4;
  if (s0 >= len) return;
  const int* pr = pre + (long)b * (nfmax + 1);
  const long ob = off[b];
  const int Fb = F[b], tail0 = mb - Fn[b];               // [tail0, mb) belongs to the next chunk
  const float g = gains ? gains[b] : 1.f;
  const float* xb = wav + (long)b * C * wav_ld;
  {
    const long f = s0 / frame;
    const int r = (int)(s0 - f * frame);
    if (s0 + 3 < len && r + 3 < frame) {                 // 4 samples of one frame
      const int t0 = pr[f];
      if (pr[f + 1] == t0) return;                       // the frame is dropped
      const int t = t0 + r;
      if (t >= Fb && t + 3 < tail0 && ob + t + 3 < out_cap) {
        for (int c = 0; c < C; ++c) {
          wj_f32x4 v = *reinterpret_cast<const wj_f32x4*>(xb + c * wav_ld + s0);
          if (g != 1.f) v *= g;
          *reinterpret_cast<wj_f32x4*>(out + c * out_ld + ob + t) = v;
        }
        return;
      }
    }
  }
  for (int k = 0; k < 4; ++k) {
    const long s = s0 + k;
    if (s >= len) break;
    const long f = s / frame;
    const int t0 = pr[f];
    if (pr[f + 1] == t0) continue;
    const int t = t0 + (int)(s - f * frame);
    const long dst = ob + t;
    if (t >= tail0 || dst >= out_cap) continue;
    if (t >= Fb) {
      for (int c = 0; c < C; ++c) {
        const float x = xb[c * wav_ld + s];
        out[c * out_ld + dst] = g != 1.f ? g * x : x;
      }
      continue;
    }
    // fade-in of this chunk over the fade-out of the previous non-empty chunk p:
    // its trimmed sample tp lies in the last frame fp with pre[p, fp] <= tp
    const int p = prevc[b];
    if (p < 0 || Fb > m[p]) continue;                    // only with overlapping documents
    const int tp = m[p] - Fb + t;
    const int* prp = pre + (long)p * (nfmax + 1);
    long flo = 0, fhi = (wj_len(lens, p, wav_ld) + frame - 1) / frame;
    while (fhi - flo > 1) {
      const long mid = (flo + fhi) >> 1;
      if (prp[mid] <= tp) flo = mid; else fhi = mid;
    }
    const long sp = flo * frame + (tp - prp[flo]);
    const float gp = gains ? gains[p] : 1.f;
    const float w = (float)(t + 1) / (float)(Fb + 1);
    const float* xp = wav + (long)p * C * wav_ld;
    for (int c = 0; c < C; ++c)
      out[c * out_ld + dst] = gp * xp[c * wav_ld + sp] * (1.f - w) + g * xb[c * wav_ld + s] * w;
  }
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_zero_kernel(
    const long* out_len, int C, int tiles, float* out, long out_ld, long out_cap) {
  const int d = blockIdx.x / tiles;
  const long N = out_len[d];
  const long i0 = ((long)(blockIdx.x % tiles) * WJ_THREADS + threadIdx.x) * 4;
  if (i0 + 4 <= N || i0 >= out_cap) return;
  out += (long)d * C * out_ld;
  for (int c = 0; c < C; ++c) {
    float* o = out + c * out_ld;
    if (i0 >= N && i0 + 4 <= out_cap) {
      *reinterpret_cast<wj_f32x4*>(o + i0) = wj_f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      for (long i = max(i0, N); i < min(i0 + 4, out_cap); ++i) o[i] = 0.f;
    }
  }
}

struct zv_wavjoin {
  int frame = 0, keep_edge = 0, max_gap = 0, fade = 0;
  float thr = 0.f;
  char* buf = nullptr;                     // scratch: offsets, plan, prefix sums, flags
  size_t bytes = 0;
  ~zv_wavjoin() {
    if (buf) (void)ZV_BLOCKING(hipFree(buf));
  }
  void init(int frame_, float thr_, int keep_edge_, int max_gap_, int fade_) {
    ZV_REQUIRE(frame_ >= 1, "frame must be at least 1");
    ZV_REQUIRE(thr_ >= 0.f, "thr must be non-negative");   // rejects NaN too
    ZV_REQUIRE(keep_edge_ >= 0, "keep_edge must be non-negative");
    ZV_REQUIRE(max_gap_ >= 0, "max_gap must be non-negative");
    ZV_REQUIRE(fade_ >= 0, "fade must be non-negative");
    frame = frame_; thr = thr_; keep_edge = keep_edge_; max_gap = max_gap_; fade = fade_;
  }
  void apply(const float* wav, long wav_ld, const int* lens, const float* gains, int B, int C,
             const int* doc_ptr, int D, float* out, long out_ld, long out_cap, long* out_len,
             int* spans, hipStream_t s) {
    const long nfmax = std::max(1L, (wav_ld + frame - 1) / frame);
    const long etiles = (nfmax + WJ_THREADS / 64 - 1) / (WJ_THREADS / 64);
    const long gtiles = std::max(1L, (wav_ld + WJ_TILE - 1) / WJ_TILE);
    const long ztiles = (out_cap + WJ_TILE - 1) / WJ_TILE;
    ZV_REQUIRE(nfmax < 0x7fffffffL && B * etiles <= 0x7fffffffL && B * gtiles <= 0x7fffffffL &&
                   ztiles <= 0x7fffffffL && D * ztiles <= 0x7fffffffL,
               "batch too large for one launch");
    // off [B] int64 | m, F, Fn, prev, doc [B] int32 | pre [B, nfmax + 1] int32 | flags [B, nfmax]
    const size_t nB = (size_t)std::max(B, 1);
    const size_t need = nB * 8 + 5 * nB * 4 + nB * (size_t)(nfmax + 1) * 4 + nB * (size_t)nfmax;
    if (need > bytes) {
      if (buf) {
        ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
        ZV_CHECK(ZV_BLOCKING(hipFree(buf)));
        buf = nullptr; bytes = 0;
      }
      ZV_CHECK(ZV_BLOCKING(hipMalloc(&buf, need)));
      bytes = need;
    }
    long* off = reinterpret_cast<long*>(buf);
    int* m = reinterpret_cast<int*>(off + nB);
    int *F = m + nB, *Fn = F + nB, *prevc = Fn + nB, *doc = prevc + nB, *pre = doc + nB;
    uint8_t* flags = reinterpret_cast<uint8_t*>(pre + nB * (size_t)(nfmax + 1));
    const dim3 blk(WJ_THREADS);
    if (B > 0) {
      hipLaunchKernelGGL(zv_wavjoin_energy_kernel, dim3((unsigned)(B * etiles)), blk, 0, s, wav,
                         wav_ld, lens, C, frame, thr * thr, (int)nfmax, (int)etiles, flags);
      ZV_LAUNCH_CHECK();
      hipLaunchKernelGGL(zv_wavjoin_plan_kernel, dim3(B), blk, 0, s, lens, wav_ld, frame,
                         keep_edge, max_gap, (int)nfmax, flags, pre, m);
      ZV_LAUNCH_CHECK();
    }
    if (D > 0) {
      hipLaunchKernelGGL(zv_wavjoin_offsets_kernel, dim3(D), blk, 0, s, m, B, doc_ptr, fade, off,
                         F, Fn, prevc, doc, out_len, spans);
      ZV_LAUNCH_CHECK();
    }
    if (B > 0 && out_cap > 0) {
      hipLaunchKernelGGL(zv_wavjoin_gather_kernel, dim3((unsigned)(B * gtiles)), blk, 0, s, wav,
                         wav_ld, lens, gains, C, frame, (int)nfmax, (int)gtiles, pre, m, off, F,
                         Fn, prevc, doc, doc_ptr, B, D, out, out_ld, out_cap);
      ZV_LAUNCH_CHECK();
    }
    if (D > 0 && out_cap > 0) {
      hipLaunchKernelGGL(zv_wavjoin_zero_kernel, dim3((unsigned)(D * ztiles)), blk, 0, s, out_len,
                         C, (int)ztiles, out, out_ld, out_cap);
      ZV_LAUNCH_CHECK();
    }
  }
};
