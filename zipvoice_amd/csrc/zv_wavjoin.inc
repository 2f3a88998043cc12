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
//
// The stateful join (zv_wavjoin_stream, one slot per open document) runs the same passes on
// the chunks of one push.  energy and plan are the kernels above.  The offsets and gather
// passes are the same device functions compiled a second time (STREAM): offsets seeds the
// chain (p, m_p, off_p) from the slot's held chunk instead of -1, withholds the last
// min(fade, m / 2) samples of the slot's last non-empty chunk through Fn (the "tail the next
// chunk owns" of the one-shot pass) unless the push closes the slot, and stores the slot's
// new words; gather reads the fading-out sample of a held predecessor from the slot's raw
// tail buffer (already trimmed: no search) and mixes it in wj_mix, the expression of the
// one-shot pass.  A tail pass, a launch of its own after the gather, emits the held samples
// that became final and then saves the new tail: held index i is read and written by the one
// thread that owns it, and the gather's reads of the old tail are complete before the launch
// starts, so one buffer per slot is enough.
#pragma once

constexpr int WJ_THREADS = 256;
constexpr int WJ_TILE = WJ_THREADS * 4;   // input samples per workgroup of the gather pass
constexpr int WJ_OFF_BLOCK = 1024;        // chunks staged in LDS per round of the offsets pass
constexpr int WJ_HELD = -2;               // prevc: the predecessor is the slot's held chunk
constexpr int WJ_SLOTS = 64;              // slots per launch of the stream's offsets pass
typedef float wj_f32x4 __attribute__((ext_vector_type(4), aligned(4)));

// one slot of a stream: its last non-empty chunk p so far (m == 0: nothing held); the raw
// samples y_p[m - H, m), H = min(fade, m / 2), are columns [0, H) of the slot's held rows
struct wj_slot { long pos; int m; float g; };
// what the later passes of one push need for a slot: H and g of the chunk held when the push
// began, the held samples now final ([0, flush)), the last non-empty chunk of the push (-1:
// none) and how many samples of its end become the new tail
struct wj_push { int H; float g; int flush, last, keep; };
// the stream's offsets pass, slots [d0, d0 + n): their chunk ranges and final bits
struct wj_slots { int ptr[WJ_SLOTS + 1]; unsigned long final; int d0, n; };

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

// the cross-fade of one sample: xp fades out under gain gp, xb fades in under gain g
__device__ __forceinline__ float wj_mix(float gp, float xp, float g, float xb, float w) {
  return gp * xp * (1.f - w) + g * xb * w;
}

// the input sample that holds trimmed sample tp of a chunk with nf frames: it lies in the
// last frame fp with pre[fp] <= tp
__device__ __forceinline__ long wj_find(const int* pr, long nf, int frame, int tp, long& fp) {
  long flo = 0, fhi = nf;
  while (fhi - flo > 1) {
    const long mid = (flo + fhi) >> 1;
    if (pr[mid] <= tp) flo = mid; else fhi = mid;
  }
  fp = flo;
  return flo * frame + (tp - pr[flo]);
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

// The offsets pass of document / slot d over its chunks [lo, hi).  STREAM: the chain starts
// from the slot's held chunk, the last non-empty chunk keeps its tail back unless `final`,
// out_len[d] is {n_d, pos_d} and n_d goes to n_out as well (the zero pass reads it there).
template <bool STREAM>
__device__ __forceinline__ void wj_offsets(const int* m, int lo, int hi, int d, int fade, long* off,
                                           int* F, int* Fn, int* prevc, int* doc, long* out_len,
                                           int* spans, const float* gains, bool final,
                                           wj_slot* slot, wj_push* rec, long* n_out) {
  __shared__ long s_off[WJ_OFF_BLOCK];
  __shared__ int s_m[WJ_OFF_BLOCK], s_F[WJ_OFF_BLOCK], s_prev[WJ_OFF_BLOCK];
  const int t = threadIdx.x;
  int p = -1, mp = 0;                                    // thread 0: the last non-empty chunk
  long offp = 0;
  int H = 0, flush = 0;
  if (STREAM && t == 0) {
    const int hm = slot->m;
    H = min(fade, hm / 2);
    if (hm > 0) { p = WJ_HELD; mp = hm; offp = (long)H - hm; }   // column 0 is y_p[m_p - H]
    flush = final ? H : 0;
  }
  for (int b0 = lo; b0 < hi; b0 += WJ_OFF_BLOCK) {
    const int nb = min(WJ_OFF_BLOCK, hi - b0);
    for (int i = t; i < nb; i += WJ_THREADS) s_m[i] = m[b0 + i];
    __syncthreads();
    if (t == 0)
      for (int i = 0; i < nb; ++i) {
        const int mb = s_m[i];
        Fn[b0 + i] = 0;
        if (mb == 0) { s_off[i] = -1; s_F[i] = 0; s_prev[i] = -1; continue; }
        const int f = p == -1 ? 0 : min(fade, min(mp / 2, mb / 2));
        const long o = p == -1 ? 0 : offp + mp - f;
        s_off[i] = o; s_F[i] = f; s_prev[i] = p;
        if (p >= 0) Fn[p] = f;
        if (STREAM && p == WJ_HELD) flush = H - f;
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
  if (t != 0) return;
  const long N = p == -1 ? 0 : offp + mp;
  if (!STREAM) { out_len[d] = N; return; }
  // an open slot keeps back the end of its last non-empty chunk; with none in this push
  // (p == WJ_HELD) that is the tail it holds already, and nothing is emitted or saved
  const int keep = final || p == -1 ? 0 : min(fade, mp / 2);
  const long n = N - keep;
  if (p >= 0) Fn[p] = keep;                              // the gather pass leaves the new tail out
  rec->H = H; rec->g = slot->g; rec->flush = flush; rec->last = max(p, -1);
  rec->keep = p >= 0 ? keep : 0;
  out_len[2 * d] = n; out_len[2 * d + 1] = slot->pos; *n_out = n;
  slot->pos += n;
  if (final) { slot->m = 0; slot->g = 0.f; }
  else if (p >= 0) { slot->m = mp; slot->g = gains ? gains[p] : 1.f; }
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_offsets_kernel(
    const int* m, int B, const int* doc_ptr, int fade, long* off, int* F, int* Fn, int* prevc,
    int* doc, long* out_len, int* spans) {
  const int d = blockIdx.x;
  int lo, hi;
  wj_doc_range(doc_ptr, d, B, lo, hi);
  wj_offsets<false>(m, lo, hi, d, fade, off, F, Fn, prevc, doc, out_len, spans, nullptr, false,
                    nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_stream_offsets_kernel(
    const int* m, wj_slots sl, int fade, long* off, int* F, int* Fn, int* prevc, int* doc,
    long* out_len, int* spans, const float* gains, wj_slot* slot, wj_push* rec, long* n_out) {
  const int i = blockIdx.x, d = sl.d0 + i;               // i < sl.n <= WJ_SLOTS
  wj_offsets<true>(m, sl.ptr[i], sl.ptr[i + 1], d, fade, off, F, Fn, prevc, doc, out_len, spans,
                   gains, (sl.final >> i) & 1, slot + d, rec + d, n_out + d);
}

// The gather pass.  STREAM: a chunk whose predecessor is WJ_HELD fades in over the slot's
// held rows (held [D, C, fade], raw samples, their gain in rec[d].g).
template <bool STREAM>
__device__ __forceinline__ void wj_gather(
    const float* wav, long wav_ld, const int* lens, const float* gains, int C, int frame,
    int nfmax, int tiles, const int* pre, const int* m, const long* off, const int* F,
    const int* Fn, const int* prevc, const int* doc, const int* doc_ptr, int B, int D,
    float* out, long out_ld, long out_cap, const float* held, const wj_push* rec, int fade) {
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
    const float* xp;
    long ldp, sp;
    float gp;
    if (STREAM && p == WJ_HELD) {                        // y_p[m_p - H, m_p) is held [0, H)
      const int H = rec[d].H;
      if (Fb > H) continue;                              // never: F_b <= H_p
      xp = held + (long)d * C * fade; ldp = fade; sp = H - Fb + t; gp = rec[d].g;
    } else {
      if (p < 0 || Fb > m[p]) continue;                  // only with overlapping documents
      long fp;
      sp = wj_find(pre + (long)p * (nfmax + 1), (wj_len(lens, p, wav_ld) + frame - 1) / frame,
                   frame, m[p] - Fb + t, fp);
      xp = wav + (long)p * C * wav_ld; ldp = wav_ld; gp = gains ? gains[p] : 1.f;
    }
    const float w = (float)(t + 1) / (float)(Fb + 1);
    for (int c = 0; c < C; ++c)
      out[c * out_ld + dst] = wj_mix(gp, xp[c * ldp + sp], g, xb[c * wav_ld + s], w);
  }
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_gather_kernel(
    const float* wav, long wav_ld, const int* lens, const float* gains, int C, int frame,
    int nfmax, int tiles, const int* pre, const int* m, const long* off, const int* F,
    const int* Fn, const int* prevc, const int* doc, const int* doc_ptr, int B, int D,
    float* out, long out_ld, long out_cap) {
  wj_gather<false>(wav, wav_ld, lens, gains, C, frame, nfmax, tiles, pre, m, off, F, Fn, prevc,
                   doc, doc_ptr, B, D, out, out_ld, out_cap, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_stream_gather_kernel(
    const float* wav, long wav_ld, const int* lens, const float* gains, int C, int frame,
    int nfmax, int tiles, const int* pre, const int* m, const long* off, const int* F,
    const int* Fn, const int* prevc, const int* doc, int B, int D, float* out, long out_ld,
    long out_cap, const float* held, const wj_push* rec, int fade) {
  wj_gather<true>(wav, wav_ld, lens, gains, C, frame, nfmax, tiles, pre, m, off, F, Fn, prevc,
                  doc, nullptr, B, D, out, out_ld, out_cap, held, rec, fade);
}

// The tail pass of a push: a thread owns held columns [i0, i0 + 4) of slot d, in every
// channel.  It first writes those of them that became final, g_p * held[0, flush), to columns
// [0, flush) of the row, then stores the new tail there: held[i] = y_b[m_b - keep + i] of the
// push's last non-empty chunk b, raw.  4 columns move as one dwordx4 when they are all final
// (all inside out_cap), or all part of the new tail and in one frame of the input.
__global__ __launch_bounds__(WJ_THREADS) void zv_wavjoin_stream_tail_kernel(
    const float* wav, long wav_ld, const int* lens, int C, int frame, int nfmax, int fade,
    int tiles, const int* pre, const int* m, const wj_push* rec, float* held, float* out,
    long out_ld, long out_cap) {
  const int d = blockIdx.x / tiles;
  const int i0 = ((blockIdx.x % tiles) * WJ_THREADS + threadIdx.x) * 4;
  if (i0 >= fade) return;
  const wj_push r = rec[d];
  held += (long)d * C * fade;
  if (i0 < r.flush) {
    out += (long)d * C * out_ld;
    const float g = r.g;
    if (i0 + 3 < r.flush && i0 + 3 < out_cap) {
      for (int c = 0; c < C; ++c) {
        wj_f32x4 v = *reinterpret_cast<const wj_f32x4*>(held + c * fade + i0);
        if (g != 1.f) v *= g;
        *reinterpret_cast<wj_f32x4*>(out + c * out_ld + i0) = v;
      }
    } else {
      for (int i = i0; i < min(i0 + 4, r.flush) && i < out_cap; ++i)
        for (int c = 0; c < C; ++c) {
          const float x = held[c * fade + i];
          out[c * out_ld + i] = g != 1.f ? g * x : x;
        }
    }
  }
  if (r.last < 0 || i0 >= r.keep) return;
  const int b = r.last;
  const int* pr = pre + (long)b * (nfmax + 1);
  const long nf = (wj_len(lens, b, wav_ld) + frame - 1) / frame;
  const float* xb = wav + (long)b * C * wav_ld;
  const int t0 = m[b] - r.keep + i0;                     // >= 0: keep <= m_b / 2
  long f;
  const long s0 = wj_find(pr, nf, frame, t0, f);
  if (i0 + 3 < r.keep && t0 + 3 < pr[f + 1]) {
    for (int c = 0; c < C; ++c)
      *reinterpret_cast<wj_f32x4*>(held + c * fade + i0) =
          *reinterpret_cast<const wj_f32x4*>(xb + c * wav_ld + s0);
    return;
  }
  for (int i = i0; i < min(i0 + 4, r.keep); ++i) {
    const long s = wj_find(pr, nf, frame, t0 + (i - i0), f);
    for (int c = 0; c < C; ++c) held[c * fade + i] = xb[c * wav_ld + s];
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
  // the scratch of one call, and the launch geometry that follows from its sizes
  struct plan_t {
    long* off; int *m, *F, *Fn, *prevc, *doc, *pre;
    long nfmax, gtiles, ztiles;
  };
  // Checks the sizes, grows the scratch and runs the energy and plan passes over the chunks.
  plan_t plan(const float* wav, long wav_ld, const int* lens, int B, int C, int D, long out_cap,
              hipStream_t s) {
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
    return plan_t{off, m, F, Fn, prevc, doc, pre, nfmax, gtiles, ztiles};
  }
  void apply(const float* wav, long wav_ld, const int* lens, const float* gains, int B, int C,
             const int* doc_ptr, int D, float* out, long out_ld, long out_cap, long* out_len,
             int* spans, hipStream_t s) {
    const plan_t p = plan(wav, wav_ld, lens, B, C, D, out_cap, s);
    const dim3 blk(WJ_THREADS);
    if (D > 0) {
      hipLaunchKernelGGL(zv_wavjoin_offsets_kernel, dim3(D), blk, 0, s, p.m, B, doc_ptr, fade,
                         p.off, p.F, p.Fn, p.prevc, p.doc, out_len, spans);
      ZV_LAUNCH_CHECK();
    }
    if (B > 0 && out_cap > 0) {
      hipLaunchKernelGGL(zv_wavjoin_gather_kernel, dim3((unsigned)(B * p.gtiles)), blk, 0, s, wav,
                         wav_ld, lens, gains, C, frame, (int)p.nfmax, (int)p.gtiles, p.pre, p.m,
                         p.off, p.F, p.Fn, p.prevc, p.doc, doc_ptr, B, D, out, out_ld, out_cap);
      ZV_LAUNCH_CHECK();
    }
    if (D > 0 && out_cap > 0) {
      hipLaunchKernelGGL(zv_wavjoin_zero_kernel, dim3((unsigned)(D * p.ztiles)), blk, 0, s,
                         out_len, C, (int)p.ztiles, out, out_ld, out_cap);
      ZV_LAUNCH_CHECK();
    }
  }
};

// The stateful join: D slots on one joiner, whose parameters and scratch it borrows.
struct zv_wavjoin_stream {
  zv_wavjoin* j = nullptr;
  int C = 0, D = 0;
  char* buf = nullptr;                     // n [D] int64 | slot [D] | rec [D] | held [D, C, fade]
  size_t bytes = 0;
  long* n = nullptr;
  wj_slot* slot = nullptr;
  wj_push* rec = nullptr;
  float* held = nullptr;
  std::vector<uint8_t> closed;             // host: the slots a final push has closed
  ~zv_wavjoin_stream() {
    if (buf) (void)ZV_BLOCKING(hipFree(buf));
  }
  void init(zv_wavjoin* j_, int C_, int D_) {
    ZV_REQUIRE(j_ != nullptr, "null wavjoin handle");
    ZV_REQUIRE(C_ == 1 || C_ == 2, "C must be 1 or 2");
    ZV_REQUIRE(D_ >= 1, "D must be at least 1");
    j = j_; C = C_; D = D_;
    const size_t nD = (size_t)D;
    static_assert(sizeof(wj_slot) == 16 && sizeof(wj_push) == 20, "slot words");
    const size_t words = nD * 8 + nD * sizeof(wj_slot) + nD * sizeof(wj_push);
    bytes = (words + 15) / 16 * 16 + nD * C * (size_t)j->fade * 4;
    ZV_CHECK(ZV_BLOCKING(hipMalloc(&buf, bytes)));
    ZV_CHECK(ZV_BLOCKING(hipMemset(buf, 0, bytes)));
    n = reinterpret_cast<long*>(buf);
    slot = reinterpret_cast<wj_slot*>(n + nD);
    rec = reinterpret_cast<wj_push*>(slot + nD);
    held = reinterpret_cast<float*>(buf + (words + 15) / 16 * 16);
    closed.assign(nD, 0);
  }
  // d == -1: every slot.  Stream-ordered: the slots' words are cleared after the pushes
  // queued before; the held rows need no clearing (a slot with m == 0 reads none of them).
  void reset(int d, hipStream_t s) {
    ZV_REQUIRE(d >= -1 && d < D, "slot out of range");
    const int d0 = d < 0 ? 0 : d, cnt = d < 0 ? D : 1;
    ZV_CHECK(hipMemsetAsync(slot + d0, 0, (size_t)cnt * sizeof(wj_slot), s));
    std::fill(closed.begin() + d0, closed.begin() + d0 + cnt, (uint8_t)0);
  }
  void push(const float* wav, long wav_ld, const int* lens, const float* gains, int B,
            const int* doc_ptr, const uint8_t* host_final, float* out, long out_ld, long out_cap,
            long* out_len, int* spans, hipStream_t s) {
    for (int d = 0; d < D; ++d) {
      const int lo = doc_ptr ? doc_ptr[d] : 0, hi = doc_ptr ? doc_ptr[d + 1] : B;
      ZV_REQUIRE(lo >= 0 && lo <= hi && hi <= B && (d > 0 || lo == 0) && (d + 1 < D || hi == B),
                 "doc_ptr must rise from 0 to B");
      ZV_REQUIRE(!closed[d] || (hi == lo && !(host_final && host_final[d])),
                 "push to a closed slot (reset it first)");
    }
    const zv_wavjoin::plan_t p = j->plan(wav, wav_ld, lens, B, C, D, out_cap, s);
    const int fade = j->fade;
    const long ttiles = (fade + WJ_TILE - 1) / WJ_TILE;
    ZV_REQUIRE(D * ttiles <= 0x7fffffffL, "too many slots for one launch");
    const dim3 blk(WJ_THREADS);
    for (int d0 = 0; d0 < D; d0 += WJ_SLOTS) {
      wj_slots sl;
      sl.d0 = d0; sl.n = std::min(WJ_SLOTS, D - d0); sl.final = 0;
      for (int i = 0; i <= sl.n; ++i) sl.ptr[i] = doc_ptr ? doc_ptr[d0 + i] : i * B;
      for (int i = sl.n + 1; i <= WJ_SLOTS; ++i) sl.ptr[i] = sl.ptr[sl.n];
      for (int i = 0; i < sl.n; ++i)
        if (host_final && host_final[d0 + i]) sl.final |= 1UL << i;
      hipLaunchKernelGGL(zv_wavjoin_stream_offsets_kernel, dim3(sl.n), blk, 0, s, p.m, sl, fade,
                         p.off, p.F, p.Fn, p.prevc, p.doc, out_len, spans, gains, slot, rec, n);
      ZV_LAUNCH_CHECK();
    }
    if (B > 0 && out_cap > 0) {
      hipLaunchKernelGGL(zv_wavjoin_stream_gather_kernel, dim3((unsigned)(B * p.gtiles)), blk, 0,
                         s, wav, wav_ld, lens, gains, C, j->frame, (int)p.nfmax, (int)p.gtiles,
                         p.pre, p.m, p.off, p.F, p.Fn, p.prevc, p.doc, B, D, out, out_ld, out_cap,
                         held, rec, fade);
      ZV_LAUNCH_CHECK();
    }
    if (ttiles > 0) {                      // after the gather: it reads the tails this replaces
      hipLaunchKernelGGL(zv_wavjoin_stream_tail_kernel, dim3((unsigned)(D * ttiles)), blk, 0, s,
                         wav, wav_ld, lens, C, j->frame, (int)p.nfmax, fade, (int)ttiles, p.pre,
                         p.m, rec, held, out, out_ld, out_cap);
      ZV_LAUNCH_CHECK();
    }
    if (out_cap > 0) {
      hipLaunchKernelGGL(zv_wavjoin_zero_kernel, dim3((unsigned)(D * p.ztiles)), blk, 0, s, n, C,
                         (int)p.ztiles, out, out_ld, out_cap);
      ZV_LAUNCH_CHECK();
    }
    if (host_final)
      for (int d = 0; d < D; ++d) closed[d] |= host_final[d] != 0;
  }
};
