// Fused FeedForward module of the decoder layers (gfx950).
//
//   C = resid + (W2 . swoosh_l(W1 . x + b1) + b2) [+ rowvec]   [; C = orig + (C - orig) * byp]
//
// FeedforwardModule (zipformer.py:1433-1439): in_proj -> SwooshL (scaling.py:1174-1180,
// :1322-1334) -> out_proj, plus the layer's residual add (zipformer.py:536, :593-598 with
// bypass_mid, :610).  One launch replaces in_proj GEMM -> (M, H) 16-bit hidden tensor in
// HBM -> out_proj GEMM: the hidden activation never leaves the CU.
//
// Row block = 4 waves, one per SIMD, each owning 32 tokens for the whole module:
//   x      the wave's 32 tokens x 512 channels, register-resident (128 VGPRs): the B operand
//          of every in-projection MFMA, read from HBM once;
//   out^T  512 outputs x 32 tokens, fp32 (16 v_mfma_f32_32x32x16 tiles = the 256 AGPRs);
//   per hidden chunk c of 32:
//     H^T = W1[c] . x^T      (32 k-steps on one 32x32 accumulator chain)
//     + b1, SwooshL, 16-bit: the accumulator's rows are the next product's K, so the tile IS
//       the B operand of out^T += W2[:, c] . H (2 k-steps x 16 output tiles) with no lane
//       movement and no LDS round trip (cdna_hip_programming.md §3, "accumulator tile as the
//       next MFMA's operand": the K order inside a step is permuted, and W2's columns are
//       stored in that order).
// Only the weights pass through LDS: one 1 KiB fragment read per 32-cycle MFMA (half the LDS
// bytes per FLOP of a GEMM that stages both operands).  Weights are stored "fragment-major"
// (each MFMA A fragment a contiguous, lane-linear 1 KiB), so a fragment is one global_load_lds
// DMA piece and one conflict-free ds_read_b128 at 16 * lane; four pieces share one M0 write.
//
// Software pipeline, one wave per SIMD: iteration c interleaves the in-projection of chunk
// c + 1 (even MFMA slots) with the out-projection of chunk c - 1 (odd slots) and, between
// them, the SwooshL of chunk c as single-instruction asm micro-ops (4 slots per element, one
// 32-cycle MFMA between dependent ops: the transcendental's result is never waited for, and
// the 24 free issue cycles of each slot hold the VALU and the fragment reads).  With hipcc's
// own scheduling the activation ran as dependent bursts between MFMA pairs and the loop took
// 2.2x its MFMA time.  Rings: W1 chunks in slots 0/1, W2 chunks in slots 2/3 (32 KiB each);
// iteration c reads W1(c + 1) and W2(c - 1) and loads W1(c + 2) and W2(c) into the slots
// iteration c - 1 retired: one vmcnt(0) + barrier per chunk.  b1 is staged in LDS.
//
// Persistent schedule (round 4).  A block is one CU for the whole launch and walks a "line"
// of w chunk steps of the launch's R x nc (row block, chunk) steps (w >= nc, blocks = ceil(R nc
// / w)): [the first chunks of a row block] [whole row blocks] [the last chunks of another].  A
// row block cut by a line boundary is run as two items: its first chunks start the next line
// (P item: accumulate, store the raw out^T tiles), its last chunks end this line (C item:
// load them as the initial accumulators, finish, epilogue).  The accumulation order per output
// is the one of the uncut block (chunk 0 .. nc-1, fp32 store/load is exact), so results are
// bit for bit those of the one-block-per-row-block schedule (w = nc).  What it buys:
//   * grid fill: R = 610 row blocks on 256 CUs took 3 rounds of blocks; as lines they take
//     ceil(610 nc / 256) chunk steps (2.4 rounds), R = 305 1.2 rounds instead of 2;
//   * epilogue de-synchronisation: line b's whole row blocks start at chunk offset (-b w) mod nc,
//     so the 10 B/output residual read-modify-write of different CUs no longer lands in the same
//     microseconds (one block per CU ran every epilogue of a round in lock step while no MFMA ran:
//     ~28 % of a launch, profiles/r03_ffn_lab.txt);
//   * the next item's first two W1 chunks are DMA'd during this item's last two chunk steps.
// Hand-off (cdna_hip_programming.md §6 Guideline 16, R1): the P item stores its tiles write-
// through (sc1 buffer stores), every wave drains vmcnt, barrier, one lane sets the line's flag
// (relaxed agent store); the C item (end of the previous line: P ends at step nc - q <= w - q,
// where its C item starts) polls it relaxed from one lane with s_sleep, one agent acquire, resets
// the flag (every flag word is zero between launches; the workspace zero-fills it once), barrier,
// plain loads.  The spin cannot deadlock -- the producer was issued no later than the consumer's
// grid (one block per CU, blocks <= the scratch's slots <= CUs, checked at launch) -- and it is
// bounded all the same: a C item that waited 0.2 s traps (the launch fails loudly) instead of
// loading tiles that were never written and leaving its flag set for a later launch.
//
// The epilogue works on the accumulators in place: v_permlane32_swap pairs give every lane 8
// consecutive outputs of its token's row (32-B fp32 loads / stores, 16-B 16-bit copy); rows
// past M clamp their reads and store to the sink, so every memory operation is unconditional.
// A launch may cover up to FFN_MAXSEG row ranges with their own pointers (the decoder's row
// blocks on several streams joined into one launch).
#pragma once
#include <cstddef>
#include "zv_gemm256.inc"
#include "zv_weights.inc"

typedef unsigned v4u32_t __attribute__((ext_vector_type(4)));
typedef unsigned v2u32_t __attribute__((ext_vector_type(2)));
constexpr int FFN_D = 512, FFN_BM = 128, FFN_HC = 32, FFN_SLOT = 32768, FFN_MAXSEG = 4;
constexpr long FFN_PART_FLOATS = (long)FFN_BM * FFN_D;   // one P item's tiles (256 KiB)

struct FfnSeg {                    // one row range and its own operand pointers
  int M, rb0;                      // rows; first row block of the range in the launch's order
  const bf16* X;                   // (M, 512) 16-bit copy of the stream (the module input; PRE: unused)
  const bf16* A;                   // PRE: (M, Kp) 16-bit pre-projection operand, row stride lda
  const float* resid; float* C;    // fp32 stream (resid may alias C)
  bf16* Ch;                        // the stream's 16-bit copy (or null)
  const float* rowvec;             // row vector (row r adds rowvec[r / rows_per_group])
  const float* orig;               // bypass original
  bf16* Cl; bf16* C2h; bf16* C2l;   // NORM outputs
};

struct FfnParams {
  int H;                           // hidden width (H % 64 == 0)
  int R, nseg;                     // row blocks over all ranges; ranges
  FfnSeg seg[FFN_MAXSEG];
  long ldx, ldc, ldch, rowvec_ld; int rows_per_group;   // shared by the ranges
  const bf16* W1f; const float* b1;  // in_proj, fragment-major [H/32][32 k-steps][64][8]
  const bf16* W2f; const float* b2;  // out_proj, fragment-major [H/32][16][2][64][8], K permuted
  const float* byp;
  // PRE (the pre-projection form): cur1 = resid + (A . Wp^T + bp) [+ rowvec] is formed in the out^T
  // tiles before the module runs, x = round16(cur1) in registers; Wpf fragment-major
  // [nkp][16][2][64][8] with K in natural order (zv_ffn_pack_wp_kernel), zero past K.  Columns
  // [K, 32 nkp) of A are read: the caller keeps them zero (finite at least: Wpf is zero there).
  // W1f's K is then in the accumulator's register order (zv_ffn_pack_w1p_kernel)
  const bf16* Wpf; const float* bp; long lda; int nkp;
  // NORM epilogue (FF3 + the layer's BiasNorm + bypass, zipformer.py:610-618, scaling.py:330-355):
  // x = resid + FF(x) is never stored; out = orig + (x * rsqrt(mean((x - nb)^2)) e^log_scale - orig)
  // * byp -> C (fp32, in place over orig) and Ch / Cl (16-bit hi / lo copy); out + rowvec ->
  // C2h / C2l (the next layer's working-stream copy) where non-null
  const float* nb; float log_scale;
  float norm_scale;                // exp(log_scale), set by launch_ffn
  float* sink;
  // schedule: w chunk steps per block (w = nc: one row block per block); part: one P item's
  // tiles per block (FFN_PART_FLOATS each), flag: one word per block (zero between launches),
  // part_slots: how many blocks the scratch was sized for (launch_ffn launches no more)
  int w;
  float* part; unsigned* flag; int part_slots;
  unsigned* err;                   // the process's device error word (zv_dev_err_word): bit 0 set by a
                                   // C item that outwaited FFN_SPIN_TICKS
  unsigned long long* dbg;         // FFN_TIMING builds (lab): per-block clock totals
};

// FFN_NORM_LDS: the FF3 + BiasNorm epilogue's constant vectors (b2, the norm bias, the bypass scale;
// and per wave its two row groups' row vectors) staged in LDS: read per group through ds_read,
// they no longer sit in the vector-memory stream, whose in-order retirement made each group's
// constant loads wait for every residual / original prefetch issued before them
#ifndef FFN_NORM_LDS
#define FFN_NORM_LDS 1
#endif
// FFN_XOVL: an item's prologue chain overlaps the tail of its x loads (counted waits) instead of
// waiting for all of them
#ifndef FFN_XOVL
#define FFN_XOVL 1
#endif
constexpr int FFN_NCONST = 3 * FFN_D + 4 * 2 * FFN_D;   // floats: b2 | nb | byp, then 4 waves x 2 rows
inline size_t ffn_lds_bytes(int H, bool norm = false) {
  return 4 * FFN_SLOT + ((size_t)H + FFN_HC) * 4 +
         (norm && FFN_NORM_LDS ? FFN_NCONST * 4 : 0);
}

// Every instruction of the pipelined loop whose position matters is inline asm: volatile asm
// statements keep their source order, so the interleave above is the one that runs.  The
// accumulators' register classes are pinned: the 16 output tiles ("+a") fill the 256 AGPRs,
// the in-projection tiles ("v") sit in VGPRs beside x and the fragments (left to itself hipcc
// put the in-projection accumulator in AGPRs and shuffled output tiles through VGPRs).
// Hazards hipcc does not see inside asm: every VALU read of an asm-MFMA result and every MFMA
// read of a VALU-written operand is an iteration (>= 64 instructions) away, or behind the
// s_nop run that ends each chunk's barrier; transcendental results are read one MFMA later.
#ifdef ZV_OPERAND_F16
#define FFN_MFMA "v_mfma_f32_32x32x16_f16"
#else
#define FFN_MFMA "v_mfma_f32_32x32x16_bf16"
#endif
// FFN_BIAS_ACC: each in-projection accumulator chain starts from b1 (the tile's 16 registers read from
// LDS, 4 ds_read_b128, right after the tile's previous chunk was activated) instead of zero, so the
// activation drops its per-element v_add (16 VALU a chunk step); the sum's rounding order changes
// (b1 first instead of last), not bitwise equal to FFN_BIAS_ACC 0.  Lab (r04_b var.txt, M = 78016,
// H = 1536, residual epilogue): persistent launch 316.6 -> 302.1 us with FFN_OUT_ASM, no-epilogue
// arm 228.9 -> 217.5 us; fused vs unfused max |diff| 1.2e-7 -> 2.5e-5 (both sum orders are exact-
// product fp32 sums)
#ifndef FFN_BIAS_ACC
#define FFN_BIAS_ACC 1
#endif
__device__ __forceinline__ void ffn_mma_v0(f32x16& acc, const bf16x8& a, const bf16x8& b) {
  asm volatile(FFN_MFMA " %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void ffn_mma_v(f32x16& acc, const bf16x8& a, const bf16x8& b) {
  asm volatile(FFN_MFMA " %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// The out-projection MFMA (FFN_OUT_ASM 1, the default) is asm as well, so the whole slot
// interleave (in-projection on even slots, out-projection on odd ones, the micro-ops between) is the
// one written: as the builtin (FFN_OUT_ASM 0) its placement was hipcc's, which ran some slots back to
// back and stacked their fillers elsewhere (-3 % of a launch).  An asm MFMA's A/B operands look dead
// to hipcc right after the statement while the MFMA still reads them, so their lifetimes are
// extended to the step end (the WAR asm statement after each step), where the barrier's s_nop run
// separates them from any reuse.
#ifndef FFN_OUT_ASM
#define FFN_OUT_ASM 1
#endif
__device__ __forceinline__ void ffn_mma_a(f32x16& acc, const bf16x8& a, const bf16x8& b) {
#if FFN_OUT_ASM
  asm volatile(FFN_MFMA " %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
#else
  acc = ZV_MFMA_32x32x16(a, b, acc, 0, 0, 0);
#endif
}
// SwooshL micro-ops: exactly zv_common.h swoosh_l's instruction sequence (v_exp_f32 / v_log_f32
// are __builtin_amdgcn_exp2f / logf; fused multiply-adds with the same literal constants).  A
// transcendental's result is read one instruction later at the earliest: exp (end of sub-op 1) and
// its reader (sub-op 2) have the in-projection MFMA (asm, its place fixed) between them; log (end of
// sub-op 2) and its reader have q's fma between them (q moved from sub-op 1 to the head of sub-op 3:
// the out-projection MFMA between sub-ops 2 and 3 is the builtin, which hipcc may move, and the
// s_nop 0 the hazard otherwise needs cost 32 x 4 cycles a chunk step).  The peeled first chunk
// runs sub-ops 0+1 and 2+3 per MFMA slot: the same distances.
struct FfnAct { float t, m, q; };
__device__ __forceinline__ void ffn_act_op(int sub, float& y, FfnAct& a, float b, float c0, float cq) {
  // (each sub-op one asm statement: between two statements hipcc's hazard recognizer, which sees
  // an asm block as a possible transcendental, put an s_nop 0)
  if (sub == 0) {
#if FFN_BIAS_ACC
    // (y = h + b1 already: the accumulator chain started from b1) t = log2e y - 4 log2e
    asm volatile("v_fmamk_f32 %0, %1, 0x3fb8aa3b, %2" : "=&v"(a.t) : "v"(y), "v"(c0));
#else
    // y = h + b1; t = log2e y - 4 log2e
    asm volatile("v_add_f32 %0, %0, %2\n\tv_fmamk_f32 %1, %0, 0x3fb8aa3b, %3" : "+&v"(y), "=&v"(a.t) : "v"(b), "v"(c0));
#endif
  } else if (sub == 1) {
    // m = 2^min(t, 126)
    asm volatile("v_min_f32 %0, 0x42fc0000, %1\n\tv_exp_f32 %0, %0" : "=&v"(a.m) : "v"(a.t));
  } else if (sub == 2) {
    // m = log2(1 + m)
    asm volatile("v_add_f32 %0, 1.0, %0\n\tv_log_f32 %0, %0" : "+v"(a.m));
  } else {
    // q = -0.08 y - 0.035; y = ln2 max(m, t) + q  (t past ~24)
    asm volatile("v_fmamk_f32 %1, %0, 0xbda3d70a, %4\n\tv_max_f32 %2, %2, %3\n\tv_fmamk_f32 %0, %2, 0x3f317218, %1"
                 : "+&v"(y), "=&v"(a.q), "+&v"(a.m) : "v"(a.t), "v"(cq));
  }
}

// MFMA slots (0..63 of a chunk step) that issue the step's four weight DMAs: W1(c + 2) halves
// into slot c & 1 (free: W1(c) was consumed in step c - 1), W2(c) halves into slot 2 + (c & 1)
// (W2(c - 2) consumed in step c - 1); each must land before the step's closing barrier
#ifndef FFN_DMA_K0
#define FFN_DMA_K0 1
#define FFN_DMA_K1 17
#define FFN_DMA_K2 33
#define FFN_DMA_K3 49
#endif
#ifndef FFN_TIMING
#define FFN_TIMING 0
#endif
// epilogue prefetch depths (groups of 8 outputs per lane whose residual / original loads are in
// flight): plain, with the bypass original (two streams), FF3 + BiasNorm (one stream per pass; the
// pass-2 original loads continue the pass-1 pipeline)
#ifndef FFN_PD
#define FFN_PD 12
#endif
#ifndef FFN_PD_OPRE
#define FFN_PD_OPRE 8
#endif
#ifndef FFN_PD_NORM
#define FFN_PD_NORM 16   // 8 before its constants moved to LDS (r04_o: M = 78,016 377 -> 368 us)
#endif
// FFN_TIMING words per wave in p.dbg: total clk, real-time ticks, vmcnt wait, barrier, chunk steps, w,
// epilogue (last step's end .. stores drained), item start (x loads landed), items, steady-state loop
constexpr int FFN_DBG_WORDS = 10;
// lab-only ablations of the chunk step (wrong results; timing only): no SwooshL micro-ops, no W1 /
// W2 fragment re-reads (every MFMA of a kind reuses the step's first four fragments)
#ifndef FFN_X_NOACT
#define FFN_X_NOACT 0
#endif
#ifndef FFN_X_NOW1
#define FFN_X_NOW1 0
#endif
#ifndef FFN_X_NOW2
#define FFN_X_NOW2 0
#endif
// FFN_EPI_T: the plain epilogue through an LDS transposer (the W2 slots, free after the last
// out-projection): per pass of 128 outputs a wave writes its 4 output tiles to its 16 KiB (rows =
// tokens, 16-B chunks XOR-swizzled by row: conflict-free both ways), reads them back as 2 rows x 512 B
// per wave instruction and does the residual read-modify-write and the 16-bit copy on those
// lane-contiguous runs (4 cache lines per row instead of 16-B pieces of 32 rows: r04_f's lane-contiguous-address
// ablation put the gain at -31 % of the epilogue)
#ifndef FFN_EPI_T
#define FFN_EPI_T 1
#endif
#ifndef FFN_PT
#define FFN_PT 16
#endif
// FFN_EPI_NT: the FF3 + BiasNorm epilogue on the transposer's layout too: pass 1 forms the
// pre-norm rows from lane-contiguous row pieces (2 rows x 512 B per wave instruction instead of
// 16-B pieces of 32 rows), keeps them in the accumulator registers it frees and sums each row's
// squares across its half-wave (an xor butterfly: every lane of the row gets the same bits);
// pass 2 writes the normalised, bypassed rows and the next layer's copies on the same layout
#ifndef FFN_EPI_NT
#define FFN_EPI_NT 1
#endif
#ifndef FFN_PT_NORM
#define FFN_PT_NORM 8
#endif
// C-item wait bound: 2 s of the 100 MHz clock.  A healthy producer can be held up by queue preemption
// or time slicing (the clock keeps running), so the bound is generous and not fatal: the C item sets
// the error word and finishes with whatever tiles it has; the next engine call reports the error
// (zv_check_dev_err) and resets the flags
constexpr unsigned long long FFN_SPIN_TICKS = 200000000;

// ABL (lab ablations, 0 in the engine): 1 no weight DMA in the loop (compute-bound rate),
// 3 no epilogue
// NORM (FF3 + BiasNorm epilogue): 0 off, 1 on (its optional outputs checked at run time)
// TP: the transposed plain epilogue (FFN_EPI_T) is allowed; the launcher clears it for a row vector
// whose groups are shorter than a wave (its per-row lookup would stall the prefetch stream)
// PRE: the pre-projection form (FfnParams: Wpf).  An item that starts a row block (whole, or a P
// item) first streams the Wp chunks through the W2 slots onto initial accumulators resid + bp
// [+ rowvec], then takes x = round16 of the tiles as its in-projection operand in place (the tile's
// registers 8 pp .. 8 pp + 7 of output tile jt are k-step 2 jt + pp: W1f's K order); the epilogue
// reads no residual.  A P item also stores x to Ch (write-through, before its flag), where its C
// item loads it in the same register order: cut and uncut row blocks stay bitwise equal
template <bool RV, bool ORIG, bool COPY, int ABL = 0, int NORM = 0, bool TP = true, bool PRE = false>
__global__ __launch_bounds__(256, 1) void zv_ffn_kernel(FfnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tl = lane & 31, hh = lane >> 5;
  const int nc = p.H / FFN_HC;
  float* b1s = reinterpret_cast<float*>(smem + 4 * FFN_SLOT);
  const long Wtot = (long)p.R * nc;
  const long start = (long)blockIdx.x * p.w;
  if (start >= Wtot) return;
  const long end = min(start + (long)p.w, Wtot);

  // one 32 KiB weight chunk into a slot: 8 DMA pieces (1 KiB) per wave, 4 per M0 write
  auto dma = [&](const bf16* W, int c, int slot, int half) {
    // (the source address is uniform; through the item lambda hipcc lost track of it: SGPRs
    // explicitly, the DMA's "s" operand)
    const unsigned long long a = (unsigned long long)W + (unsigned long long)((long)c * FFN_SLOT + wave * 8192 + half * 4096);
    // (readfirstlane returns int: through unsigned, so the low word is not sign-extended)
    const unsigned long long b =
        ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32) |
        (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)a);
    glds16s_x4(reinterpret_cast<const void*>(b), (unsigned)lane * 16u, smem + slot * FFN_SLOT + wave * 8192 + half * 4096);
  };
  // the item starting at tape position ps (row block r, chunks [ca, cb)); see the header
  auto item_at = [&](long ps, int& r, int& ca, int& cb) {
    r = (int)(ps / nc);
    const int c = (int)(ps - (long)r * nc);
    if (c != 0) { ca = 0; cb = nc - c; }                  // P item (a line's first)
    else if (ps + nc <= end) { ca = 0; cb = nc; }
    else { ca = nc - (int)(end - ps); cb = nc; }         // C item (a line's last)
  };

  int r, ca, cb;
  item_at(start, r, ca, cb);
  dma(p.W1f, ca, 0, 0); dma(p.W1f, ca, 0, 1);
  dma(p.W1f, ca + 1, 1, 0); dma(p.W1f, ca + 1, 1, 1);
  for (int i = tid; i < p.H + FFN_HC; i += 256) b1s[i] = i < p.H ? p.b1[i] : 0.f;
  // FF3 + BiasNorm constants (FFN_NORM_LDS; visible after the first item's barrier)
  constexpr bool NLDS = NORM && FFN_NORM_LDS;
  float* ncs = b1s + p.H + FFN_HC;
  if constexpr (NLDS) {
    for (int i = tid; i < FFN_D; i += 256) {
      ncs[i] = p.b2[i];
      ncs[FFN_D + i] = p.nb[i];
      ncs[2 * FFN_D + i] = p.byp[i];
    }
  }

  float c0 = -5.77078016355585362f, cq = -0.035f;
  asm volatile("" : "+v"(c0), "+v"(cq));   // in VGPRs (VOP2 literal forms take the other constant)
  const int lfrag = lane * 16;
  // the W1 fragment of k-step s of the chunk in W1 slot sl; the W2 fragment (tile j, step s2).  The
  // W2 slots sit past 64 KiB, beyond ds_read's 16-bit offset: their own base register (opaque, or
  // hipcc folds it back and adds per read), so every fragment read is base + immediate
  int lfrag2 = lane * 16 + 2 * FFN_SLOT;
  asm volatile("" : "+v"(lfrag2));
  auto w1f = [&](int sl, int s) { return *reinterpret_cast<const bf16x8*>(smem + sl * FFN_SLOT + s * 1024 + lfrag); };
  auto w2f = [&](int sl, int i) { return *reinterpret_cast<const bf16x8*>(smem + sl * FFN_SLOT + i * 1024 + lfrag2); };
  // the activated element r (register r of the tile) -> the B fragment of k-step r >> 3
  auto put = [&](bf16x8 (&hb)[2], int rr, float y) { hb[rr >> 3][rr & 7] = (bf16)y; };
  const __amdgpu_buffer_rsrc_t part_rs = __builtin_amdgcn_make_buffer_rsrc(p.part, 0, 0x7fffffff, 0x00020000);

#if FFN_TIMING
  unsigned long long tm_vm = 0, tm_bar = 0, tm_steps = 0, tm_epi = 0, tm_x = 0, tm_items = 0, tm_loop = 0;
  const unsigned long long tm_t0 = __builtin_amdgcn_s_memtime(), tm_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  // one item: KIND 0 a whole row block, 1 a P item (first chunks: tiles to this line's slot),
  // 2 a C item (last chunks from the next line's tiles); each kind its own straight-line code
  // (one body with the kinds as runtime branches merged the zero and the loaded tiles and spilled)
  auto item = [&](auto KIND_, int r, int ca, int cb, bool has_next, int nca) {
    constexpr int KIND = decltype(KIND_)::value;
    constexpr bool split_in = KIND == 2, split_out = KIND == 1;
    const int nxt_c0 = has_next ? nca : cb - 1;            // W1 chunk for this item's step cb - 2
    const int nxt_c1 = has_next ? nca + 1 : cb - 1;        // ... and step cb - 1
    f32x16 out[16];
    int sg = 0;
#pragma unroll
    for (int i = 1; i < FFN_MAXSEG; ++i) sg = (i < p.nseg && r >= p.seg[i].rb0) ? i : sg;
    // the range's fields straight from the kernel-argument segment (scalar loads at a computed
    // offset): indexing the by-value parameter copied it to scratch, and the copy's reloads sat
    // in the chunk loop behind vmcnt(0) waits
    typedef __attribute__((address_space(4))) const FfnSeg KSeg;
    KSeg& S = ((KSeg*)((__attribute__((address_space(4))) const char*)__builtin_amdgcn_kernarg_segment_ptr() +
                       offsetof(FfnParams, seg)))[sg];
    const int t0 = (r - S.rb0) * FFN_BM + wave * 32;

    if constexpr (split_in) {
      // C item: the out^T tiles the next line's P item stored (its flag), as the initial
      // accumulators
      if (tid == 0) {
        GLOBAL unsigned* fl = (GLOBAL unsigned*)(p.flag + blockIdx.x + 1);
        const unsigned long long t_give_up = wall_clock64() + FFN_SPIN_TICKS;
        while (__hip_atomic_load(fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
          __builtin_amdgcn_s_sleep(2);
          if (wall_clock64() > t_give_up) {                   // a lost producer: report, do not hang
            if (p.err) __hip_atomic_store(p.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __hip_atomic_store(fl, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      // (lane through an opaque copy: the tile addresses are loop-invariant, and hoisted out of
      // the item loop they took 128 VGPRs for the whole launch and spilled)
      int lv = lane;
      asm volatile("" : "+v"(lv));
      const f32x4* src = reinterpret_cast<const f32x4*>(p.part + (long)(blockIdx.x + 1) * FFN_PART_FLOATS) + wave * 4096 + lv;
      // (tile by tile: a scheduling barrier per tile keeps the loads from being hoisted en bloc,
      // which took 256 VGPRs beside x and spilled)
      static_for<16>([&](auto J_) {
        constexpr int j = decltype(J_)::value;
        f32x4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = src[(j * 4 + q) * 64];
        // a whole new tile value (element inserts into out[j] would keep the previous item's tile
        // live across the item loop)
        out[j] = f32x16{v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3],
                        v[2][0], v[2][1], v[2][2], v[2][3], v[3][0], v[3][1], v[3][2], v[3][3]};
        __builtin_amdgcn_sched_barrier(0);
      });
    } else if constexpr (!PRE) {
#pragma unroll
      for (int j = 0; j < 16; ++j) out[j] = f32x16{};
    }
    // the output tiles live in the AGPRs (left to itself the allocator gave some of them VGPRs
    // once they were written / read outside the MFMAs, and spilled)
    // (PRE: the pre-projection below writes a starting row block's tiles)
    if constexpr (!PRE || split_in) {
#pragma unroll
      for (int j = 0; j < 16; ++j) asm volatile("" : "+a"(out[j]));
    }
#if FFN_TIMING
    const unsigned long long tx0 = __builtin_amdgcn_s_memtime();
    ++tm_items;
#endif
    // FF3 + BiasNorm: this wave's two row groups' row vectors to its LDS rows (row groups of >= 32
    // rows: a wave spans at most two), loaded with x
    const bool nrv = NLDS && !split_out && S.rowvec != nullptr && p.rows_per_group >= 32;
    const int nrv_g0 = nrv ? min(t0, S.M - 1) / p.rows_per_group : 0;
    f32x4 nrvv[4];
    if constexpr (NLDS && !split_out) {
      if (nrv) {
        const int g1 = min(nrv_g0 + 1, (S.M - 1) / p.rows_per_group);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = (q * 64 + lane) * 4;            // float f of the two rows (1024 floats)
          const int grp = f < FFN_D ? nrv_g0 : g1;
          nrvv[q] = *reinterpret_cast<const f32x4*>(S.rowvec + (long)grp * p.rowvec_ld + (f & (FFN_D - 1)));
        }
      }
    }
    bf16x8 xf[32];
    if constexpr (!PRE) {
      const int tr = min(t0 + tl, S.M - 1);
      const bf16* xr = S.X + (long)tr * p.ldx + 8 * hh;
#pragma unroll
      for (int s = 0; s < 32; ++s) xf[s] = *reinterpret_cast<const bf16x8*>(xr + 16 * s);
    } else if constexpr (split_in) {
      // PRE, C item: x as its P item stored it (Ch), in the accumulator's register order: element e of
      // k-step s is channel 16 s + 8 (e >> 2) + 4 hh + (e & 3), two 8-B pieces
      const int tr = min(t0 + tl, S.M - 1);
      const bf16* xr = S.Ch + (long)tr * p.ldch + 4 * hh;
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(xr + 16 * s), hi = *reinterpret_cast<const bf16x4*>(xr + 16 * s + 8);
        xf[s] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
    }
    // the x loads are the last 32 vector-memory operations: everything older (the weight DMA, the
    // previous item's stores, the row vectors) has landed at vmcnt(32); each x fragment's own wait
    // is hipcc's (counted, before its first in-projection MFMA), so the prologue chain starts as the
    // first fragments arrive
    wait_vmcnt<(FFN_XOVL && !PRE) ? 32 : 0>();
    if constexpr (NLDS && !split_out) {
      if (nrv) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<f32x4*>(ncs + 3 * FFN_D + wave * 2 * FFN_D + (q * 64 + lane) * 4) = nrvv[q];
      }
    }
    __syncthreads();
#if FFN_TIMING
    tm_x += __builtin_amdgcn_s_memtime() - tx0;
#endif

    if constexpr (PRE && !split_in) {
      // ---- the pre-projection: out^T = resid + bp [+ rowvec] + Wp . A^T, then x = round16(out^T).
      // Every slot's readers are behind the barrier above: Wp chunk kc streams through W2 slot
      // 2 + (kc & 1), one vmcnt(0) + barrier per chunk; the wave's rows of A, resid and Ch through
      // buffer resources (rows past M read 0, their stores are dropped)
      int lvp = lane;
      asm volatile("" : "+v"(lvp));          // (lane-invariant offsets not hoisted out of the item loop)
      const int ptl = lvp & 31, phh = lvp >> 5;
      const int wr = max(0, min(32, S.M - t0));
      const __amdgpu_buffer_rsrc_t rs_a =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(S.A + (long)t0 * p.lda), 0, wr * (int)p.lda * 2, 0x00020000);
      const __amdgpu_buffer_rsrc_t rs_pr =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(S.resid + (long)t0 * p.ldc), 0, wr * (int)p.ldc * 4, 0x00020000);
      const int a_off = (ptl * (int)p.lda + 8 * phh) * 2, r_off = (ptl * (int)p.ldc + 4 * phh) * 4;
      auto load_a = [&](int kc, int s) {
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_off + kc * 64 + s * 32, 0, 0));
      };
      dma(p.Wpf, 0, 2, 0); dma(p.Wpf, 0, 2, 1);
      bf16x8 ac[2], an[2];
      ac[0] = load_a(0, 0); ac[1] = load_a(0, 1);
      // the initial accumulators: register 4 q + e of tile j is output 32 j + 8 q + 4 hh + e of token tl
      const bool hrv = S.rowvec != nullptr;
      const int rpg = hrv ? p.rows_per_group : 1;
      auto tile_of = [&](const f32x4 (&v)[4]) {
        return f32x16{v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3],
                      v[2][0], v[2][1], v[2][2], v[2][3], v[3][0], v[3][1], v[3][2], v[3][3]};
      };
      if (!hrv || rpg >= 32) {
        // bp + the wave's two row groups' row vectors staged in the wave's 4 KiB of W2 slot 3 (free
        // until chunk 1's DMA, issued behind the first chunk barrier); the residual pieces PDT tiles ahead
        float* cvs = reinterpret_cast<float*>(smem + 3 * FFN_SLOT) + wave * 2 * FFN_D;
        const int g0 = hrv ? min(t0, S.M - 1) / rpg : 0;
        const int g1 = hrv ? min(g0 + 1, (S.M - 1) / rpg) : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = (q * 64 + lvp) * 4, ch = f & (FFN_D - 1);
          f32x4 v = *reinterpret_cast<const f32x4*>(p.bp + ch);
          if (hrv) v += *reinterpret_cast<const f32x4*>(S.rowvec + (long)(f < FFN_D ? g0 : g1) * p.rowvec_ld + ch);
          *reinterpret_cast<f32x4*>(cvs + f) = v;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const float* cvp = cvs + ((hrv && t0 + ptl >= (g0 + 1) * rpg) ? FFN_D : 0) + 4 * phh;
        constexpr int PDT = 6;
        f32x4 ri[16][4];
        auto pf = [&](int j) {
          if (j < 16) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              ri[j][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_pr, r_off + (32 * j + 8 * q) * 4, 0, 0));
          }
        };
#pragma unroll
        for (int j = 0; j < PDT; ++j) pf(j);
        static_for<16>([&](auto J_) {
          constexpr int j = decltype(J_)::value;
          pf(j + PDT);
          f32x4 v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = ri[j][q] + *reinterpret_cast<const f32x4*>(cvp + 32 * j + 8 * q);
          out[j] = tile_of(v);
          asm volatile("" : "+a"(out[j]));
          __builtin_amdgcn_sched_barrier(0);
        });
      } else {
        // row groups shorter than a wave: each lane its own row's vector
        const int grp = min(t0 + ptl, S.M - 1) / rpg;
        const float* vrow = S.rowvec + (long)grp * p.rowvec_ld + 4 * phh;
        const float* bpl = p.bp + 4 * phh;
        static_for<16>([&](auto J_) {
          constexpr int j = decltype(J_)::value;
          f32x4 v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 r4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_pr, r_off + (32 * j + 8 * q) * 4, 0, 0));
            v[q] = r4 + (*reinterpret_cast<const f32x4*>(bpl + 32 * j + 8 * q) + *reinterpret_cast<const f32x4*>(vrow + 32 * j + 8 * q));
          }
          out[j] = tile_of(v);
          asm volatile("" : "+a"(out[j]));
          if constexpr ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        });
      }
      auto pstep = [&](auto PAR_, int kc) {
        constexpr int PAR = decltype(PAR_)::value;       // kc & 1: the chunk's slot
        wait_vmcnt<0>();                     // this wave's DMA pieces and A fragments of chunk kc
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();        // ... everyone's, and everyone is done with the other slot
        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
        if (kc + 1 < p.nkp) { dma(p.Wpf, kc + 1, 3 - PAR, 0); dma(p.Wpf, kc + 1, 3 - PAR, 1); }
        const int kn = min(kc + 1, p.nkp - 1);
        an[0] = load_a(kn, 0); an[1] = load_a(kn, 1);
        bf16x8 fb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) fb[q] = w2f(PAR, q);
        static_for<32>([&](auto I_) {
          constexpr int i = decltype(I_)::value;
          ffn_mma_a(out[i >> 1], fb[i & 3], ac[i & 1]);
          if constexpr (i + 4 < 32) fb[i & 3] = w2f(PAR, i + 4);
        });
        // (WAR: the asm MFMAs read their operands during their passes, see the chunk step below)
        asm volatile("" ::"v"(ac[0]), "v"(ac[1]), "v"(fb[0]), "v"(fb[1]), "v"(fb[2]), "v"(fb[3]));
        ac[0] = an[0]; ac[1] = an[1];
      };
      int kc = 0;
      for (; kc + 1 < p.nkp; kc += 2) {
        pstep(std::integral_constant<int, 0>{}, kc);
        pstep(std::integral_constant<int, 1>{}, kc + 1);
      }
      if (kc < p.nkp) pstep(std::integral_constant<int, 0>{}, kc);
      // MFMA result -> accvgpr read: 18 wait states; then x in place
      asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
#pragma unroll
      for (int j = 0; j < 16; ++j) asm volatile("" : "+a"(out[j]));
      static_for<32>([&](auto S_) {
        constexpr int s = decltype(S_)::value, jt = s >> 1, pp = s & 1;
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[s][e] = (bf16)out[jt][8 * pp + e];
      });
#pragma unroll
      for (int j = 0; j < 16; ++j) asm volatile("" : "+a"(out[j]));
      if constexpr (split_out) {
        // P item: x to the stream's 16-bit copy for its C item, write-through like the tiles (the flag
        // is raised behind this wave's vmcnt(0))
        const __amdgpu_buffer_rsrc_t rs_xh =
            __builtin_amdgcn_make_buffer_rsrc(S.Ch + (long)t0 * p.ldch, 0, wr * (int)p.ldch * 2, 0x00020000);
        const int h_off = (ptl * (int)p.ldch + 4 * phh) * 2;
        static_for<32>([&](auto S_) {
          constexpr int s = decltype(S_)::value;
          const v4u32_t w = __builtin_bit_cast(v4u32_t, xf[s]);
          __builtin_amdgcn_raw_buffer_store_b64(v2u32_t{w[0], w[1]}, rs_xh, h_off + 32 * s, 0, 16);
          __builtin_amdgcn_raw_buffer_store_b64(v2u32_t{w[2], w[3]}, rs_xh, h_off + 32 * s + 16, 0, 16);
        });
      }
      // x is VALU-written: its converts are done, and a wait-state run passes, before the prologue's
      // asm MFMAs read it
#pragma unroll
      for (int s = 0; s < 32; ++s) asm volatile("" : "+v"(xf[s]));
      asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
      // every wave is done with the Wp slots before the chunk loop's first W2 DMA: that DMA follows
      // the prologue's barrier
    }

    // bias quad q of chunk c: hidden rows 32 c + 8 q + 4 hh + 0..3 (accumulator registers 4q..4q+3)
    auto bias4 = [&](int c, int q) { return *reinterpret_cast<const f32x4*>(b1s + c * FFN_HC + 8 * q + 4 * hh); };
    // the bias tile of chunk c (FFN_BIAS_ACC: an in-projection chain's initial accumulator)
    auto bias_tile = [&](int c) {
      const f32x4 q0 = bias4(c, 0), q1 = bias4(c, 1), q2 = bias4(c, 2), q3 = bias4(c, 3);
      return f32x16{q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3],
                    q2[0], q2[1], q2[2], q2[3], q3[0], q3[1], q3[2], q3[3]};
    };
    // prologue: H^T chunk ca
    f32x16 h0, h1;
#if FFN_BIAS_ACC
    h0 = bias_tile(ca);
    h1 = bias_tile(ca + 1);
#endif
    {
      bf16x8 f[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) f[q] = w1f(0, q);
      static_for<32>([&](auto S_) {
        constexpr int s = decltype(S_)::value;
        if constexpr (s == 0 && !FFN_BIAS_ACC) ffn_mma_v0(h0, f[0], xf[0]);
        else ffn_mma_v(h0, f[s & 3], xf[s]);
        if constexpr (s + 4 < 32) f[s & 3] = w1f(0, s + 4);
      });
    }
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(h0));
    __builtin_amdgcn_s_barrier();        // every wave is done with W1 slot 0 (chunk ca + 2 lands there)

    auto sync = [&]() {
#if FFN_TIMING
      const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#endif
      wait_vmcnt<0>();                   // this wave's DMA pieces landed
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#if FFN_TIMING
      const unsigned long long ts1 = __builtin_amdgcn_s_memtime();
#endif
      __builtin_amdgcn_s_barrier();      // ... everyone's, and everyone is done with the slots
#if FFN_TIMING
      const unsigned long long ts2 = __builtin_amdgcn_s_memtime();
      tm_vm += ts1 - ts0;
      tm_bar += ts2 - ts1;
      ++tm_steps;
#endif
      // the loop exit is where hipcc re-homes the output tiles between AGPRs, reading the last
      // chunk's asm-MFMA results: 20 wait states here (~20 cycles a chunk)
      asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
    };
    // the W1 chunk step c (its DMA into slot c & 1) fetches: c + 2 of this item, else the next
    // item's first two (uniform selects: the loop stays branch-free)
    auto w1_next = [&](int c) { return c + 2 <= cb - 1 ? c + 2 : (c + 2 == cb ? nxt_c0 : nxt_c1); };

    // iteration ca (peeled: no out-projection yet): SwooshL of chunk ca under the in-projection
    // of chunk ca + 1, two activation sub-ops per MFMA
    bf16x8 hb0[2], hb1[2];
    {
      const int c1 = w1_next(ca);
      dma(p.W1f, c1, 0, 0); dma(p.W1f, c1, 0, 1);
      dma(p.W2f, ca, 2, 0); dma(p.W2f, ca, 2, 1);
      f32x4 bq = FFN_BIAS_ACC ? f32x4{} : bias4(ca, 0);
      FfnAct a{};
      bf16x8 f[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) f[q] = w1f(1, q);
      static_for<32>([&](auto S_) {
        constexpr int s = decltype(S_)::value, rr = s >> 1;
        if constexpr (s == 0 && !FFN_BIAS_ACC) ffn_mma_v0(h1, f[0], xf[0]);
        else ffn_mma_v(h1, f[s & 3], xf[s]);
        if constexpr (s + 4 < 32) f[s & 3] = w1f(1, s + 4);
        if constexpr ((rr & 3) == 0 && (s & 1) == 0 && !FFN_BIAS_ACC) bq = bias4(ca, rr >> 2);
        float y = h0[rr];
        ffn_act_op(2 * (s & 1), y, a, bq[rr & 3], c0, cq);
        ffn_act_op(2 * (s & 1) + 1, y, a, bq[rr & 3], c0, cq);
        h0[rr] = y;
        if constexpr (s & 1) put(hb0, rr, y);
      });
#if FFN_BIAS_ACC
      h0 = bias_tile(min(ca + 2, nc));       // step ca + 1's in-projection (chunk ca + 2) starts from it
#endif
      asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(h1));
      sync();
      asm volatile("" ::"v"(f[0]), "v"(f[1]), "v"(f[2]), "v"(f[3]));
    }

    // the epilogue's row operands (resid, and the bypass original where the epilogue mixes it in
    // per group): its first PD groups are loaded during the last chunk's out-projection
    const int m = t0 + tl;
    const bool row_ok = m < S.M;
    const long mr = min(m, S.M - 1);
    const float* rrow = S.resid + mr * p.ldc;
    const float* orow = (ORIG || NORM) ? S.orig + mr * p.ldc : nullptr;
    constexpr bool OPRE = ORIG && !NORM;   // NORM reads the original in its second pass
    // (j, half) groups whose operands are in flight: the x registers are dead from the last
    // in-projection on, so the epilogue may hold FFN_PD groups of 8 fp32 per lane in flight
    constexpr int PD = NORM ? FFN_PD_NORM : OPRE ? FFN_PD_OPRE : FFN_PD;
    f32x4 rr[32][2], ro[OPRE ? 32 : 1][2];
    auto prefetch = [&](int g) {
      if (g < 32) {
        const int n = 16 * g + 8 * hh;     // g = 2 j + pp: outputs 32 j + 16 pp + 8 hh .. + 7
        if constexpr (!PRE) {   // (PRE: the residual is in the tiles already)
          rr[g][0] = *reinterpret_cast<const f32x4*>(rrow + n);
          rr[g][1] = *reinterpret_cast<const f32x4*>(rrow + n + 4);
        }
        if constexpr (OPRE) {
          ro[g][0] = *reinterpret_cast<const f32x4*>(orow + n);
          ro[g][1] = *reinterpret_cast<const f32x4*>(orow + n + 4);
        }
      }
    };

    // the transposed epilogue's operands (FFN_EPI_T, plain epilogue only): k = 16 pass + i holds rows
    // 2 i + (lane >> 5), outputs 128 pass + 4 (lane & 31) .. + 3 of this wave's 32 rows
    // Addressing: buffer resources over the wave's own rows (range = its rows below M), so rows past
    // M read 0 and their stores are dropped by the hardware range check: one per-lane offset VGPR,
    // the row pair in a per-load add, the pass in the instruction offset
    constexpr bool EPT = FFN_EPI_T && TP && !NORM && ABL != 3;
    // (NORM: the transposed BiasNorm epilogue; the row vector's rows staged in LDS, TP's condition)
    constexpr bool EPN = FFN_EPI_NT && TP && NORM && NLDS && ABL != 3 && !split_out;
    constexpr bool TORIG = EPT && ORIG;                  // the bypass original on the coalesced layout
    constexpr int PT = NORM ? FFN_PT_NORM : FFN_PT;
    // (lane through an opaque copy: the epilogue's lane-invariant LDS / row offsets hoisted out of
    // the item loop took ~50 VGPRs for the whole launch and spilled)
    int lve = lane;
    asm volatile("" : "+v"(lve));
    const int lr = lve >> 5, lc = lve & 31, ltl = lve & 31, lhh = lve >> 5;
    const int wrows = max(0, min(32, S.M - t0));           // the wave's rows below M
    // (EPN: one operand stream over both passes, the residual's 64 pieces then the original's)
    f32x4 tq[EPT ? 64 : EPN ? 128 : 1], to[TORIG ? 64 : 1];
    const __amdgpu_buffer_rsrc_t rs_r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(S.resid + (long)t0 * p.ldc), 0, wrows * (int)p.ldc * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(
        (TORIG || EPN) ? const_cast<float*>(S.orig + (long)t0 * p.ldc) : p.sink, 0,
        (TORIG || EPN) ? wrows * (int)p.ldc * 4 : 0, 0x00020000);
    const int toff = (lr * (int)p.ldc + 4 * lc) * 4, tstep = 2 * (int)p.ldc * 4;
    // the transposed epilogues' per-pass constant vectors (b2, the bypass scale, the row vector's two
    // groups), loaded for all 4 passes before the operand prefetch stream starts: the loads of a
    // wave retire in order, so a constant loaded at a pass start made its first use wait for every
    // prefetch issued before it (one pipeline drain per pass)
    const bool has_rv = EPT && RV;
    const bool rv_two = has_rv && p.rows_per_group >= 32;   // a wave's rows span <= 2 row groups
    const int rv_g0 = has_rv ? min(t0, S.M - 1) / p.rows_per_group : 0;
    const int rv_g1 = has_rv ? min(rv_g0 + 1, (S.M - 1) / p.rows_per_group) : 0;
    const int rv_bnd = has_rv ? (rv_g0 + 1) * p.rows_per_group - t0 : 0;   // first wave row of group g1
    // (hoisted for the plain epilogues without the bypass original: with it, the extra 32 VGPRs spill)
    constexpr bool TCONST = EPT && !ORIG;
    f32x4 cb2[TCONST ? 4 : 1], cby[TCONST ? 4 : 1], crv0[TCONST ? 4 : 1], crv1[TCONST ? 4 : 1];
    auto load_consts = [&]() {
      if constexpr (TCONST) {
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          const int col = ps * 128 + 4 * lc;
          if constexpr (EPT) cb2[ps] = *reinterpret_cast<const f32x4*>(p.b2 + col);
          if constexpr (TORIG) cby[ps] = *reinterpret_cast<const f32x4*>(p.byp + col);
          if (rv_two) {
            crv0[ps] = *reinterpret_cast<const f32x4*>(S.rowvec + (long)rv_g0 * p.rowvec_ld + col);
            crv1[ps] = *reinterpret_cast<const f32x4*>(S.rowvec + (long)rv_g1 * p.rowvec_ld + col);
          }
        }
      }
    };
    auto tprefetch = [&](int k) {
      if constexpr (EPN) {
        if (k < 128 && !(PRE && k < 64)) {
          // (the row pair and the pass in the scalar offset: per-piece VGPR offsets, kept for
          // pass 2's stores, spilled)
          int so = (k & 15) * tstep;
          asm volatile("" : "+s"(so));   // (recomputed per piece, not CSE'd across the passes)
          tq[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
              k < 64 ? rs_r : rs_o, toff, so + ((k >> 4) & 3) * 512, 0));
        }
      }
      if constexpr (EPT) {
        if (k < 64) {
          const int off = toff + (k & 15) * tstep + (k >> 4) * 512;
          if constexpr (!PRE) tq[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_r, off, 0, 0));
          if constexpr (ORIG) to[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_o, off, 0, 0));
        }
      }
    };

    // iteration c > ca: 64 MFMA slots; even slot 2i: in-projection step i of chunk c + 1 (W1 slot
    // (c + 1) & 1); odd slot 2i + 1: out-projection MFMA i of chunk c - 1 (tile i >> 1, step i & 1;
    // W2 slot (c - 1) & 1); activation element r of chunk c in slots 4r .. 4r + 3.
    // MODE: 0 the full step; 1 (c = cb - 1) no in-projection (chunk cb is not this item's); 2
    // (c = cb) the out-projection of the last chunk only, with the epilogue's first loads issued
    // ahead of it and no closing barrier (the epilogue does not touch LDS)
    // (PAR = c & 1 at compile time: every slot index, and so every fragment's LDS address, is an
    // immediate offset from two base registers instead of a v_add_u32 per read)
    auto step = [&](auto MODE_, auto PAR_, int c, f32x16& cur, f32x16& nxt, bf16x8 (&hbw)[2], const bf16x8 (&hbr)[2]) {
      constexpr int MODE = decltype(MODE_)::value, PAR = decltype(PAR_)::value;
      constexpr int s1 = (PAR + 1) & 1, s2 = (PAR + 1) & 1;
      const int c1 = w1_next(c);
      if constexpr (MODE == 2) {
        if constexpr ((EPT || EPN) && !split_out) {
          load_consts();
#pragma unroll
          for (int k = 0; k < PT; ++k) tprefetch((PRE && EPN) ? 64 + k : k);   // (PRE: the original only)
        } else {
#pragma unroll
          for (int g = 0; g < PD; ++g) prefetch(g);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (MODE == 0) fa[q] = w1f(s1, q);
        fb[q] = w2f(s2, q);
      }
      f32x4 bq = FFN_BIAS_ACC ? f32x4{} : bias4(c, 0);
      FfnAct a{};
      float y = 0.f;
      static_for<64>([&](auto K_) {     // fully unrolled: every register index a constant
        constexpr int k = decltype(K_)::value, i = k >> 1;
        if constexpr ((k & 1) == 0) {
          if constexpr (MODE == 0) {
            if constexpr (i == 0 && !FFN_BIAS_ACC) ffn_mma_v0(nxt, fa[0], xf[0]);
            else ffn_mma_v(nxt, fa[i & 3], xf[i]);
            if constexpr (i + 4 < 32 && !FFN_X_NOW1) fa[i & 3] = w1f(s1, i + 4);
          }
        } else {
          ffn_mma_a(out[i >> 1], fb[i & 3], hbr[i & 1]);
          if constexpr (i + 4 < 32 && !FFN_X_NOW2) fb[i & 3] = w2f(s2, i + 4);
        }
        if constexpr (ABL != 1 && MODE <= 1) {
          if constexpr (k == FFN_DMA_K0) dma(p.W1f, c1, PAR, 0);
          if constexpr (k == FFN_DMA_K1) dma(p.W1f, c1, PAR, 1);
          if constexpr (k == FFN_DMA_K2) dma(p.W2f, c, 2 + PAR, 0);
          if constexpr (k == FFN_DMA_K3) dma(p.W2f, c, 2 + PAR, 1);
        }
        if constexpr (MODE <= 1) {
          constexpr int rg = k >> 2, sub = k & 3;
          if constexpr (sub == 0) {
            if constexpr ((rg & 3) == 0 && !FFN_BIAS_ACC) bq = bias4(c, rg >> 2);
            y = cur[rg];
          }
          if constexpr (!FFN_X_NOACT) ffn_act_op(sub, y, a, bq[rg & 3], c0, cq);
          if constexpr (sub == 3) put(hbw, rg, y);
        }
      });
#if FFN_BIAS_ACC
      // cur is activated (its last pair converted at k = 63): it becomes step c + 1's in-projection
      // tile (chunk c + 2); the reads land under the closing barrier
      if constexpr (MODE == 0) {
        asm volatile("" ::"v"(hbw[0]), "v"(hbw[1]));   // the activated pairs are converted first
        cur = bias_tile(c + 2);
      }
#endif
      if constexpr (MODE <= 1) sync();
      // WAR: an MFMA reads its A/B registers during its passes, after the asm statement has
      // "consumed" them -- left alone, hipcc gave the next chunk's activation (VALU) the registers
      // of this chunk's B fragments right behind their last MFMAs.  Their lifetimes end here,
      // behind the barrier and its s_nop run (the last step: behind the s_nop run below).
      if constexpr (MODE == 0)
        asm volatile("" ::"v"(hbr[0]), "v"(hbr[1]), "v"(fa[0]), "v"(fa[1]), "v"(fa[2]), "v"(fa[3]),
                     "v"(fb[0]), "v"(fb[1]), "v"(fb[2]), "v"(fb[3]));
      else
        asm volatile("" ::"v"(hbr[0]), "v"(hbr[1]), "v"(fb[0]), "v"(fb[1]), "v"(fb[2]), "v"(fb[3]));
    };
    using M0 = std::integral_constant<int, 0>;
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
#if FFN_TIMING
    const unsigned long long tl0 = __builtin_amdgcn_s_memtime();
#endif
    for (int c = ca + 1; c <= cb - 3; c += 2) {
      step(M0{}, P1{}, c, h1, h0, hb1, hb0);        // c - ca odd, ca even: c odd
      step(M0{}, P0{}, c + 1, h0, h1, hb0, hb1);
    }
#if FFN_TIMING
    tm_loop += __builtin_amdgcn_s_memtime() - tl0;
#endif
    step(std::integral_constant<int, 1>{}, P1{}, cb - 1, h1, h0, hb1, hb0);
    step(std::integral_constant<int, 2>{}, P0{}, cb, h0, h1, hb0, hb1);
    // MFMA result -> VALU / accvgpr read: 18 wait states (also behind the last sync's run)
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
#if FFN_TIMING
    const unsigned long long te0 = __builtin_amdgcn_s_memtime();
#endif

    // the range's output bases once per item (read inside the groups, each of the 32 groups got
    // two scalar loads and their waits): NORM keeps them in SGPRs, the plain epilogue as per-lane
    // row addresses (rows past M store to the sink: a per-lane stride of 0 keeps them there); each
    // form the one that does not spill its variant
    float* Cp = S.C;
    bf16* Chp = S.Ch;
    if constexpr (NORM) asm volatile("" : "+s"(Cp), "+s"(Chp));
    const unsigned long long c_base = row_ok ? (unsigned long long)(Cp + (long)m * p.ldc) : (unsigned long long)(p.sink + lane * 8);
    const unsigned c_mul = row_ok ? 4u : 0u;
    const unsigned long long h_base = (COPY && row_ok) ? (unsigned long long)(Chp + (long)m * p.ldch)
                                                       : (unsigned long long)(p.sink + 512 + lane * 4);
    const unsigned h_mul = (COPY && row_ok) ? 2u : 0u;
    if constexpr (ABL == 3 && !split_out) {
#pragma unroll
      for (int j = 0; j < 16; ++j) asm volatile("" : "+a"(out[j]));
    } else if constexpr (split_out) {
      // ---- P item: the raw tiles to this line's slot, write-through; then the flag
      int lv = lane;
      asm volatile("" : "+v"(lv));          // (not hoisted out of the item loop, as above)
      const int base = (wave * 4096 + lv) * 16;
#pragma unroll
      for (int j = 0; j < 16; ++j) asm volatile("" : "+a"(out[j]));
      static_for<16>([&](auto J_) {
        constexpr int j = decltype(J_)::value;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v = {out[j][4 * q], out[j][4 * q + 1], out[j][4 * q + 2], out[j][4 * q + 3]};
          __builtin_amdgcn_raw_buffer_store_b128(v, part_rs, base + (j * 4 + q) * 1024,
                                                 (int)(blockIdx.x * FFN_PART_FLOATS * 4), 16);
        }
        __builtin_amdgcn_sched_barrier(0);
      });
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains
      __syncthreads();
      if (tid == 0) {
        unsigned long long fa = (unsigned long long)(p.flag + blockIdx.x);
        asm volatile("" : "+v"(fa));   // a vector store (sc1), never through the scalar path
        __hip_atomic_store((GLOBAL unsigned*)fa, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else if constexpr (EPN) {
      // ---- FF3 + BiasNorm + bypass, transposed (FFN_EPI_NT, see the header of the switch)
      __builtin_amdgcn_s_barrier();        // every wave's last W2 fragment read is done
      float* tb = reinterpret_cast<float*>(smem + 2 * FFN_SLOT) + wave * 4096;
      float ssr[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) ssr[i] = 0.f;
      static_for<4>([&](auto P_) {
        constexpr int ps = decltype(P_)::value;
        static_for<4>([&](auto J_) {
          constexpr int jj = decltype(J_)::value, j = 4 * ps + jj;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int ch = (8 * jj + 2 * q + lhh) ^ (ltl & 7);
            *reinterpret_cast<f32x4*>(tb + ltl * 128 + ch * 4) =
                f32x4{out[j][4 * q], out[j][4 * q + 1], out[j][4 * q + 2], out[j][4 * q + 3]};
          }
        });
        __builtin_amdgcn_sched_barrier(0);
        // (per-pass opaque copies of the lane's row / column: the per-piece LDS addresses, CSE'd
        // over the passes, stayed live through both passes and spilled)
        int plr = lr, plc = lc;
        asm volatile("" : "+v"(plr), "+v"(plc));
        const int col = ps * 128 + 4 * plc;
        const f32x4 bb = *reinterpret_cast<const f32x4*>(ncs + col);
        const f32x4 nbv = *reinterpret_cast<const f32x4*>(ncs + FFN_D + col);
        static_for<16>([&](auto I_) {
          constexpr int i = decltype(I_)::value, k = 16 * ps + i;
          if constexpr (!PRE) tprefetch(k + PT);
          const int row = 2 * i + plr;
          const f32x4 a = *reinterpret_cast<const f32x4*>(tb + row * 128 + ((plc ^ (row & 7)) * 4));
          // x = resid + (acc + b2) into the freed accumulators: tile 4 ps + i / 4, registers 4 (i % 4) ..
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = PRE ? a[e] + bb[e] : tq[k][e] + (a[e] + bb[e]);
            const float d = x - nbv[e];
            // (PRE: explicit fused multiply-adds.  Left to contraction, an item kind's instantiation
            // may sum d * d as packed multiplies and adds where another fuses them, and a cut row
            // block's C item then differs from the whole row block in the last bit of a row's scale)
            if constexpr (PRE) ssr[i] = __builtin_fmaf(d, d, ssr[i]);
            else ssr[i] += d * d;
            out[4 * ps + (i >> 2)][4 * (i & 3) + e] = x;
          }
          if constexpr ((i & 3) == 3) asm volatile("" : "+a"(out[4 * ps + (i >> 2)]));
          __builtin_amdgcn_sched_barrier(0);
        });
      });
      // each row's sum over its half-wave (row 2 i + lr: lanes lc = 0..31); partners add the same
      // two values, so every lane ends with the same sum
#pragma unroll
      for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) ssr[i] += __shfl_xor(ssr[i], o, 64);
        ssr[i] = rsqrtf(ssr[i] / (float)FFN_D) * p.norm_scale;
      }
      // the outputs: row pieces at the transposed layout's offsets (rows past M dropped by range)
      auto rsrc = [&](void* base, long ld, int esz) {
        return __builtin_amdgcn_make_buffer_rsrc(base ? base : (void*)p.sink, 0, base ? wrows * (int)ld * esz : 0, 0x00020000);
      };
      bf16* Clp = S.Cl;
      bf16* C2hp = S.C2h;
      bf16* C2lp = S.C2l;
      asm volatile("" : "+s"(Clp), "+s"(C2hp), "+s"(C2lp));
      const __amdgpu_buffer_rsrc_t rs_c = rsrc(Cp + (long)t0 * p.ldc, p.ldc, 4);
      const __amdgpu_buffer_rsrc_t rs_h = rsrc(Chp + (long)t0 * p.ldch, p.ldch, 2);
      const __amdgpu_buffer_rsrc_t rs_l = rsrc(Clp ? Clp + (long)t0 * p.ldch : nullptr, p.ldch, 2);
      const __amdgpu_buffer_rsrc_t rs_2h = rsrc(C2hp ? C2hp + (long)t0 * p.ldch : nullptr, p.ldch, 2);
      const __amdgpu_buffer_rsrc_t rs_2l = rsrc(C2lp ? C2lp + (long)t0 * p.ldch : nullptr, p.ldch, 2);
      const int hoff = (lr * (int)p.ldch + 4 * lc) * 2, hstep = 2 * (int)p.ldch * 2;
      // the next layer's copy adds the row vector (the wave's two row groups, staged in LDS)
      const int rv_b = nrv ? (nrv_g0 + 1) * p.rows_per_group - t0 : 1 << 30;   // first row of the second group
      static_for<4>([&](auto P_) {
        constexpr int ps = decltype(P_)::value;
        int plr = lr, plc = lc;
        asm volatile("" : "+v"(plr), "+v"(plc));
        const int col = ps * 128 + 4 * plc;
        const f32x4 byv = *reinterpret_cast<const f32x4*>(ncs + 2 * FFN_D + col);
        f32x4 w0{}, w1{};
        if (nrv) {
          w0 = *reinterpret_cast<const f32x4*>(ncs + 3 * FFN_D + wave * 2 * FFN_D + col);
          w1 = *reinterpret_cast<const f32x4*>(ncs + 3 * FFN_D + wave * 2 * FFN_D + FFN_D + col);
        }
        static_for<16>([&](auto I_) {
          constexpr int i = decltype(I_)::value, k = 16 * ps + i;
          tprefetch(64 + k + PT);
          const int row = 2 * i + plr;
          f32x4 y;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float o = tq[64 + k][e];
            if constexpr (PRE) y[e] = __builtin_fmaf(__builtin_fmaf(out[4 * ps + (i >> 2)][4 * (i & 3) + e], ssr[i], -o), byv[e], o);
            else y[e] = o + (out[4 * ps + (i >> 2)][4 * (i & 3) + e] * ssr[i] - o) * byv[e];
          }
          int fo = i * tstep, ho = i * hstep;   // (scalar offsets, per piece as above)
          asm volatile("" : "+s"(fo), "+s"(ho));
          fo += ps * 512;
          ho += ps * 256;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32_t, y), rs_c, toff, fo, 0);
          bf16x4 h, l;
#pragma unroll
          for (int e = 0; e < 4; ++e) h[e] = (bf16)y[e];
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32_t, h), rs_h, hoff, ho, 0);
          if (Clp) {
#pragma unroll
            for (int e = 0; e < 4; ++e) l[e] = (bf16)(y[e] - (float)h[e]);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32_t, l), rs_l, hoff, ho, 0);
          }
          if (C2hp) {
            if (nrv) {
              const bool second = row >= rv_b;
#pragma unroll
              for (int e = 0; e < 4; ++e) y[e] += second ? w1[e] : w0[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (bf16)y[e];
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32_t, h), rs_2h, hoff, ho, 0);
            if (C2lp) {
#pragma unroll
              for (int e = 0; e < 4; ++e) l[e] = (bf16)(y[e] - (float)h[e]);
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32_t, l), rs_2l, hoff, ho, 0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);   // (the loads stay PT ahead, not hoisted en bloc)
        });
      });
    } else if constexpr (NORM) {
      // ---- FF3 + BiasNorm + bypass: rows are whole per lane pair (lane, lane ^ 32): pass 1 forms
      // x = resid + (acc + b2) in place (in the swapped register order) and the row's sum of
      // squares; pass 2 writes the normalised, bypassed row
      float ss = 0.f;
      f32x4 rq[32][2];
      auto pre_o = [&](int g) {
        if (g < 32) {
          const int n = 16 * g + 8 * hh;
          rq[g][0] = *reinterpret_cast<const f32x4*>(orow + n);
          rq[g][1] = *reinterpret_cast<const f32x4*>(orow + n + 4);
        }
      };
      static_for<32>([&](auto G_) {
        constexpr int g = decltype(G_)::value, j = g >> 1, pp = g & 1;
        // one pipeline over both passes: past the residual's last group, pass 2's original
        if constexpr (g + PD < 32) prefetch(g + PD);
        else pre_o(g + PD - 32);
        const int n = 16 * g + 8 * hh;
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(out[j][8 * pp + e]),
                                                           __float_as_uint(out[j][8 * pp + 4 + e]), false, false);
          v[e] = __uint_as_float(sw[0]);
          v[4 + e] = __uint_as_float(sw[1]);
        }
        const float* b2c = NLDS ? ncs : p.b2;
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(b2c + n);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(b2c + n + 4);
        const float* nbc = NLDS ? ncs + FFN_D : p.nb;
        const f32x4 n0 = *reinterpret_cast<const f32x4*>(nbc + n);
        const f32x4 n1 = *reinterpret_cast<const f32x4*>(nbc + n + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = PRE ? v[e] + b0[e] : rr[g][0][e] + (v[e] + b0[e]);
          v[4 + e] = PRE ? v[4 + e] + b1[e] : rr[g][1][e] + (v[4 + e] + b1[e]);
          const float d0 = v[e] - n0[e], d1 = v[4 + e] - n1[e];
          if constexpr (PRE) ss = __builtin_fmaf(d1, d1, __builtin_fmaf(d0, d0, ss));
          else ss += d0 * d0 + d1 * d1;
          out[j][8 * pp + e] = v[e];
          out[j][8 * pp + 4 + e] = v[4 + e];
        }
      });
      ss += __shfl_xor(ss, 32, 64);
      const float scale = rsqrtf(ss / (float)FFN_D) * p.norm_scale;
      const float* vrow = (S.rowvec && !nrv) ? S.rowvec + (mr / p.rows_per_group) * p.rowvec_ld : nullptr;
      // (FFN_NORM_LDS) this lane's token's row vector among the wave's two staged rows
      const int vl_off = 3 * FFN_D + wave * 2 * FFN_D + ((t0 + tl >= (nrv_g0 + 1) * p.rows_per_group) ? FFN_D : 0);
      // the optional outputs' bases in SGPRs once (uniform), per-lane row offsets
      bf16* Clp = S.Cl;
      bf16* C2hp = S.C2h;
      bf16* C2lp = S.C2l;
      asm volatile("" : "+s"(Clp), "+s"(C2hp), "+s"(C2lp));
      // (a 16-bit output's per-lane address: the row's, or the sink's for rows past M)
      auto adr16 = [&](bf16* base, long oh) {
        unsigned long long a = row_ok ? (unsigned long long)(base + oh) : (unsigned long long)(p.sink + 512 + lane * 4);
        asm volatile("" : "+v"(a));
        return (GLOBAL bf16x8*)a;
      };
      auto adr32 = [&](float* base, long o) {
        unsigned long long a = row_ok ? (unsigned long long)(base + o) : (unsigned long long)(p.sink + lane * 8);
        asm volatile("" : "+v"(a));
        return (GLOBAL f32x4*)a;
      };
      static_for<32>([&](auto G_) {
        constexpr int g = decltype(G_)::value, j = g >> 1, pp = g & 1;
        pre_o(g + PD);
        const int n = 16 * g + 8 * hh;
        const float* byc = NLDS ? ncs + 2 * FFN_D : p.byp;
        const f32x4 c0v = *reinterpret_cast<const f32x4*>(byc + n);
        const f32x4 c1v = *reinterpret_cast<const f32x4*>(byc + n + 4);
        float y[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (PRE) {
            y[e] = __builtin_fmaf(__builtin_fmaf(out[j][8 * pp + e], scale, -rq[g][0][e]), c0v[e], rq[g][0][e]);
            y[4 + e] = __builtin_fmaf(__builtin_fmaf(out[j][8 * pp + 4 + e], scale, -rq[g][1][e]), c1v[e], rq[g][1][e]);
          } else {
            y[e] = rq[g][0][e] + (out[j][8 * pp + e] * scale - rq[g][0][e]) * c0v[e];
            y[4 + e] = rq[g][1][e] + (out[j][8 * pp + 4 + e] * scale - rq[g][1][e]) * c1v[e];
          }
        }
        const long o = (long)m * p.ldc + n, oh = (long)m * p.ldch + n;
        GLOBAL f32x4* ca = adr32(Cp, o);
        ca[0] = f32x4{y[0], y[1], y[2], y[3]};
        ca[1] = f32x4{y[4], y[5], y[6], y[7]};
        bf16x8 h, l;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (bf16)y[e];
        *adr16(Chp, oh) = h;
        if (Clp) {
#pragma unroll
          for (int e = 0; e < 8; ++e) l[e] = (bf16)(y[e] - (float)h[e]);
          if (row_ok) *reinterpret_cast<bf16x8*>(Clp + oh) = l;
        }
        if (C2hp) {
          if (nrv) {
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(ncs + vl_off + n);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(ncs + vl_off + n + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { y[e] += w0[e]; y[4 + e] += w1[e]; }
          } else if (vrow) {
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(vrow + n);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(vrow + n + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { y[e] += w0[e]; y[4 + e] += w1[e]; }
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) { h[e] = (bf16)y[e]; l[e] = (bf16)(y[e] - (float)h[e]); }
          if (row_ok) {
            *reinterpret_cast<bf16x8*>(C2hp + oh) = h;
            if (C2lp) *reinterpret_cast<bf16x8*>(C2lp + oh) = l;
          }
        }
      });
    } else if constexpr (EPT) {
      // ---- transposed epilogue (FFN_EPI_T, see the header of the switch)
      __builtin_amdgcn_s_barrier();        // every wave's last W2 fragment read is done
      float* tb = reinterpret_cast<float*>(smem + 2 * FFN_SLOT) + wave * 4096;
      const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc(Cp + (long)t0 * p.ldc, 0, wrows * (int)p.ldc * 4, 0x00020000);
      const __amdgpu_buffer_rsrc_t rs_h =
          __builtin_amdgcn_make_buffer_rsrc(COPY ? (void*)(Chp + (long)t0 * p.ldch) : (void*)p.sink, 0, COPY ? wrows * (int)p.ldch * 2 : 0, 0x00020000);
      const int hoff = (lr * (int)p.ldch + 4 * lc) * 2, hstep = 2 * (int)p.ldch * 2;
      static_for<4>([&](auto P_) {
        constexpr int ps = decltype(P_)::value;
        // tiles 4 ps .. 4 ps + 3: register 4 q + e of tile j is output 32 j + 8 q + 4 hh + e of
        // token tl -> row tl, 16-B chunk (8 (j - 4 ps) + 2 q + hh) ^ (tl & 7)
        static_for<4>([&](auto J_) {
          constexpr int jj = decltype(J_)::value, j = 4 * ps + jj;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int ch = (8 * jj + 2 * q + lhh) ^ (ltl & 7);
            *reinterpret_cast<f32x4*>(tb + ltl * 128 + ch * 4) =
                f32x4{out[j][4 * q], out[j][4 * q + 1], out[j][4 * q + 2], out[j][4 * q + 3]};
          }
        });
        __builtin_amdgcn_sched_barrier(0);
        const int col = ps * 128 + 4 * lc;
        f32x4 bb, sc4{};
        if constexpr (TCONST) bb = cb2[ps];
        else {
          bb = *reinterpret_cast<const f32x4*>(p.b2 + col);
          if constexpr (ORIG) sc4 = *reinterpret_cast<const f32x4*>(p.byp + col);
        }
        // the row vector: both row groups' vectors per pass (load_consts), a select per row;
        // groups shorter than a wave take the per-row division
        const f32x4 rv0 = crv0[ps], rv1 = crv1[ps];
        static_for<16>([&](auto I_) {
          constexpr int i = decltype(I_)::value, k = 16 * ps + i;
          tprefetch(k + PT);
          const int row = 2 * i + lr;
          const f32x4 a = *reinterpret_cast<const f32x4*>(tb + row * 128 + ((lc ^ (row & 7)) * 4));
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = PRE ? a[e] + bb[e] : tq[k][e] + (a[e] + bb[e]);
          const int mrow = t0 + row;
          if constexpr (RV) {
            // (groups of >= 32 rows, the launcher's condition for TP: two per wave at most)
            const bool second = row >= rv_bnd;
            f32x4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = second ? rv1[e] : rv0[e];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += w[e];
          }
          if constexpr (ORIG) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              v[e] = PRE ? __builtin_fmaf(v[e] - to[k][e], sc4[e], to[k][e]) : to[k][e] + (v[e] - to[k][e]) * sc4[e];
          }
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32_t, v), rs_c, toff + i * tstep + ps * 512, 0, 0);
          if constexpr (COPY) {
            bf16x4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (bf16)v[e];
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32_t, h), rs_h, hoff + i * hstep + ps * 256, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);   // (the loads stay PT ahead, not hoisted en bloc)
        });
      });
    } else {
      // ---- epilogue: out[j] register r = output 32 j + (r & 3) + 8 (r >> 2) + 4 hh of token t0 + tl
      const float* vrow = RV ? S.rowvec + (mr / p.rows_per_group) * p.rowvec_ld : nullptr;
      static_for<32>([&](auto G_) {
        constexpr int g = decltype(G_)::value, j = g >> 1, pp = g & 1;
        prefetch(g + PD);
        const int n = 16 * g + 8 * hh;
        // registers 8 pp + e (rows 16 pp + 4 hh + e) and 8 pp + 4 + e (16 pp + 8 + 4 hh + e):
        // after the swap the lower half holds rows 16 pp + 0..7, the upper 16 pp + 8..15
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(out[j][8 * pp + e]),
                                                           __float_as_uint(out[j][8 * pp + 4 + e]), false, false);
          v[e] = __uint_as_float(sw[0]);
          v[4 + e] = __uint_as_float(sw[1]);
        }
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.b2 + n);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.b2 + n + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = PRE ? v[e] + b0[e] : rr[g][0][e] + (v[e] + b0[e]);
          v[4 + e] = PRE ? v[4 + e] + b1[e] : rr[g][1][e] + (v[4 + e] + b1[e]);
        }
        if constexpr (RV) {
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(vrow + n);
          const f32x4 w1 = *reinterpret_cast<const f32x4*>(vrow + n + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] += w0[e]; v[4 + e] += w1[e]; }
        }
        if constexpr (ORIG) {
          const f32x4 s0 = *reinterpret_cast<const f32x4*>(p.byp + n);
          const f32x4 s1 = *reinterpret_cast<const f32x4*>(p.byp + n + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = ro[g][0][e] + (v[e] - ro[g][0][e]) * s0[e];
            v[4 + e] = ro[g][1][e] + (v[4 + e] - ro[g][1][e]) * s1[e];
          }
        }
        unsigned long long cadr = c_base + (unsigned long long)(n * c_mul);
        asm volatile("" : "+v"(cadr));
        *(GLOBAL f32x4*)(cadr) = f32x4{v[0], v[1], v[2], v[3]};
        *(GLOBAL f32x4*)(cadr + 16) = f32x4{v[4], v[5], v[6], v[7]};
        if constexpr (COPY) {
          bf16x8 h;
#pragma unroll
          for (int e = 0; e < 8; ++e) h[e] = (bf16)v[e];
          unsigned long long ha2 = h_base + (unsigned long long)(n * h_mul);
          asm volatile("" : "+v"(ha2));
          *(GLOBAL bf16x8*)(ha2) = h;
        }
      });
    }
#if FFN_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    tm_epi += __builtin_amdgcn_s_memtime() - te0;
#endif
  };

  long pos = start;
  for (;;) {
    // the item (r, ca, cb) and the next one's first chunk (its first two W1 chunks are DMA'd in
    // this item's last two steps; the line's last item loads harmless copies of its own last chunk)
    const bool split_in = ca > 0, split_out = cb < nc;
    const long npos = split_out ? (long)(r + 1) * nc : (split_in ? end : pos + nc);
    const bool has_next = npos < end;
    int nr = 0, nca = 0, ncb = 0;
    if (has_next) item_at(npos, nr, nca, ncb);
    if (split_out) item(std::integral_constant<int, 1>{}, r, ca, cb, has_next, nca);
    else if (split_in) item(std::integral_constant<int, 2>{}, r, ca, cb, has_next, nca);
    else item(std::integral_constant<int, 0>{}, r, ca, cb, has_next, nca);
    if (!has_next) break;
    pos = npos; r = nr; ca = nca; cb = ncb;
  }
#if FFN_TIMING
  if (lane == 0) {
    unsigned long long* d = p.dbg + ((long)blockIdx.x * 4 + wave) * FFN_DBG_WORDS;
    d[0] = __builtin_amdgcn_s_memtime() - tm_t0;
    d[1] = __builtin_amdgcn_s_memrealtime() - tm_r0;
    d[2] = tm_vm; d[3] = tm_bar; d[4] = tm_steps; d[5] = (unsigned long long)p.w;
    d[6] = tm_epi; d[7] = tm_x; d[8] = tm_items; d[9] = tm_loop;
  }
#endif
}

// weight packing (once, at load): Linear hi arrays [Npad][Kpad] -> fragment-major
//   W1f[c][s][lane][j] = W1[32 c + (lane & 31)][16 s + 8 (lane >> 5) + j]
//   W2f[c][jb][s][lane][j] = W2[32 jb + (lane & 31)][32 c + 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)]
// (the second: element j of lane half h of k-step s is hidden row 16 s + 8 (j >> 2) + 4 h + (j & 3)
// of the SwooshL tile, the 32x32 accumulator's register order)
static __global__ void zv_ffn_pack_w1_kernel(const bf16* W, long ldw, int H, bf16* out) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)H * FFN_D) return;
  const int j = (int)(i & 7);
  long r = i >> 3;
  const int l = (int)(r & 63); r >>= 6;
  const int s = (int)(r & 31), c = (int)(r >> 5);
  out[i] = W[(long)(32 * c + (l & 31)) * ldw + 16 * s + 8 * (l >> 5) + j];
}
static __global__ void zv_ffn_pack_w2_kernel(const bf16* W, long ldw, int H, bf16* out) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)H * FFN_D) return;
  const int j = (int)(i & 7);
  long r = i >> 3;
  const int l = (int)(r & 63); r >>= 6;
  const int s = (int)(r & 1); r >>= 1;
  const int jb = (int)(r & 15), c = (int)(r >> 4);
  out[i] = W[(long)(32 * jb + (l & 31)) * ldw + 32 * c + 16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)];
}
// the PRE form's packings: W1 with its K in the out^T tile's register order (x is read in place from
// the accumulators), and the pre-projection weight Wp (512, K) in the W2 chunk format with K in natural
// order, zero past K:
//   W1fp[c][s][lane][j] = W1[32 c + (lane & 31)][16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)]
//   Wpf[kc][jb][s][lane][j] = Wp[32 jb + (lane & 31)][32 kc + 16 s + 8 (lane >> 5) + j]
static __global__ void zv_ffn_pack_w1p_kernel(const bf16* W, long ldw, int H, bf16* out) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)H * FFN_D) return;
  const int j = (int)(i & 7);
  long r = i >> 3;
  const int l = (int)(r & 63); r >>= 6;
  const int s = (int)(r & 31), c = (int)(r >> 5);
  out[i] = W[(long)(32 * c + (l & 31)) * ldw + 16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)];
}
static __global__ void zv_ffn_pack_wp_kernel(const bf16* W, long ldw, int K, int nkp, bf16* out) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)nkp * FFN_HC * FFN_D) return;
  const int j = (int)(i & 7);
  long r = i >> 3;
  const int l = (int)(r & 63); r >>= 6;
  const int s = (int)(r & 1); r >>= 1;
  const int jb = (int)(r & 15), kc = (int)(r >> 4);
  const int k = 32 * kc + 16 * s + 8 * (l >> 5) + j;
  out[i] = k < K ? W[(long)(32 * jb + (l & 31)) * ldw + k] : (bf16)0.f;
}
inline int ffn_pre_chunks(int K) { return (K + FFN_HC - 1) / FFN_HC; }
// L1: the FeedForward's in_proj -> w1fp (H * 512); Lp: the pre-projection (512, K) -> wpf (ffn_pre_chunks(K) * 32 * 512)
static void ffn_pack_pre_weights(const Linear& L1, int H, bf16* w1fp, const Linear& Lp, bf16* wpf, hipStream_t s) {
  const long n = (long)H * FFN_D, np = (long)ffn_pre_chunks(Lp.K) * FFN_HC * FFN_D;
  hipLaunchKernelGGL(zv_ffn_pack_w1p_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, L1.hi, (long)L1.Kpad, H, w1fp);
  hipLaunchKernelGGL(zv_ffn_pack_wp_kernel, dim3(cdiv(np, 256)), dim3(256), 0, s, Lp.hi, (long)Lp.Kpad, Lp.K,
                     ffn_pre_chunks(Lp.K), wpf);
  ZV_LAUNCH_CHECK();
}
// both packings of one FeedForward (L1: in_proj (H, 512), L2: out_proj (512, H)) into w1f / w2f, H * 512 each
static void ffn_pack_weights(const Linear& L1, const Linear& L2, int H, bf16* w1f, bf16* w2f, hipStream_t s) {
  const long n = (long)H * FFN_D;
  hipLaunchKernelGGL(zv_ffn_pack_w1_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, L1.hi, (long)L1.Kpad, H, w1f);
  hipLaunchKernelGGL(zv_ffn_pack_w2_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, L2.hi, (long)L2.Kpad, H, w2f);
  ZV_LAUNCH_CHECK();
}

// the persistent schedule of a launch: chunk steps per block (w) and blocks, for R row blocks of
// nc chunks on `blocks_max` CUs.  Lines of w >= nc steps only (a C item must start after its P
// item ends); w even (items of whole chunk pairs); below one row block per CU: one per block
struct FfnSchedule { int w, blocks; };
inline FfnSchedule ffn_schedule(int R, int nc, int blocks_max, bool persistent) {
  if (!persistent || R <= blocks_max) return {nc, R};
  const long W = (long)R * nc;
  long w = (W + blocks_max - 1) / blocks_max;
  w = std::max<long>(round_up(w, 2), nc);
  return {(int)w, (int)((W + w - 1) / w)};
}

template <bool RV, bool ORIG, bool COPY, int ABL = 0, int NORM = 0, bool TP = true, bool PRE = false>
static void launch_ffn_t(const FfnParams& p, int blocks, hipStream_t s, const char* tag) {
  static unsigned long long attr = 0;   // per device
  const size_t lds = ffn_lds_bytes(p.H, NORM != 0);
  if (!((attr >> zv_cur_device()) & 1)) {
    ZV_CHECK(hipFuncSetAttribute((const void*)zv_ffn_kernel<RV, ORIG, COPY, ABL, NORM, TP, PRE>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr |= 1ull << zv_cur_device();
  }
  double M = 0, extra = 0;
  for (int i = 0; i < p.nseg; ++i) {
    const FfnSeg& g = p.seg[i];
    M += g.M;
    if (NORM) extra += (double)g.M * FFN_D * ((g.Cl ? 2 : 0) + (g.C2h ? 2 : 0) + (g.C2l ? 2 : 0));
  }
  const double outs = M * FFN_D;
  // (PRE: no x read; the pre-projection's operand, weight and FLOPs)
  const double Kp = PRE ? (double)p.nkp * FFN_HC : 0.0;
  const double bytes = (PRE ? (M + FFN_D) * Kp * 2 : outs * 2) + 2.0 * FFN_D * p.H * 2 +
                       (NORM ? outs * (4 + 4 + 4 + 2) + extra : outs * (8 + (COPY ? 2 : 0) + (ORIG ? 4 : 0)));
  g_zv_last_launch = ZvLaunchRec{FFN_BM, FFN_D, 1, (int)RV | (int)ORIG << 1 | (int)COPY << 2 | (int)TP << 3 | (int)PRE << 4, NORM,
                                 0, blocks, p.w};
  ZvProfScope prof(tag, 4.0 * M * FFN_D * (double)p.H + 2.0 * M * FFN_D * Kp, bytes, s);
  hipLaunchKernelGGL((zv_ffn_kernel<RV, ORIG, COPY, ABL, NORM, TP, PRE>), dim3(blocks), dim3(256), lds, s, p);
  ZV_LAUNCH_CHECK();
}

// p.seg[0 .. nseg) filled (M, X and the epilogue pointers); rb0, R, the schedule and the sink are
// set here.  part / flag / part_slots: the persistent schedule's scratch (null: one row block per block)
template <int ABL = 0>
static void launch_ffn(FfnParams p, hipStream_t s, const char* tag, int blocks_max = 0) {
  ZV_REQUIRE(p.H > 0 && p.H % (2 * FFN_HC) == 0 && ffn_lds_bytes(p.H, p.nb != nullptr) <= 160 * 1024,
             "fused FeedForward: hidden width a multiple of 64 (LDS: at most 8160, 2496 with the BiasNorm epilogue)");
  ZV_REQUIRE(p.nseg >= 1 && p.nseg <= FFN_MAXSEG, "fused FeedForward: 1..4 row ranges");
  ZV_REQUIRE(p.W1f && p.W2f && p.b1 && p.b2 && (p.Wpf || (p.ldx % 8 == 0 && p.ldx >= FFN_D)) && p.ldc % 4 == 0 &&
                 p.ldc >= FFN_D && (p.ldch == 0 || (p.ldch % 8 == 0 && p.ldch >= FFN_D)),
             "fused FeedForward operands (16-B aligned rows of at least 512)");
  const bool rv = p.seg[0].rowvec != nullptr, og = p.seg[0].orig != nullptr, cp = p.seg[0].Ch != nullptr;
  const bool pre = p.Wpf != nullptr;
  // the pre-projection form: A's columns [K, 32 nkp) are read (the caller keeps them zero), so its
  // rows hold at least 32 nkp elements
  ZV_REQUIRE(!pre || (p.bp && p.nkp >= 1 && p.lda >= (long)p.nkp * FFN_HC && p.lda % 8 == 0 && cp && og),
             "fused FeedForward pre-projection operands (lda >= Kp, 16-B aligned rows, the bypass or BiasNorm site)");
  int R = 0;
  for (int i = 0; i < p.nseg; ++i) {
    FfnSeg& g = p.seg[i];
    ZV_REQUIRE(!pre || g.A, "fused FeedForward pre-projection operand");
    ZV_REQUIRE(g.M > 0 && (g.X || pre) && g.resid && g.C && (g.Ch != nullptr) == cp && (g.rowvec != nullptr) == rv &&
                   (g.orig != nullptr) == og && (!g.Ch || p.ldch > 0),
               "fused FeedForward row range operands");
    g.rb0 = R;
    R += cdiv(g.M, FFN_BM);
  }
  ZV_REQUIRE(og == (p.byp != nullptr) && (!rv || p.rows_per_group > 0), "fused FeedForward bypass / row vector");
  p.R = R;
  p.sink = zv_epi_sink();
  p.err = zv_dev_err_word();
  const int nc = p.H / FFN_HC;
  const bool pers = p.part && p.flag;
  // blocks_max (the lab's grid-size arm) never exceeds the CU count -- the line schedule's hand-off
  // needs every block resident -- nor, persistent, the scratch's slots and flag words
  int bmax = blocks_max > 0 ? std::min(blocks_max, zv_num_cus()) : zv_num_cus();
  if (pers) {
    ZV_REQUIRE(p.part_slots > 0, "fused FeedForward: persistent scratch without its slot count");
    bmax = std::min(bmax, p.part_slots);
  }
  const FfnSchedule sc = ffn_schedule(R, nc, bmax, pers);
  ZV_REQUIRE(!pers || sc.w == nc || sc.blocks <= bmax, "fused FeedForward: more lines than scratch slots");
  p.w = sc.w;
  if (p.nb) {   // FF3 + BiasNorm + bypass
    for (int i = 0; i < p.nseg; ++i)
      ZV_REQUIRE(p.seg[i].orig && p.seg[i].C == p.seg[i].orig && p.seg[i].Ch,
                 "fused FeedForward + BiasNorm operands");
    ZV_REQUIRE(p.byp, "fused FeedForward + BiasNorm bypass");
    p.norm_scale = expf(p.log_scale);
    // (the transposed epilogue takes the row vector's rows from LDS: groups of >= 32 rows)
    const bool tp = !(p.seg[0].rowvec && p.rows_per_group < 32);
    if (pre) {
      if (tp) launch_ffn_t<false, false, true, 0, 1, true, true>(p, sc.blocks, s, tag);
      else launch_ffn_t<false, false, true, 0, 1, false, true>(p, sc.blocks, s, tag);
    } else if (tp) launch_ffn_t<false, false, true, 0, 1>(p, sc.blocks, s, tag);
    else launch_ffn_t<false, false, true, 0, 1, false>(p, sc.blocks, s, tag);
    return;
  }
  if constexpr (ABL != 0) { launch_ffn_t<false, false, true, ABL>(p, sc.blocks, s, tag); return; }
  if (pre) {   // the bypass site: the row vector, if any, belongs to the pre-projection
    ZV_REQUIRE(og && cp, "fused FeedForward pre-projection: the bypass site");
    launch_ffn_t<false, true, true, 0, 0, true, true>(p, sc.blocks, s, tag);
    return;
  }
  if (!rv && !og && cp) launch_ffn_t<false, false, true>(p, sc.blocks, s, tag);
  else if (!rv && !og && !cp) launch_ffn_t<false, false, false>(p, sc.blocks, s, tag);
  else if (rv && !og && cp) {
    if (p.rows_per_group >= 32) launch_ffn_t<true, false, true>(p, sc.blocks, s, tag);
    else launch_ffn_t<true, false, true, 0, 0, false>(p, sc.blocks, s, tag);
  }
  else if (!rv && og && cp) launch_ffn_t<false, true, true>(p, sc.blocks, s, tag);
  else throw std::invalid_argument("fused FeedForward: unsupported epilogue combination");
}
