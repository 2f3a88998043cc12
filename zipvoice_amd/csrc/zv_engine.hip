// ZipVoice MI355X engine: weights, workspace, layer orchestration and the C ABI.
//
// Data layout in HBM: activations are (rows, channels) row-major with
// rows = batch-major (b * L + l), i.e. (B, L, C); the reference's (L, B, C)
// order inside the Zipformer is a layout choice, not a semantic one.  The
// residual stream (src / cur) is always fp32; GEMM operands are bf16 (ZV_BF16)
// or bf16 hi/lo pairs (ZV_FP32).  Weights are stored [Npad][Kpad] bf16 hi
// (+ lo) zero-padded to the GEMM tile grid, biases fp32.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <exception>
#include <functional>
#include <tuple>
#include <vector>


#include "zv_common.h"
#include "zv_gemm.inc"
#include "zv_gemm256.inc"
#include "zv_ffn.inc"
#include "zv_attn.inc"
#include "zv_elem.inc"
#include "zv_session.inc"
#include "zv_flash.inc"
#include "zv_flash2.inc"
#include "zv_weights.inc"
#include "zv_linear.inc"
#include "../../include/zipvoice_hip.h"

static thread_local std::string g_last_error;
ZvProfiler g_zv_prof;

namespace {

struct LayerW {
  Linear attn_in;
  float* pos_w = nullptr;   // (H*pd, pos_dim)
  Linear sa_in[2], sa_out[2];
  Linear ff_in[3], ff_out[3];
  // the fused FeedForward kernel's fragment-major copies of ff_in / ff_out (zv_ffn.inc; decoder
  // layers of width 512 with hidden widths a multiple of 64, 16-bit modes)
  bf16* ffn_w1f[3] = {nullptr, nullptr, nullptr};
  bf16* ffn_w2f[3] = {nullptr, nullptr, nullptr};
  // the pre-projection form (ZV_FFN=3): FF2 / FF3's in_proj with its K in the accumulator's register
  // order (a second packed copy, H * 512 each: the natural-order copy stays for the sites and row
  // counts that keep the conv_sa_out linear), and conv_sa_out[c] in the W2 chunk format
  bf16* ffn_w1fp[3] = {nullptr, nullptr, nullptr};
  bf16* ffn_wpf[2] = {nullptr, nullptr};
  Linear na_in, na_out;
  Linear conv_in[2], conv_out[2];
  // bf16 mode: [conv_out[c] | sa_out[c]] concatenated along K (bias summed): one GEMM finishes
  // both the SelfAttention and the convolution residual updates (zv_engine::layer)
  Linear conv_sa_out[2];
  float* dw_w[2] = {nullptr, nullptr};
  float* dw_b[2] = {nullptr, nullptr};
  int ks = 0;
  float* bypass = nullptr;
  float* bypass_mid = nullptr;
  float* norm_bias = nullptr;
  float norm_log_scale = 0.f;
};

struct StackW {
  int ds = 1;
  std::vector<LayerW> layers;
  float* pos_w_all = nullptr;   // every layer's linear_pos weight, (layers, H*pd, pos_dim)
  Linear time_emb;          // fp32 small linear (time_embed_dim -> dim)
  float* ds_w = nullptr;    // softmax(downsample.bias)
  float* combiner = nullptr;
};

struct ZipformerW {
  int dim = 0, ff = 0, heads = 0, qd = 0, pd = 0, vd = 0, pos_dim = 0, temb_dim = -1;
  std::vector<Linear> in_proj, out_proj;
  std::vector<StackW> stacks;
  bool has_time = false, has_guid = false;
  Linear te0, te2, guid;    // fp32 small linears
  // weights built for the second-generation attention consumers (zv_flash2.inc: log2(e) on the
  // attention-score projection's k / p rows, 16-row value heads); its 16-bit layers launch them
  bool b2 = false;
};

// bumped whenever a workspace buffer moves: captured HIP graphs bake in
// workspace addresses and are dropped when it changes
static unsigned long g_ws_generation = 0;

// grow-only device buffer
struct DBuf {
  void* p = nullptr;
  size_t bytes = 0;
  template <typename T> T* get(size_t n) {
    size_t need = n * sizeof(T) + 256;
    if (need > bytes) {
      ++g_ws_generation;
      if (p) { ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize())); ZV_CHECK(ZV_BLOCKING(hipFree(p))); }
      ZV_CHECK(ZV_BLOCKING(hipMalloc(&p, need)));
      ZV_CHECK(ZV_BLOCKING(hipMemset(p, 0, need)));
      // the memset runs on the null stream, which does not order against the engine's
      // non-blocking streams (graph / split-decoder streams): finish it before any use
      ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
      bytes = need;
    }
    return reinterpret_cast<T*>(p);
  }
  ~DBuf() { if (p) (void)ZV_BLOCKING(hipFree(p)); }
};

struct ActBuf {
  DBuf h, l, q, qs;
  // fp8: also the MX-fp8 copy of the first `cols` columns; with16 = false: that copy only
  Act get(long rows, long ld, bool split, bool fp8 = false, long cols = 0, bool with16 = true) {
    Act a;
    a.ld = ld;
    a.h = with16 ? h.get<bf16>((size_t)rows * ld) : nullptr;
    a.l = split ? l.get<bf16>((size_t)rows * ld) : nullptr;
    if (fp8) {
      a.ldq = round_up(cols ? cols : ld, MX8_KSTEP);
      a.q = q.get<uint8_t>((size_t)rows * a.ldq);
      a.qs = qs.get<uint8_t>((size_t)rows * a.ldq / MX8_BLOCK);
    }
    return a;
  }
  size_t bytes() const { return h.bytes + l.bytes + q.bytes + qs.bytes; }
};

struct Workspace {
  // fp32 residual streams
  DBuf main, dsrc, cur, temb0, temb1, tstack, tvec, gvec, posP, mask2, maskds, vout, stats;
  // bf16 (hi/lo) GEMM operands
  ActBuf xin, main_a, dsrc_a, cur_a, qkp, W, hidden, na_y, na_xt, na_o, sa_vt, sa_o, glu, dw, emb;
  ActBuf cur8;   // fp8 mode: the working stream's MX-fp8 copy
  ActBuf dwo;    // bf16 mode: [depthwise-conv output | SelfAttention output] (the K-concatenated
                 // out-projection's operand)
  // the fused FeedForward's persistent schedule (zv_ffn.inc): one 256 KiB tile slot per CU, one
  // flag word per CU (zero between launches) and the spin-timeout counter
  DBuf ffn_part, ffn_flag;
  // the rows' lengths (int32 per decoder row, zv_row_len_kernel): taken by every masked pass with a
  // downsampled stack, written and read in the row padding mode (ZV_PAD_ROW) only
  DBuf rowlen;
  // per-stack positional projections, kept across the Euler steps of one solve (they depend on
  // the stack's length and weights only; Pass::posp_reuse)
  static constexpr int POSP_STACKS = 8;
  DBuf posPs[POSP_STACKS];
  // what each posPs slot holds (written with it): a later step reuses it only on a match
  struct PosPKey { int L = -1, nl = 0; const void* w = nullptr; const void* buf = nullptr; };
  PosPKey posk[POSP_STACKS];
  size_t bytes() const {
    size_t s = 0;
    for (const DBuf& b : posPs) s += b.bytes;
    for (const DBuf* b : {&main, &dsrc, &cur, &temb0, &temb1, &tstack, &tvec, &gvec, &posP, &mask2,
                          &maskds, &vout, &stats, &ffn_part, &ffn_flag, &rowlen})
      s += b->bytes;
    for (const ActBuf* b : {&xin, &main_a, &dsrc_a, &cur_a, &qkp, &W, &hidden, &na_y, &na_xt, &na_o,
                            &sa_vt, &sa_o, &glu, &dw, &emb, &cur8, &dwo})
      s += b->bytes();
    return s;
  }
};

// what a forward pass is told by its caller (decoder / text_encode fill it; zipformer, stack and
// layer read it)
struct Pass {
  bool io_split = false;     // ZV_MIXED's decoder: split in/out projections, weight-split
                             // attention-score projections
  bool posp_reuse = false;   // the stacks' posP buffers hold this solve's values (euler_loop's
                             // later steps)
  long batch_rows = 0;       // the whole batch's rows (N) while a split decoder runs one row block
                             // (0: not split): the fused / unfused FeedForward choice follows
                             // the batch, not the row block
};

// Engine streams come from a per-device process-wide pool of stream sets: an engine takes a set
// for its lifetime (its decoder row-block streams and its graph stream) and returns it when it is
// destroyed; a later engine reuses a returned set.  Streams are multiplexed onto the process's few
// hardware queues (GPU_MAX_HW_QUEUES, 4); streams created after others were destroyed were mapped
// so that the decoder's row blocks shared queues: a second engine in one process ran C5 at 341 ms
// per step against 216 ms for the first (profiles/r03_stream_pool_ab.txt).  Reusing sets keeps
// every engine on the mapping of the first, and no two live engines share a stream (one engine
// capturing its Euler-loop graph while another launches on the same stream would corrupt both).
constexpr int ZV_STREAM_SET = 4;
struct StreamSet { hipStream_t s[ZV_STREAM_SET] = {}; int dev = -1; };
static std::mutex g_stream_pool_mu;
static std::vector<StreamSet>& stream_pool_free() { static std::vector<StreamSet> v; return v; }
static StreamSet acquire_stream_set() {
  int dev = 0;
  ZV_CHECK(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> lock(g_stream_pool_mu);
    auto& fr = stream_pool_free();
    for (size_t i = 0; i < fr.size(); ++i)
      if (fr[i].dev == dev) {
        StreamSet set = fr[i];
        fr.erase(fr.begin() + i);
        return set;
      }
  }
  // (the whole set up front: creating the streams on first use instead -- a process then holds
  // only the streams it launches on -- left one engine alone equal but put a later engine of the
  // same process on a worse queue mapping: the bench's fp32 leg 991 -> 1087 ms,
  // profiles/r05_streams_ab.txt)
  StreamSet set;
  set.dev = dev;
  for (int i = 0; i < ZV_STREAM_SET; ++i)
    ZV_CHECK(ZV_BLOCKING(hipStreamCreateWithFlags(&set.s[i], hipStreamNonBlocking)));
  return set;
}
static void release_stream_set(const StreamSet& set) {
  if (set.dev < 0) return;
  for (hipStream_t st : set.s)
    if (st) (void)ZV_BLOCKING(hipStreamSynchronize(st));
  std::lock_guard<std::mutex> lock(g_stream_pool_mu);
  stream_pool_free().push_back(set);
}

}  // namespace

// A solve session's state (zv_session_*; the body is zv_engine::session_*, the kernels and the tick's
// plan zv_session.inc).  Device: the slot buffers.  Host: per slot the row's schedule (num_step 0: the
// slot is free), its grid, its length and the steps it has done, so which rows finish is known from
// the schedules alone.
struct zv_engine;
struct zv_session {
  zv_engine* eng = nullptr;                  // null once the engine is gone: every entry then fails
  int slots = 0, maxT = 0;
  DBuf x, tc, sc, pad;                       // (slots, maxT, Fx / Ft / Fx) floats, (slots, maxT) bytes
  float *dx = nullptr, *dtc = nullptr, *dsc = nullptr;
  uint8_t* dpad = nullptr;
  std::vector<SchedRow> rows;
  std::vector<std::vector<float>> ts;
  std::vector<int> lens, done;
  int64_t ticks = 0, dec_rows = 0, dec_row_frames = 0, last_T = 0;
  ~zv_session();
};

// ===========================================================================
struct zv_engine : LinearPolicy {   // (zv_linear.inc: linear<SPLIT> and the fused-epilogue launches)
  zv_config cfg;
  WeightStore store;
  ZipformerW dec, txt;
  float* embed_table = nullptr;   // (vocab, text_embed_dim)
  float* spk_table = nullptr;     // (2, feat_dim)
  float* temb_freqs = nullptr;    // (time_embed_dim/2)
  Workspace ws_dec, ws_txt;
  static constexpr int MAX_SPLIT = 4;
  Workspace ws_split[MAX_SPLIT - 1];   // row blocks 1.. of the split decoder
  int split_streams = 3;           // ZV_SPLIT_STREAMS: decoder row blocks on this many streams
                                   // (<= 1: one stream; bench A/B: profiles/r02_split_tp_ab.txt)
  long split_min_rows = 0;         // ... for N*T >= this many rows (ZV_SPLIT_MIN_ROWS)
  hipStream_t split_stream[MAX_SPLIT - 1] = {};
  hipEvent_t split_fork = nullptr, split_join[MAX_SPLIT - 1] = {};

  bool materialize_attn = false;   // A/B: ZV_ATTN_MATERIALIZE=1 keeps the W-materialising path
  // ZV_FFN: the decoder FeedForward modules as one fused kernel each (zv_ffn.inc: in_proj ->
  // SwooshL -> out_proj -> residual without the hidden tensor in HBM) for launches of at
  // least ffn_min_rows rows; 2 (default): FF3 also carries the layer's BiasNorm + bypass in its
  // epilogue.  C2 bench 445 -> 431 ms per step with the pipelined depthwise conv
  // (profiles/r03_ffn_ab.txt).  3 (default): FF2 and FF3 also run the conv + SelfAttention
  // out-projection (conv_sa_out) as their first phase where the K-concatenated linear would run in
  // front of them (layer<1>): no gemm_bf16_resid_rv launch, no fp32 stream round trip between the two
  int ffn_fused = 3;
  // ZV_FFN_MIN_ROWS: launches under this many rows run the unfused pair, which fills the chip
  // better there (a fused block owns a CU and takes 128 rows: 10k rows = 78 blocks for 256
  // CUs).  C2 435 -> 426-432 ms (profiles/r03_ffn_policy_ab.txt); C3 (16 utterances, no
  // CFG: ~6.5k rows per decoder stream) 88.4 -> 74.6 ms and C5 246 -> 220 ms with the pair
  // (profiles/r03_ffn_configs_ab.txt).  The choice follows the launch's rows, so an
  // utterance's rounding can depend on its batch (as any shape-dependent kernel choice);
  // ZV_FFN_MIN_ROWS=0 pins the fused kernel for a batch-invariant engine
  // (tests/test_gpu_fullsize.py batch rows test).  10k -> 15k in round 5, after the small-launch
  // tiles sped up the pair: C5's half-rate stacks (13.5k rows) 183.6 -> 176.2 ms per step; C2 /
  // C3 / C4 have no stack in [10k, 15k) (profiles/r05_ffn_min_rows_ab.txt)
  long ffn_min_rows = 15000;
  int fp8_fuse = 7;                // ZV_FP8_FUSE (fp8 mode): which bf16 producers write the fp8 copy
                                   // themselves (2 depthwise conv, 4 BiasNorm; no code reads bit 1);
                                   // the others are followed by the pack kernel
  int sa_tp = 1;                   // ZV_SA_TP: 16-bit modes' SelfAttention with the positional
                                   // term on the MFMA chain (zv_attn_sa_tp_kernel), the head-0
                                   // stats / NonlinAttention scoring too; 0 = VALU forms
                                   // (3: A/B arm, SA with the one-wave register budget)
  // ZV_MIXED_SA (fp16 parity mode): the SelfAttention value projection as a weight-split product and
  // its out-projection's residual update as a split product (the K-concatenated conv + SelfAttention
  // out-projection runs [dw | o_hi | o_lo | o_hi] . [conv_out | sa_out_hi | sa_out_hi | sa_out_lo]):
  // the families the emulation names for the random T = 203 input's 1.08e-3 -> 8.9e-4
  // (tools/precision_study.py --velocity, profiles/r04_precision_study_r04_velocity_T203.txt)
  bool mixed_sa = true;
  // ZV_ATTN2 (default 1): second-generation attention consumers (zv_flash2.inc): log2(e) folded
  // into the attention-score projection's k / p rows, the SelfAttention value projection padded to
  // 16 rows per head (ones row 12), no statistics pass.  bf16 / fp8 engines: decoder and text
  // encoder; the fp16 parity mode (ZV_MIXED): the decoder (its text encoder runs the split products)
  bool attn_b2 = false, attn_b2_dec = false;
  // ZV_ATTN2_EXACT (test infrastructure, default 0): every second-generation consumer wave / block
  // takes its exact path (row maximum subtracted) instead of only those whose range check fails
  int attn2_exact = 0;
  // ZV_GLU_DW (default 1): the convolution module's GLU linear and depthwise conv (+ SwooshR) as one
  // launch (zv_gemm256.inc g256_epi_glu_dw) in the 16-bit modes; bitwise equal to the pair
  int glu_dw = 1;
  // exact-path counters of the second-generation consumers (FlashParams::fallback; zv_attn_fallbacks)
  unsigned* attn_fallback = nullptr;
  // zv_set_padding: how the downsampled stacks right-pad a masked row's last group of ds frames.
  // ZV_PAD_BATCH: with the batch tensor's frames past the row's end, as the reference does on the
  // padded batch (zv_downsample_kernel); ZV_PAD_ROW: with the row's own last frame, as the reference
  // does on the row alone (zv_row_len_kernel once per zipformer() call, zv_downsample_row_kernel)
  int padding = ZV_PAD_BATCH;

  explicit zv_engine(const zv_config& c) : cfg(c) {
    auto envi = [](const char* k, int d) { const char* v = getenv(k); return v ? atoi(v) : d; };
    materialize_attn = envi("ZV_ATTN_MATERIALIZE", 0) == 1;
    graph_mode = envi("ZV_GRAPH", 2);
    sa_tp = envi("ZV_SA_TP", 1);
    fp8_fuse = envi("ZV_FP8_FUSE", 7);
    ffn_fused = envi("ZV_FFN", 3);
    ffn_min_rows = envi("ZV_FFN_MIN_ROWS", 15000);
    ffn_persist = envi("ZV_FFN_PERSIST", 1);
    split_streams = envi("ZV_SPLIT_STREAMS", 3);
    split_min_rows = envi("ZV_SPLIT_MIN_ROWS", 8192);
    mixed_sa = envi("ZV_MIXED_SA", 1) != 0;
    attn_b2 = envi("ZV_ATTN2", 1) != 0 && (cfg.precision == ZV_BF16 || cfg.precision == ZV_FP8);
    attn_b2_dec = attn_b2 || (envi("ZV_ATTN2", 1) != 0 && cfg.precision == ZV_MIXED);
    attn2_exact = envi("ZV_ATTN2_EXACT", 0) != 0;
    glu_dw = envi("ZV_GLU_DW", 1);
  }
  // ---------------------------------------------------------------- HIP graphs
  // The whole N-step Euler solve (~250 launches per step) is captured once per
  // (shape, schedule) on an engine-owned stream over engine-owned staging copies
  // of the inputs, then replayed with one hipGraphLaunch: the host launch cost
  // (which bounds small-batch / single-sentence latency) goes away.  The first
  // call of a key runs uncaptured (it sizes the workspace); ZV_GRAPH=0 disables
  // capture.  The cache is bounded (LRU over MAX_GRAPHS executable graphs, each
  // destroyed on eviction), so a server with varying shapes does not grow it.
  struct GraphKey {
    int B, T, N, has_pad;
    float g, t0, t1, shift;
    int cfg_mode;            // 0: scalar g; 1: per-row g with CFG; 2: per-row g without CFG
    int padding;             // zv_padding: a solve captured in one mode is never replayed in the other
    unsigned long gen;
    bool operator<(const GraphKey& o) const {
      return std::tie(B, T, N, has_pad, g, t0, t1, shift, cfg_mode, padding, gen) <
             std::tie(o.B, o.T, o.N, o.has_pad, o.g, o.t0, o.t1, o.shift, o.cfg_mode, o.padding, o.gen);
    }
  };
  static constexpr size_t MAX_GRAPHS = 8, MAX_SEEN = 256;
  struct GraphEntry { hipGraphExec_t exec; unsigned long last_use; };
  std::map<GraphKey, GraphEntry> graphs;
  std::map<GraphKey, int> graph_seen;
  unsigned long graph_clock = 0;
  hipStream_t gstream = nullptr;
  hipEvent_t gev_in = nullptr, gev_out = nullptr;
  DBuf gx, gtc, gsc, gpad, ggrows;
  // ZV_GRAPH: 0 plain launches, 1 always replay the captured Euler loop, 2 (default) replay it
  // unless the decoder splits its rows over streams.  A replayed multi-stream graph ran 10 ms
  // per C2 step slower than the same launches made directly on the three engine streams
  // (419.8 vs 410.0 ms, profiles/r03_graph_ab.txt; the runtime's own graph queues add the
  // cross-branch waits), while single-stream shapes (one sentence) are launch-bound and
  // need the graph
  int graph_mode = 2;

  // ---------------------------------------------------------------- fused FeedForward sites
  // ZV_FFN_PERSIST (default 1): fused FeedForward launches on the persistent line schedule
  // (zv_ffn.inc; results equal to one row block per block bit for bit).  The scratch is sized for
  // one line per CU; launch_ffn never launches more blocks than that (it checks)
  int ffn_persist = 1;
  void attach_ffn_scratch(FfnParams& q, Workspace& ws) {
    if (!ffn_persist) return;
    const int cus = zv_num_cus();
    q.part = ws.ffn_part.get<float>((size_t)cus * FFN_PART_FLOATS);
    unsigned* fl = ws.ffn_flag.get<unsigned>((size_t)cus + 64);
    q.flag = fl;
    q.part_slots = cus;
  }
  void ffn_site(FfnParams q, Workspace& ws, hipStream_t s, const char* tag) {
    attach_ffn_scratch(q, ws);
    launch_ffn(q, s, tag);
  }

  // the device error word (zv_dev_err_word) read without synchronising: a fused FeedForward C item
  // that outwaited its producer finished on unwritten tiles, so the results of the calls since the
  // last check are invalid.  Let every launch drain, clear the persistent schedule's flag words
  // (a late producer may have left its flag set for a later launch), report once
  void check_dev_err() {
    volatile unsigned* e = zv_dev_err_host();
    if (*e == 0) return;
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    auto clear = [](Workspace& w) {
      if (w.ffn_flag.p) ZV_CHECK(ZV_BLOCKING(hipMemset(w.ffn_flag.p, 0, w.ffn_flag.bytes)));
    };
    clear(ws_dec); clear(ws_txt);
    for (Workspace& w : ws_split) clear(w);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    *e = 0;
    throw std::runtime_error("fused FeedForward: a C item waited more than 2 s for its producer's tiles; "
                             "the outputs of the calls since the previous one are invalid (schedule flags reset)");
  }

  void drop_graphs() {
    for (auto& kv : graphs) (void)ZV_BLOCKING(hipGraphExecDestroy(kv.second.exec));
    graphs.clear();
  }
  void evict_lru_graph() {
    auto victim = graphs.begin();
    for (auto it = graphs.begin(); it != graphs.end(); ++it)
      if (it->second.last_use < victim->second.last_use) victim = it;
    // its last replay may still run on gstream: destroy only after it drained
    ZV_CHECK(ZV_BLOCKING(hipStreamSynchronize(gstream)));
    ZV_CHECK(ZV_BLOCKING(hipGraphExecDestroy(victim->second.exec)));
    graphs.erase(victim);
  }

  StreamSet streams;                // this engine's stream set (acquire_stream_set), taken lazily
  hipStream_t engine_stream(int slot) {
    static_assert(MAX_SPLIT <= ZV_STREAM_SET, "stream set holds the split streams and the graph stream");
    if (streams.dev < 0) streams = acquire_stream_set();
    // (row-block streams at the greatest / least priority lost 1.9 % / 0.6 % per C2 step, round 4:
    // profiles/r04_stream_prio.txt; all streams at the default priority)
    if (!streams.s[slot]) ZV_CHECK(ZV_BLOCKING(hipStreamCreateWithFlags(&streams.s[slot], hipStreamNonBlocking)));
    return streams.s[slot];
  }

  ~zv_engine() {
    for (zv_session* q : sessions) q->eng = nullptr;   // a session left behind answers with an error
    drop_graphs();
    // the stream set outlives the engine: drain what this engine queued on it, then return it
    release_stream_set(streams);
    // the scheduled solve's staging: a queued upload on the caller's stream may still read a slot
    if (!sched_slots.empty()) (void)ZV_BLOCKING(hipDeviceSynchronize());
    for (SchedSlot& sl : sched_slots) (void)ZV_BLOCKING(hipHostFree(sl.base));
    if (gev_in) (void)ZV_BLOCKING(hipEventDestroy(gev_in));
    if (gev_out) (void)ZV_BLOCKING(hipEventDestroy(gev_out));
    for (int i = 0; i < MAX_SPLIT - 1; ++i)
      if (split_join[i]) (void)ZV_BLOCKING(hipEventDestroy(split_join[i]));
    if (split_fork) (void)ZV_BLOCKING(hipEventDestroy(split_fork));
  }

  // ---------------------------------------------------------------- weights
  // perm (optional): row n of the device matrix is row perm[n] of the reference weight
  Linear make_linear(const std::string& prefix, int N, int K, bool bias, bool keep_f32,
                     const std::vector<int>* perm = nullptr, bool fp8 = false) {
    const auto& w = store.take(prefix + ".weight", (size_t)N * K);
    const std::vector<float>* b = bias ? &store.take(prefix + ".bias", N) : nullptr;
    std::vector<float> wp, bp;               // the permuted rows
    if (perm) {
      wp.resize((size_t)N * K);
      for (int n = 0; n < N; ++n)
        memcpy(&wp[(size_t)n * K], &w[(size_t)(*perm)[n] * K], (size_t)K * sizeof(float));
      if (b) {
        bp.resize(N);
        for (int n = 0; n < N; ++n) bp[n] = (*b)[(*perm)[n]];
      }
    }
    const float* rows = perm ? wp.data() : w.data();
    Linear L = store.make_linear(rows, N, K, !b ? nullptr : perm ? bp.data() : b->data());
    if (fp8 && cfg.precision == ZV_FP8 && K % MX8_KSTEP == 0) {
      // MX-fp8 copy of the (permuted) fp32 weight, rows zero-padded to Npad
      L.Kq = K;
      std::vector<float> wz((size_t)L.Npad * K, 0.f);
      memcpy(wz.data(), rows, (size_t)N * K * sizeof(float));
      std::vector<uint8_t> q((size_t)L.Npad * K), sc((size_t)L.Npad * K / MX8_BLOCK);
      mx8_quantize_host(wz.data(), K, L.Npad, K, q.data(), K, sc.data());
      L.q8 = store.upload(q.data(), q.size());
      L.s8 = store.upload(sc.data(), sc.size());
    }
    if (keep_f32) L.w32 = store.upload(w.data(), (size_t)N * K);
    return L;
  }
  // [a | b] concatenated along K (a: N x Ka, b: N x Kb; bias a + b), rows padded like
  // make_linear: the operand is [a's input (Ka columns) | b's input (Kb columns)]
  // b_split: b's columns three times as [b_hi | b_hi | b_lo] (the operand [a | x_hi | x_lo | x_hi]:
  // x . b as the split product x_hi b_hi + x_lo b_hi + x_hi b_lo in a 16-bit GEMM; lo array unused):
  // the third block's source is b's fp32 remainder v - hi, whose hi half is b_lo
  Linear make_linear_kcat(const std::string& pa, int Ka, const std::string& pb, int Kb, int N,
                          bool b_split = false) {
    const int K = Ka + (b_split ? 3 : 1) * Kb;
    const auto& wa = store.take(pa + ".weight", (size_t)N * Ka);
    const auto& wb = store.take(pb + ".weight", (size_t)N * Kb);
    std::vector<float> w((size_t)N * K);
    for (int n = 0; n < N; ++n) {
      float* row = &w[(size_t)n * K];
      memcpy(row, &wa[(size_t)n * Ka], (size_t)Ka * sizeof(float));
      for (int blk = 0; Ka + blk * Kb < K; ++blk)
        for (int k = 0; k < Kb; ++k) {
          const float v = wb[(size_t)n * Kb + k];
          row[Ka + blk * Kb + k] = blk == 2 ? v - (float)(bf16)v : v;
        }
    }
    const auto& ba = store.take(pa + ".bias", N);
    const auto& bb = store.take(pb + ".bias", N);
    std::vector<float> b(N);
    for (int n = 0; n < N; ++n) b[n] = ba[n] + bb[n];
    return store.make_linear(w.data(), N, K, b.data());
  }
  // NonlinAttention in_proj rows [s | x | y] -> groups of 48 = [s16 | x16 | y16]
  static std::vector<int> perm_na(int hid) {
    std::vector<int> p(3 * hid);
    for (int g = 0; g < hid / 16; ++g)
      for (int i = 0; i < 16; ++i) {
        p[g * 48 + i] = g * 16 + i;
        p[g * 48 + 16 + i] = hid + g * 16 + i;
        p[g * 48 + 32 + i] = 2 * hid + g * 16 + i;
      }
    return p;
  }
  // ConvolutionModule in_proj rows [x | s] -> groups of 32 = [x16 | s16]
  static std::vector<int> perm_glu(int C) {
    std::vector<int> p(2 * C);
    for (int g = 0; g < C / 16; ++g)
      for (int i = 0; i < 16; ++i) {
        p[g * 32 + i] = g * 16 + i;
        p[g * 32 + 16 + i] = C + g * 16 + i;
      }
    return p;
  }
  // staged copy of prefix.{weight, bias} with rows [r0, r1) multiplied by f (the second-generation
  // attention's base-2 scores: log2(e) on the k and p rows of the attention-score projection)
  std::string stage_rows_scaled(const std::string& prefix, int N, int K, int r0, int r1, float f) {
    std::vector<float> w = store.take(prefix + ".weight", (size_t)N * K), b = store.take(prefix + ".bias", N);
    for (int n = r0; n < r1; ++n) {
      for (int k = 0; k < K; ++k) w[(size_t)n * K + k] *= f;
      b[n] *= f;
    }
    const std::string np = prefix + "#b2";
    store.derived[np + ".weight"] = std::move(w);
    store.derived[np + ".bias"] = std::move(b);
    return np;
  }
  // staged copy of a SelfAttention value projection (heads * vd rows) laid out 16 rows per head:
  // [vd value rows | a zero row with bias 1 | zero rows]: its V^T carries the softmax denominator's
  // ones row (zv_flash2.inc)
  std::string stage_value_heads16(const std::string& prefix, int heads, int vd, int K) {
    const auto& w = store.take(prefix + ".weight", (size_t)heads * vd * K);
    const auto& b = store.take(prefix + ".bias", (size_t)heads * vd);
    std::vector<float> w2((size_t)heads * 16 * K, 0.f), b2((size_t)heads * 16, 0.f);
    for (int h = 0; h < heads; ++h) {
      for (int d = 0; d < vd; ++d) {
        memcpy(&w2[(size_t)(h * 16 + d) * K], &w[(size_t)(h * vd + d) * K], (size_t)K * sizeof(float));
        b2[h * 16 + d] = b[h * vd + d];
      }
      b2[h * 16 + 12] = 1.f;
    }
    const std::string np = prefix + "#v16";
    store.derived[np + ".weight"] = std::move(w2);
    store.derived[np + ".bias"] = std::move(b2);
    return np;
  }
  Linear make_small(const std::string& prefix, int N, int K, bool bias) {
    Linear L;
    L.N = N; L.K = K;
    L.w32 = store.upload_key(prefix + ".weight", (size_t)N * K);
    if (bias) L.b = store.upload_key(prefix + ".bias", N);
    return L;
  }

  // is_decoder: the flow-matching decoder (the fp8 mode's fp8 weight copies, the fused FeedForward's
  // packed copies and conv_sa_out belong to it; the text encoder has none)
  void build_zipformer(ZipformerW& Z, const std::string& pre, int dim, int ff, int heads,
                       const std::vector<int>& ds, const std::vector<int>& layers,
                       const std::vector<int>& ks, std::vector<int> in_dims,
                       std::vector<int> out_dims, bool two_stream, int temb_dim, bool guid,
                       bool is_decoder = false, bool b2 = false) {
    Z.dim = dim; Z.ff = ff; Z.heads = heads; Z.b2 = b2;
    Z.qd = cfg.query_head_dim; Z.pd = cfg.pos_head_dim; Z.vd = cfg.value_head_dim;
    Z.pos_dim = cfg.pos_dim; Z.temb_dim = temb_dim;
    ZV_REQUIRE(Z.qd == ATT_QD && Z.pd == ATT_PD, "engine supports query_head_dim=32, pos_head_dim=4");
    ZV_REQUIRE(Z.pos_dim % 2 == 0 && Z.pos_dim <= POSP_MAXD, "pos_dim must be even and <= 64");
    ZV_REQUIRE(heads * Z.vd <= 64, "num_heads * value_head_dim must be <= 64");
    for (size_t i = 0; i < in_dims.size(); ++i) {
      std::string s = two_stream ? "." + std::to_string(i) : "";
      Z.in_proj.push_back(make_linear(pre + "in_proj" + s, dim, in_dims[i], true, false));
      Z.out_proj.push_back(make_linear(pre + "out_proj" + s, out_dims[i], dim, true, false));
    }
    const int qkp = (2 * Z.qd + Z.pd) * heads;
    for (size_t s = 0; s < ds.size(); ++s) {
      StackW S;
      S.ds = ds[s];
      std::string sp = pre + "encoders." + std::to_string(s) + ".";
      std::string ep = S.ds != 1 ? sp + "encoder." : sp;
      if (S.ds != 1) {
        ZV_REQUIRE(S.ds <= 8, "downsampling factor > 8 unsupported");
        const auto& b = store.take(sp + "downsample.bias", S.ds);
        float mx = -INFINITY;
        for (float v : b) mx = std::max(mx, v);
        std::vector<float> w(S.ds);
        float sum = 0.f;
        for (int k = 0; k < S.ds; ++k) { w[k] = expf(b[k] - mx); sum += w[k]; }
        for (int k = 0; k < S.ds; ++k) w[k] /= sum;
        S.ds_w = store.dalloc<float>(S.ds);
        ZV_CHECK(ZV_BLOCKING(hipMemcpy(S.ds_w, w.data(), S.ds * sizeof(float), hipMemcpyHostToDevice)));
        S.combiner = store.upload_key(sp + "out_combiner.bypass_scale", dim);
      }
      if (temb_dim > 0) S.time_emb = make_small(ep + "time_emb.1", dim, temb_dim, true);
      const size_t pw_n = (size_t)heads * Z.pd * Z.pos_dim;
      S.pos_w_all = store.dalloc<float>(pw_n * std::max(layers[s], 1));
      for (int li = 0; li < layers[s]; ++li) {
        std::string lp = ep + "layers." + std::to_string(li) + ".";
        LayerW W;
        W.attn_in = make_linear(b2 ? stage_rows_scaled(lp + "self_attn_weights.in_proj", qkp, dim,
                                                            heads * Z.qd, qkp, 1.4426950408889634f)
                                        : lp + "self_attn_weights.in_proj",
                                qkp, dim, true, false);
        {
          const auto& pw = store.take(lp + "self_attn_weights.linear_pos.weight", pw_n);
          W.pos_w = S.pos_w_all + li * pw_n;
          ZV_CHECK(ZV_BLOCKING(hipMemcpy(W.pos_w, pw.data(), pw_n * sizeof(float), hipMemcpyHostToDevice)));
        }
        for (int a = 0; a < 2; ++a) {
          std::string ap = lp + "self_attn" + std::to_string(a + 1) + ".";
          if (b2) {
            ZV_REQUIRE(Z.vd <= 12, "value_head_dim <= 12 for the padded value heads");
            W.sa_in[a] = make_linear(stage_value_heads16(ap + "in_proj", heads, Z.vd, dim), heads * 16, dim,
                                     true, false);
          } else {
            W.sa_in[a] = make_linear(ap + "in_proj", heads * Z.vd, dim, true, false);
          }
          W.sa_out[a] = make_linear(ap + "out_proj", dim, heads * Z.vd, true, false);
        }
        const int hs[3] = {ff * 3 / 4, ff, ff * 5 / 4};
        for (int f = 0; f < 3; ++f) {
          std::string fp = lp + "feed_forward" + std::to_string(f + 1) + ".";
          W.ff_in[f] = make_linear(fp + "in_proj", hs[f], dim, true, false, nullptr, is_decoder);
          W.ff_out[f] = make_linear(fp + "out_proj", dim, hs[f], true, false, nullptr, is_decoder);
          if (ffn_fused && is_decoder && dim == FFN_D && hs[f] % (2 * FFN_HC) == 0 &&
              (cfg.precision == ZV_BF16 || cfg.precision == ZV_MIXED)) {
            const long n = (long)hs[f] * FFN_D;
            W.ffn_w1f[f] = store.dalloc<bf16>(n);
            W.ffn_w2f[f] = store.dalloc<bf16>(n);
            ffn_pack_weights(W.ff_in[f], W.ff_out[f], hs[f], W.ffn_w1f[f], W.ffn_w2f[f], nullptr);
            ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
          }
        }
        const int hid = 3 * dim / 4;
        ZV_REQUIRE(hid % 16 == 0 && dim % 64 == 0, "encoder dim must be a multiple of 64");
        const std::vector<int> pna = perm_na(hid), pglu = perm_glu(dim);
        W.na_in = make_linear(lp + "nonlin_attention.in_proj", 3 * hid, dim, true, false, &pna);
        W.na_out = make_linear(lp + "nonlin_attention.out_proj", dim, hid, true, false, nullptr, is_decoder);
        W.ks = ks[s];
        for (int c = 0; c < 2; ++c) {
          std::string cp = lp + "conv_module" + std::to_string(c + 1) + ".";
          W.conv_in[c] = make_linear(cp + "in_proj", 2 * dim, dim, true, false, &pglu, is_decoder);
          W.conv_out[c] = make_linear(cp + "out_proj", dim, dim, true, false, nullptr, is_decoder);
          if (is_decoder && (cfg.precision == ZV_BF16 || cfg.precision == ZV_MIXED))
            W.conv_sa_out[c] = make_linear_kcat(cp + "out_proj", dim,
                                                lp + "self_attn" + std::to_string(c + 1) + ".out_proj",
                                                heads * Z.vd, dim, cfg.precision == ZV_MIXED && mixed_sa);
          if (ffn_fused >= 3 && W.conv_sa_out[c].hi && W.ffn_w1f[c + 1]) {
            const int f = c + 1;                      // conv(c) is followed by FF(c + 2)
            W.ffn_w1fp[f] = store.dalloc<bf16>((long)hs[f] * FFN_D);
            W.ffn_wpf[c] = store.dalloc<bf16>((long)ffn_pre_chunks(W.conv_sa_out[c].K) * FFN_HC * FFN_D);
            ffn_pack_pre_weights(W.ff_in[f], hs[f], W.ffn_w1fp[f], W.conv_sa_out[c], W.ffn_wpf[c], nullptr);
            ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
          }
          W.dw_w[c] = store.upload_key(cp + "depthwise_conv.weight", (size_t)dim * W.ks);
          W.dw_b[c] = store.upload_key(cp + "depthwise_conv.bias", dim);
        }
        W.bypass = store.upload_key(lp + "bypass.bypass_scale", dim);
        W.bypass_mid = store.upload_key(lp + "bypass_mid.bypass_scale", dim);
        W.norm_bias = store.upload_key(lp + "norm.bias", dim);
        W.norm_log_scale = store.take(lp + "norm.log_scale", 1)[0];
        S.layers.push_back(std::move(W));
      }
      Z.stacks.push_back(std::move(S));
    }
    if (temb_dim > 0) {
      Z.has_time = true;
      Z.te0 = make_small(pre + "time_embed.0", 2 * temb_dim, temb_dim, true);
      Z.te2 = make_small(pre + "time_embed.2", temb_dim, 2 * temb_dim, true);
      if (guid) {
        Z.has_guid = true;
        Z.guid = make_small(pre + "guidance_scale_embed", temb_dim, temb_dim, false);
      }
    }
  }

  bool stereo() const { return cfg.variant == ZV_DIALOG_STEREO; }
  bool distill() const { return cfg.variant == ZV_DISTILL; }
  bool dialog() const { return cfg.variant == ZV_DIALOG || cfg.variant == ZV_DIALOG_STEREO; }

  void finalize() {
    const int F = cfg.feat_dim;
    std::vector<int> ds, nl, ks;
    for (int s = 0; s < cfg.num_stacks; ++s) {
      ds.push_back(cfg.downsampling_factor[s]);
      nl.push_back(cfg.num_layers[s]);
      ks.push_back(cfg.cnn_module_kernel[s]);
    }
    std::vector<int> in_dims = stereo() ? std::vector<int>{5 * F, 3 * F} : std::vector<int>{3 * F};
    std::vector<int> out_dims = stereo() ? std::vector<int>{2 * F, F} : std::vector<int>{F};
    build_zipformer(dec, "fm_decoder.", cfg.fm_decoder_dim, cfg.fm_decoder_feedforward_dim,
                    cfg.fm_decoder_num_heads, ds, nl, ks, in_dims, out_dims, stereo(),
                    cfg.time_embed_dim, distill(), /*is_decoder=*/true, attn_b2_dec);
    build_zipformer(txt, "text_encoder.", cfg.text_encoder_dim, cfg.text_encoder_feedforward_dim,
                    cfg.text_encoder_num_heads, {1}, {cfg.text_encoder_num_layers},
                    {cfg.text_encoder_cnn_module_kernel}, {cfg.text_embed_dim}, {F}, false, -1,
                    false, attn_b2);
    embed_table = store.upload_key("embed.weight", (size_t)cfg.vocab_size * cfg.text_embed_dim);
    if (dialog()) spk_table = store.upload_key("spk_embed.weight", (size_t)2 * F);
    // timestep-embedding frequencies, float32 as zipformer.py:56-60
    const int half = cfg.time_embed_dim / 2;
    std::vector<float> fr(half);
    for (int k = 0; k < half; ++k)
      fr[k] = expf((float)(-log(10000.0)) * (float)k / (float)half);
    temb_freqs = store.dalloc<float>(half);
    ZV_CHECK(ZV_BLOCKING(hipMemcpy(temb_freqs, fr.data(), half * sizeof(float), hipMemcpyHostToDevice)));
    attn_fallback = store.dalloc<unsigned>(4);
    ZV_CHECK(ZV_BLOCKING(hipMemset(attn_fallback, 0, 4 * sizeof(unsigned))));
    // strict=True: nothing left over
    size_t expected = count_expected();
    if (expected != store.staged.size())
      throw std::invalid_argument("state dict has " + std::to_string(store.staged.size()) +
                                  " tensors, config expects " + std::to_string(expected) +
                                  " (unexpected keys present)");
    store.staged.clear();
    store.derived.clear();
    store.ready = true;
  }

  size_t count_expected() const {
    auto zf = [&](const ZipformerW& Z) {
      size_t n = 4 * Z.in_proj.size();
      for (const auto& S : Z.stacks) {
        if (S.ds != 1) n += 2;
        if (Z.temb_dim > 0) n += 2;
        n += S.layers.size() * 43;
      }
      if (Z.has_time) n += 4;
      if (Z.has_guid) n += 1;
      return n;
    };
    return zf(dec) + zf(txt) + 1 + (dialog() ? 1 : 0);
  }

  // ---------------------------------------------------------------- launch helpers
  void small_linear(const Linear& L, const float* in, int ldin, int M, float* out, int ldout,
                    int pre, const float* add, hipStream_t s) {
    launch_small_linear(in, ldin, L.w32, L.K, L.b, add, out, ldout, M, L.N, L.K, pre, -1, s);
  }

  bool fp8_mode() const { return cfg.precision == ZV_FP8; }

  // ---------------------------------------------------------------- fused attention consumers
  // NonlinAttention's head-0 consumer: the second-generation kernel (a2), the Toeplitz MFMA scoring
  // (tp_na) or the VALU form (attn_na_v1, zv_flash.inc)
  template <int SPLIT>
  void attn_na(const FlashParams& f, int hid, bool a2, bool tp_na, hipStream_t s) {
    if constexpr (SPLIT == 1) {
      if (a2) return launch_attn_na_b2(f, hid, na_b2_form(f.L), s);
      if (tp_na) return attn_na_v1<1, 1>(f, hid, s);
    }
    attn_na_v1<SPLIT, 0>(f, hid, s);
  }
  // SelfAttention's consumer
  template <int SPLIT>
  void attn_sa(const FlashParams& f, bool a2, hipStream_t s) {
    if constexpr (SPLIT == 1) {
      if (a2) return launch_attn_sa_b2(f, sa_b2_form(f.L), s);
      if (sa_tp) {                 // positional term as a Toeplitz MFMA product
        if (sa_tp == 3) launch_attn_sa_tp<0, 1>(f, s);   // A/B: the compiler's one-wave register budget
        else launch_attn_sa_tp<0>(f, s);
        return;
      }
    }
    launch_attn_sa<SPLIT>(f, s);
  }

  // ---------------------------------------------------------------- one layer
  // Zipformer2EncoderLayer.forward at inference (zipformer.py:489-642).
  // src/src_a: layer input (kept as src_orig, overwritten with the output);
  // cur/cur_a: src + temb on entry (working residual stream).
  template <int SPLIT>
  void layer(const Pass& pass, const ZipformerW& Z, const LayerW& W, Workspace& ws, float* src,
             Act src_a, float* cur, Act cur_a, int B, int L, const uint8_t* pad, const float* posP,
             const float* temb, bool has_next, hipStream_t s, bool fresh8 = false) {
    const bool split = SPLIT == 3;
    const long M = (long)B * L;
    // the batch's rows: the fused / unfused FeedForward choice must not depend on how the decoder
    // split its rows over streams (every row block makes the same choice; bitwise equal to one stream)
    const long Mtot = pass.batch_rows > 0 ? pass.batch_rows * (long)L : M;
    const int D = Z.dim, H = Z.heads;
    const long Lpad = round_up(L, 64);
    const char* tag_att = split ? "gemm_attn_fp32" : "gemm_attn_bf16";
    // posP: this layer's positional projection (2L-1, H*pd), written at stack entry
    // attention weights from the layer input (zipformer.py:526)
    const int qkpN = W.attn_in.N;
    Act qkp = ws.qkp.get(M, qkpN, split);
    {
      // mixed mode: the attention-score projection as a weight-split product (attn_in_wsplit;
      // the fully split form is retired, zv_linear.inc); q, k, p stay 16-bit
      Out o; o.act = qkp;
      if (SPLIT == 1 && pass.io_split) attn_in_wsplit(W.attn_in, src_a, M, o, s);
      else linear<SPLIT>(W.attn_in, src_a, M, o, s);
    }
    // head-0 scoring of the stats / NonlinAttention pair: Toeplitz MFMA form in the 16-bit modes
    // (the fp16 parity mode included, without the table's lo half, which would not fit the
    // NonlinAttention image at dialog lengths; profiles/r03_mixed_ab.txt, zv_linear.inc)
    const bool tp_na = SPLIT == 1 && sa_tp;
    // attention: either materialise W (reference structure; A/B path, and the
    // fallback for lengths whose fused LDS images do not fit) or keep only
    // per-row softmax statistics and recompute scores inside each consumer
    // (sa_plo 0: no mode keeps the lo half of the SelfAttention Toeplitz table)
    const int sa_plo = (SPLIT == 1 && sa_tp) ? 0 : -1;
    // second-generation consumers (zv_flash2.inc: base-2 scores from the log2(e)-scaled k / p
    // weights, no running maximum, no statistics pass) wherever this stack's weights were built for
    // them (Z.b2: the bf16 / fp8 engines, and the fp16 parity mode's decoder)
    const bool a2 = SPLIT == 1 && Z.b2;
    const bool materialize = materialize_attn || (a2 ? !fused_attn2_fits(L, W.na_in.N / 3)
                                                     : !fused_attn_fits<SPLIT>(L, W.na_in.N / 3, sa_plo, tp_na ? 1 : 0));
    Act Wt;
    FlashParams fp{};
    if (materialize) {
      Wt = ws.W.get((long)H * M, Lpad, split);
      AttnParams ap{qkp.h, qkp.l, qkpN, posP, pad, Wt.h, Wt.l, Lpad, B, L, H, a2 ? 1 : 0};
      launch_attn_softmax<SPLIT>(ap, s);
    } else {
      fp.qh = qkp.h; fp.ql = qkp.l; fp.ldq = qkpN; fp.P = posP; fp.key_pad = pad;
      fp.B = B; fp.L = L; fp.H = H;
      fp.force_exact = attn2_exact; fp.fallback = attn_fallback;
      if (!a2) {
        fp.stats = ws.stats.get<float2>((size_t)M);     // head 0 only (NonlinAttention)
        if constexpr (SPLIT == 1)
          if (tp_na) launch_attn_stats<1, 1>(fp, s);
          else launch_attn_stats<1>(fp, s);
        else launch_attn_stats<SPLIT>(fp, s);
      }
    }
    // fp8 mode: the working stream also carries an MX-fp8 copy (the A operand of the fp8
    // feed-forward / convolution in-projections), written by every producer of the stream:
    // the residual linears' epilogues, the previous layer's BiasNorm (fresh8); packed here only
    // at a stack's first layer
    const bool f8 = SPLIT == 1 && fp8_mode() && W.ff_in[0].q8 != nullptr;
    Act c8;
    if (f8) {
      c8 = ws.cur8.get(M, D, false, true, D, false);
      cur_a.q = c8.q; cur_a.qs = c8.qs; cur_a.ldq = c8.ldq;
      if (!fresh8 || !(fp8_fuse & 4)) pack8(cur_a, M, D, s);
    }
    Out res;                       // cur = cur + module(cur), with the hi/lo copy
    res.C = cur; res.ldc = D; res.resid = cur; res.act = cur_a;
    // fused FeedForward module f on the working stream: its operands (a site adds its epilogue's)
    auto ffn_params = [&](int f) {
      FfnParams q{};
      q.H = W.ff_in[f].N; q.nseg = 1;
      q.seg[0].M = (int)M; q.seg[0].X = cur_a.h; q.ldx = cur_a.ld;
      q.W1f = W.ffn_w1f[f]; q.b1 = W.ff_in[f].b; q.W2f = W.ffn_w2f[f]; q.b2 = W.ff_out[f].b;
      return q;
    };
    std::function<void(FfnParams&, int)> ffn_pre_operands;   // (set below, where [dw | o] is known)
    auto ff = [&](int f, const Out& oe, int pre_c = -1) {
      if constexpr (SPLIT == 1) {
        if (ffn_fused && W.ffn_w1f[f] && !(f8 && W.ff_in[f].q8) && oe.C && oe.resid &&
            !oe.act.l && !oe.residh && Mtot >= ffn_min_rows && cur_a.ld % 8 == 0) {
          FfnParams q = ffn_params(f);
          FfnSeg& g = q.seg[0];
          g.resid = oe.resid; g.C = oe.C; q.ldc = oe.ldc; g.Ch = oe.act.h; q.ldch = oe.act.ld;
          g.rowvec = oe.rowvec; q.rowvec_ld = oe.rowvec_ld; q.rows_per_group = oe.rows_per_group;
          g.orig = oe.orig; q.byp = oe.byp;
          if (pre_c >= 0) ffn_pre_operands(q, pre_c);
          ffn_site(q, ws, s, "ffn_bf16");
          return;
        }
      }
      ZV_REQUIRE(pre_c < 0, "the pre-projection site fell off the fused FeedForward");
      // fp8: the SwooshL output only as the fp8 out-projection's operand (decided per in/out
      // pair: a 16-bit out-projection reads the bf16 hidden copy)
      const bool f8f = f8 && W.ff_in[f].q8 && W.ff_out[f].q8;
      Act hid = ws.hidden.get(M, W.ff_in[f].N, split, f8f, W.ff_in[f].N, !f8f);
      Out o1; o1.act = hid; o1.act_fn = 1;          // SwooshL fused (scaling.py:1322-1334)
      linear<SPLIT>(W.ff_in[f], cur_a, M, o1, s);
      linear<SPLIT>(W.ff_out[f], hid, M, oe, s);
    };
    {
      // FF1 (:536): its residual is the layer input + the time embedding (src + temb, what the
      // working stream holds on entry): read from src with the row vector, so neither BiasNorm
      // nor the stack entry writes the fp32 working stream (only its bf16 / fp8 copies)
      Out e1 = res;
      e1.resid = src;
      if (temb) { e1.rowvec = temb; e1.rowvec_ld = D; e1.rows_per_group = L; }
      ff(0, e1);
    }
    {                                                 // NonlinAttention (:542-562)
      const int hid = W.na_in.N / 3;
      Act y = ws.na_y.get(M, hid, split);
      Act xt = ws.na_xt.get((long)B * hid, Lpad, split);
      GemmParams p = gp_linear(W.na_in, cur_a, M);
      p.Ch = y.h; p.Cl = y.l; p.ldch = y.ld;
      p.Cth = xt.h; p.Ctl = xt.l; p.ldct = Lpad; p.rpb = L; p.sCt = (long)hid * Lpad;
      launch_na_in<SPLIT>(p, s);
      Act nao = ws.na_o.get(M, round_up(hid, 64), split, f8, hid);
      if (materialize) {
        GemmParams q{};
        q.M = L; q.N = hid; q.K = L; q.nz2 = B; q.Brows = hid;
        q.Ah = Wt.h; q.Al = Wt.l; q.lda = Lpad; q.sA2 = (long)L * Lpad;     // head 0
        q.Bh = xt.h; q.Bl = xt.l; q.ldb = Lpad; q.sB2 = (long)hid * Lpad;
        q.Ch = nao.h; q.Cl = nao.l; q.ldch = nao.ld; q.sCh2 = (long)L * nao.ld;
        q.mulh = y.h; q.mull = y.l; q.ldmul = y.ld; q.smul2 = (long)L * y.ld;
        q.rows_per_group = 1; q.rpb = 1;
        launch_gemm<128, 128, 2, 2, SPLIT, EPI_STD>(q, B, s, tag_att);
      } else {
        FlashParams f = fp;
        f.vh = xt.h; f.vl = xt.l; f.ldv = Lpad; f.sv_b = (long)hid * Lpad; f.vrows_per_head = 0;
        f.nv = hid;
        f.mulh = y.h; f.mull = y.l; f.ldmul = y.ld;
        f.oh = nao.h; f.ol = nao.l; f.ldo = nao.ld; f.ocol_per_head = 0;
        attn_na<SPLIT>(f, hid, a2, tp_na, s);
      }
      if (f8) pack8(nao, M, hid, s);
      linear<SPLIT>(W.na_out, nao, M, res, s);
    }
    // bf16 mode: the SelfAttention output lands next to the depthwise-conv output ([dw | o],
    // K = D + HV) and the convolution out-projection [conv_out | sa_out] finishes both residual
    // updates in one GEMM; the SelfAttention out-projection itself only writes the bf16 copy of
    // the stream the convolution module reads (cur + sa + temb: 6 B per element, not 10)
    const bool kcat = SPLIT == 1 && !f8 && temb && W.conv_sa_out[0].hi &&
                      !materialize && (W.conv_sa_out[0].K == D + H * Z.vd || sa_tp);
    Act dwo;
    if (kcat) dwo = ws.dwo.get(M, round_up(W.conv_sa_out[0].K, 64), false);
    // fp16 parity mode's split SelfAttention products (mixed_sa; the weights were built for it)
    const bool sa_split = kcat && pass.io_split && W.conv_sa_out[0].K == D + 3 * H * Z.vd;
    ZV_REQUIRE(!kcat || sa_split || W.conv_sa_out[0].K == D + H * Z.vd, "conv + SelfAttention out-projection width");
    // ZV_FFN=3: conv(c)'s K-concatenated out-projection runs as the first phase of the fused
    // FeedForward behind it (FF2 with bypass_mid, FF3 with BiasNorm + bypass), under exactly the
    // conditions that put that FeedForward on the fused kernel; decided on the batch's rows
    const bool ffn_norm = SPLIT == 1 && ffn_fused >= 2 && W.ffn_w1f[2] && !f8 && D == FFN_D &&
                          Mtot >= ffn_min_rows && cur_a.ld == src_a.ld && cur_a.ld % 8 == 0;
    auto pre_fits = [&](int c) {
      return kcat && ffn_fused >= 3 && D == FFN_D && W.ffn_w1fp[c + 1] && W.ffn_wpf[c] && !cur_a.l &&
             Mtot >= ffn_min_rows && cur_a.ld % 8 == 0 && dwo.ld % 8 == 0 &&
             dwo.ld >= (long)ffn_pre_chunks(W.conv_sa_out[c].K) * FFN_HC;
    };
    const bool pre_site[2] = {pre_fits(0), pre_fits(1) && ffn_norm};
    ffn_pre_operands = [&](FfnParams& q, int c) {
      FfnSeg& g = q.seg[0];
      g.X = nullptr; g.A = dwo.h; q.lda = dwo.ld;
      q.W1f = W.ffn_w1fp[c + 1]; q.Wpf = W.ffn_wpf[c]; q.bp = W.conv_sa_out[c].b;
      q.nkp = ffn_pre_chunks(W.conv_sa_out[c].K);
      g.rowvec = temb; q.rowvec_ld = D; q.rows_per_group = L;
    };
    auto self_attn = [&](int a) {                     // SelfAttention (:564-570, :600-606)
      const int vd = Z.vd, HV = H * vd;
      // V^T rows per head: vd, or 16 where the value projection was built padded (sa_vpad: rows
      // [12 values | ones | 3 zeros] per head, the second-generation kernel's operand)
      const int VR = W.sa_in[a].N, vph = VR / H;
      Act vt = ws.sa_vt.get((long)B * VR, Lpad, split);
      Act o = ws.sa_o.get(M, 64, split);
      if (kcat) { o = dwo; o.h += D; }               // columns [D, D + HV) of [dw | o]
      GemmParams p = gp_linear(W.sa_in[a], cur_a, M);
      p.Cth = vt.h; p.Ctl = vt.l; p.ldct = Lpad; p.rpb = L; p.sCt = (long)VR * Lpad;
      launch_value_t<SPLIT>(p, sa_split, W.sa_in[a].lo != nullptr, s);
      if (materialize) {
        GemmParams q{};
        q.M = L; q.N = vd; q.K = L; q.nz2 = B; q.Brows = vd;
        q.Ah = Wt.h; q.Al = Wt.l; q.lda = Lpad; q.sA1 = M * Lpad; q.sA2 = (long)L * Lpad;
        q.Bh = vt.h; q.Bl = vt.l; q.ldb = Lpad; q.sB1 = (long)vph * Lpad; q.sB2 = (long)VR * Lpad;
        q.Ch = o.h; q.Cl = o.l; q.ldch = o.ld; q.sCh1 = vd; q.sCh2 = (long)L * o.ld;
        q.rows_per_group = 1; q.rpb = 1;
        launch_gemm<128, 16, 4, 1, SPLIT, EPI_STD>(q, H * B, s, tag_att);
      } else {
        FlashParams f = fp;
        f.vh = vt.h; f.vl = vt.l; f.ldv = Lpad; f.sv_b = (long)VR * Lpad; f.vrows_per_head = vph;
        f.nv = vd;
        f.oh = o.h; f.ol = o.l; f.ldo = o.ld; f.ocol_per_head = vd;
        if (sa_split) { f.ol = o.h + HV; f.oh2 = o.h + 2 * HV; }   // [o_hi | o_lo | o_hi]
        attn_sa<SPLIT>(f, a2, s);
      }
      Out e = res;
      if (temb) { e.rowvec = temb; e.rowvec_ld = D; e.rows_per_group = L; }
      if (kcat) e.C = nullptr;                        // fp32 update: the conv out-projection's
      linear<SPLIT>(W.sa_out[a], o, M, e, s);         // (+ the stream's fp8 copy)
    };
    auto conv = [&](int c) {                          // ConvolutionModule (:1638-1680)
      const bool g8 = f8 && W.conv_in[c].q8;
      Act dw = kcat ? dwo : ws.dw.get(M, D, split, f8, D);
      bool fused = false;
      if constexpr (SPLIT == 1) {
        // in_proj + GLU + masked_fill + depthwise conv + SwooshR in one launch: the GLU output
        // never reaches HBM (zv_gemm256.inc, g256_epi_glu_dw)
        if (glu_dw && !f8) {
          GemmParams p = gp_linear(W.conv_in[c], cur_a, M);
          p.Ch = dw.h; p.ldch = dw.ld; p.rowmask = pad;
          p.dw_w = W.dw_w[c]; p.dw_b = W.dw_b[c]; p.dw_out = dw.h; p.ld_dw = dw.ld; p.dw_L = L;
          fused = glu_dw_fits(p, D, W.ks);
          if (fused) launch_glu_dw(p, W.ks, s, "gemm_bf16_glu_dw");
        }
      }
      if (!fused) {
        Act g = ws.glu.get(M, D, split);
        GemmParams p = g8 ? gp_linear8(W.conv_in[c], cur_a, M) : gp_linear(W.conv_in[c], cur_a, M);
        p.Ch = g.h; p.Cl = g.l; p.ldch = g.ld; p.rowmask = pad;
        launch_glu_in<SPLIT>(p, g8, s);
        const bool dq = f8 && (fp8_fuse & 2);
        launch_dwconv(g.h, g.l, g.ld, W.dw_w[c], W.dw_b[c], dw.h, dw.l, dw.ld, B, L, D, W.ks, s,
                      dq ? dw.q : nullptr, dw.qs, dw.ldq);
        if (f8 && !dq) pack8(dw, M, D, s);
      }
      if (kcat && pre_site[c]) {
        // (the FeedForward behind this module runs the out-projection)
      } else if (kcat) {                              // cur += [dw | o] . [conv_out | sa_out]^T + temb
        Out e = res;
        e.rowvec = temb; e.rowvec_ld = D; e.rows_per_group = L;
        linear<SPLIT>(W.conv_sa_out[c], dw, M, e, s);
      } else {
        linear<SPLIT>(W.conv_out[c], dw, M, res, s);
      }
    };
    self_attn(0);                                     // SA1 (+ temb)
    conv(0);                                          // conv1
    {                                                 // FF2 + bypass_mid (:593-598)
      Out e = res; e.byp = W.bypass_mid;
      e.orig = src;
      ff(1, e, pre_site[0] ? 0 : -1);
    }
    self_attn(1);                                     // SA2 (+ temb)
    conv(1);                                          // conv2
    // FF3 + BiasNorm + bypass in the fused FeedForward kernel's norm epilogue (the FF3 output
    // never reaches HBM; zv_ffn.inc)
    if (ffn_norm) {
      FfnParams q = ffn_params(2);
      FfnSeg& g = q.seg[0];
      g.resid = cur; g.orig = src; g.C = src; q.ldc = D;
      g.Ch = src_a.h; g.Cl = src_a.l; q.ldch = src_a.ld;
      q.byp = W.bypass; q.nb = W.norm_bias; q.log_scale = W.norm_log_scale;
      g.rowvec = temb; q.rowvec_ld = D; q.rows_per_group = L;
      g.C2h = has_next ? cur_a.h : nullptr; g.C2l = has_next ? cur_a.l : nullptr;
      if (pre_site[1]) ffn_pre_operands(q, 1);
      ffn_site(q, ws, s, "ffn_norm_bf16");
    } else {                                          // FF3: only the fp32 stream feeds BiasNorm
      Out e = res;                                    // (which rewrites both copies): no bf16 copy
      e.act = Act{};
      ff(2, e);
    }
    // BiasNorm + bypass -> src; next layer's working copy (src + temb) -> cur
    if (!ffn_norm) {
      // fp8: the next layer's working stream's fp8 copy as well (its fresh8)
      const bool q2 = f8 && has_next && (fp8_fuse & 4);
      ZV_REQUIRE(!q2 || D % 256 == 0, "fp8 BiasNorm copy: channels a multiple of 256");
      launch_biasnorm_bypass(cur, src, W.norm_bias, W.norm_log_scale, W.bypass, src, src_a.h, src_a.l,
                             has_next ? cur_a.h : nullptr, has_next ? cur_a.l : nullptr, D, temb, L, M, D,
                             q2 ? c8.q : nullptr, q2 ? c8.qs : nullptr, q2 ? c8.ldq : 0L, s);
    }
  }

  // ---------------------------------------------------------------- one stack
  template <int SPLIT>
  void stack(const Pass& pass, const ZipformerW& Z, const StackW& S, int si, Workspace& ws, float* src,
             Act src_a, int B, int L, const uint8_t* pad, const float* temb, hipStream_t s) {
    const long M = (long)B * L;
    const bool split = SPLIT == 3;
    float* cur = ws.cur.get<float>(M * Z.dim);
    Act cur_a = ws.cur_a.get(M, Z.dim, split);
    // the fp32 working stream is not written here: the first layer's FF1 reads src + temb
    launch_stack_entry(src, temb, nullptr, src_a.h, src_a.l, cur_a.h, cur_a.l, Z.dim, M, Z.dim, L, s);
    // positional encoding of length L and every layer's linear_pos projection of it, in one
    // launch into the workspace (zipformer.py:983-1056, :1239): no host table, no cache, no
    // synchronisation, graph-capturable.  It depends on L and the stack's weights only: inside
    // one Euler solve the first step writes it into the stack's own buffer and the later steps
    // (same rows, same L, same workspace per row block) read it again (posp_reuse)
    const int R = 2 * L - 1, HPD = Z.heads * Z.pd, nl = (int)S.layers.size();
    const size_t pn = (size_t)std::max(nl, 1) * R * HPD;
    const bool own = si >= 0 && si < Workspace::POSP_STACKS;
    float* posP = own ? ws.posPs[si].get<float>(pn) : ws.posP.get<float>(pn);
    bool reuse = false;
    if (own) {
      Workspace::PosPKey& k = ws.posk[si];
      reuse = pass.posp_reuse && k.L == L && k.nl == nl && k.w == S.pos_w_all && k.buf == posP;
      k = Workspace::PosPKey{L, nl, S.pos_w_all, posP};
    }
    if (!reuse) launch_posp(S.pos_w_all, posP, L, nl, HPD, Z.pos_dim, s);
    for (size_t li = 0; li < S.layers.size(); ++li)
      layer<SPLIT>(pass, Z, S.layers[li], ws, src, src_a, cur, cur_a, B, L, pad,
                   posP + li * (size_t)R * HPD, temb, li + 1 < S.layers.size(), s, li > 0);
  }

  // ---------------------------------------------------------------- TTSZipformer
  // TTSZipformer.forward (zipformer.py:242-293).  xin: bf16 hi/lo (N*T, Fin); t/g (N).
  template <int SPLIT>
  void zipformer(const Pass& pass, const ZipformerW& Z, Workspace& ws, Act xin, int sidx, int N,
                 int T, const uint8_t* pad, const float* t, const float* g, float* out, hipStream_t s) {
    const long M = (long)N * T;
    const int D = Z.dim;
    const bool split = SPLIT == 3;
    float* main = ws.main.get<float>(M * D);
    // mixed mode: the input / output projections as split products (xin and the last
    // BiasNorm's copy main_a carry the lo halves)
    const bool ios = SPLIT == 1 && pass.io_split;
    Act main_a = ws.main_a.get(M, D, split || ios);
    {
      Out o; o.C = main; o.ldc = D;
      if (ios) linear<3>(Z.in_proj[sidx], xin, M, o, s);
      else linear<SPLIT>(Z.in_proj[sidx], xin, M, o, s);
    }
    // time embedding MLP (zipformer.py:267-278) + per-stack projections (:726-729)
    float* tstack = nullptr;
    if (Z.has_time) {
      const int E = Z.temb_dim;
      float* e0 = ws.temb0.get<float>((size_t)N * 2 * E);
      float* e1 = ws.temb1.get<float>((size_t)N * 2 * E);
      launch_timestep_embed(t, temb_freqs, e0, N, E, s);
      if (Z.has_guid) {
        launch_timestep_embed(g, temb_freqs, e1, N, E, s);
        small_linear(Z.guid, e1, E, N, e0, E, 0, e0, s);   // e0 += guidance_scale_embed(e1)
      }
      small_linear(Z.te0, e0, E, N, e1, 2 * E, 0, nullptr, s);
      small_linear(Z.te2, e1, 2 * E, N, e0, E, 1, nullptr, s);
      tstack = ws.tstack.get<float>(Z.stacks.size() * (size_t)N * D);
      for (size_t si = 0; si < Z.stacks.size(); ++si)
        small_linear(Z.stacks[si].time_emb, e0, E, N, tstack + si * (size_t)N * D, D, 1, nullptr,
                     s);
    }
    // the rows' lengths, once for all downsampled stacks (the mask is at full rate).  The table is
    // taken in either mode, so a reservation made in one sizes the other; without a mask there is
    // no row end to honour and the batch kernel runs
    const int* nrow = nullptr;
    if (pad && std::any_of(Z.stacks.begin(), Z.stacks.end(), [](const StackW& S) { return S.ds > 1; })) {
      int* n = ws.rowlen.get<int>((size_t)N);
      if (padding == ZV_PAD_ROW) {
        launch_row_len(pad, n, N, T, s);
        nrow = n;
      }
    }
    for (size_t si = 0; si < Z.stacks.size(); ++si) {
      const StackW& S = Z.stacks[si];
      const float* te = tstack ? tstack + si * (size_t)N * D : nullptr;
      if (S.ds == 1) {
        stack<SPLIT>(pass, Z, S, (int)si, ws, main, main_a, N, T, pad, te, s);
      } else {
        const int dL = (T + S.ds - 1) / S.ds;
        float* d = ws.dsrc.get<float>((size_t)N * dL * D);
        Act d_a = ws.dsrc_a.get((long)N * dL, D, split || ios);
        if (nrow) launch_downsample_row(main, d, nrow, N, T, dL, D, S.ds, S.ds_w, s);
        else launch_downsample(main, d, N, T, dL, D, S.ds, S.ds_w, s);
        uint8_t* pds = nullptr;
        if (pad) {
          pds = ws.maskds.get<uint8_t>((size_t)N * dL);
          launch_mask_downsample(pad, pds, N, T, dL, S.ds, s);
        }
        stack<SPLIT>(pass, Z, S, (int)si, ws, d, d_a, N, dL, pds, te, s);
        launch_upsample_combine(main, d, S.combiner, main, N, T, dL, D, S.ds, s);
      }
    }
    // factors end with 1: the last stack's final BiasNorm wrote main_a
    ZV_REQUIRE(Z.stacks.back().ds == 1, "last stack must have downsampling factor 1");
    {
      Out o; o.C = out; o.ldc = Z.out_proj[sidx].N;
      if (ios) linear<3>(Z.out_proj[sidx], main_a, M, o, s);
      else linear<SPLIT>(Z.out_proj[sidx], main_a, M, o, s);
    }
  }

  Act build_xin(Workspace& ws, const float* x, const float* tc, const float* sc, int B, int T,
                int Fx, int copies, int zero_speech, hipStream_t s) {
    const int Ft = cfg.feat_dim, Fin = 2 * Fx + Ft;
    const bool split = cfg.precision == ZV_FP32 || cfg.precision == ZV_MIXED;   // split input projection
    const long N = (long)copies * B;
    Act xin = ws.xin.get(N * T, round_up(Fin, 64), split);
    launch_build_input(x, tc, sc, xin.h, xin.l, xin.ld, B, T, Fx, Ft, Fx, copies, zero_speech, s);
    return xin;
  }

  void decoder_rows(const Pass& pass, Workspace& ws, Act xin, int sidx, int N, int T,
                    const uint8_t* pad, const float* t, const float* g, float* out, hipStream_t s) {
    if (cfg.precision == ZV_FP32) zipformer<3>(pass, dec, ws, xin, sidx, N, T, pad, t, g, out, s);
    else zipformer<1>(pass, dec, ws, xin, sidx, N, T, pad, t, g, out, s);
  }

  // whether a guided call doubles its rows (conditional + unconditional copies), and whether a
  // decoder call of N rows of T frames runs its row blocks on their own streams
  bool cfg_doubles(float g, const float* grows, bool cfg_rows) const {
    return cfg_plan(0.f, g, grows != nullptr, cfg_rows, distill()).copies == 2;
  }
  bool splits_rows(long N, int T) const { return split_streams >= 2 && N >= 2 && N * T >= split_min_rows; }

  // posp_reuse: a later Euler step of one solve (Pass::posp_reuse)
  void decoder(Act xin, int Fin, int N, int T, const uint8_t* pad, const float* t, const float* g,
               float* out, bool posp_reuse, hipStream_t s) {
    int sidx = 0;
    if (stereo()) sidx = (Fin == dec.in_proj[0].K) ? 0 : 1;
    ZV_REQUIRE(Fin == dec.in_proj[sidx].K, "decoder input width does not match in_proj");
    Pass pass;
    pass.io_split = cfg.precision == ZV_MIXED;
    pass.posp_reuse = posp_reuse;
    // (profiled passes run the same launches as the timed ones -- the same row blocks, kernels and
    // shapes -- but one row block after another on the caller's stream, so each launch's events time
    // it alone: with the blocks overlapping on three streams an event pair timed the co-running
    // kernels as well; rocprofv3's kernel trace serialises the dispatches the same way)
    if (!splits_rows(N, T)) {
      decoder_rows(pass, ws_dec, xin, sidx, N, T, pad, t, g, out, s);
      return;
    }
    // Independent row blocks on their own streams (rows never interact on this path): the
    // kernels of one block (GEMMs: MFMA/LDS) co-run with another block's (attention: VALU;
    // epilogues: HBM) instead of the whole batch passing each kernel in lock step.
    // Bitwise equal to the single-stream decoder (tests/test_gpu_split_streams.py): every kernel
    // choice that depends on a row count takes the batch's (Pass::batch_rows), not the row block's.
    const int parts = std::min(split_streams, std::min(N, MAX_SPLIT));
    if (!split_fork) {
      ZV_CHECK(ZV_BLOCKING(hipEventCreateWithFlags(&split_fork, hipEventDisableTiming)));
      for (int i = 0; i < MAX_SPLIT - 1; ++i)
        ZV_CHECK(ZV_BLOCKING(hipEventCreateWithFlags(&split_join[i], hipEventDisableTiming)));
    }
    for (int i = 1; i < parts; ++i)   // (only the streams this split uses)
      if (!split_stream[i - 1]) split_stream[i - 1] = engine_stream(i - 1);
    const int outN = dec.out_proj[sidx].N;
    ZV_CHECK(hipEventRecord(split_fork, s));
    pass.batch_rows = N;   // every row block makes the batch's fused / unfused FeedForward choice
    int r0 = 0;
    for (int i = 0; i < parts; ++i) {
      const int n = N / parts + (i < N % parts ? 1 : 0);
      const long rows = (long)r0 * T;
      Act xi = xin;
      xi.h += rows * xin.ld;
      if (xin.l) xi.l += rows * xin.ld;
      const bool serial = g_zv_prof.on;
      hipStream_t si = (i == 0 || serial) ? s : split_stream[i - 1];
      if (i > 0 && !serial) ZV_CHECK(hipStreamWaitEvent(si, split_fork, 0));
      Workspace* wsi = i == 0 ? &ws_dec : &ws_split[i - 1];
      const uint8_t* padi = pad ? pad + rows : nullptr;
      const float* ti = t + r0;
      const float* gi = g ? g + r0 : nullptr;
      float* oi = out + rows * outN;
      decoder_rows(pass, *wsi, xi, sidx, n, T, padi, ti, gi, oi, si);
      r0 += n;
    }
    for (int i = 1; i < parts && !g_zv_prof.on; ++i) {
      ZV_CHECK(hipEventRecord(split_join[i - 1], split_stream[i - 1]));
      ZV_CHECK(hipStreamWaitEvent(s, split_join[i - 1], 0));
    }
  }

  // guided velocity at scalar t for B un-doubled rows (solver.py:40-165).
  // grows (device, B floats, may be null): per-utterance guidance scales, the reference's
  // guidance_scale tensor of shape (batch, 1, 1); cfg_on says whether any is nonzero
  // ((guidance_scale == 0.0).all() selects the unguided branch, solver.py:71)
  void velocity(float t, float gscale, const float* grows, bool cfg_rows, const float* x,
                const float* tc, const float* sc, const uint8_t* pad, int B, int T, float* vout,
                bool euler, float dt, bool posp_reuse, hipStream_t s) {
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim;
    const int Fin = 2 * Fx + cfg.feat_dim;
    const CfgPlan plan = cfg_plan(t, gscale, grows != nullptr, cfg_rows, distill());
    const bool cfg_on = plan.copies == 2;
    const int copies = plan.copies, zero_speech = plan.zero_speech;
    const int N = copies * B;
    const float g = plan.g, gmul = plan.gmul;
    Act xin = build_xin(ws_dec, x, tc, sc, B, T, Fx, copies, zero_speech, s);
    const uint8_t* padN = pad;
    if (pad && copies == 2) {
      uint8_t* p2 = ws_dec.mask2.get<uint8_t>((size_t)N * T);
      launch_copy_u8(pad, p2, (long)B * T, 2, s);
      padN = p2;
    }
    float* tv = ws_dec.tvec.get<float>(N);
    launch_fill(tv, t, N, s);
    const float* gv = nullptr;
    if (distill()) {
      if (grows) {
        gv = grows;   // the guidance embedding takes the per-row scales as they are
      } else {
        float* g1 = ws_dec.gvec.get<float>(N);
        launch_fill(g1, gscale, N, s);
        gv = g1;
      }
    }
    const long n = (long)B * T * Fx;
    float* v = (copies == 2 || euler) ? ws_dec.vout.get<float>((size_t)N * T * Fx) : vout;
    decoder(xin, Fin, N, T, padN, tv, gv, v, posp_reuse, s);
    const float* gr = cfg_on ? grows : nullptr;
    if (euler) {
      launch_euler_update(const_cast<float*>(x), v, n, copies == 2 ? 1 : 0, g, dt, gr, gmul, (long)T * Fx, s);
    } else if (copies == 2) {
      launch_cfg_combine(vout, v, n, g, gr, gmul, (long)T * Fx, s);
    }
  }

  void euler_loop(float* x, const float* tc, const float* sc, const uint8_t* pad, int B, int T,
                  const std::vector<float>& ts, float g, const float* grows, bool cfg_rows,
                  hipStream_t s) {
    const int num_step = (int)ts.size() - 1;
    // steps after the first reuse the stacks' positional projections (same shapes and row
    // blocks every step; a graph replays the first step's launches)
    for (int k = 0; k < num_step; ++k)
      velocity(ts[k], g, grows, cfg_rows, x, tc, sc, pad, B, T, nullptr, true, ts[k + 1] - ts[k], k > 0, s);
  }

  // zv_euler_sample body: graph replay when possible, plain launches otherwise
  void euler_sample(float* x, const float* tc, const float* sc, const uint8_t* pad, int B, int T,
                    int num_step, float g, const float* grows, bool cfg_rows, float t0, float t1,
                    float shift, hipStream_t s) {
    const std::vector<float> ts = solve_time_steps(t0, t1, num_step, shift);
    bool graph = graph_mode != 0 && !g_zv_prof.on;
    if (graph && graph_mode == 2)     // no graph where the decoder splits its (CFG-doubled) rows
      graph = !splits_rows((cfg_doubles(g, grows, cfg_rows) ? 2L : 1L) * B, T);
    if (!graph) {
      euler_loop(x, tc, sc, pad, B, T, ts, g, grows, cfg_rows, s);
      return;
    }
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim;
    const size_t nx = (size_t)B * T * Fx, nt = (size_t)B * T * cfg.feat_dim;
    // staging buffers first (they count towards the workspace generation)
    float* sx = gx.get<float>(nx);
    float* stc = gtc.get<float>(nt);
    float* ssc = gsc.get<float>(nx);
    uint8_t* spad = pad ? gpad.get<uint8_t>((size_t)B * T) : nullptr;
    float* sgr = grows ? ggrows.get<float>((size_t)B) : nullptr;
    GraphKey key{B, T, num_step, pad ? 1 : 0, grows ? 0.f : g, t0, t1, shift,
                 grows ? (cfg_rows ? 1 : 2) : 0, padding, g_ws_generation};
    auto it = graphs.find(key);
    // seen-once shapes are keyed without the workspace generation: the warm-up run itself grows
    // the workspace, and the next call of the shape should capture, not warm up again
    GraphKey seen_key = key;
    seen_key.gen = 0;
    if (it == graphs.end() && graph_seen[seen_key] == 0) {
      if (graph_seen.size() > MAX_SEEN) { graph_seen.clear(); graph_seen[seen_key] = 0; }
      graph_seen[seen_key] = 1;                  // warm-up: sizes the workspace
      euler_loop(x, tc, sc, pad, B, T, ts, g, grows, cfg_rows, s);
      return;
    }
    if (!gstream) {
      gstream = engine_stream(MAX_SPLIT - 1);
      ZV_CHECK(ZV_BLOCKING(hipEventCreateWithFlags(&gev_in, hipEventDisableTiming)));
      ZV_CHECK(ZV_BLOCKING(hipEventCreateWithFlags(&gev_out, hipEventDisableTiming)));
    }
    ZV_CHECK(hipEventRecord(gev_in, s));
    ZV_CHECK(hipStreamWaitEvent(gstream, gev_in, 0));
    ZV_CHECK(hipMemcpyAsync(sx, x, nx * 4, hipMemcpyDeviceToDevice, gstream));
    ZV_CHECK(hipMemcpyAsync(stc, tc, nt * 4, hipMemcpyDeviceToDevice, gstream));
    ZV_CHECK(hipMemcpyAsync(ssc, sc, nx * 4, hipMemcpyDeviceToDevice, gstream));
    if (pad) ZV_CHECK(hipMemcpyAsync(spad, pad, (size_t)B * T, hipMemcpyDeviceToDevice, gstream));
    if (grows) ZV_CHECK(hipMemcpyAsync(sgr, grows, (size_t)B * 4, hipMemcpyDeviceToDevice, gstream));
    if (it == graphs.end()) {
      if (key.gen != g_ws_generation) drop_graphs();
      while (graphs.size() >= MAX_GRAPHS) evict_lru_graph();
      hipGraph_t graph = nullptr;
      ZV_CHECK(hipStreamBeginCapture(gstream, hipStreamCaptureModeThreadLocal));
      const unsigned long gen0 = g_ws_generation;
      try {
        euler_loop(sx, stc, ssc, spad, B, T, ts, g, sgr, cfg_rows, gstream);
      } catch (...) {
        (void)hipStreamEndCapture(gstream, &graph);
        if (graph) (void)ZV_BLOCKING(hipGraphDestroy(graph));
        throw;
      }
      ZV_CHECK(hipStreamEndCapture(gstream, &graph));
      ZV_REQUIRE(gen0 == g_ws_generation, "workspace moved during graph capture");
      hipGraphExec_t exec = nullptr;
      ZV_CHECK(ZV_BLOCKING(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)));
      ZV_CHECK(ZV_BLOCKING(hipGraphDestroy(graph)));
      it = graphs.emplace(key, GraphEntry{exec, 0}).first;
    }
    it->second.last_use = ++graph_clock;
    ZV_CHECK(hipGraphLaunch(it->second.exec, gstream));
    ZV_CHECK(hipMemcpyAsync(x, sx, nx * 4, hipMemcpyDeviceToDevice, gstream));
    ZV_CHECK(hipEventRecord(gev_out, gstream));
    ZV_CHECK(hipStreamWaitEvent(s, gev_out, 0));
  }

  // ---------------------------------------------------------------- scheduled solve
  // zv_euler_sample_sched body: rows with their own grids and scales in one solve (sched_plan,
  // zv_elem.inc).  The host plans every step and uploads one table per solve: per step the row map
  // [N], the decoder's t [N], the updates [A] and the guidance embedding's scales [A] (distill), so a
  // step's t / g vectors are slices of it (no fill launch).  Plain launches on the caller's stream.
  //
  // Staging: the table is written into a pinned slot and copied with hipMemcpyAsync; a one-thread
  // kernel queued behind the copy then writes the upload's sequence number into the slot's
  // host-mapped word.  A slot is taken again only when that word shows its last upload done (one
  // volatile host read: no runtime call, so a warm solve stays at zero host-blocking calls), a
  // fresh slot is allocated otherwise: solves queued back to back each keep their own table until
  // the GPU has read it.
  struct SchedSlot {
    unsigned* base = nullptr;   // pinned + mapped: word 0 the completion mark, the table from byte 64
    unsigned* mark_dev = nullptr;
    size_t cap = 0;             // table bytes
    unsigned issued = 0;
    bool idle() const { return *reinterpret_cast<volatile unsigned*>(base) == issued; }
  };
  std::vector<SchedSlot> sched_slots;
  DBuf sched_tab;
  int64_t sched_rows_run = 0, sched_steps_run = 0;
  SchedSlot& sched_slot(size_t bytes) {
    for (SchedSlot& sl : sched_slots)
      if (sl.cap >= bytes && sl.idle()) return sl;
    return sched_slot_new(bytes);
  }
  SchedSlot& sched_slot_new(size_t bytes) {
    SchedSlot sl;
    sl.cap = (size_t)round_up((long)std::max<size_t>(bytes, 64 * 1024), 4096);
    ZV_CHECK(ZV_BLOCKING(hipHostMalloc((void**)&sl.base, sl.cap + 64, hipHostMallocMapped | hipHostMallocPortable)));
    sl.base[0] = 0;
    ZV_CHECK(ZV_BLOCKING(hipHostGetDevicePointer((void**)&sl.mark_dev, (void*)sl.base, 0)));
    sched_slots.push_back(sl);
    return sched_slots.back();
  }
  // the first `words` words of a slot's table to the device table, the completion mark behind them
  // (the device table is sized for 64 KiB at least: tables of a few KB never move it)
  unsigned* sched_send(SchedSlot& sl, size_t words, hipStream_t s) {
    unsigned* dtab = sched_tab.get<unsigned>(std::max<size_t>(words, 16 * 1024));
    ZV_CHECK(hipMemcpyAsync(dtab, sl.base + 16, words * 4, hipMemcpyHostToDevice, s));
    sl.issued += 1;
    hipLaunchKernelGGL(zv_mark_kernel, dim3(1), dim3(1), 0, s, sl.mark_dev, sl.issued);
    ZV_LAUNCH_CHECK();
    return dtab;
  }

  void euler_sample_sched(float* x, const float* tc, const float* sc, const uint8_t* pad, int B, int T,
                          const SchedRow* rows, hipStream_t s) {
    const SchedPlan plan = sched_plan(rows, B, distill());
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim;
    const int Ft = cfg.feat_dim, Fin = 2 * Fx + Ft;
    const bool split = cfg.precision == ZV_FP32 || cfg.precision == ZV_MIXED;   // as build_xin
    // the table: 4-byte words, step after step
    struct Off { size_t map, t, upd, g; };
    std::vector<Off> off(plan.K);
    size_t words = 0;
    for (int k = 0; k < plan.K; ++k) {
      const SchedStep& st = plan.steps[k];
      const size_t N = (size_t)st.U + st.A;
      off[k] = Off{words, words + N, words + 2 * N, words + 2 * N + 5 * (size_t)st.A};
      words += 2 * N + 6 * (size_t)st.A;
    }
    static_assert(sizeof(SchedUpd) == 20, "SchedUpd is five 4-byte words");
    SchedSlot& sl = sched_slot(words * 4);
    unsigned* tab = sl.base + 16;
    for (int k = 0; k < plan.K; ++k) {
      const SchedStep& st = plan.steps[k];
      const int N = st.U + st.A;
      int* m = reinterpret_cast<int*>(tab + off[k].map);
      for (int j = 0; j < N; ++j) m[j] = sched_map_entry(st.src[j], st.zt[j] != 0, st.zs[j] != 0);
      memcpy(tab + off[k].t, st.t.data(), (size_t)N * 4);
      memcpy(tab + off[k].upd, st.upd.data(), (size_t)st.A * sizeof(SchedUpd));
      memcpy(tab + off[k].g, st.gdec.data(), (size_t)st.A * 4);
    }
    unsigned* dtab = sched_send(sl, words, s);
    sched_rows_run = 0;
    sched_steps_run = 0;
    for (int k = 0; k < plan.K; ++k) {
      const SchedStep& st = plan.steps[k];
      const int N = st.U + st.A;
      const int* map = reinterpret_cast<const int*>(dtab + off[k].map);
      Act xin = ws_dec.xin.get((long)N * T, round_up(Fin, 64), split);
      launch_build_input_map(x, tc, sc, xin.h, xin.l, xin.ld, map, N, T, Fx, Ft, Fx, s);
      const uint8_t* padN = pad;
      if (pad && !(st.U == 0 && st.A == B)) {     // (no copy and every row active: the batch is the input)
        uint8_t* p2 = ws_dec.mask2.get<uint8_t>((size_t)N * T);
        launch_gather_u8(pad, p2, map, N, T, s);
        padN = p2;
      }
      float* v = ws_dec.vout.get<float>((size_t)N * T * Fx);
      const float* tv = reinterpret_cast<const float*>(dtab + off[k].t);
      // distill: the conditional rows are the whole batch (U = 0), so the active-order scales are its g
      const float* gv = distill() ? reinterpret_cast<const float*>(dtab + off[k].g) : nullptr;
      decoder(xin, Fin, N, T, padN, tv, gv, v, k > 0, s);
      launch_euler_update_sched(x, v, reinterpret_cast<const SchedUpd*>(dtab + off[k].upd), st.A, (long)T * Fx, s);
      sched_rows_run += N;
      sched_steps_run += 1;
    }
  }

  // ---------------------------------------------------------------- solve session
  // zv_session_* bodies: continuous batching.  The scheduled solve with its state kept across calls: a
  // row enters a free slot between any two steps (admit), every tick runs one Euler step of each
  // active slot at the slot's own step index (session_tick, zv_session.inc: sched_step over the active
  // slots), and a finished row is read out and its slot freed (retire).  Rows never move: the tick's
  // row map gathers the active slots into the decoder batch at T_k = the longest active row.
  // Every table (admit / retire rows, the tick's map | t | updates | scales) goes up through the
  // scheduled solve's staging and device table; all of it is ordered on the caller's stream.  open
  // sizes the decoder workspace for 2 * slots rows of max_frames and leaves SESSION_STAGING staging
  // slots allocated, so a warm admit / tick / retire makes no host-blocking runtime call while no
  // more uploads than that are in flight.
  // posp_reuse is false on every tick.  The stack's key (stack<SPLIT>) is rewritten only where the
  // host code of stack<> runs; a replayed graph of zv_euler_sample runs its captured launch_posp into
  // the same buffers with its own L and leaves the key as it was, so between two calls the key does
  // not say what the buffers hold.  (The reuse inside one solve is safe: nothing else runs in it.)
  static constexpr size_t SESSION_STAGING = 8;
  std::vector<zv_session*> sessions;

  zv_session* session_open(int slots, int maxT) {
    ZV_REQUIRE(slots >= 1 && slots <= SESSION_MAX_SLOTS, "session: slots must be in [1, 32767]");
    ZV_REQUIRE(maxT >= 1, "session: max_frames must be at least 1");
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim, Ft = cfg.feat_dim;
    sess_check_sizes(maxT, Fx, Ft);
    std::unique_ptr<zv_session> q(new zv_session());
    q->slots = slots;
    q->maxT = maxT;
    const size_t nx = (size_t)slots * maxT * Fx, nt = (size_t)slots * maxT * Ft;
    q->dx = q->x.get<float>(nx);               // (zero-filled: every slot starts as an all-zero row)
    q->dtc = q->tc.get<float>(nt);
    q->dsc = q->sc.get<float>(nx);
    q->dpad = q->pad.get<uint8_t>((size_t)slots * maxT);
    q->rows.assign(slots, SchedRow{0, 0.f, 0.f, 0.f, 0.f});
    q->ts.resize(slots);
    q->lens.assign(slots, 0);
    q->done.assign(slots, 0);
    // the workspace, as zv_reserve: one uncaptured guided velocity over every slot at max_frames, and
    // the two buffers a tick takes that this velocity may not (distill has no copies)
    const size_t nrows = (distill() ? 1 : 2) * (size_t)slots;
    (void)ws_dec.mask2.get<uint8_t>(nrows * maxT);
    (void)ws_dec.vout.get<float>(nrows * maxT * Fx);
    DBuf bv;
    float* v = bv.get<float>(nx);
    velocity(0.25f, 1.0f, nullptr, false, q->dx, q->dtc, q->dsc, q->dpad, slots, maxT, v, false, 0.f, false, nullptr);
    ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
    (void)sched_tab.get<unsigned>(16 * 1024);
    while (sched_slots.size() < SESSION_STAGING) (void)sched_slot_new(0);
    q->eng = this;
    sessions.push_back(q.get());
    return q.release();
  }

  void session_admit(zv_session& q, int n, const int32_t* slot, const int32_t* len, const SchedRow* rows,
                     const float* x0, const float* tc0, const float* sc0, int T_in, hipStream_t s) {
    ZV_REQUIRE(n >= 1, "session: admit takes at least one row");
    ZV_REQUIRE(slot && len && rows && x0 && tc0 && sc0, "session: admit: null argument");
    ZV_REQUIRE(T_in >= 1, "session: admit: T_in must be at least 1");
    std::vector<char> seen(q.slots, 0);
    for (int i = 0; i < n; ++i) {
      const std::string at = "session: admit row " + std::to_string(i) + ": ";
      ZV_REQUIRE(slot[i] >= 0 && slot[i] < q.slots, at + "slot outside [0, slots)");
      ZV_REQUIRE(q.rows[slot[i]].num_step == 0, at + "slot is not free");
      ZV_REQUIRE(!seen[slot[i]], at + "slot named twice");
      seen[slot[i]] = 1;
      ZV_REQUIRE(len[i] >= 1 && len[i] <= T_in && len[i] <= q.maxT, at + "length must be in [1, min(T_in, max_frames)]");
      sched_check_row(rows[i], at);
    }
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim, Ft = cfg.feat_dim;
    static_assert(sizeof(SessRow) == 8, "SessRow is two 4-byte words");
    SchedSlot& sl = sched_slot((size_t)n * sizeof(SessRow));
    SessRow* tab = reinterpret_cast<SessRow*>(sl.base + 16);
    for (int i = 0; i < n; ++i) tab[i] = SessRow{slot[i], len[i]};
    const SessRow* dtab = reinterpret_cast<const SessRow*>(sched_send(sl, 2 * (size_t)n, s));
    launch_session_admit(x0, tc0, sc0, n, T_in, q.dx, q.dtc, q.dsc, q.dpad, dtab, q.maxT, Fx, Ft, s);
    for (int i = 0; i < n; ++i) {
      const int b = slot[i];
      q.rows[b] = rows[i];
      q.ts[b] = solve_time_steps(rows[i].t_start, rows[i].t_end, rows[i].num_step, rows[i].t_shift);
      q.lens[b] = len[i];
      q.done[b] = 0;
    }
  }

  void session_step(zv_session& q, hipStream_t s) {
    const SessTick tk = session_tick(q.rows.data(), q.done.data(), q.lens.data(), q.ts, q.slots, distill());
    const SchedStep& st = tk.st;
    if (st.A == 0) return;
    const int N = st.U + st.A, Tk = tk.Tk;
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim;
    const int Ft = cfg.feat_dim, Fin = 2 * Fx + Ft;
    const bool split = cfg.precision == ZV_FP32 || cfg.precision == ZV_MIXED;   // as build_xin
    // the tick's table, as one step of the scheduled solve's: map [N] | t [N] | updates [A] | scales [A]
    const size_t o_t = N, o_upd = 2 * (size_t)N, o_g = o_upd + 5 * (size_t)st.A, words = o_g + st.A;
    SchedSlot& sl = sched_slot(words * 4);
    unsigned* tab = sl.base + 16;
    int* m = reinterpret_cast<int*>(tab);
    for (int j = 0; j < N; ++j) m[j] = sched_map_entry(st.src[j], st.zt[j] != 0, st.zs[j] != 0);
    memcpy(tab + o_t, st.t.data(), (size_t)N * 4);
    memcpy(tab + o_upd, st.upd.data(), (size_t)st.A * sizeof(SchedUpd));
    memcpy(tab + o_g, st.gdec.data(), (size_t)st.A * 4);
    const unsigned* dtab = sched_send(sl, words, s);
    const int* map = reinterpret_cast<const int*>(dtab);
    Act xin = ws_dec.xin.get((long)N * Tk, round_up(Fin, 64), split);
    launch_session_build_input(q.dx, q.dtc, q.dsc, xin.h, xin.l, xin.ld, map, N, Tk, q.maxT, Fx, Ft, Fx, s);
    uint8_t* padN = ws_dec.mask2.get<uint8_t>((size_t)N * Tk);
    launch_session_gather_u8(q.dpad, padN, map, N, Tk, q.maxT, s);
    float* v = ws_dec.vout.get<float>((size_t)N * Tk * Fx);
    const float* tv = reinterpret_cast<const float*>(dtab + o_t);
    const float* gv = distill() ? reinterpret_cast<const float*>(dtab + o_g) : nullptr;
    decoder(xin, Fin, N, Tk, padN, tv, gv, v, false, s);
    launch_session_euler_update(q.dx, v, reinterpret_cast<const SchedUpd*>(dtab + o_upd), st.A, (long)Tk * Fx,
                                (long)q.maxT * Fx, s);
    for (const SchedUpd& u : st.upd) q.done[u.row] += 1;
    q.ticks += 1;
    q.dec_rows += N;
    q.dec_row_frames += (int64_t)N * Tk;
    q.last_T = Tk;
  }

  void session_retire(zv_session& q, int n, const int32_t* slot, float* out, int T_out, hipStream_t s) {
    ZV_REQUIRE(n >= 1, "session: retire takes at least one row");
    ZV_REQUIRE(slot && out, "session: retire: null argument");
    std::vector<char> seen(q.slots, 0);
    for (int i = 0; i < n; ++i) {
      const std::string at = "session: retire row " + std::to_string(i) + ": ";
      ZV_REQUIRE(slot[i] >= 0 && slot[i] < q.slots, at + "slot outside [0, slots)");
      ZV_REQUIRE(q.rows[slot[i]].num_step > 0, at + "slot is free");
      ZV_REQUIRE(q.done[slot[i]] == q.rows[slot[i]].num_step, at + "slot has steps left");
      ZV_REQUIRE(!seen[slot[i]], at + "slot named twice");
      seen[slot[i]] = 1;
      ZV_REQUIRE(T_out >= q.lens[slot[i]], at + "T_out is shorter than the row");
    }
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim;
    SchedSlot& sl = sched_slot((size_t)n * sizeof(SessRow));
    SessRow* tab = reinterpret_cast<SessRow*>(sl.base + 16);
    for (int i = 0; i < n; ++i) tab[i] = SessRow{slot[i], q.lens[slot[i]]};
    const SessRow* dtab = reinterpret_cast<const SessRow*>(sched_send(sl, 2 * (size_t)n, s));
    launch_session_retire(q.dx, out, n, T_out, dtab, q.maxT, Fx, s);
    for (int i = 0; i < n; ++i) {
      q.rows[slot[i]].num_step = 0;
      q.done[slot[i]] = 0;
      q.lens[slot[i]] = 0;
    }
  }

  // zv_session_admit_edit / zv_session_retire_edit bodies: a row of a speech edit enters and leaves its
  // slot straight from a pool of stored frames under the edit's frame table (zv_session.inc, "Edit
  // rows").  The rules run on the host before anything is queued; the table (rows | segments) goes up
  // through the same staging as every other table of the session.
  struct SessState {
    std::vector<int> left;
    SessView view;
  };
  static void session_view(const zv_session& q, SessState& st) {
    st.left.resize(q.slots);
    for (int b = 0; b < q.slots; ++b) st.left[b] = q.rows[b].num_step > 0 ? q.rows[b].num_step - q.done[b] : -1;
    st.view = SessView{q.slots, q.maxT, st.left.data(), q.lens.data()};
  }
  const unsigned* session_edit_send(const SessEditReq& e, const std::vector<int>& T, hipStream_t s) {
    const size_t words = sess_edit_words(e);
    SchedSlot& sl = sched_slot(words * 4);
    sess_edit_fill(sl.base + 16, e, T);
    return sched_send(sl, words, s);
  }

  void session_admit_edit(zv_session& q, const SessEditReq& e, const SchedRow* rows, const float* x0,
                          const float* tc0, int T_in, const float* pool, hipStream_t s) {
    ZV_REQUIRE(x0 && tc0 && pool, "session: admit_edit: null argument");
    SessState st;
    session_view(q, st);
    std::vector<int> T;
    sess_edit_check_admit(st.view, e, rows, T_in, T);
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim, Ft = cfg.feat_dim;
    const unsigned* dtab = session_edit_send(e, T, s);
    launch_session_admit_edit(x0, tc0, e.n, T_in, pool, q.dx, q.dtc, q.dsc, q.dpad, dtab, q.maxT, Fx, Ft, s);
    for (int i = 0; i < e.n; ++i) {
      const int b = e.slot[i];
      q.rows[b] = rows[i];
      q.ts[b] = solve_time_steps(rows[i].t_start, rows[i].t_end, rows[i].num_step, rows[i].t_shift);
      q.lens[b] = T[i];
      q.done[b] = 0;
    }
  }

  void session_retire_edit(zv_session& q, const SessEditReq& e, const float* pool, bool keep, float* out,
                           uint8_t* mask, int T_out, hipStream_t s) {
    ZV_REQUIRE(pool && out, "session: retire_edit: null argument");
    SessState st;
    session_view(q, st);
    std::vector<int> T;
    sess_edit_check_retire(st.view, e, T_out, T);
    const int Fx = stereo() ? 2 * cfg.feat_dim : cfg.feat_dim;
    const unsigned* dtab = session_edit_send(e, T, s);
    launch_session_retire_edit(q.dx, pool, out, mask, e.n, T_out, dtab, q.maxT, Fx, keep, s);
    for (int i = 0; i < e.n; ++i) {
      q.rows[e.slot[i]].num_step = 0;
      q.done[e.slot[i]] = 0;
      q.lens[e.slot[i]] = 0;
    }
  }

  void text_encode(const int64_t* tok, const uint8_t* pad, const int8_t* spk, int B, int S,
                   float* out, hipStream_t s) {
    const long n = (long)B * S;
    const int E = cfg.text_embed_dim;
    const bool split = cfg.precision == ZV_FP32 || cfg.precision == ZV_MIXED;   // mixed: the text encoder is split too
    Act emb = ws_txt.emb.get(n, round_up(E, 64), split);
    launch_embed(tok, embed_table, emb.h, emb.l, emb.ld, n, E, s);
    const Pass pass;
    if (split) zipformer<3>(pass, txt, ws_txt, emb, 0, B, S, pad, nullptr, nullptr, out, s);
    else zipformer<1>(pass, txt, ws_txt, emb, 0, B, S, pad, nullptr, nullptr, out, s);
    if (spk && spk_table) launch_spk_add(out, spk, spk_table, n, cfg.feat_dim, s);
  }
};

// whether any slot holds a row (admitted and not yet retired)
static bool session_occupied(const zv_session& q) {
  return std::any_of(q.rows.begin(), q.rows.end(), [](const SchedRow& r) { return r.num_step > 0; });
}

zv_session::~zv_session() {
  if (!eng) return;
  std::vector<zv_session*>& v = eng->sessions;
  v.erase(std::remove(v.begin(), v.end(), this), v.end());
}

#include "zv_vocoder.inc"
#include "zv_bigvgan.inc"
#include "zv_fbank.inc"
#include "zv_resample.inc"
#include "zv_wavjoin.inc"
#include "zv_edit.inc"
#include "zv_voice.inc"

// ===========================================================================
// C ABI
// ===========================================================================
#define ZV_API_BEGIN try {
#define ZV_API_END                                     \
  return 0;                                            \
  }                                                    \
  catch (const std::exception& e) {                    \
    g_last_error = e.what();                           \
    return 1;                                          \
  }                                                    \
  catch (...) {                                        \
    g_last_error = "unknown error";                    \
    return 1;                                          \
  }

static void check_ready(zv_handle h) {
  ZV_REQUIRE(h != nullptr, "null engine handle");
  ZV_REQUIRE(h->store.ready, "engine weights not finalized (call zv_finalize)");
  h->check_dev_err();
}

// the bodies the handles' entry points share (engine, vocoder, BigVGAN: `what` names the handle)
template <class H>
static int api_set_weight(H* h, const char* what, const char* name, const float* host_data, int64_t numel) {
  ZV_API_BEGIN
  ZV_REQUIRE(h, "bad arguments");
  h->store.set(what, name, host_data, numel);
  ZV_API_END
}
template <class H>
static int api_finalize(H* h, const char* null_msg) {
  ZV_API_BEGIN
  ZV_REQUIRE(h != nullptr, null_msg);
  h->finalize();
  ZV_API_END
}
// *_create: make() validates, builds and returns the handle; a failure leaves the message and null
template <class F>
static auto api_create(F make) -> decltype(make()) {
  try {
    return make();
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return nullptr;
  }
}

#include "zv_checks.inc"
#include "zv_noise.inc"

extern "C" {

const char* zv_last_error(void) { return g_last_error.c_str(); }
#ifndef ZV_SRC_HASH
#define ZV_SRC_HASH "unknown"
#endif
const char* zv_version(void) {
  return "zipvoice_hip 0.3 (gfx950, " ZV_OPERAND_NAME " operands" ") src=" ZV_SRC_HASH;
}

zv_handle zv_create(const zv_config* cfg) {
  return api_create([&] {
    ZV_REQUIRE(cfg != nullptr, "null config");
    ZV_REQUIRE(cfg->num_stacks >= 1 && cfg->num_stacks <= ZV_MAX_STACKS, "bad num_stacks");
    ZV_REQUIRE(cfg->variant >= 0 && cfg->variant <= 3, "bad variant");
    ZV_REQUIRE(cfg->precision == ZV_FP32 || cfg->precision == ZV_BF16 || cfg->precision == ZV_MIXED ||
                   (cfg->precision == ZV_FP8 && std::string(ZV_OPERAND_NAME) == "bf16"),
               "bad precision");
    return new zv_engine(*cfg);
  });
}

void zv_destroy(zv_handle h) { delete h; }

int zv_set_weight(zv_handle h, const char* name, const float* host_data, int64_t numel) {
  return api_set_weight(h, "engine", name, host_data, numel);
}

int zv_finalize(zv_handle h) { return api_finalize(h, "null engine handle"); }

int zv_reserve(zv_handle h, int max_batch, int max_frames) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(max_batch > 0 && max_frames > 0, "bad reservation");
  // one uncaptured guided velocity at the largest shape sizes every decoder workspace
  // buffer (CFG-doubled rows, positional projections, attention images), so later calls
  // up to this shape never reallocate and captured graphs stay valid
  const int Fx = h->stereo() ? 2 * h->cfg.feat_dim : h->cfg.feat_dim;
  const size_t nx = (size_t)max_batch * max_frames * Fx;
  const size_t nt = (size_t)max_batch * max_frames * h->cfg.feat_dim;
  // zero-filled inputs and the output, freed on return (as every fresh buffer, they move the
  // workspace generation: reserve before the solves whose graphs are to stay)
  DBuf bx, btc, bv, bpad;
  const float *x = bx.get<float>(nx), *tc = btc.get<float>(nt);
  float* v = bv.get<float>(nx);
  const uint8_t* pad = bpad.get<uint8_t>((size_t)max_batch * max_frames);
  // the graph path's staging copies of the inputs, too
  (void)h->gx.get<float>(nx);
  (void)h->gtc.get<float>(nt);
  (void)h->gsc.get<float>(nx);
  (void)h->gpad.get<uint8_t>((size_t)max_batch * max_frames);
  (void)h->ggrows.get<float>((size_t)max_batch);
  h->velocity(0.25f, 1.0f, nullptr, false, x, tc, x, pad, max_batch, max_frames, v, false,
              0.f, false, nullptr);
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  ZV_API_END
}

int zv_set_padding(zv_handle h, int mode) {
  ZV_API_BEGIN
  ZV_REQUIRE(h != nullptr, "null engine handle");
  ZV_REQUIRE(mode == ZV_PAD_BATCH || mode == ZV_PAD_ROW, "zv_set_padding: the mode is ZV_PAD_BATCH or ZV_PAD_ROW");
  for (const zv_session* q : h->sessions)
    ZV_REQUIRE(!session_occupied(*q), "zv_set_padding: a session of this engine has an occupied slot "
                                      "(retire its rows first: a row's solve never changes mode midway)");
  h->padding = mode;
  ZV_API_END
}

int zv_get_padding(zv_handle h) { return h ? h->padding : -1; }

int zv_attn_fallbacks(zv_handle h, int reset, int64_t* host_counts) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(host_counts != nullptr, "null counts");
  unsigned c[4] = {0, 0, 0, 0};
  ZV_CHECK(ZV_BLOCKING(hipDeviceSynchronize()));
  ZV_CHECK(ZV_BLOCKING(hipMemcpy(c, h->attn_fallback, sizeof c, hipMemcpyDeviceToHost)));
  for (int i = 0; i < 3; ++i) host_counts[i] = c[i];
  if (reset) ZV_CHECK(ZV_BLOCKING(hipMemset(h->attn_fallback, 0, sizeof c)));
  ZV_API_END
}

int zv_profile(int enable) {
  ZV_API_BEGIN
  for (auto& r : g_zv_prof.recs) { (void)ZV_BLOCKING(hipEventDestroy(r.e0)); (void)ZV_BLOCKING(hipEventDestroy(r.e1)); }
  g_zv_prof.recs.clear();
  g_zv_prof.on = enable != 0;
  g_zv_prof.detail = enable == 2;
  ZV_API_END
}

int zv_profile_report(char* buf, int buflen) {
  ZV_API_BEGIN
  ZV_REQUIRE(buf && buflen > 0, "bad buffer");
  struct Agg { int n = 0; double flops = 0, bytes = 0, ms = 0; };
  std::map<std::string, Agg> agg;
  for (auto& r : g_zv_prof.recs) {
    ZV_CHECK(ZV_BLOCKING(hipEventSynchronize(r.e1)));
    float ms = 0.f;
    ZV_CHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
    Agg& a = agg[r.name];
    a.n += 1; a.flops += r.flops; a.bytes += r.bytes; a.ms += ms;
  }
  std::string js = "{";
  bool first = true;
  for (auto& kv : agg) {
    char tmp[512];
    snprintf(tmp, sizeof(tmp), "%s\"%s\": {\"launches\": %d, \"flops\": %.6e, \"bytes\": %.6e, \"ms\": %.6f}",
             first ? "" : ", ", kv.first.c_str(), kv.second.n, kv.second.flops, kv.second.bytes,
             kv.second.ms);
    js += tmp;
    first = false;
  }
  js += "}";
  ZV_REQUIRE((int)js.size() < buflen, "report buffer too small");
  memcpy(buf, js.c_str(), js.size() + 1);
  ZV_API_END
}

int64_t zv_host_block_count(void) { return (int64_t)g_zv_host_blocks.load(); }

int64_t zv_device_bytes(zv_handle h) {
  if (!h) return 0;
  return (int64_t)(h->store.weight_bytes + h->ws_dec.bytes() + h->ws_split[0].bytes() + h->ws_split[1].bytes() +
                   h->ws_split[2].bytes() + h->ws_txt.bytes() + h->gx.bytes +
                   h->gtc.bytes + h->gsc.bytes + h->gpad.bytes + h->ggrows.bytes + h->sched_tab.bytes);
}

int zv_fm_decoder(zv_handle h, const float* t, const float* guidance, const float* xt,
                  const float* text_c, const float* speech_c, const uint8_t* pad, int N, int T,
                  int Fx, float* v_out, void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(N > 0 && T > 0, "empty batch");
  ZV_REQUIRE(!h->distill() || guidance, "distill model needs a guidance_scale");
  hipStream_t s = (hipStream_t)stream;
  const int Fin = 2 * Fx + h->cfg.feat_dim;
  Act xin = h->build_xin(h->ws_dec, xt, text_c, speech_c, N, T, Fx, 1, 0, s);
  h->decoder(xin, Fin, N, T, pad, t, h->distill() ? guidance : nullptr, v_out, false, s);
  ZV_API_END
}

int zv_velocity(zv_handle h, float t, float guidance_scale, const float* x, const float* text_c,
                const float* speech_c, const uint8_t* pad, int B, int T, float* v_out,
                void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(B > 0 && T > 0, "empty batch");
  h->velocity(t, guidance_scale, nullptr, false, x, text_c, speech_c, pad, B, T, v_out, false,
              0.f, false, (hipStream_t)stream);
  ZV_API_END
}

// (guidance_scale == 0).all() of a device vector: one small D2H copy at API entry (the
// reference evaluates the same predicate on the host every step, solver.py:71)
static bool any_nonzero_rows(const float* grows, int B, hipStream_t s) {
  std::vector<float> h(B);
  ZV_CHECK(ZV_BLOCKING(hipMemcpyAsync(h.data(), grows, (size_t)B * 4, hipMemcpyDeviceToHost, s)));
  ZV_CHECK(ZV_BLOCKING(hipStreamSynchronize(s)));
  for (float v : h) if (v != 0.0f) return true;
  return false;
}

int zv_velocity_rows(zv_handle h, float t, const float* guidance_rows, const float* x,
                     const float* text_c, const float* speech_c, const uint8_t* pad, int B, int T,
                     float* v_out, void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(B > 0 && T > 0, "empty batch");
  ZV_REQUIRE(guidance_rows != nullptr, "null guidance_rows");
  hipStream_t s = (hipStream_t)stream;
  const bool on = any_nonzero_rows(guidance_rows, B, s);
  h->velocity(t, 0.f, guidance_rows, on, x, text_c, speech_c, pad, B, T, v_out, false, 0.f, false, s);
  ZV_API_END
}

int zv_euler_sample(zv_handle h, float* x, const float* text_c, const float* speech_c,
                    const uint8_t* pad, int B, int T, int num_step, float guidance_scale,
                    float t_start, float t_end, float t_shift, void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(B > 0 && T > 0 && num_step > 0, "empty batch or zero steps");
  h->euler_sample(x, text_c, speech_c, pad, B, T, num_step, guidance_scale, nullptr, false,
                  t_start, t_end, t_shift, (hipStream_t)stream);
  ZV_API_END
}

int zv_euler_sample_rows(zv_handle h, float* x, const float* text_c, const float* speech_c,
                         const uint8_t* pad, int B, int T, int num_step,
                         const float* guidance_rows, float t_start, float t_end, float t_shift,
                         void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(B > 0 && T > 0 && num_step > 0, "empty batch or zero steps");
  ZV_REQUIRE(guidance_rows != nullptr, "null guidance_rows");
  hipStream_t s = (hipStream_t)stream;
  const bool on = any_nonzero_rows(guidance_rows, B, s);
  h->euler_sample(x, text_c, speech_c, pad, B, T, num_step, 0.f, guidance_rows, on, t_start,
                  t_end, t_shift, s);
  ZV_API_END
}

static_assert(sizeof(zv_row_sched) == sizeof(SchedRow), "SchedRow mirrors zv_row_sched");

int zv_euler_sample_sched(zv_handle h, float* x, const float* text_c, const float* speech_c,
                          const uint8_t* pad, int B, int T, const zv_row_sched* rows, void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(B > 0 && T > 0, "empty batch");
  ZV_REQUIRE(x && text_c && speech_c && rows, "zv_euler_sample_sched: null argument");
  h->euler_sample_sched(x, text_c, speech_c, pad, B, T, reinterpret_cast<const SchedRow*>(rows),
                        (hipStream_t)stream);
  ZV_API_END
}

int zv_sched_stats(zv_handle h, int64_t* out) {
  ZV_API_BEGIN
  ZV_REQUIRE(h != nullptr && out != nullptr, "zv_sched_stats: null argument");
  out[0] = h->sched_rows_run;
  out[1] = h->sched_steps_run;
  ZV_API_END
}

// ---------------------------------------------------------------- solve session
static zv_engine* session_engine(zv_session_handle q) {
  ZV_REQUIRE(q != nullptr, "null session handle");
  ZV_REQUIRE(q->eng != nullptr, "the solve session's engine has been destroyed");
  check_ready(q->eng);
  return q->eng;
}

zv_session_handle zv_session_create(zv_handle h, int slots, int max_frames) {
  return api_create([&] {
    check_ready(h);
    return h->session_open(slots, max_frames);
  });
}

void zv_session_destroy(zv_session_handle q) { delete q; }

int zv_session_admit(zv_session_handle q, int n, const int32_t* host_slots, const int32_t* host_lens,
                     const zv_row_sched* host_rows, const float* x0, const float* text_c, const float* speech_c,
                     int T_in, void* stream) {
  ZV_API_BEGIN
  session_engine(q)->session_admit(*q, n, host_slots, host_lens, reinterpret_cast<const SchedRow*>(host_rows), x0,
                                   text_c, speech_c, T_in, (hipStream_t)stream);
  ZV_API_END
}

int zv_session_step(zv_session_handle q, void* stream) {
  ZV_API_BEGIN
  session_engine(q)->session_step(*q, (hipStream_t)stream);
  ZV_API_END
}

int zv_session_retire(zv_session_handle q, int n, const int32_t* host_slots, float* out, int T_out, void* stream) {
  ZV_API_BEGIN
  session_engine(q)->session_retire(*q, n, host_slots, out, T_out, (hipStream_t)stream);
  ZV_API_END
}

int zv_session_admit_edit(zv_session_handle q, int n, const int32_t* host_slots, const zv_row_sched* host_rows,
                          const float* x0, const float* text_c, int T_in, const float* pool, int pool_rows,
                          const int32_t* host_offsets, const int32_t* host_lens, const int32_t* host_table,
                          const int32_t* host_row_ptr, void* stream) {
  ZV_API_BEGIN
  const SessEditReq e{n, host_slots, host_offsets, host_lens, host_table, host_row_ptr, pool_rows};
  session_engine(q)->session_admit_edit(*q, e, reinterpret_cast<const SchedRow*>(host_rows), x0, text_c, T_in, pool,
                                        (hipStream_t)stream);
  ZV_API_END
}

int zv_session_retire_edit(zv_session_handle q, int n, const int32_t* host_slots, const float* pool, int pool_rows,
                           const int32_t* host_offsets, const int32_t* host_lens, const int32_t* host_table,
                           const int32_t* host_row_ptr, int keep_original, float* out, uint8_t* mask_out, int T_out,
                           void* stream) {
  ZV_API_BEGIN
  const SessEditReq e{n, host_slots, host_offsets, host_lens, host_table, host_row_ptr, pool_rows};
  session_engine(q)->session_retire_edit(*q, e, pool, keep_original != 0, out, mask_out, T_out, (hipStream_t)stream);
  ZV_API_END
}

int zv_session_state(zv_session_handle q, int32_t* host_steps_left, int64_t* stats) {
  ZV_API_BEGIN
  session_engine(q);
  for (int b = 0; host_steps_left && b < q->slots; ++b)
    host_steps_left[b] = q->rows[b].num_step > 0 ? q->rows[b].num_step - q->done[b] : -1;
  if (stats) {
    stats[0] = q->ticks; stats[1] = q->dec_rows; stats[2] = q->dec_row_frames; stats[3] = q->last_T;
  }
  ZV_API_END
}

int zv_text_encode(zv_handle h, const int64_t* tokens, const uint8_t* pad, const int8_t* spk,
                   int B, int S, float* out, void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(B > 0 && S > 0, "empty token batch");
  h->text_encode(tokens, pad, spk, B, S, out, (hipStream_t)stream);
  ZV_API_END
}

int zv_text_condition(zv_handle h, const float* embed, int B, int S, const int32_t* tok_lens,
                      const int32_t* feat_lens, int T, float* out, void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(embed && tok_lens && feat_lens && out, "zv_text_condition: null argument");
  launch_text_cond(embed, S, h->cfg.feat_dim, tok_lens, feat_lens, out, B, T, (hipStream_t)stream);
  ZV_API_END
}

int zv_speech_condition(zv_handle h, const float* prompt, int B, int Tp, int F,
                        const int32_t* prompt_lens, int T, float* out, void* stream) {
  ZV_API_BEGIN
  check_ready(h);
  ZV_REQUIRE(prompt && prompt_lens && out, "zv_speech_condition: null argument");
  launch_speech_cond(prompt, Tp, prompt_lens, out, B, T, F, (hipStream_t)stream);
  ZV_API_END
}

// ---------------------------------------------------------------- vocoder
zv_vocoder_handle zv_vocoder_create(const zv_vocoder_config* cfg) {
  return api_create([&] {
    ZV_REQUIRE(cfg != nullptr, "null vocoder config");
    ZV_REQUIRE(cfg->precision == ZV_FP32 || cfg->precision == ZV_BF16, "bad precision");
    ZV_REQUIRE(cfg->n_mels > 0 && cfg->dim > 0 && cfg->intermediate_dim > 0 && cfg->num_layers > 0,
               "bad vocoder dimensions");
    ZV_REQUIRE(cfg->embed_kernel % 2 == 1, "embed kernel must be odd");
    return new zv_vocoder(*cfg);
  });
}

void zv_vocoder_destroy(zv_vocoder_handle v) { delete v; }

int zv_vocoder_set_weight(zv_vocoder_handle v, const char* name, const float* host_data,
                          int64_t numel) {
  return api_set_weight(v, "vocoder", name, host_data, numel);
}

int zv_vocoder_finalize(zv_vocoder_handle v) { return api_finalize(v, "null vocoder handle"); }

int zv_vocoder_decode(zv_vocoder_handle v, const float* mel, int layout, float feat_scale,
                      float feat_bias, const int32_t* lens, int B, int T, float* wav, int clamp,
                      void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(v != nullptr && v->store.ready, "vocoder not finalized (call zv_vocoder_finalize)");
  ZV_REQUIRE(B > 0 && T > 0, "empty batch");
  ZV_REQUIRE(layout == 0 || layout == 1, "layout must be 0 (B,C,T) or 1 (B,T,C)");
  ZV_REQUIRE(feat_scale != 0.f, "feat_scale must be nonzero");
  hipStream_t s = (hipStream_t)stream;
  if (v->cfg.precision == ZV_FP32)
    v->decode<3>(mel, layout, feat_scale, feat_bias, lens, B, T, wav, clamp, s);
  else
    v->decode<1>(mel, layout, feat_scale, feat_bias, lens, B, T, wav, clamp, s);
  ZV_API_END
}

// ---------------------------------------------------------------- BigVGAN
zv_bigvgan_handle zv_bigvgan_create(const zv_bigvgan_config* cfg) {
  return api_create([&] {
    ZV_REQUIRE(cfg != nullptr, "null bigvgan config");
    ZV_REQUIRE(cfg->precision == ZV_FP32 || cfg->precision == ZV_BF16, "bad precision");
    ZV_REQUIRE(cfg->num_mels > 0 && cfg->upsample_initial_channel > 0, "bad bigvgan dimensions");
    return new zv_bigvgan(*cfg);
  });
}

void zv_bigvgan_destroy(zv_bigvgan_handle v) { delete v; }

int zv_bigvgan_set_weight(zv_bigvgan_handle v, const char* name, const float* host_data,
                          int64_t numel) {
  return api_set_weight(v, "bigvgan", name, host_data, numel);
}

int zv_bigvgan_finalize(zv_bigvgan_handle v) { return api_finalize(v, "null bigvgan handle"); }

int zv_bigvgan_decode(zv_bigvgan_handle v, const float* mel, int layout, float feat_scale,
                      float feat_bias, const int32_t* lens, int B, int T, float* wav,
                      void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(v != nullptr && v->store.ready, "bigvgan not finalized (call zv_bigvgan_finalize)");
  ZV_REQUIRE(B > 0 && T > 0, "empty batch");
  ZV_REQUIRE(layout == 0 || layout == 1, "layout must be 0 (B,C,T) or 1 (B,T,C)");
  ZV_REQUIRE(feat_scale != 0.f, "feat_scale must be nonzero");
  hipStream_t s = (hipStream_t)stream;
  if (v->cfg.precision == ZV_FP32)
    v->decode<3>(mel, layout, feat_scale, feat_bias, lens, B, T, wav, s);
  else
    v->decode<1>(mel, layout, feat_scale, feat_bias, lens, B, T, wav, s);
  ZV_API_END
}

int64_t zv_bigvgan_device_bytes(zv_bigvgan_handle v) { return v ? (int64_t)v->device_bytes() : 0; }

zv_fbank_handle zv_fbank_create(int n_fft, int hop, int n_mels, const float* host_window,
                                const float* host_fb) {
  return api_create([&] {
    ZV_REQUIRE(host_window && host_fb, "null window / filterbank");
    std::unique_ptr<zv_fbank> f(new zv_fbank());
    f->init(n_fft, hop, n_mels, host_window, host_fb);
    return f.release();
  });
}

void zv_fbank_destroy(zv_fbank_handle f) { delete f; }

int zv_fbank_configure(zv_fbank_handle f, int frame_offset, float mag_eps, float log_floor) {
  ZV_API_BEGIN
  ZV_REQUIRE(f != nullptr, "null fbank handle");
  ZV_REQUIRE(frame_offset >= 0 && frame_offset <= f->n_fft / 2 && 2 * frame_offset >= f->n_fft - f->hop,
             "frame_offset must be in [(n_fft - hop) / 2, n_fft / 2]");
  ZV_REQUIRE(mag_eps >= 0.f && log_floor > 0.f, "bad mag_eps / log_floor");
  f->off = frame_offset; f->mag_eps = mag_eps; f->log_floor = log_floor;
  ZV_API_END
}

int zv_fbank_extract(zv_fbank_handle f, const float* wav, int64_t wav_ld, const int32_t* lens,
                     int B, int T_out, float* out, int64_t out_ld, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(f != nullptr, "null fbank handle");
  ZV_REQUIRE(B > 0 && T_out > 0 && wav && lens && out, "bad arguments");
  ZV_REQUIRE(out_ld >= f->n_mels, "out_ld < n_mels");
  f->extract(wav, (long)wav_ld, lens, B, T_out, out, (long)out_ld, (hipStream_t)stream);
  ZV_API_END
}

zv_resample_handle zv_resample_create(int o, int n, int S, const int32_t* host_start,
                                      const float* host_table) {
  return api_create([&] {
    ZV_REQUIRE(host_start && host_table, "null host_start / host_table");
    std::unique_ptr<zv_resample> h(new zv_resample());
    h->init(o, n, S, host_start, host_table);
    return h.release();
  });
}

void zv_resample_destroy(zv_resample_handle h) { delete h; }

int zv_resample_apply(zv_resample_handle h, const float* wav, int64_t wav_ld, const int32_t* lens,
                      int R, float* out, int64_t out_ld, int64_t out_cols, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(h != nullptr, "null resample handle");
  ZV_REQUIRE(R > 0 && R <= 65535 && wav && lens && out, "bad arguments (R must be in [1, 65535])");
  ZV_REQUIRE(out_cols > 0 && out_ld >= out_cols, "out_cols must be in [1, out_ld]");
  ZV_REQUIRE(out_cols <= (int64_t)h->E * 0x7fffffff, "out_cols too large");
  h->apply(wav, (long)wav_ld, lens, R, out, (long)out_ld, (long)out_cols, (hipStream_t)stream);
  ZV_API_END
}

int64_t zv_resample_device_bytes(zv_resample_handle h) { return h ? (int64_t)h->bytes : 0; }

zv_wavjoin_handle zv_wavjoin_create(int frame, float thr, int keep_edge, int max_gap, int fade) {
  return api_create([&] {
    std::unique_ptr<zv_wavjoin> h(new zv_wavjoin());
    h->init(frame, thr, keep_edge, max_gap, fade);
    return h.release();
  });
}

void zv_wavjoin_destroy(zv_wavjoin_handle h) { delete h; }

int zv_wavjoin_apply_docs(zv_wavjoin_handle h, const float* wav, int64_t wav_ld, const int32_t* lens,
                          const float* gains, int B, int C, const int32_t* doc_ptr, int D,
                          float* out, int64_t out_ld, int64_t out_cap, int64_t* out_len,
                          int32_t* spans, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(h != nullptr, "null wavjoin handle");
  ZV_REQUIRE(C == 1 || C == 2, "C must be 1 or 2");
  ZV_REQUIRE(B >= 0, "B must be non-negative");
  ZV_REQUIRE(D >= 0, "D must be non-negative");
  ZV_REQUIRE(D > 0 || B == 0, "D must be positive when B > 0");
  ZV_REQUIRE(doc_ptr || D == 1, "doc_ptr is NULL but D is not 1");
  ZV_REQUIRE(out_cap <= out_ld, "out_cap exceeds out_ld");
  ZV_REQUIRE(out_cap >= 0 && wav_ld >= 0 && wav_ld <= 0x7fffffffLL, "bad out_cap / wav_ld");
  ZV_REQUIRE((out_len || D == 0) && (out || out_cap == 0 || D == 0) && ((wav && lens) || B == 0),
             "null argument");
  static_assert(sizeof(long) == sizeof(int64_t), "64-bit positions");
  h->apply(wav, (long)wav_ld, lens, gains, B, C, doc_ptr, D, out, (long)out_ld, (long)out_cap,
           reinterpret_cast<long*>(out_len), spans, (hipStream_t)stream);
  ZV_API_END
}

int zv_wavjoin_apply(zv_wavjoin_handle h, const float* wav, int64_t wav_ld, const int32_t* lens,
                     const float* gains, int B, int C, float* out, int64_t out_ld, int64_t out_cap,
                     int64_t* out_len, int32_t* spans, void* stream) {
  return zv_wavjoin_apply_docs(h, wav, wav_ld, lens, gains, B, C, nullptr, 1, out, out_ld, out_cap,
                               out_len, spans, stream);
}

int64_t zv_wavjoin_device_bytes(zv_wavjoin_handle h) { return h ? (int64_t)h->bytes : 0; }

zv_wavjoin_stream_handle zv_wavjoin_stream_create(zv_wavjoin_handle joiner, int C, int D) {
  return api_create([&] {
    std::unique_ptr<zv_wavjoin_stream> h(new zv_wavjoin_stream());
    h->init(joiner, C, D);
    return h.release();
  });
}

void zv_wavjoin_stream_destroy(zv_wavjoin_stream_handle s) { delete s; }

int zv_wavjoin_stream_reset(zv_wavjoin_stream_handle s, int d, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(s != nullptr, "null wavjoin stream handle");
  s->reset(d, (hipStream_t)stream);
  ZV_API_END
}

int zv_wavjoin_stream_push(zv_wavjoin_stream_handle s, const float* wav, int64_t wav_ld,
                           const int32_t* lens, const float* gains, int B, const int32_t* doc_ptr,
                           const uint8_t* host_final, float* out, int64_t out_ld, int64_t out_cap,
                           int64_t* out_len, int32_t* spans, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(s != nullptr, "null wavjoin stream handle");
  ZV_REQUIRE(B >= 0, "B must be non-negative");
  ZV_REQUIRE(doc_ptr || s->D == 1, "doc_ptr is NULL but D is not 1");
  ZV_REQUIRE(out_cap <= out_ld, "out_cap exceeds out_ld");
  ZV_REQUIRE(out_cap >= 0 && wav_ld >= 0 && wav_ld <= 0x7fffffffLL, "bad out_cap / wav_ld");
  ZV_REQUIRE(out_len && (out || out_cap == 0) && ((wav && lens) || B == 0), "null argument");
  s->push(wav, (long)wav_ld, lens, gains, B, doc_ptr, host_final, out, (long)out_ld, (long)out_cap,
          reinterpret_cast<long*>(out_len), spans, (hipStream_t)stream);
  ZV_API_END
}

int64_t zv_wavjoin_stream_device_bytes(zv_wavjoin_stream_handle s) {
  return s ? (int64_t)s->bytes : 0;
}

zv_edit_handle zv_edit_create(void) {
  return api_create([&] { return new zv_edit(); });
}

void zv_edit_destroy(zv_edit_handle h) { delete h; }

int64_t zv_edit_device_bytes(zv_edit_handle h) { return h ? (int64_t)h->device_bytes() : 0; }

int zv_edit_gather(zv_edit_handle h, const float* feat, int B, int Lmax, int F, const int32_t* host_lens,
                   const float* fill, const int32_t* host_table, const int32_t* host_row_ptr, int T,
                   float* out, uint8_t* mask, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(h != nullptr, "null edit handle");
  ZV_REQUIRE(B >= 1 && B <= 65535, "B must be in [1, 65535]");
  ZV_REQUIRE(Lmax >= 1 && F >= 1 && T >= 1, "Lmax, F and T must be at least 1");
  ZV_REQUIRE((int64_t)B * T * F <= (int64_t)1 << 40 && (int64_t)B * Lmax * F <= (int64_t)1 << 40,
             "batch too large");
  ZV_REQUIRE(feat && host_lens && host_row_ptr && out, "zv_edit_gather: null argument");
  ZV_REQUIRE(host_table || host_row_ptr[B] == 0, "zv_edit_gather: null table");
  h->gather(feat, B, Lmax, F, host_lens, fill, host_table, host_row_ptr, T, out, mask, (hipStream_t)stream);
  ZV_API_END
}

int zv_edit_splice(zv_edit_handle h, const float* orig, int64_t ld, const int32_t* host_lens, const float* gen,
                   int64_t ldg, const int32_t* host_gen_lens, int B, int C, const int32_t* host_table,
                   const int32_t* host_row_ptr, const float* host_gains, int fade, float* out, int64_t out_ld,
                   int64_t out_cols, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(h != nullptr, "null edit handle");
  ZV_REQUIRE(B >= 1, "B must be at least 1");
  ZV_REQUIRE(C == 1 || C == 2, "C must be 1 or 2");
  ZV_REQUIRE(fade >= 0, "fade must be non-negative");
  ZV_REQUIRE(ld >= 1 && ld <= 0x7fffffffLL && ldg >= 1 && ldg <= 0x7fffffffLL, "bad ld / ldg");
  ZV_REQUIRE(out_cols >= 1 && out_cols <= out_ld && out_cols <= 0x7fffffffLL, "out_cols must be in [1, out_ld]");
  ZV_REQUIRE(orig && host_lens && gen && host_gen_lens && host_row_ptr && host_gains && out,
             "zv_edit_splice: null argument");
  ZV_REQUIRE(host_table || host_row_ptr[B] == 0, "zv_edit_splice: null table");
  h->splice(orig, (long)ld, host_lens, gen, (long)ldg, host_gen_lens, B, C, host_table, host_row_ptr, host_gains,
            fade, out, (long)out_ld, (long)out_cols, (hipStream_t)stream);
  ZV_API_END
}

int zv_prompt_rms(const float* wav, int64_t ld, const int32_t* lens, const int32_t* host_lens, int B, float target,
                  float* rms, float* gain_in, float* gain_out, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(B >= 1 && B <= 65535 && ld >= 1 && ld <= 0x7fffffffLL, "zv_prompt_rms: B in [1, 65535], ld in [1, 2^31)");
  ZV_REQUIRE(wav && lens && host_lens && rms && gain_in && gain_out, "zv_prompt_rms: null argument");
  ZV_REQUIRE(target > 0.f, "zv_prompt_rms: target must be positive");
  voice_check_lens(host_lens, B, (long)ld, "zv_prompt_rms");
  launch_prompt_rms(wav, (long)ld, lens, B, target, rms, gain_in, gain_out, (hipStream_t)stream);
  ZV_API_END
}

int zv_prompt_scale(const float* wav, int64_t ld, const int32_t* lens, const int32_t* host_lens, const float* rms, int B,
                    float target, float* out, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(B >= 1 && B <= 65535 && ld >= 1 && ld <= 0x7fffffffLL, "zv_prompt_scale: B in [1, 65535], ld in [1, 2^31)");
  ZV_REQUIRE(wav && lens && host_lens && rms && out, "zv_prompt_scale: null argument");
  ZV_REQUIRE(target > 0.f, "zv_prompt_scale: target must be positive");
  voice_check_lens(host_lens, B, (long)ld, "zv_prompt_scale");
  launch_prompt_scale(wav, (long)ld, lens, rms, B, target, out, (hipStream_t)stream);
  ZV_API_END
}

zv_voice_handle zv_voice_create(void) {
  return api_create([&] { return new zv_voice(); });
}

void zv_voice_destroy(zv_voice_handle h) { delete h; }

int64_t zv_voice_device_bytes(zv_voice_handle h) { return h ? (int64_t)h->stage.device_bytes() : 0; }

int zv_voice_gather(zv_voice_handle h, const float* pool, int pool_rows, int F, const int32_t* host_table, int n, int T,
                    float* out, const float* gains_pool, float* gains_out, void* stream) {
  ZV_API_BEGIN
  ZV_REQUIRE(h != nullptr, "null voice handle");
  ZV_REQUIRE(n >= 1 && n <= 65535, "voice table: n must be in [1, 65535]");
  ZV_REQUIRE(pool_rows >= 1 && F >= 1 && T >= 1 && (int64_t)T * F < ((int64_t)1 << 30),
             "zv_voice_gather: pool_rows, F and T at least 1, T * F under 2^30");
  ZV_REQUIRE(pool && host_table && out, "zv_voice_gather: null argument");
  ZV_REQUIRE((gains_pool != nullptr) == (gains_out != nullptr), "zv_voice_gather: gains_pool and gains_out go together");
  h->gather(pool, pool_rows, F, host_table, n, T, out, gains_pool, gains_out, (hipStream_t)stream);
  ZV_API_END
}

int64_t zv_vocoder_device_bytes(zv_vocoder_handle v) {
  if (!v) return 0;
  return (int64_t)(v->store.weight_bytes + v->x.bytes + v->frames.bytes + v->col.bytes() +
                   v->h.bytes() + v->hid.bytes() + v->spec.bytes());
}

}  // extern "C"
