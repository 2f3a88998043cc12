// Weights in HBM: the padded bf16 hi/lo form of a linear, and the store the engine, the vocoder
// and BigVGAN stage their state dicts in and allocate their device weights from.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "zv_common.h"

namespace {

constexpr int W_NPAD = 128;   // weight row padding (GEMM BN)
constexpr int W_KPAD = 64;    // weight column padding (multiple of GEMM BK)

struct Linear {
  int N = 0, K = 0, Npad = 0, Kpad = 0;
  bf16* hi = nullptr;
  bf16* lo = nullptr;
  uint8_t* q8 = nullptr;  // fp8 mode: MX-fp8 weight [Npad][Kq] + scales [Npad][Kq / 32] (zv_mx8.inc)
  uint8_t* s8 = nullptr;
  int Kq = 0;
  float* w32 = nullptr;   // fp32 copy (small linears only)
  float* b = nullptr;
};

struct WeightStore {
  std::map<std::string, std::vector<float>> staged;    // the state dict, until finalize
  std::map<std::string, std::vector<float>> derived;   // re-laid-out copies (the engine's stage_rows_scaled, ...)
  std::vector<void*> allocs;
  size_t weight_bytes = 0;
  bool ready = false;

  WeightStore() = default;
  WeightStore(const WeightStore&) = delete;
  WeightStore& operator=(const WeightStore&) = delete;
  ~WeightStore() {
    for (void* p : allocs) (void)ZV_BLOCKING(hipFree(p));
  }

  // the C ABI's *_set_weight; `what` names the handle in the message
  void set(const char* what, const char* name, const float* host_data, int64_t numel) {
    ZV_REQUIRE(name && (host_data || numel == 0), "bad arguments");
    ZV_REQUIRE(!ready, std::string(what) + " already finalized");
    staged[name].assign(host_data, host_data + numel);
  }
  template <typename T> T* dalloc(size_t n) {
    void* p = nullptr;
    ZV_CHECK(ZV_BLOCKING(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T))));
    allocs.push_back(p);
    weight_bytes += n * sizeof(T);
    return reinterpret_cast<T*>(p);
  }
  const std::vector<float>& take(const std::string& k, size_t numel) const {
    auto it = derived.find(k);
    if (it == derived.end()) {
      it = staged.find(k);
      if (it == staged.end()) throw std::invalid_argument("missing weight: " + k);
    }
    if (it->second.size() != numel)
      throw std::invalid_argument("weight " + k + ": expected " + std::to_string(numel) +
                                  " elements, got " + std::to_string(it->second.size()));
    return it->second;
  }
  template <typename T> T* upload(const T* host, size_t n) {
    T* d = dalloc<T>(n);
    ZV_CHECK(ZV_BLOCKING(hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice)));
    return d;
  }
  float* upload(const std::vector<float>& v) { return upload(v.data(), v.size()); }
  float* upload_key(const std::string& k, size_t numel) { return upload(take(k, numel)); }
  // host matrix w (N x K, row-major) -> the device weight [Npad][Kpad], zero padded: bf16 hi and
  // the lo half v - hi (the fp32-accurate modes' second operand); bias (N) optional
  Linear make_linear(const float* w, int N, int K, const float* bias) {
    Linear L;
    L.N = N; L.K = K;
    L.Npad = (int)round_up(N, W_NPAD);
    L.Kpad = (int)round_up(K, W_KPAD);
    std::vector<bf16> hi((size_t)L.Npad * L.Kpad, (bf16)0.f), lo(hi.size(), (bf16)0.f);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) {
        const float v = w[(size_t)n * K + k];
        const bf16 h = (bf16)v;
        hi[(size_t)n * L.Kpad + k] = h;
        lo[(size_t)n * L.Kpad + k] = (bf16)(v - (float)h);
      }
    L.hi = upload(hi.data(), hi.size());
    L.lo = upload(lo.data(), lo.size());
    if (bias) L.b = upload(bias, (size_t)N);
    return L;
  }
};

}  // namespace
