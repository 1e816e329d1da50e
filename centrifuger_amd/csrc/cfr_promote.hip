// cfr_promote.hip — the device side of centrifuger-promote (gfx950).  Semantics and the per-read code: cfr_promote_core.hpp.
//
//   k_promote_table   once per (taxonomy, level), one lane per node: the walk towards the root, promo[node] = the node it ends at.
//                     The walks of a wave have different lengths (the depth of the level below each node, a handful of steps);
//                     the kernel runs once over ~1e5..1e6 nodes and every step is two small gathers into tables that sit in L2.
//   k_promote_reads   one lane per read, rank mode: one gather of promo per match (a sequence-level match goes through seq_to_tax
//                     first) and one of tax_orig; duplicates are dropped by comparing with the slots the read has already kept,
//                     in place in global memory - a list has any length (max_result <= 0 is legal), so nothing is kept per lane.
//                     A read's slots are its own 24-byte records: lanes of a wave touch neighbouring lists, never the same line twice.
//   k_promote_lca     one lane per read, lca mode: the fold of the script's lca() with tax_depth and tax_parent.
// No lane keeps an array; the loops differ in length between lanes (1..k matches) and that is all the divergence there is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "cfr_hip_util.hpp"
#include "cfr_promote.hpp"

namespace cfr {

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_promote_table(PromoteTables T, PromoteLevel L, uint32_t *promo) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= T.node_cnt) return;
  promo[i] = promote_walk(T, L, i);
}

__global__ __launch_bounds__(kBlock) void k_promote_reads(PromoteTables T, const uint32_t *promo, cfr_result *results, cfr_match *matches, uint64_t n,
                                                          uint64_t match_base, uint64_t *src) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    cfr_result r = results[i];
    if (r.n_match <= 0) continue;
    const int32_t before = r.n_match;
    promote_read_rank(T, promo, r, matches, r.match_begin - match_base, src);
    if (r.n_match != before) results[i].n_match = r.n_match;
  }
}

__global__ __launch_bounds__(kBlock) void k_promote_lca(PromoteTables T, cfr_result *results, cfr_match *matches, uint64_t n, uint64_t match_base,
                                                        uint64_t *src) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    cfr_result r = results[i];
    if (r.n_match <= 0) continue;
    const int32_t before = r.n_match;
    promote_read_lca(T, r, matches, r.match_begin - match_base, src);
    if (r.n_match != before) results[i].n_match = r.n_match;
  }
}

template <class T> void upload(DevBuf<T> &d, const std::vector<T> &v, hipStream_t st) {
  d.alloc(v.size());
  if (!v.empty()) HIP_CHECK(hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
}

class PromoteDeviceImpl : public PromoteDevice {
 public:
  PromoteDeviceImpl(int device, const Taxonomy &t, const std::vector<uint32_t> &depth, uint64_t one_node, const PromoteLevel &L) : device_(device), level_(L) {
    if (!device_exists(device)) throw HipError{"cfr_promote: no HIP device " + std::to_string(device), -1};
    DeviceScope scope(device);
    stream_.create();
    for (auto &e : ev_) e.create();
    upload(parent_, t.parent, stream_); upload(orig_, t.orig_taxid, stream_); upload(seq_to_tax_, t.seq_to_tax, stream_);
    upload(rank_, t.rank, stream_); upload(depth_, depth, stream_);
    tables_ = PromoteTables{parent_, orig_, seq_to_tax_, rank_, depth_, t.node_cnt, t.seq_cnt, t.root, one_node};
    promo_.alloc(t.node_cnt);
    if (!L.lca) {
      HIP_CHECK(hipEventRecord(ev_[0], stream_));
      promote_launch_table(tables_, L, promo_, stream_);
      HIP_CHECK(hipEventRecord(ev_[1], stream_));
    }
    HIP_CHECK(hipStreamSynchronize(stream_));    // (the host vectors are the caller's)
    if (!L.lca) (void)hipEventElapsedTime(&table_ms_, ev_[0], ev_[1]);
  }
  ~PromoteDeviceImpl() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }
  void apply(cfr_result *results, cfr_match *matches, size_t n, uint64_t extent, uint64_t *src_slot) override {
    DeviceScope scope(device_);
    if (n > cap_n_) { const size_t cap = std::max<size_t>(n, 1u << 12); DevBuf<cfr_result> d(cap); d_res_ = std::move(d); cap_n_ = cap; }
    if (extent > cap_m_) {
      const size_t cap = std::max<size_t>(extent, 1u << 12);
      DevBuf<cfr_match> d(cap);
      DevBuf<uint64_t> s(cap);
      d_match_ = std::move(d); d_src_ = std::move(s); cap_m_ = cap;
    }
    HIP_CHECK(hipMemcpyAsync(d_res_, results, n * sizeof(cfr_result), hipMemcpyHostToDevice, stream_));
    if (extent) HIP_CHECK(hipMemcpyAsync(d_match_, matches, extent * sizeof(cfr_match), hipMemcpyHostToDevice, stream_));
    if (src_slot && extent) HIP_CHECK(hipMemcpyAsync(d_src_, src_slot, extent * 8, hipMemcpyHostToDevice, stream_));   // (slots no read keeps stay the caller's)
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    promote_launch_reads(tables_, level_, promo_, d_res_, d_match_, n, 0, src_slot ? d_src_.get() : nullptr, stream_);
    HIP_CHECK(hipEventRecord(ev_[1], stream_));
    HIP_CHECK(hipMemcpyAsync(results, d_res_, n * sizeof(cfr_result), hipMemcpyDeviceToHost, stream_));
    if (extent) HIP_CHECK(hipMemcpyAsync(matches, d_match_, extent * sizeof(cfr_match), hipMemcpyDeviceToHost, stream_));
    if (src_slot && extent) HIP_CHECK(hipMemcpyAsync(src_slot, d_src_, extent * 8, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    (void)hipEventElapsedTime(&reads_ms_, ev_[0], ev_[1]);
  }
  float table_ms() const override { return table_ms_; }
  float reads_ms() const override { return reads_ms_; }

 private:
  int device_;
  PromoteLevel level_;
  Stream stream_;                  // first: the last to go
  Event ev_[2];
  DevBuf<uint64_t> parent_, orig_, seq_to_tax_;
  DevBuf<uint8_t> rank_;
  DevBuf<uint32_t> depth_, promo_;
  PromoteTables tables_{};
  DevBuf<cfr_result> d_res_;
  DevBuf<cfr_match> d_match_;
  DevBuf<uint64_t> d_src_;
  size_t cap_n_ = 0, cap_m_ = 0;
  float table_ms_ = 0.f, reads_ms_ = 0.f;
};

}  // namespace

void promote_launch_table(const PromoteTables &T, const PromoteLevel &L, uint32_t *d_promo, hipStream_t st) {
  if (T.node_cnt == 0) return;
  hipLaunchKernelGGL(k_promote_table, dim3(grid_for(T.node_cnt, kBlock)), dim3(kBlock), 0, st, T, L, d_promo);
  HIP_CHECK(hipGetLastError());
}

void promote_launch_reads(const PromoteTables &T, const PromoteLevel &L, const uint32_t *d_promo, cfr_result *d_results, cfr_match *d_matches,
                          size_t n, uint64_t match_base, uint64_t *d_src, hipStream_t st, unsigned max_blocks) {
  if (n == 0) return;
  const unsigned grid = max_blocks ? std::min(grid_for(n, kBlock), max_blocks) : grid_for(n, kBlock);
  if (L.lca) hipLaunchKernelGGL(k_promote_lca, dim3(grid), dim3(kBlock), 0, st, T, d_results, d_matches, (uint64_t)n, match_base, d_src);
  else hipLaunchKernelGGL(k_promote_reads, dim3(grid), dim3(kBlock), 0, st, T, d_promo, d_results, d_matches, (uint64_t)n, match_base, d_src);
  HIP_CHECK(hipGetLastError());
}

PromoteDevice *make_promote_device(int device, const Taxonomy &t, const std::vector<uint32_t> &depth, uint64_t one_node, const PromoteLevel &L) {
  return new PromoteDeviceImpl(device, t, depth, one_node, L);
}

}  // namespace cfr
