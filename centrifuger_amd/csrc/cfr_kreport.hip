// cfr_kreport.hip — the device side of centrifuger-kreport (gfx950).  Semantics and the per-read code: cfr_kreport_core.hpp.
//
//   k_kreport_fold         one lane per read, grid-stride: the filters and the fold of the script's lca() (the walks of k_promote_lca),
//                          bin[i] = the read's bin (0xffffffff: dropped) and score[i] = its score.  It reads results and matches and
//                          writes nothing else, so running it again over the same reads leaves the same values.
//   k_kreport_accumulate   the histogram: count[bin] += 1 and maxscore[bin] = max(.., score) over bin[0..n) / score[0..n).
//                          Real samples are skewed (one species may own a third of the reads), so no read sends an atomic of its own
//                          to HBM.  Three levels:
//                          wave   up to kRounds times the first lane that still waits names its bin (ballot + readlane); the lanes
//                                 that hold the same bin hand their number (a popcount) and their maximum (a butterfly, run only
//                                 when there is more than one such lane) to that leader and are done.  kRounds is small on purpose:
//                                 a wave of 64 different bins would otherwise take 64 serial rounds to combine nothing; the heavy
//                                 bins of a skewed sample are met in the first rounds with high probability, whatever is left
//                                 goes on lane by lane and meets the LDS atomics, which are correct for any order.
//                          block  an open-addressing table in LDS (slots keys, counts and maxima, linear probing, kProbes tries):
//                                 LDS atomics, one per lane that still holds something.
//                          grid   at the end every occupied slot sends one atomic add and, with a score, one atomic max to HBM.
//                                 A lane that finds no slot in kProbes tries (more distinct bins in the block than the table takes)
//                                 sends its pair straight to HBM.
//                          Everything is an integer: every order gives the same bins, the host twin's exactly.
// Two kernels and not one because the device pipeline may compute a sub-batch twice: the fold is idempotent,
// the histogram is not.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "cfr_hip_util.hpp"
#include "cfr_kreport.hpp"

namespace cfr {

namespace {

constexpr int kBlock = 256;
constexpr int kRounds = 8;
constexpr int kProbes = 8;
constexpr uint32_t kEmpty = 0xffffffffu;

__global__ __launch_bounds__(kBlock) void k_kreport_fold(PromoteTables T, KreportOptions opt, const cfr_result *results, const cfr_match *matches, uint64_t n,
                                                         uint64_t match_base, uint32_t *bin, uint64_t *score) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const cfr_result r = results[i];
    bin[i] = kreport_read_bin(T, opt, r, matches, r.match_begin - match_base);
    score[i] = r.score;
  }
}

__global__ __launch_bounds__(kBlock) void k_kreport_accumulate(const uint32_t *bin, const uint64_t *score, uint64_t n, unsigned long long *count,
                                                               unsigned long long *maxscore, uint32_t n_bins, uint32_t slots) {
  extern __shared__ unsigned long long lds[];
  unsigned long long *s_max = lds, *s_cnt = lds + slots;
  uint32_t *s_key = (uint32_t *)(lds + 2 * (size_t)slots);
  for (uint32_t s = threadIdx.x; s < slots; s += kBlock) { s_key[s] = kEmpty; s_cnt[s] = 0; s_max[s] = 0; }
  __syncthreads();
  const uint32_t shift = 32u - (uint32_t)(__ffs((int)slots) - 1);
  const int lane = (int)(threadIdx.x & 63u);
  // (the trip count is the block's, not the lane's: every lane of a wave is in the ballots and shuffles below)
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = base + threadIdx.x;
    uint32_t b = kEmpty;
    unsigned long long v = 0, c = 1;
    if (i < n) { b = bin[i]; v = score[i]; }
    bool pending = b < n_bins;                       // (a dropped read, and anything that is no bin)
    bool cand = pending;
    for (int r = 0; r < kRounds; ++r) {
      const unsigned long long waiting = __ballot(cand);
      if (!waiting) break;
      const int leader = __ffsll(waiting) - 1;
      const uint32_t lb = (uint32_t)__shfl((int)b, leader);
      const bool same = cand && b == lb;
      const int k = __popcll(__ballot(same));
      if (k > 1) {                                   // (the same for the whole wave)
        unsigned long long w = same ? v : 0;
        for (int off = 32; off; off >>= 1) { const unsigned long long o = __shfl_xor(w, off); w = o > w ? o : w; }
        if (lane == leader) { c = (unsigned long long)k; v = w; }
        else if (same) pending = false;
      }
      if (same) cand = false;
    }
    if (pending) {
      const uint32_t h = (b * 0x9E3779B1u) >> shift;
      bool placed = false;
      for (int p = 0; p < kProbes && !placed; ++p) {
        const uint32_t s = (h + (uint32_t)p) & (slots - 1);
        const uint32_t old = atomicCAS(&s_key[s], kEmpty, b);
        if (old == kEmpty || old == b) {
          atomicAdd(&s_cnt[s], c);
          if (v) atomicMax(&s_max[s], v);
          placed = true;
        }
      }
      if (!placed) {
        atomicAdd(&count[b], c);
        if (v) atomicMax(&maxscore[b], v);
      }
    }
  }
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < slots; s += kBlock) {
    const uint32_t key = s_key[s];
    if (key == kEmpty) continue;
    atomicAdd(&count[key], s_cnt[s]);
    if (s_max[s]) atomicMax(&maxscore[key], s_max[s]);
  }
}

template <class T> void upload(DevBuf<T> &d, const std::vector<T> &v, hipStream_t st) {
  d.alloc(v.size());
  if (!v.empty()) HIP_CHECK(hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
}

class KreportDeviceImpl : public KreportDevice {
 public:
  KreportDeviceImpl(int device, const Taxonomy &t, const std::vector<uint32_t> &depth, uint64_t one_node, const KreportOptions &opt, unsigned max_blocks,
                    uint32_t slots)
      : device_(device), opt_(opt), max_blocks_(max_blocks), slots_(slots), n_bins_((uint32_t)t.node_cnt + 1) {
    if (!device_exists(device)) throw HipError{"cfr_kreport: no HIP device " + std::to_string(device), -1};
    DeviceScope scope(device);
    stream_.create();
    for (auto &e : ev_) e.create();
    upload(parent_, t.parent, stream_); upload(orig_, t.orig_taxid, stream_); upload(seq_to_tax_, t.seq_to_tax, stream_); upload(depth_, depth, stream_);
    tables_ = PromoteTables{parent_, orig_, seq_to_tax_, nullptr, depth_, t.node_cnt, t.seq_cnt, t.root, one_node};     // (no rank: the fold reads none)
    count_.alloc(n_bins_); maxscore_.alloc(n_bins_);
    HIP_CHECK(hipMemsetAsync(count_, 0, (size_t)n_bins_ * 8, stream_));
    HIP_CHECK(hipMemsetAsync(maxscore_, 0, (size_t)n_bins_ * 8, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));    // (the host vectors are the caller's)
  }
  ~KreportDeviceImpl() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }
  void add(const cfr_result *results, const cfr_match *matches, size_t n, uint64_t extent) override {
    DeviceScope scope(device_);
    if (n > cap_n_) {
      const size_t cap = std::max<size_t>(n, 1u << 12);
      DevBuf<cfr_result> d(cap);
      DevBuf<uint32_t> b(cap);
      DevBuf<uint64_t> s(cap);
      d_res_ = std::move(d); d_bin_ = std::move(b); d_score_ = std::move(s); cap_n_ = cap;
    }
    if (extent > cap_m_) { const size_t cap = std::max<size_t>(extent, 1u << 12); DevBuf<cfr_match> d(cap); d_match_ = std::move(d); cap_m_ = cap; }
    HIP_CHECK(hipMemcpyAsync(d_res_, results, n * sizeof(cfr_result), hipMemcpyHostToDevice, stream_));
    if (extent) HIP_CHECK(hipMemcpyAsync(d_match_, matches, extent * sizeof(cfr_match), hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    kreport_launch_fold(tables_, opt_, d_res_, d_match_, n, 0, d_bin_, d_score_, stream_, max_blocks_);
    HIP_CHECK(hipEventRecord(ev_[1], stream_));
    kreport_launch_accumulate(d_bin_, d_score_, n, count_, maxscore_, n_bins_, stream_, max_blocks_, slots_);
    HIP_CHECK(hipEventRecord(ev_[2], stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    (void)hipEventElapsedTime(&fold_ms_, ev_[0], ev_[1]);
    (void)hipEventElapsedTime(&acc_ms_, ev_[1], ev_[2]);
  }
  void download(uint64_t *count, uint64_t *maxscore) override {
    DeviceScope scope(device_);
    HIP_CHECK(hipMemcpyAsync(count, count_, (size_t)n_bins_ * 8, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(maxscore, maxscore_, (size_t)n_bins_ * 8, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }
  float fold_ms() const override { return fold_ms_; }
  float accumulate_ms() const override { return acc_ms_; }

 private:
  int device_;
  KreportOptions opt_;
  unsigned max_blocks_;
  uint32_t slots_, n_bins_;
  Stream stream_;                  // first: the last to go
  Event ev_[3];
  DevBuf<uint64_t> parent_, orig_, seq_to_tax_;
  DevBuf<uint32_t> depth_;
  PromoteTables tables_{};
  DevBuf<uint64_t> count_, maxscore_;
  DevBuf<cfr_result> d_res_;
  DevBuf<cfr_match> d_match_;
  DevBuf<uint32_t> d_bin_;
  DevBuf<uint64_t> d_score_;
  size_t cap_n_ = 0, cap_m_ = 0;
  float fold_ms_ = 0.f, acc_ms_ = 0.f;
};

}  // namespace

void kreport_launch_fold(const PromoteTables &T, const KreportOptions &opt, const cfr_result *d_results, const cfr_match *d_matches, size_t n,
                         uint64_t match_base, uint32_t *d_bin, uint64_t *d_score, hipStream_t st, unsigned max_blocks) {
  if (n == 0) return;
  const unsigned grid = max_blocks ? std::min(grid_for(n, kBlock), max_blocks) : grid_for(n, kBlock);
  hipLaunchKernelGGL(k_kreport_fold, dim3(grid), dim3(kBlock), 0, st, T, opt, d_results, d_matches, (uint64_t)n, match_base, d_bin, d_score);
  HIP_CHECK(hipGetLastError());
}

void kreport_launch_accumulate(const uint32_t *d_bin, const uint64_t *d_score, size_t n, uint64_t *d_count, uint64_t *d_maxscore, uint32_t n_bins,
                               hipStream_t st, unsigned max_blocks, uint32_t slots) {
  if (n == 0) return;
  if (slots == 0) slots = kKreportSlots;
  if (slots < 64 || slots > 2048 || (slots & (slots - 1))) throw HipError{"cfr_kreport: the LDS table takes a power of two of 64..2048 slots", 0};
  // a block per 4 * kBlock reads and at most 2048 of them (8 per CU) unless the caller caps it: every block pays for one table
  // flush, so it should have reads to fold in
  const unsigned want = (unsigned)std::min<size_t>(grid_for((n + 3) / 4, kBlock), 2048);
  const unsigned grid = max_blocks ? std::min(want, max_blocks) : want;
  hipLaunchKernelGGL(k_kreport_accumulate, dim3(grid), dim3(kBlock), (size_t)slots * 20, st, d_bin, d_score, (uint64_t)n, (unsigned long long *)d_count,
                     (unsigned long long *)d_maxscore, n_bins, slots);
  HIP_CHECK(hipGetLastError());
}

KreportDevice *make_kreport_device(int device, const Taxonomy &t, const std::vector<uint32_t> &depth, uint64_t one_node, const KreportOptions &opt,
                                   unsigned max_blocks, uint32_t slots) {
  return new KreportDeviceImpl(device, t, depth, one_node, opt, max_blocks, slots);
}

}  // namespace cfr
