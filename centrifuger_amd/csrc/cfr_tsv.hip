// cfr_tsv.hip — the rows of a batch made in HBM (gfx950).  What a row is: cfr_tsv_core.hpp; the host twin: cfr_tsv.cpp.
//
//   k_tsv_len     one lane per read, grid-stride: the bytes of the read's rows as a 64-bit length; the lane behind the last read
//                 writes the zero the scan ends on.
//   (hipcub::DeviceScan::ExclusiveSum over n + 1 lengths: row_offsets; its last entry, the total, goes to the host - the one wait
//    inside a call - which grows the text buffer if it must.)
//   k_tsv_write   a block of 256 lanes owns 256 consecutive reads, whose rows are ONE contiguous span of the text.
//                 staged   the span is at most tile_bytes long: every lane writes its rows into LDS at its offset inside the span,
//                          and behind the barrier the block streams the span out with 16-byte stores (the span lies in LDS at the
//                          same residue modulo 16 as in HBM, so both sides of a store are aligned; the unaligned head and tail go
//                          as bytes).  A lane per read storing bytes straight to HBM is 64 uncoalesced byte streams per wave.
//                 direct   a longer span (long ids, many rows per read): every lane writes its rows to HBM itself.  Slower, and
//                          counted (direct_blocks).
//                 Which path a block takes depends on its span alone, so it is the same for all its lanes: the barriers are met
//                 by every lane.
// Every index a kernel forms was checked on the host (tsv_check_args) or made by the classifier's own kernels; a sequence or node id
// outside the tables prints as cfr_format_tsv prints it and reads nothing.  No lane keeps an array: no scratch.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstring>
#include <stdexcept>

#include "cfr_hip_util.hpp"
#include "cfr_tsv.hpp"

namespace cfr {

namespace {

constexpr int kBlock = kTsvBlock;

__global__ __launch_bounds__(kBlock) void k_tsv_len(TsvView v, const cfr_result *results, const cfr_match *matches, TsvIds ids, uint64_t n, uint64_t *len) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kBlock) {
    if (i == n) { len[i] = 0; continue; }
    const cfr_result r = results[i];
    uint64_t id_len;
    (void)tsv_id(ids, i, id_len);
    len[i] = tsv_read_len(v, r, r.n_match > 0 ? matches + r.match_begin : nullptr, id_len);
  }
}

// lds_bytes of dynamic LDS = tile_bytes rounded up to 16, plus 16
__global__ __launch_bounds__(kBlock) void k_tsv_write(TsvView v, const cfr_result *results, const cfr_match *matches, TsvIds ids, uint64_t n, const uint64_t *off,
                                                      char *text, uint32_t tile_bytes, unsigned long long *direct_blocks) {
  extern __shared__ uint4 s_tile4[];
  char *s_tile = reinterpret_cast<char *>(s_tile4);
  const uint64_t n_blocks = (n + kBlock - 1) / kBlock;
  for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const uint64_t first = b * kBlock, last = first + kBlock < n ? first + kBlock : n;
    const uint64_t sb = off[first], span = off[last] - sb;
    const uint64_t i = first + threadIdx.x;
    const bool staged = span <= tile_bytes;            // (the same for every lane of the block)
    const uint32_t shift = (uint32_t)(sb & 15u);
    if (!staged && threadIdx.x == 0) atomicAdd(direct_blocks, 1ull);
    if (i < last) {                                    // one copy of the row code: into LDS, or straight to HBM
      const cfr_result r = results[i];
      uint64_t id_len;
      const char *id = tsv_id(ids, i, id_len);
      TsvBytes o{staged ? s_tile + shift + (uint32_t)(off[i] - sb) : text + off[i]};
      tsv_rows(v, r, r.n_match > 0 ? matches + r.match_begin : nullptr, id, id_len, o);
    }
    if (staged) {
      __syncthreads();
      char *dst = text + sb;
      const uint32_t len = (uint32_t)span;
      const uint32_t head = std::min((16u - shift) & 15u, len);
      const uint32_t nvec = (len - head) >> 4, tail = head + (nvec << 4);
      if (threadIdx.x < head) dst[threadIdx.x] = s_tile[shift + threadIdx.x];
      const uint4 *src4 = reinterpret_cast<const uint4 *>(s_tile + shift + head);      // (shift + head is 0 or 16 whenever nvec > 0)
      uint4 *dst4 = reinterpret_cast<uint4 *>(dst + head);
      for (uint32_t j = threadIdx.x; j < nvec; j += kBlock) dst4[j] = src4[j];
      if (tail + threadIdx.x < len) dst[tail + threadIdx.x] = s_tile[shift + tail + threadIdx.x];     // (fewer than 16 bytes)
      __syncthreads();                           // the next span of this block is written into the same LDS
    }
  }
}

template <class T> void grow(DevBuf<T> &b, size_t &cap, size_t need) {      // by doubling; the old contents are not kept
  if (need <= cap) return;
  const size_t c = std::max(need, cap * 2);
  cap = 0;                 // (alloc lets go of the old block first: a throw must not leave the old capacity beside a null pointer)
  b.alloc(c);
  cap = c;
}

template <class T> void upload(DevBuf<T> &d, const std::vector<T> &v, hipStream_t st) {
  d.alloc(v.size());
  if (!v.empty()) HIP_CHECK(hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
}

class TsvDevice : public Tsv {
 public:
  TsvDevice(int device, const TsvTables &t, const cfr_tsv_options &o) : device_(device) {
    if (!device_exists(device)) throw HipError{"cfr_tsv_open: no HIP device " + std::to_string(device), -1};
    tile_ = o.tile_bytes > 0 ? (uint32_t)o.tile_bytes : kTsvTileDefault;
    if (tile_ < 16 || tile_ > kTsvTileMax) throw std::invalid_argument("cfr_tsv_open: tile_bytes is 0 (the default) or in [16, 163776]");
    max_blocks_ = o.max_blocks > 0 ? (unsigned)o.max_blocks : 0u;
    lds_bytes_ = ((size_t)tile_ + 15) / 16 * 16 + 16;
    DeviceScope scope(device);
    // more than 64 KiB of dynamic LDS per block is asked for by attribute
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_tsv_write), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes_));
    stream_.create();
    for (auto &e : ev_) e.create();
    upload(names_, t.names, stream_); upload(name_off_, t.name_off, stream_); upload(rank_, t.rank, stream_);
    upload(rank_text_, t.rank_text, stream_); upload(rank_off_, t.rank_off, stream_);
    const TsvView hv = t.view();
    view_ = TsvView{names_, name_off_, rank_, rank_text_, rank_off_, hv.seq_cnt, hv.node_cnt};
    d_direct_.alloc(1);
    h_back_.alloc(2);
    HIP_CHECK(hipStreamSynchronize(stream_));    // (the host vectors are the caller's)
  }
  ~TsvDevice() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }

  bool format(const cfr_result *results, const cfr_match *matches, size_t n_slots, size_t n, const char *id_bytes, const uint64_t *id_offsets,
              char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets) override {
    tsv_check_args(results, matches, n_slots, n, id_bytes, id_offsets, text, cap, len);
    check_count(n);
    DeviceScope scope(device_);
    // the slots the reads use (the rest of the caller's array stays where it is)
    uint64_t extent = 0;
    for (size_t i = 0; i < n; ++i) if (results[i].n_match > 0) extent = std::max<uint64_t>(extent, results[i].match_begin + (uint64_t)results[i].n_match);
    grow(d_res_, cap_res_, std::max<size_t>(n, 1));
    grow(d_match_, cap_match_, std::max<size_t>(extent, 1));
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    if (n) HIP_CHECK(hipMemcpyAsync(d_res_, results, n * sizeof(cfr_result), hipMemcpyHostToDevice, stream_));
    if (extent) HIP_CHECK(hipMemcpyAsync(d_match_, matches, extent * sizeof(cfr_match), hipMemcpyHostToDevice, stream_));
    const TsvIds ids = upload_ids(n, id_bytes, id_offsets);
    return run(d_res_, d_match_, n, ids, text, cap, len, row_offsets);
  }

  bool format_resident(const cfr_result *d_results, const cfr_match *d_matches, size_t n, const TsvIds &ids_in, bool host_ids,
                       char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets) override {
    if (!len || (!text && cap)) throw std::invalid_argument("cfr_tsv: null argument");
    if (host_ids) tsv_check_ids(n, ids_in.bytes, ids_in.off);
    else if (n && (!ids_in.bytes || !ids_in.rec)) throw std::invalid_argument("cfr_tsv: the tokeniser's text and records are null");
    check_count(n);
    DeviceScope scope(device_);
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    const TsvIds ids = host_ids ? upload_ids(n, ids_in.bytes, ids_in.off) : ids_in;
    return run(d_results, d_matches, n, ids, text, cap, len, row_offsets);
  }

  void stats(cfr_tsv_stats *st) const override { *st = st_; }

 private:
  static void check_count(size_t n) {
    if ((uint64_t)n + 1 > (uint64_t)INT_MAX) throw std::invalid_argument("cfr_tsv: more than 2^31 - 2 reads in one call: hand over less");
  }

  // ids to HBM behind ev_[0] on the stream: the bytes in front of the last offset, the offsets as they are
  TsvIds upload_ids(size_t n, const char *id_bytes, const uint64_t *id_offsets) {
    const uint64_t total = id_offsets[n];
    grow(d_id_off_, cap_id_off_, n + 1);
    grow(d_id_bytes_, cap_id_bytes_, std::max<uint64_t>(total, 1));
    HIP_CHECK(hipMemcpyAsync(d_id_off_, id_offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream_));
    if (total) HIP_CHECK(hipMemcpyAsync(d_id_bytes_, id_bytes, total, hipMemcpyHostToDevice, stream_));
    return TsvIds{d_id_bytes_, d_id_off_, nullptr};
  }

  bool run(const cfr_result *d_res, const cfr_match *d_match, size_t n, const TsvIds &ids, char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets) {
    st_ = cfr_tsv_stats{};
    grow(d_len_, cap_len_, 2 * (n + 1));
    uint64_t *d_len = d_len_, *d_off = d_len + (n + 1);
    HIP_CHECK(hipEventRecord(ev_[1], stream_));
    const unsigned want = grid_for(n + 1, kBlock);
    hipLaunchKernelGGL(k_tsv_len, dim3(max_blocks_ ? std::min(want, max_blocks_) : want), dim3(kBlock), 0, stream_, view_, d_res, d_match, ids, (uint64_t)n, d_len);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev_[2], stream_));
    {
      size_t need = 0;
      HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, d_len, d_off, (int)(n + 1), stream_));
      grow(tmp_, cap_tmp_, need);
      need = cap_tmp_;
      HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp_.get(), need, d_len, d_off, (int)(n + 1), stream_));
    }
    HIP_CHECK(hipEventRecord(ev_[3], stream_));
    HIP_CHECK(hipMemcpyAsync(h_back_.get(), d_off + n, 8, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    const uint64_t total = h_back_.get()[0];
    *len = total;
    (void)hipEventElapsedTime(&st_.upload_ms, ev_[0], ev_[1]);
    (void)hipEventElapsedTime(&st_.len_ms, ev_[1], ev_[2]);
    (void)hipEventElapsedTime(&st_.scan_ms, ev_[2], ev_[3]);
    st_.blocks = (n + kBlock - 1) / kBlock;
    if (total > cap) return false;
    grow(d_text_, cap_text_, total + 16);
    HIP_CHECK(hipMemsetAsync(d_direct_, 0, 8, stream_));
    HIP_CHECK(hipEventRecord(ev_[4], stream_));
    if (n) {
      const unsigned blocks = (unsigned)st_.blocks;
      hipLaunchKernelGGL(k_tsv_write, dim3(max_blocks_ ? std::min(blocks, max_blocks_) : blocks), dim3(kBlock), lds_bytes_, stream_, view_, d_res, d_match, ids,
                         (uint64_t)n, d_off, d_text_.get(), tile_, d_direct_.get());
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(ev_[5], stream_));
    if (total) HIP_CHECK(hipMemcpyAsync(text, d_text_, total, hipMemcpyDeviceToHost, stream_));
    if (row_offsets) HIP_CHECK(hipMemcpyAsync(row_offsets, d_off, (n + 1) * 8, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(h_back_.get() + 1, d_direct_, 8, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipEventRecord(ev_[6], stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    (void)hipEventElapsedTime(&st_.write_ms, ev_[4], ev_[5]);
    (void)hipEventElapsedTime(&st_.download_ms, ev_[5], ev_[6]);
    st_.direct_blocks = h_back_.get()[1];
    return true;
  }

  int device_;
  uint32_t tile_ = 0;
  unsigned max_blocks_ = 0;
  size_t lds_bytes_ = 0;
  Stream stream_;                  // first: the last to go
  Event ev_[7];                    // start, ids and results up, lengths, scan, (the wait,) write begins, write done, copies out
  DevBuf<char> names_, rank_text_, d_id_bytes_, d_text_;
  DevBuf<uint64_t> name_off_, d_id_off_, d_len_;
  DevBuf<uint8_t> rank_, tmp_;
  DevBuf<uint32_t> rank_off_;
  DevBuf<cfr_result> d_res_;
  DevBuf<cfr_match> d_match_;
  DevBuf<unsigned long long> d_direct_;
  PinnedBuf<uint64_t> h_back_;     // [0]: the total, [1]: direct_blocks
  TsvView view_{};
  size_t cap_res_ = 0, cap_match_ = 0, cap_id_off_ = 0, cap_id_bytes_ = 0, cap_len_ = 0, cap_tmp_ = 0, cap_text_ = 0;
  cfr_tsv_stats st_{};
};

}  // namespace

Tsv *make_tsv_device(int device, const TsvTables &t, const cfr_tsv_options &o) { return new TsvDevice(device, t, o); }

}  // namespace cfr
