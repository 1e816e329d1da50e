// cfr_tokenize.hip — the device form of the tokeniser (gfx950).  The grammar and the per-unit rules: cfr_tokenize_core.hpp; the host
// twin that states them in plain loops: cfr_tokenize_host.cpp.  The whole chunk goes up once, everything else is kernels on the
// handle's stream:
//
//   k_tok_count     every lane takes 16 bytes (one 16-byte load): the '\n' bytes and, at line starts, the '>' bytes of a block's 4096.
//   (hipcub::DeviceScan::ExclusiveSum over the blocks' counts; the totals - lines L, FASTA headers H - go to the host, which sizes
//    the tables.  That is the one wait in the middle of a call.)
//   k_tok_lines     the same 16 bytes again; a scan inside the block gives every '\n' its line number j: lcend[j] (the '\n', moved left over
//                   a run of '\r' - the run may reach into the bytes of another lane or block, so it is read from memory),
//                   lstart[j + 1], for FASTA line_rec[j] and hdr_line[r]; the last line that is not empty (one atomicMax per block).
//   k_tok_records   one lane per unit (a FASTQ record, a FASTA line): the rules of the core header; cfr_read_record, the unit's weight,
//                   atomicMin of the first record that breaks a rule.
//   (ExclusiveSum over the weights: every unit's place in the flat buffer.)
//   k_tok_gather    one wave per unit: its sequence bytes to the flat buffer, 64 consecutive bytes per step (a lane per read would be
//                   64 uncoalesced streams).  A unit has any length: the wave walks it.
//   k_tok_offsets   one lane per record: the 64-bit offsets of the delivered records; lane 0 writes the summary the host reads back.
//   k_tok_id_len, k_tok_ids   cfr_tokenizer_fetch_ids: the delivered records' id lengths, (ExclusiveSum), 16 lanes per record copy its id.
// cfr_tokenize_resident takes the text from this device's memory: one device-to-device copy into the same padded buffer, then the same kernels.
// No kernel waits for another block: the scans are launches of their own.  No lane keeps an array.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "cfr_hip_util.hpp"
#include "cfr_tokenize_core.hpp"

namespace cfr {

namespace {

constexpr int kBlock = 256;
constexpr int kLaneBytes = 16;
constexpr int kSpan = kBlock * kLaneBytes;       // the bytes of one block of k_tok_count / k_tok_lines
constexpr int kWave = 64;

// bit k of the result: byte k of w equals c (exact per byte: no borrow runs from one byte into the next)
__device__ inline uint32_t byte_eq4(uint32_t w, uint32_t c) {
  const uint32_t x = w ^ (c * 0x01010101u);
  const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);       // 0x80 in every byte of x that is zero
  return (((z >> 7) * 0x01020408u) >> 24) & 0xfu;
}
__device__ inline uint32_t byte_eq16(const uint4 &w, uint32_t c) {
  return byte_eq4(w.x, c) | (byte_eq4(w.y, c) << 4) | (byte_eq4(w.z, c) << 8) | (byte_eq4(w.w, c) << 12);
}
// the lane's 16 bytes at pos (a multiple of 16, below eff; the buffer is zero from eff to the end of its last 16 bytes):
// nl: the '\n' bytes; hd: the '>' bytes that start a line
__device__ inline void tok_masks(const uint8_t *text, uint64_t pos, uint32_t &nl, uint32_t &hd) {
  const uint4 w = *reinterpret_cast<const uint4 *>(text + pos);
  nl = byte_eq16(w, '\n');
  const uint32_t prev = pos == 0 ? 1u : (text[pos - 1] == '\n' ? 1u : 0u);
  hd = ((nl << 1) | prev) & byte_eq16(w, '>') & 0xffffu;
}

// counts of a block, '\n' in the low half and headers in the high half (at most 4096 and 2048: no carry between the halves)
__global__ __launch_bounds__(kBlock) void k_tok_count(const uint8_t *text, uint64_t eff, uint32_t nb, uint32_t *blk_nl, uint32_t *blk_hd) {
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const uint64_t pos = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kLaneBytes;
  uint32_t nl = 0, hd = 0;
  if (pos < eff) tok_masks(text, pos, nl, hd);
  uint32_t packed = __popc(nl) | (__popc(hd) << 16);
  for (int off = kWave / 2; off > 0; off >>= 1) packed += __shfl_down(packed, off);
  if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(&s_sum, packed);
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_nl[blockIdx.x] = s_sum & 0xffffu;
    blk_hd[blockIdx.x] = s_sum >> 16;
    if (blockIdx.x == 0) { blk_nl[nb] = 0; blk_hd[nb] = 0; }     // (the scans run over nb + 1 entries: the last one is the total)
  }
}

__global__ __launch_bounds__(kBlock) void k_tok_lines(const uint8_t *text, uint64_t eff, const uint32_t *blk_nl_ex, const uint32_t *blk_hd_ex, uint32_t L,
                                                      int fastq, uint32_t *lstart, uint32_t *lcend, uint32_t *hdr_line, uint32_t *line_rec,
                                                      uint32_t *last_nonempty) {
  __shared__ uint32_t s_wave[kBlock / kWave];
  __shared__ uint32_t s_max;
  if (threadIdx.x == 0) s_max = 0;
  const uint64_t pos = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kLaneBytes;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint32_t nl = 0, hd = 0;
  if (pos < eff) tok_masks(text, pos, nl, hd);
  const uint32_t packed = __popc(nl) | (__popc(hd) << 16);
  uint32_t incl = packed;
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == kWave - 1) s_wave[wave] = incl;
  __syncthreads();
  uint32_t excl = incl - packed;
  for (int w = 0; w < wave; ++w) excl += s_wave[w];
  const uint32_t j0 = blk_nl_ex[blockIdx.x] + (excl & 0xffffu), h0 = blk_hd_ex[blockIdx.x] + (excl >> 16);

  if (pos == 0 && L) lstart[0] = 0;
  uint32_t my_max = 0, j = j0;
  for (uint32_t m = nl; m; m &= m - 1, ++j) {
    const int k = __ffs(m) - 1;
    const uint64_t p = pos + k;
    uint64_t e = p;
    while (e > 0 && text[e - 1] == '\r') --e;          // (stops at the previous line's '\n' at the latest)
    lcend[j] = (uint32_t)e;
    if (j + 1 < L) lstart[j + 1] = (uint32_t)(p + 1);
    if (!fastq) line_rec[j] = h0 + __popc(hd & ((2u << k) - 1)) - 1;
    if (e > 0 && text[e - 1] != '\n') my_max = j + 1;
  }
  if (!fastq) {
    uint32_t h = h0;
    for (uint32_t m = hd; m; m &= m - 1, ++h) {
      const int k = __ffs(m) - 1;
      hdr_line[h] = j0 + __popc(nl & ((1u << k) - 1));
    }
  }
  if (my_max) atomicMax(&s_max, my_max);
  __syncthreads();
  if (threadIdx.x == 0 && s_max) atomicMax(last_nonempty, s_max);
}

// lanes 0 .. units: the last one writes the zero the scan of the weights ends on
__global__ __launch_bounds__(kBlock) void k_tok_records(TokTables t, uint32_t units, cfr_read_record *records, uint32_t *weight, uint32_t *first_bad,
                                                        const uint32_t *last_nonempty) {
  const uint64_t u64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (u64 > units) return;
  const uint32_t u = (uint32_t)u64;
  if (u == units) { weight[u] = 0; return; }
  const uint32_t cand = tok_candidates(t, *last_nonempty);
  uint32_t w = 0;
  if (t.fastq) {
    cfr_read_record rec;
    const bool ok = tok_fastq_unit(t, u, cand, rec, w);
    records[u] = rec;
    if (!ok) atomicMin(first_bad, u);
  } else {
    if (!tok_fasta_unit(t, u, cand, records, w)) atomicMin(first_bad, t.line_rec[u]);
  }
  weight[u] = w;
}

__global__ __launch_bounds__(kBlock) void k_tok_gather(TokTables t, uint32_t units, const uint32_t *weight, const uint32_t *dst, uint8_t *bases) {
  const uint64_t u64 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  if (u64 >= units) return;
  const uint32_t u = (uint32_t)u64, n = weight[u];
  if (n == 0) return;
  const uint8_t *src = t.text + t.lstart[t.fastq ? 4 * u + 1 : u];
  uint8_t *out = bases + dst[u];
  for (uint32_t i = threadIdx.x & (kWave - 1); i < n; i += kWave) out[i] = src[i];
}

// lanes 0 .. n_max (the records there can be at most)
__global__ __launch_bounds__(kBlock) void k_tok_offsets(TokTables t, uint32_t n_max, const uint32_t *dst, const uint32_t *first_bad, const uint32_t *last_nonempty,
                                                        uint64_t max_records, uint64_t *offsets, TokSummary *summary) {
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r > n_max) return;
  const TokSummary s = tok_summary(t, dst, *last_nonempty, *first_bad, max_records);
  if (r <= s.n_records) offsets[r] = tok_offset(t, dst, (uint32_t)r);
  if (r == 0) *summary = s;
}

// the ids of the delivered records (cfr_tokenizer_fetch_ids): lanes 0 .. n write the lengths, the last one the zero the scan ends on
__global__ __launch_bounds__(kBlock) void k_tok_id_len(const cfr_read_record *records, uint64_t n, uint32_t *len) {
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r <= n) len[r] = r == n ? 0u : records[r].id_len;
}
// kIdLanes lanes per record copy its id (the id_len bytes behind the header character) to its place
constexpr int kIdLanes = 16;
__global__ __launch_bounds__(kBlock) void k_tok_ids(const uint8_t *text, const cfr_read_record *records, uint64_t n, const uint32_t *off, uint8_t *ids) {
  const uint64_t r = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kIdLanes;
  if (r >= n) return;
  const uint8_t *src = text + records[r].header + 1;
  uint8_t *dst = ids + off[r];
  const uint32_t len = records[r].id_len;
  for (uint32_t i = threadIdx.x & (kIdLanes - 1); i < len; i += kIdLanes) dst[i] = src[i];
}

template <class T> void grow(DevBuf<T> &b, size_t &cap, size_t need) {      // by doubling; the old contents are not kept
  if (need <= cap) return;
  const size_t c = std::max(need, cap * 2);
  cap = 0;                 // (alloc lets go of the old block first: a throw must not leave the old capacity beside a null pointer)
  b.alloc(c);
  cap = c;
}

class TokenizerDevice : public Tokenizer {
 public:
  explicit TokenizerDevice(int device) : device_(device) {
    if (!device_exists(device)) throw HipError{"cfr_tokenizer_open: no HIP device " + std::to_string(device), -1};
    DeviceScope scope(device);
    stream_.create();
    for (auto &e : ev_) e.create();
    scal_.alloc(2);
    d_summary_.alloc(1);
    h_back_.alloc(8);
    grow(offsets_, cap_offsets_, 1);
    grow(bases_, cap_bases_, 16);
    HIP_CHECK(hipMemsetAsync(offsets_, 0, 8, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }
  ~TokenizerDevice() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }

  void tokenize(const uint8_t *text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info) override {
    DeviceScope scope(device_);
    memset(info, 0, sizeof(*info));
    n_records_ = 0; total_bases_ = 0; copy_in_ms_ = kernel_ms_ = 0.0;
    if (len) info->fastq = text[0] == '@';
    bool virtual_newline = false;
    const uint64_t eff = tok_effective_len(text, len, final, virtual_newline);
    run(text, hipMemcpyHostToDevice, len, eff, virtual_newline, final, max_records, info);
  }

  // the same with the text in this device's memory: the first byte, and the last one (final) or the last '\n' (looked for from the
  // end in pieces of kEdge bytes), come to the host to decide what tok_effective_len decides from host text
  // (text that is to be continued and has no '\n' in its last kEdge bytes costs one small copy and one wait per kEdge bytes until one
  // is found: len / 65536 round trips at the worst, for a text without any line end - one record of many MB)
  bool tokenize_resident(const void *d_text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info) override {
    DeviceScope scope(device_);
    memset(info, 0, sizeof(*info));
    n_records_ = 0; total_bases_ = 0; copy_in_ms_ = kernel_ms_ = 0.0;
    const uint8_t *src = static_cast<const uint8_t *>(d_text);
    bool virtual_newline = false;
    uint64_t eff = 0;
    if (len) {
      if (!h_edge_) h_edge_.alloc(kEdge);
      uint8_t *h = h_edge_.get();
      HIP_CHECK(hipMemcpyAsync(h, src, 1, hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipMemcpyAsync(h + 1, src + len - 1, 1, hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
      if (h[0] != '>' && h[0] != '@') throw std::invalid_argument("cfr_tokenize_resident: the text starts with neither '>' (FASTA) nor '@' (FASTQ)");
      info->fastq = h[0] == '@';
      if (final) { virtual_newline = h[1] != '\n'; eff = len + (virtual_newline ? 1 : 0); }
      else if (h[1] == '\n') eff = len;
      else
        for (uint64_t end = len; end > 0 && eff == 0;) {
          const uint64_t piece = std::min<uint64_t>(end, kEdge), lo = end - piece;
          HIP_CHECK(hipMemcpyAsync(h, src + lo, piece, hipMemcpyDeviceToHost, stream_));
          HIP_CHECK(hipStreamSynchronize(stream_));
          if (const void *nl = memrchr(h, '\n', piece)) eff = lo + (uint64_t)((const uint8_t *)nl - h) + 1;
          end = lo;
        }
    }
    run(src, hipMemcpyDeviceToDevice, len, eff, virtual_newline, final, max_records, info);
    return true;
  }

  bool fetch_ids(char *ids, uint64_t cap, uint64_t *id_off, uint64_t *need) override {
    DeviceScope scope(device_);
    const uint64_t n = n_records_;
    if ((uint64_t)n + 1 > (uint64_t)INT_MAX) throw CapacityError{"cfr_tokenizer_fetch_ids: more than 2^31 - 2 records"};
    grow(idlen_, cap_idlen_, 2 * ((size_t)n + 1));
    uint32_t *len = idlen_, *off = len + n + 1;
    hipLaunchKernelGGL(k_tok_id_len, dim3(grid_for((size_t)n + 1, kBlock)), dim3(kBlock), 0, stream_, (const cfr_read_record *)records_.get(), n, len);
    HIP_CHECK(hipGetLastError());
    scan(len, off, (size_t)n + 1);
    h_idoff_.resize((size_t)n + 1);
    HIP_CHECK(hipMemcpyAsync(h_idoff_.data(), off, (n + 1) * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    const uint64_t total = h_idoff_[n];
    *need = total;
    if (ids && total > cap) return false;
    if (ids && total) {
      grow(ids_, cap_ids_, total);
      hipLaunchKernelGGL(k_tok_ids, dim3(grid_for((size_t)n * kIdLanes, kBlock)), dim3(kBlock), 0, stream_, (const uint8_t *)text_.get(),
                         (const cfr_read_record *)records_.get(), n, (const uint32_t *)off, ids_.get());
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(ids, ids_, total, hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    if (id_off)
      for (uint64_t r = 0; r <= n; ++r) id_off[r] = h_idoff_[r];
    return true;
  }

 private:
  static constexpr uint64_t kEdge = 1u << 16;

  // src: len bytes of host or device memory (kind says which); eff and virtual_newline as tok_effective_len gives them
  void run(const uint8_t *text, hipMemcpyKind kind, uint64_t len, uint64_t eff, bool virtual_newline, int final, uint64_t max_records, cfr_token_info *info) {
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    if (eff == 0) {
      HIP_CHECK(hipMemsetAsync(offsets_, 0, 8, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
      return;
    }
    // the text, zero up to the end of its last 16 bytes, and the tokeniser's own '\n' where the text ends without one
    const uint64_t padded = (eff + kLaneBytes - 1) / kLaneBytes * kLaneBytes, copied = std::min(len, eff);
    grow(text_, cap_text_, padded);
    grow(bases_, cap_bases_, eff);
    HIP_CHECK(hipMemcpyAsync(text_, text, copied, kind, stream_));
    if (padded > copied) HIP_CHECK(hipMemsetAsync(text_.get() + copied, 0, padded - copied, stream_));
    if (virtual_newline) HIP_CHECK(hipMemsetAsync(text_.get() + len, '\n', 1, stream_));
    HIP_CHECK(hipEventRecord(ev_[1], stream_));

    const uint32_t nb = (uint32_t)((eff + kSpan - 1) / kSpan);
    grow(blk_, cap_blk_, 4 * ((size_t)nb + 1));
    uint32_t *blk_nl = blk_, *blk_hd = blk_nl + nb + 1, *blk_nl_ex = blk_hd + nb + 1, *blk_hd_ex = blk_nl_ex + nb + 1;
    hipLaunchKernelGGL(k_tok_count, dim3(nb), dim3(kBlock), 0, stream_, text_.get(), eff, nb, blk_nl, blk_hd);
    HIP_CHECK(hipGetLastError());
    scan(blk_nl, blk_nl_ex, (size_t)nb + 1);
    scan(blk_hd, blk_hd_ex, (size_t)nb + 1);
    uint32_t *h_tot = reinterpret_cast<uint32_t *>(h_back_.get());
    HIP_CHECK(hipMemcpyAsync(h_tot, blk_nl_ex + nb, 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(h_tot + 1, blk_hd_ex + nb, 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));

    TokTables t{};
    t.L = h_tot[0]; t.H = info->fastq ? 0 : h_tot[1];
    t.len = len; t.eff = eff; t.fastq = info->fastq; t.final = final ? 1 : 0;
    const uint32_t units = tok_units(t), n_max = t.fastq ? units : t.H;
    if ((uint64_t)t.L + 1 > (uint64_t)INT_MAX) throw CapacityError{"cfr_tokenize: more than 2^31 - 2 lines in one call on the device: hand over less text"};
    grow(lines_, cap_lines_, 2 * (size_t)t.L);
    if (!t.fastq) grow(fasta_, cap_fasta_, (size_t)t.L + t.H);
    grow(records_, cap_records_, std::max<size_t>(n_max, 1));
    grow(units_, cap_units_, 2 * ((size_t)units + 1));
    grow(offsets_, cap_offsets_, (size_t)n_max + 1);
    uint32_t *lstart = lines_, *lcend = lstart + t.L, *line_rec = fasta_, *hdr_line = t.fastq ? nullptr : line_rec + t.L;
    uint32_t *weight = units_, *dst = weight + units + 1;
    uint32_t *first_bad = scal_, *last_nonempty = first_bad + 1;
    t.text = text_; t.lstart = lstart; t.lcend = lcend; t.hdr_line = hdr_line; t.line_rec = line_rec;
    HIP_CHECK(hipMemsetAsync(first_bad, 0xff, 4, stream_));
    HIP_CHECK(hipMemsetAsync(last_nonempty, 0, 4, stream_));
    hipLaunchKernelGGL(k_tok_lines, dim3(nb), dim3(kBlock), 0, stream_, text_.get(), eff, blk_nl_ex, blk_hd_ex, t.L, (int)t.fastq, lstart, lcend, hdr_line,
                       line_rec, last_nonempty);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_tok_records, dim3(grid_for((size_t)units + 1, kBlock)), dim3(kBlock), 0, stream_, t, units, records_.get(), weight, first_bad,
                       last_nonempty);
    HIP_CHECK(hipGetLastError());
    scan(weight, dst, (size_t)units + 1);
    if (units) {
      hipLaunchKernelGGL(k_tok_gather, dim3(grid_for((size_t)units * kWave, kBlock)), dim3(kBlock), 0, stream_, t, units, weight, dst, bases_.get());
      HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tok_offsets, dim3(grid_for((size_t)n_max + 1, kBlock)), dim3(kBlock), 0, stream_, t, n_max, dst, first_bad, last_nonempty, max_records,
                       offsets_.get(), d_summary_.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev_[2], stream_));
    TokSummary *h_sum = reinterpret_cast<TokSummary *>(h_back_.get() + 2);
    HIP_CHECK(hipMemcpyAsync(h_sum, d_summary_, sizeof(TokSummary), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipEventRecord(ev_[3], stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    float ms = 0.f, copy_ms = 0.f, kernel_ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[0], ev_[3]);
    (void)hipEventElapsedTime(&copy_ms, ev_[0], ev_[1]);
    (void)hipEventElapsedTime(&kernel_ms, ev_[1], ev_[2]);
    copy_in_ms_ = copy_ms; kernel_ms_ = kernel_ms;
    info->n_records = h_sum->n_records; info->consumed = h_sum->consumed; info->total_bases = h_sum->total_bases;
    info->irregular = h_sum->irregular; info->irregular_at = h_sum->irregular_at; info->device_ms = ms;
    n_records_ = h_sum->n_records; total_bases_ = h_sum->total_bases;
  }

 public:
  void fetch(cfr_read_record *records, uint64_t *offsets, uint8_t *bases) override {
    DeviceScope scope(device_);
    if (records && n_records_) HIP_CHECK(hipMemcpyAsync(records, records_, n_records_ * sizeof(cfr_read_record), hipMemcpyDeviceToHost, stream_));
    if (offsets) HIP_CHECK(hipMemcpyAsync(offsets, offsets_, (n_records_ + 1) * 8, hipMemcpyDeviceToHost, stream_));
    if (bases && total_bases_) HIP_CHECK(hipMemcpyAsync(bases, bases_, total_bases_, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  void stats(cfr_token_stats *st) const override { st->copy_in_ms = copy_in_ms_; st->kernel_ms = kernel_ms_; }

  bool device_reads(const void **d_bases, const void **d_offsets) override {
    if (d_bases) *d_bases = bases_.get();
    if (d_offsets) *d_offsets = offsets_.get();
    return true;
  }

  bool device_records(const void **d_text, const void **d_records) override {
    if (d_text) *d_text = text_.get();
    if (d_records) *d_records = records_.get();
    return true;
  }

 private:
  void scan(const uint32_t *in, uint32_t *out, size_t count) {
    size_t need = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)count, stream_));
    grow(tmp_, cap_tmp_, need);
    need = cap_tmp_;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp_.get(), need, in, out, (int)count, stream_));
  }

  int device_;
  Stream stream_;                  // first: the last to go
  Event ev_[4];                    // start, copy in done, kernels done, end
  DevBuf<uint8_t> text_, bases_, tmp_;
  DevBuf<uint32_t> blk_, lines_, fasta_, units_, scal_;
  DevBuf<cfr_read_record> records_;
  DevBuf<uint64_t> offsets_;
  DevBuf<TokSummary> d_summary_;
  PinnedBuf<uint64_t> h_back_;     // [0]: the two totals; [2..]: the summary
  PinnedBuf<uint8_t> h_edge_;      // tokenize_resident: the text's first and last byte, or a piece of its end
  DevBuf<uint32_t> idlen_;         // fetch_ids: the ids' lengths, then their exclusive sum
  DevBuf<uint8_t> ids_;
  std::vector<uint32_t> h_idoff_;
  size_t cap_idlen_ = 0, cap_ids_ = 0;
  size_t cap_text_ = 0, cap_bases_ = 0, cap_tmp_ = 0, cap_blk_ = 0, cap_lines_ = 0, cap_fasta_ = 0, cap_units_ = 0, cap_records_ = 0, cap_offsets_ = 0;
  uint64_t n_records_ = 0, total_bases_ = 0;
  double copy_in_ms_ = 0.0, kernel_ms_ = 0.0;
};

}  // namespace

Tokenizer *make_tokenizer_device(int device) { return new TokenizerDevice(device); }

}  // namespace cfr
