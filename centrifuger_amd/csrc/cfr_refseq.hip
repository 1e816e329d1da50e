// cfr_refseq.hip — the device form of the reference-text front end of the index writer (gfx950, nucleotide only).  The grammar, the
// three reader states and the maps between them: cfr_refseq_core.hpp; the host twin that states them as one byte loop: cfr_refseq.cpp.
// A chunk goes up once; everything else is kernels on the handle's stream.  A block is 256 lanes and 4096 bytes; wave v of a block
// walks bytes [1024 v, 1024 v + 1024) of it in 16 rounds of 64, one byte per lane and round.
//
//   k_ref_maps      every lane looks at 16 bytes: the block's last '\n' (one atomicMax in LDS) and the byte behind it give the block's map.
//   (hipcub::DeviceScan::ExclusiveScan over the maps with "first a, then b": the map from the chunk's first state to every block's.)
//   k_ref_mark      per wave and round, ballots of '\n' and '>' give the line starts of the 64 bytes; a lane finds the start of its own
//                   line with one count-leading-zeros and reads there whether the line is a header.  The state walks on from round to
//                   round; the states the waves of a block start in come from the waves' own maps through LDS.  Every byte gets its
//                   mark (dropped, kept, header, '>' of a header); the block counts its kept bytes and its headers.
//   (two ExclusiveSums: where every block's kept bytes and headers go; the totals come to the host, which sizes the record table.
//    That is the one wait in the middle of a call.)
//   k_ref_compact   the marks again: kept bytes to the staging buffer, back to back; every '>' writes its offset and the number of kept
//                   bytes before it.
//   k_ref_records   one lane per header: header_len, id_len, kept = the difference to the next header's count.
//   k_pack_text     (cfr_pack_text.hpp, the suffix sorter's) the staging buffer to 2-bit words at the chunk's place in U.
//   k_ref_assemble  one lane per word of T: binary search of the first segment, then every segment that overlaps the word gives its
//                   symbols with one funnel shift (key32) each; one plain store, no atomics.
//   k_ref_unpack    T back to ASCII (tests).
// No kernel waits for another block.  No lane keeps an array.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "cfr_hip_util.hpp"
#include "cfr_pack_text.hpp"
#include "cfr_refseq_core.hpp"

namespace cfr {

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kRounds = 16;
constexpr int kWaveSpan = kWave * kRounds;       // 1024 bytes
constexpr int kSpan = kBlock * kRounds;          // 4096 bytes
constexpr int kLaneBytes = 16;                   // k_ref_maps: 256 lanes x 16 bytes = one block's span

struct MapThen { __host__ __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return refseq_map_then(a, b); } };

// text: padded bytes (zero from eff to a multiple of kSpan, and 16 more), nb blocks; maps[nb] is written too (the scans run over nb + 1 entries)
__global__ __launch_bounds__(kBlock) void k_ref_maps(const uint8_t *text, uint32_t nb, uint32_t *maps) {
  __shared__ uint32_t s_last;                    // 1 + the offset of the block's last '\n' in the block, 0: none
  if (threadIdx.x == 0) s_last = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kSpan;
  const uint4 v = *reinterpret_cast<const uint4 *>(text + base + (uint64_t)threadIdx.x * kLaneBytes);
  uint32_t last = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t w = k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) if (((w >> (8 * b)) & 0xffu) == '\n') last = threadIdx.x * kLaneBytes + 4 * k + b + 1;
  }
  if (last) atomicMax(&s_last, last);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t q = s_last;
    maps[blockIdx.x] = refseq_map_of(q != 0, q == (uint32_t)kSpan, q != 0 && q < (uint32_t)kSpan && text[base + q] == '>', text[base] == '>');
    if (blockIdx.x == 0) maps[nb] = kRefMapIdentity;
  }
}

// the masks of one round of a wave: nl, gt: the lanes whose byte is '\n', '>'
// the state behind the 64 bytes, from the state s before them
__device__ __forceinline__ uint32_t round_next(uint64_t nl, uint64_t gt, uint32_t s) {
  if (nl >> 63) return kLs;
  const uint64_t ls = (nl << 1) | (s == kLs ? 1ull : 0ull);      // the lanes whose byte begins a line
  if (!ls) return s;
  const int p = 63 - __clzll((long long)ls);
  return (gt >> p) & 1ull ? kHdr : kSeq;
}

// eff: the bytes of the chunk that count; s0: the state before byte 0; pre: the scanned maps (pre[b]: from byte 0 to block b's first byte)
__global__ __launch_bounds__(kBlock) void k_ref_mark(const uint8_t *text, uint64_t eff, uint32_t s0, const uint32_t *pre, uint32_t nb, uint8_t *marks,
                                                     uint32_t *blk_kept, uint32_t *blk_hdr) {
  __shared__ uint32_t s_map[kWaves];
  __shared__ uint32_t s_kept, s_hdr;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (threadIdx.x == 0) { s_kept = 0; s_hdr = 0; }
  const uint64_t wbase = (uint64_t)blockIdx.x * kSpan + (uint64_t)wave * kWaveSpan;
  // the wave's own map: the three states walk through its 16 rounds side by side
  {
    uint32_t a = kLs, b = kSeq, c = kHdr;
    for (int r = 0; r < kRounds; ++r) {
      const uint32_t ch = text[wbase + r * kWave + lane];
      const uint64_t nl = __ballot(ch == '\n'), gt = __ballot(ch == '>');
      a = round_next(nl, gt, a); b = round_next(nl, gt, b); c = round_next(nl, gt, c);
    }
    if (lane == 0) s_map[wave] = a | (b << 2) | (c << 4);
  }
  __syncthreads();
  uint32_t s = refseq_map_apply(pre[blockIdx.x], s0);
  for (int v = 0; v < wave; ++v) s = refseq_map_apply(s_map[v], s);
  uint32_t kept = 0, hdr = 0;
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t i = wbase + r * kWave + lane;
    const uint32_t ch = text[i];
    const uint64_t nl = __ballot(ch == '\n'), gt = __ballot(ch == '>');
    const uint64_t ls = (nl << 1) | (s == kLs ? 1ull : 0ull), open = ls & gt;
    const uint64_t mine = ls & (~0ull >> (63 - lane));             // the line starts at or before this lane
    const bool in_hdr = mine ? ((open >> (63 - __clzll((long long)mine))) & 1ull) != 0 : s == kHdr;
    const bool is_open = ((open >> lane) & 1ull) != 0;
    const bool is_kept = !in_hdr && i < eff && refseq_kept_nt(ch);
    if (i < eff) marks[i] = is_open ? kMarkOpen : in_hdr ? kMarkHdr : is_kept ? kMarkKept : kMarkDrop;
    kept += (uint32_t)__popcll(__ballot(is_kept));
    hdr += (uint32_t)__popcll(open);                                // (the bytes from eff on are zero: no '>' among them)
    s = round_next(nl, gt, s);
  }
  if (lane == 0) { atomicAdd(&s_kept, kept); atomicAdd(&s_hdr, hdr); }
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_kept[blockIdx.x] = s_kept; blk_hdr[blockIdx.x] = s_hdr;
    if (blockIdx.x == 0) { blk_kept[nb] = 0; blk_hdr[nb] = 0; }
  }
}

// kept_ex / hdr_ex: the exclusive sums of the blocks' counts
__global__ __launch_bounds__(kBlock) void k_ref_compact(const uint8_t *text, const uint8_t *marks, uint64_t eff, const uint32_t *kept_ex, const uint32_t *hdr_ex,
                                                        uint8_t *stage, uint32_t *rec_header, uint32_t *rec_before) {
  __shared__ uint32_t s_kept[kWaves], s_hdr[kWaves];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint64_t wbase = (uint64_t)blockIdx.x * kSpan + (uint64_t)wave * kWaveSpan;
  {
    uint32_t kept = 0, hdr = 0;
    for (int r = 0; r < kRounds; ++r) {
      const uint64_t i = wbase + r * kWave + lane;
      const uint32_t m = i < eff ? marks[i] : (uint32_t)kMarkDrop;
      kept += (uint32_t)__popcll(__ballot(m == kMarkKept));
      hdr += (uint32_t)__popcll(__ballot(m == kMarkOpen));
    }
    if (lane == 0) { s_kept[wave] = kept; s_hdr[wave] = hdr; }
  }
  __syncthreads();
  uint32_t kat = kept_ex[blockIdx.x], hat = hdr_ex[blockIdx.x];
  for (int v = 0; v < wave; ++v) { kat += s_kept[v]; hat += s_hdr[v]; }
  const uint64_t below = ~(~0ull << lane);                           // the lanes before this one
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t i = wbase + r * kWave + lane;
    const uint32_t m = i < eff ? marks[i] : (uint32_t)kMarkDrop;
    const uint64_t km = __ballot(m == kMarkKept), hm = __ballot(m == kMarkOpen);
    const uint32_t before = kat + (uint32_t)__popcll(km & below);
    if (m == kMarkKept) stage[before] = text[i];
    if (m == kMarkOpen) {
      const uint32_t h = hat + (uint32_t)__popcll(hm & below);
      rec_header[h] = (uint32_t)i;
      rec_before[h] = before;
    }
    kat += (uint32_t)__popcll(km);
    hat += (uint32_t)__popcll(hm);
  }
}

// lanes 0 .. H - 1: the records; lane 0 also writes lead[0] = the kept bytes before the first header
__global__ __launch_bounds__(kBlock) void k_ref_records(const uint8_t *text, uint64_t eff, const uint32_t *rec_header, const uint32_t *rec_before, uint32_t H,
                                                        uint32_t total_kept, cfr_refseq_record *records, uint32_t *lead) {
  const uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (h == 0) lead[0] = H ? rec_before[0] : total_kept;
  if (h >= H) return;
  const uint32_t at = rec_header[h];
  uint64_t e = at;
  while (e < eff && text[e] != '\n') ++e;
  cfr_refseq_record rec;
  rec.header = at;
  rec.header_len = (uint32_t)(e - at);
  rec.id_len = refseq_id_len(text + at, rec.header_len);
  rec.kept = (h + 1 < H ? rec_before[h + 1] : total_kept) - rec_before[h];
  records[h] = rec;
}

struct Seg { uint64_t src, len, dst; };
static_assert(sizeof(Seg) == sizeof(cfr_refseq_segment), "segments are uploaded as they are");

// word w of T = the symbols [32 w, min(32 w + 32, n)): U holds a word behind the last one a segment touches
__global__ __launch_bounds__(kBlock) void k_ref_assemble(const uint64_t *U, const Seg *segs, uint64_t n_segs, uint64_t n, uint64_t n_words, uint64_t *T) {
  const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= n_words) return;
  uint64_t pos = w * 32;
  const uint64_t end = pos + 32 < n ? pos + 32 : n;
  uint64_t lo = 0, hi = n_segs;                  // the last segment that starts at or before pos
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (segs[mid].dst <= pos) lo = mid; else hi = mid;
  }
  uint64_t out = 0;
  for (uint64_t s = lo; pos < end && s < n_segs; ++s) {
    const Seg g = segs[s];
    const uint64_t stop = g.dst + g.len < end ? g.dst + g.len : end;
    const uint32_t take = (uint32_t)(stop - pos);                    // 1 .. 32 symbols of this segment
    const uint64_t bits = key32(U, g.src + (pos - g.dst)) & (take == 32 ? ~0ull : ~(~0ull >> (2 * take)));
    out |= bits >> (2 * (uint32_t)(pos - w * 32));
    pos = stop;
  }
  T[w] = out;
}

__global__ __launch_bounds__(kBlock) void k_ref_unpack(const uint64_t *T, uint64_t lo, uint64_t count, uint8_t *ascii) {
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= count) return;
  ascii[k] = (uint8_t)((0x54474341u >> (8 * sym_at(T, lo + k))) & 0xffu);      // "ACGT"
}

template <class T> void grow(DevBuf<T> &b, size_t &cap, size_t need) {      // by doubling; the old contents are not kept
  if (need <= cap) return;
  const size_t c = std::max(need, cap * 2);
  cap = 0;
  b.alloc(c);
  cap = c;
}

class RefseqDevice : public Refseq {
 public:
  explicit RefseqDevice(int device) : device_(device) {
    if (!device_exists(device)) throw HipError{"cfr_refseq_open: no HIP device " + std::to_string(device), -1};
    DeviceScope scope(device);
    stream_.create();
    for (auto &e : ev_) e.create();
    scal_.alloc(4);
    h_back_.alloc(4);
    HIP_CHECK(hipMemsetAsync(scal_, 0, 16, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }
  ~RefseqDevice() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }
  int device() const override { return device_; }

  void feed(const uint8_t *text, uint64_t len, int at_line_start, int final, cfr_refseq_info *info) override {
    DeviceScope scope(device_);
    memset(info, 0, sizeof(*info));
    n_records_ = 0;
    if (assembled_) throw std::invalid_argument("cfr_refseq_feed: the handle has assembled its text already");
    const uint64_t eff = refseq_effective_len(text, len, at_line_start, final);
    const uint64_t u_start = (u_len_ + 31) / 32 * 32;
    info->consumed = eff; info->u_start = u_start; info->at_line_start = eff ? (text[eff - 1] == '\n') : (at_line_start != 0);
    if (eff == 0) return;
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    const uint32_t nb = (uint32_t)((eff + kSpan - 1) / kSpan);
    const uint64_t padded = (uint64_t)nb * kSpan + kLaneBytes;
    grow(text_, cap_text_, padded);
    grow(marks_, cap_marks_, eff);
    grow(stage_, cap_stage_, eff);
    HIP_CHECK(hipMemcpyAsync(text_, text, eff, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemsetAsync(text_.get() + eff, 0, padded - eff, stream_));
    HIP_CHECK(hipEventRecord(ev_[1], stream_));

    grow(blk_, cap_blk_, 6 * ((size_t)nb + 1));
    uint32_t *maps = blk_, *pre = maps + nb + 1, *blk_kept = pre + nb + 1, *blk_hdr = blk_kept + nb + 1, *kept_ex = blk_hdr + nb + 1, *hdr_ex = kept_ex + nb + 1;
    hipLaunchKernelGGL(k_ref_maps, dim3(nb), dim3(kBlock), 0, stream_, (const uint8_t *)text_.get(), nb, maps);
    HIP_CHECK(hipGetLastError());
    {
      size_t need = 0;
      HIP_CHECK(hipcub::DeviceScan::ExclusiveScan(nullptr, need, maps, pre, MapThen(), (uint32_t)kRefMapIdentity, (int)(nb + 1), stream_));
      grow(tmp_, cap_tmp_, need);
      need = cap_tmp_;
      HIP_CHECK(hipcub::DeviceScan::ExclusiveScan(tmp_.get(), need, maps, pre, MapThen(), (uint32_t)kRefMapIdentity, (int)(nb + 1), stream_));
    }
    hipLaunchKernelGGL(k_ref_mark, dim3(nb), dim3(kBlock), 0, stream_, (const uint8_t *)text_.get(), eff, at_line_start ? (uint32_t)kLs : (uint32_t)kSeq,
                       (const uint32_t *)pre, nb, marks_.get(), blk_kept, blk_hdr);
    HIP_CHECK(hipGetLastError());
    sum(blk_kept, kept_ex, (size_t)nb + 1);
    sum(blk_hdr, hdr_ex, (size_t)nb + 1);
    uint32_t *h_tot = h_back_.get();
    HIP_CHECK(hipMemcpyAsync(h_tot, kept_ex + nb, 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(h_tot + 1, hdr_ex + nb, 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    const uint32_t kept = h_tot[0], H = h_tot[1];

    grow(rec_, cap_rec_, 2 * std::max<size_t>(H, 1));
    grow(records_, cap_records_, std::max<size_t>(H, 1));
    uint32_t *rec_header = rec_, *rec_before = rec_header + std::max<size_t>(H, 1);
    hipLaunchKernelGGL(k_ref_compact, dim3(nb), dim3(kBlock), 0, stream_, (const uint8_t *)text_.get(), (const uint8_t *)marks_.get(), eff, (const uint32_t *)kept_ex,
                       (const uint32_t *)hdr_ex, stage_.get(), rec_header, rec_before);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ref_records, dim3(grid_for(std::max<size_t>(H, 1), kBlock)), dim3(kBlock), 0, stream_, (const uint8_t *)text_.get(), eff,
                       (const uint32_t *)rec_header, (const uint32_t *)rec_before, H, kept, records_.get(), scal_.get());
    HIP_CHECK(hipGetLastError());
    if (kept) {
      reserve_u(u_start + kept);
      hipLaunchKernelGGL(k_pack_text, dim3(grid_for(((size_t)kept + 31) / 32, kBlock)), dim3(kBlock), 0, stream_, (const uint8_t *)stage_.get(), (uint64_t)kept,
                         u_.get() + u_start / 32, scal_.get() + 1);
      HIP_CHECK(hipGetLastError());
      u_len_ = u_start + kept;
    }
    HIP_CHECK(hipEventRecord(ev_[2], stream_));
    HIP_CHECK(hipMemcpyAsync(h_tot + 2, scal_, 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    float ms = 0.f, copy_ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[0], ev_[2]);
    (void)hipEventElapsedTime(&copy_ms, ev_[0], ev_[1]);
    info->n_records = H; info->kept = kept; info->lead_kept = h_tot[2]; info->device_ms = ms;
    n_records_ = H;
    feed_ms_ += ms; copy_in_ms_ += copy_ms;
  }

  void fetch(cfr_refseq_record *records) override {
    DeviceScope scope(device_);
    if (records && n_records_) {
      HIP_CHECK(hipMemcpyAsync(records, records_, n_records_ * sizeof(cfr_refseq_record), hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
  }

  void assemble(const cfr_refseq_segment *segments, uint64_t n_segments, uint64_t n) override {
    DeviceScope scope(device_);
    refseq_check_segments(segments, n_segments, n, u_len_);
    if (n == 0) throw std::invalid_argument("cfr_refseq_assemble: an empty text");
    const uint64_t n_words = (n + 31) / 32;
    DevBuf<Seg> d_segs(n_segments);
    t_.alloc(n_words + 4);
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    HIP_CHECK(hipMemcpyAsync(d_segs, segments, n_segments * sizeof(Seg), hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemsetAsync(t_.get() + n_words, 0, 4 * 8, stream_));
    hipLaunchKernelGGL(k_ref_assemble, dim3(grid_for(n_words, kBlock)), dim3(kBlock), 0, stream_, (const uint64_t *)u_.get(), (const Seg *)d_segs.get(), n_segments, n,
                       n_words, t_.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev_[1], stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[0], ev_[1]);
    assemble_ms_ = ms;
    n_ = n;
    assembled_ = true;
    u_.reset(); cap_u_ = 0; u_len_ = 0;
    text_.reset(); marks_.reset(); stage_.reset(); cap_text_ = cap_marks_ = cap_stage_ = 0;
  }

  void text(uint8_t *ascii_out) override {
    DeviceScope scope(device_);
    if (!t_.get()) throw std::invalid_argument("cfr_refseq_text: no assembled text in the handle");
    const uint64_t piece = 1ull << 26;
    DevBuf<uint8_t> d_ascii(std::min(piece, std::max<uint64_t>(n_, 1)));
    for (uint64_t lo = 0; lo < n_; lo += piece) {
      const uint64_t cnt = std::min(piece, n_ - lo);
      hipLaunchKernelGGL(k_ref_unpack, dim3(grid_for(cnt, kBlock)), dim3(kBlock), 0, stream_, (const uint64_t *)t_.get(), lo, cnt, d_ascii.get());
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(ascii_out + lo, d_ascii, cnt, hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
  }
  uint64_t text_len() const override { return n_; }
  void stats(cfr_refseq_stats *st) const override { st->feed_ms = feed_ms_; st->copy_in_ms = copy_in_ms_; st->assemble_ms = assemble_ms_; }
  uint64_t *release_device_text() override { n_ = 0; return t_.release(); }

 private:
  void sum(const uint32_t *in, uint32_t *out, size_t count) {
    size_t need = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)count, stream_));
    grow(tmp_, cap_tmp_, need);
    need = cap_tmp_;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp_.get(), need, in, out, (int)count, stream_));
  }
  // U holds `symbols` symbols and the word behind them (key32 reads it); grown by doubling, the old words are kept
  void reserve_u(uint64_t symbols) {
    const size_t need = (size_t)((symbols + 31) / 32 + 2);
    if (need <= cap_u_) return;
    const size_t c = std::max(need, cap_u_ * 2);
    DevBuf<uint64_t> bigger(c);
    const size_t have = (size_t)((u_len_ + 31) / 32);
    if (have) HIP_CHECK(hipMemcpyAsync(bigger, u_, have * 8, hipMemcpyDeviceToDevice, stream_));
    HIP_CHECK(hipMemsetAsync(bigger.get() + have, 0, (c - have) * 8, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    u_ = std::move(bigger);
    cap_u_ = c;
  }

  int device_;
  Stream stream_;                  // first: the last to go
  Event ev_[3];
  DevBuf<uint8_t> text_, marks_, stage_, tmp_;
  DevBuf<uint32_t> blk_, rec_, scal_;             // scal_[0]: lead_kept; [1]: k_pack_text's flag (never raised: only A,C,G,T are kept)
  DevBuf<cfr_refseq_record> records_;
  DevBuf<uint64_t> u_, t_;
  PinnedBuf<uint32_t> h_back_;     // [0], [1]: the two totals; [2]: lead_kept
  size_t cap_text_ = 0, cap_marks_ = 0, cap_stage_ = 0, cap_tmp_ = 0, cap_blk_ = 0, cap_rec_ = 0, cap_records_ = 0, cap_u_ = 0;
  uint64_t u_len_ = 0, n_ = 0, n_records_ = 0;
  bool assembled_ = false;
  double feed_ms_ = 0.0, copy_in_ms_ = 0.0, assemble_ms_ = 0.0;
};

}  // namespace

Refseq *make_refseq_device(int device) { return new RefseqDevice(device); }

}  // namespace cfr
