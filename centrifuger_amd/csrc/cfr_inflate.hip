// cfr_inflate.hip — BGZF members in HBM inflated and CRC-checked there (gfx950).  What the text and the statuses are:
// cfr_inflate_core.hpp (inf_member is the decoder, this file is its maker's part); the host twin: cfr_inflate.cpp.
//
// The host walks the headers (inf_walk: 18 + 8 bytes per member) and so knows every member's place, ISIZE and CRC, and the text's
// size, which it needs to refuse 4 GiB of text and to size the buffers before anything is launched.  The compressed bytes, the member
// table, the members' text sizes and the statuses the framing decided go up; an exclusive scan of the sizes
// (hipcub::DeviceScan::ExclusiveSum) gives every member's place in the text; one kernel runs; the statuses come back, the text only
// when the caller asks for it.
//
//   k_bgzf_inflate   one wave (a workgroup of 64) owns a member at a time, the workgroups stride over the members.
//     Decode scheme (a): the bit stream is serial, so the wave walks it as one - every lane runs inf_member on the same values (the
//     branches are uniform), and the lanes split up only what has width: building the tables, a run of literals, a match copy, a
//     stored block, the CRC.  The rate this gives and why the feature stands on it: DESIGN.md, section 4l.
//     Bit reader: each lane holds one 32-bit word of a 256-byte window of the stream in a register (bytes behind the stream's end are
//     zero, every byte load is checked against the end); peek takes two neighbouring words by readlane.  No LDS, no memory access per
//     token; the window is reloaded every 63 words.
//     Decode tables of the current block, in LDS: first-level tables of 10 / 9 / 7 bits (literal/length, distance, code-length code)
//     of 16-bit entries, the symbols in canonical order and the counts per length for the overflow walk (inf_decode).  The wave builds
//     them: counts per length by LDS atomics, inf_check_set, first index and first code per length, then 64 symbols at a time - a
//     symbol's rank among the symbols of its length is the running count plus the equal lengths on the lanes below it (four ballots) -
//     and every lane fills its symbol's table entries.
//     LDS: 2048 + 1024 + 256 (tables) + 576 + 64 + 40 (symbols) + 96 + 64 + 96 (counts, atomics, ranks) + 320 + 20 (lengths) + 1024 (CRC
//     table) = 5628 bytes a workgroup, 5636 as the compiler lays them out.  That would let 29 workgroups share a CU's 160 KiB; a
//     workgroup is one wave, so the registers decide: 111 VGPRs, at most 128 (tests/test_kernel_resources_inflate.py), is 4 waves per
//     SIMD, 16 workgroups per CU.
//     Literals are held back, one per lane, and stored 64 at a time or when a copy or the block's end comes.
//     Match copies: the text is written to HBM, not staged in LDS - a member's text is up to 64 KiB, which with the tables is more
//     than a workgroup's 64 KiB of static LDS and would leave two workgroups per CU.  A copy reads what OTHER lanes of this wave
//     stored, so the stores must have left the wave before the loads are issued: a workgroup-scope release / acquire
//     (__syncthreads(): the stores are waited for - vmcnt(0) - and the wave's CU has one L1, write-through, which the workgroup
//     scope relies on) stands between them.  The machine remembers the output position of its last fence and fences again only
//     when a copy's source reaches beyond it; within a copy no lane reads what the copy writes (src[i % distance] lies in front of it).
//     Trailer: inf_member compares the byte count with ISIZE; then, behind one more fence, the CRC32 of the text with a slice of
//     kGzCrcSlice bytes per lane and six joins, as k_gz_deflate does it.  A member with a status has its text zeroed (behind a fence:
//     the zeros must not overtake the stores they replace).
// Untrusted input: every load of the stream is checked against the stream's end (load_window, and copy_stored behind inf_member's
// check), every store and every copy source against [0, ISIZE) by inf_member before the call.  No lane keeps an array: no scratch.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "cfr_hip_util.hpp"
#include "cfr_inflate.hpp"

namespace cfr {

namespace {

constexpr int kLanes = 64;

struct DevMachine {
  const uint8_t *in;             // the deflate stream
  uint32_t n_in;
  uint8_t *out;                  // the member's text: isize bytes
  uint32_t lane;
  uint32_t *cnt32;               // 16: the counts while they are atomics
  uint16_t *bidx, *bcode, *run;  // 16 each: first index and first code of a length, the symbols of it placed so far
  uint32_t win, wq;              // word wq + lane of the stream
  uint32_t lit, nlit, lit_at;    // the literals held back: lane k has the byte for text[lit_at + k], k < nlit
  uint32_t fenced;               // every store below this output position has left the wave

  __device__ void load_window(uint32_t q) {
    wq = q;
    const uint32_t b = 4 * (q + lane);
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (b + k < n_in) v |= (uint32_t)in[b + k] << (8 * k);
    win = v;
  }
  __device__ uint32_t peek(uint32_t pos) {
    const uint32_t q = pos >> 5;
    if (q < wq || q + 1 >= wq + kLanes) load_window(q);               // (pos is the same in every lane)
    const uint32_t k = __builtin_amdgcn_readfirstlane(q - wq);
    const uint32_t lo = __builtin_amdgcn_readlane(win, k), hi = __builtin_amdgcn_readlane(win, k + 1);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (pos & 31));
  }
  __device__ void sync() { __syncthreads(); }
  __device__ void set_len(uint8_t *a, uint32_t i, uint32_t n, uint32_t v) {
    for (uint32_t k = lane; k < n; k += kLanes) a[i + k] = (uint8_t)v;
  }
  __device__ void fixed_lens(uint8_t *lens) {
    for (uint32_t s = lane; s < kInfLitSyms; s += kLanes) lens[s] = (uint8_t)gz_fixed_len(s);
    if (lane < kInfDistSyms) lens[kInfLitSyms + lane] = 5;
  }
  __device__ bool build(const uint8_t *lens, uint32_t n, int32_t kind, uint16_t *tab, uint32_t tbits, uint16_t *cnt, uint16_t *sym) {
    __syncthreads();                                                   // the lengths are written; the old tables are read no more
    if (lane < 16) cnt32[lane] = 0;
    for (uint32_t k = lane; k < (1u << tbits); k += kLanes) tab[k] = 0;
    __syncthreads();
    for (uint32_t s = lane; s < n; s += kLanes) {
      const uint32_t l = lens[s];
      if (l) atomicAdd(&cnt32[l], 1u);
    }
    __syncthreads();
    if (lane < 16) cnt[lane] = (uint16_t)cnt32[lane];
    __syncthreads();
    if (!inf_check_set(cnt, kind)) return false;                       // (the same answer in every lane)
    if (lane == 0) {
      uint32_t idx = 0, code = 0;
      bidx[0] = 0; bcode[0] = 0; run[0] = 0;
      for (uint32_t l = 1; l < 16; ++l) {
        code = (code + cnt[l - 1]) << 1;
        idx += cnt[l - 1];
        bidx[l] = (uint16_t)idx; bcode[l] = (uint16_t)code; run[l] = 0;
      }
    }
    __syncthreads();
    for (uint32_t base = 0; base < n; base += kLanes) {
      const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
      uint64_t same = __ballot(l != 0);                                // the lanes whose symbol has this lane's length
      for (uint32_t b = 0; b < 4; ++b) {
        const uint64_t bal = __ballot((l >> b) & 1);
        same &= ((l >> b) & 1) ? bal : ~bal;
      }
      const uint32_t r = run[l] + (uint32_t)__popcll(same & ((1ull << lane) - 1));
      __syncthreads();
      if (l) {
        sym[bidx[l] + r] = (uint16_t)s;
        if (l <= tbits)
          for (uint32_t k = gz_rev(bcode[l] + r, l); k < (1u << tbits); k += 1u << l) tab[k] = inf_entry(s, l);
        if (((same >> lane) >> 1) == 0) run[l] = (uint16_t)(r + 1);    // the highest lane of its length
      }
      __syncthreads();
    }
    return true;
  }
  __device__ void flush() {
    if (nlit) {
      if (lane < nlit) out[lit_at + lane] = (uint8_t)lit;
      nlit = 0;
    }
  }
  __device__ void literal(uint32_t at, uint32_t byte) {
    if (nlit == 0) lit_at = at;
    if (lane == nlit) lit = byte;
    if (++nlit == kLanes) flush();
  }
  __device__ void copy_stored(uint32_t src, uint32_t at, uint32_t n) {
    flush();
    for (uint32_t i = lane; i < n; i += kLanes) out[at + i] = in[src + i];
  }
  __device__ void copy_match(uint32_t at, uint32_t dist, uint32_t n) {
    flush();
    if (at - dist + min(n, dist) > fenced) { __syncthreads(); fenced = at; }
    const uint8_t *src = out + (at - dist);
    for (uint32_t i = lane; i < n; i += kLanes) out[at + i] = src[i < dist ? i : i % dist];
  }
};

__global__ __launch_bounds__(kLanes) void k_bgzf_inflate(const uint8_t *members, const InfMember *table, const uint64_t *text_off, uint64_t n_members,
                                                         uint8_t *text, uint8_t *status, const uint32_t *crc_adv) {
  __shared__ uint16_t s_ltab[1u << kInfLitBits], s_dtab[1u << kInfDistBits], s_ctab[1u << kInfClBits];
  __shared__ uint16_t s_lsym[kInfLitSyms], s_dsym[kInfDistSyms], s_csym[kGzClSyms + 1];
  __shared__ uint16_t s_cnt[3 * 16], s_rank[3 * 16];
  __shared__ uint32_t s_cnt32[16], s_crc[256];
  __shared__ uint8_t s_lens[kInfLitSyms + kInfDistSyms], s_cllen[kGzClSyms + 1];
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = lane; i < 256; i += kLanes) s_crc[i] = gz_crc_entry(i);
  __syncthreads();
  const InfWork w{s_ltab, s_dtab, s_ctab, s_lsym, s_dsym, s_csym, s_cnt, s_cnt + 16, s_cnt + 32, s_lens, s_cllen};
  for (uint64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
    if (status[m]) continue;                                           // refused by its framing: it owns no text
    const InfMember mem = table[m];
    const uint32_t n_in = mem.size - mem.head - kGzTrailer, n = mem.isize;
    uint8_t *out = text + text_off[m];
    DevMachine machine{members + mem.off + mem.head, n_in, out, lane, s_cnt32, s_rank, s_rank + 16, s_rank + 32, 0, 0, 0, 0, 0, 0};
    machine.load_window(0);
    int32_t st = inf_member(machine, w, n_in * 8, n);
    __syncthreads();                                                   // every store of the text has left the wave
    if (st == CFR_INF_OK) {
      // CRC32: lane l owns the slice that ends l * kGzCrcSlice bytes in front of the text's end
      uint32_t crc = 0;
      const uint32_t back = lane * kGzCrcSlice;
      if (back < n) {
        const uint32_t hi = n - back, lo = hi > kGzCrcSlice ? hi - kGzCrcSlice : 0;
        if (lo == 0) crc = 0xffffffffu;
        for (uint32_t i = lo; i < hi; ++i) crc = gz_crc_byte(s_crc, crc, out[i]);
      }
      for (uint32_t k = 0; k < kGzCrcLevels; ++k) {
        const uint32_t other = __shfl_down(crc, 1u << k, kLanes);
        if ((lane & ((2u << k) - 1)) == 0 && lane + (1u << k) < kLanes) crc ^= gz_gf2_times(crc_adv + 32 * k, other);
      }
      crc = __shfl(crc, 0, kLanes);
      if (n == 0) crc = 0xffffffffu;                                   // (no lane had a slice)
      if ((crc ^ 0xffffffffu) != mem.crc) st = CFR_INF_BAD_CRC;
    }
    if (st != CFR_INF_OK) {
      for (uint32_t i = lane; i < n; i += kLanes) out[i] = 0;
      if (lane == 0) status[m] = (uint8_t)st;
    }
    __syncthreads();                                                   // the next member of this workgroup uses the same LDS
  }
}

template <class T> void grow(DevBuf<T> &b, size_t &cap, size_t need) {      // by doubling; the old contents are not kept
  if (need <= cap) return;
  const size_t c = std::max(need, cap * 2);
  cap = 0;
  b.alloc(c);
  cap = c;
}

class InflateDevice : public Inflate {
 public:
  explicit InflateDevice(int device) : device_(device) {
    if (!device_exists(device)) throw HipError{"cfr_inflate_open: no HIP device " + std::to_string(device), -1};
    DeviceScope scope(device);
    stream_.create();
    for (auto &e : ev_) e.create();
    uint32_t adv[32 * kGzCrcLevels];
    gz_crc_advance_tables(adv);
    d_adv_.alloc(32 * kGzCrcLevels);
    int cus = 0, per_cu = 0;                               // as many workgroups as the device holds at once; they stride over the members
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bgzf_inflate, kLanes, 0));
    resident_ = (unsigned)std::max(cus, 1) * (unsigned)std::max(per_cu, 1);
    HIP_CHECK(hipMemcpyAsync(d_adv_, adv, sizeof(adv), hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }
  ~InflateDevice() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }

  void inflate(const uint8_t *members, uint64_t n, int fetch_text, const uint8_t **text, uint64_t *text_n, cfr_inflate_info *info) override {
    if (!text || !text_n || !info) throw std::invalid_argument("cfr_inflate_bgzf: null argument");
    text_n_ = 0;
    st_ = cfr_inflate_stats{};
    inf_walk(members, n, members_, text_off_, status_);                // throws before anything is launched
    const uint64_t total = text_off_.back(), count = members_.size();
    *text = nullptr;
    *text_n = total;
    if (count) {
      DeviceScope scope(device_);
      grow(d_in_, cap_in_, n);
      grow(d_table_, cap_table_, count);
      grow(d_off_, cap_off_, 2 * (count + 1));
      if ((uint64_t)count + 1 > (uint64_t)INT_MAX) throw std::invalid_argument("cfr_inflate_bgzf: more than 2^31 - 2 members in one call: hand over less");
      sizes_.resize(count + 1);                                        // the members' text sizes and the zero the scan ends on
      for (uint64_t m = 0; m <= count; ++m) sizes_[m] = m < count ? text_off_[m + 1] - text_off_[m] : 0;
      uint64_t *d_sizes = d_off_, *d_off = d_sizes + (count + 1);
      grow(d_status_, cap_status_, count);
      grow(d_text_, cap_text_, std::max<uint64_t>(total, 1));
      if (count > cap_hstatus_) { cap_hstatus_ = 0; h_status_.alloc(count * 2); cap_hstatus_ = count * 2; }
      HIP_CHECK(hipEventRecord(ev_[0], stream_));
      HIP_CHECK(hipMemcpyAsync(d_in_, members, n, hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipMemcpyAsync(d_table_, members_.data(), count * sizeof(InfMember), hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipMemcpyAsync(d_sizes, sizes_.data(), (count + 1) * 8, hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipMemcpyAsync(d_status_, status_.data(), count, hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipEventRecord(ev_[1], stream_));
      {
        size_t need = 0;
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, d_sizes, d_off, (int)(count + 1), stream_));
        grow(tmp_, cap_tmp_, need);
        need = cap_tmp_;
        HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp_.get(), need, d_sizes, d_off, (int)(count + 1), stream_));
      }
      const unsigned grid = (unsigned)std::min<uint64_t>(count, resident_);
      hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(kLanes), 0, stream_, (const uint8_t *)d_in_.get(), (const InfMember *)d_table_.get(),
                         (const uint64_t *)d_off, count, d_text_.get(), d_status_.get(), (const uint32_t *)d_adv_.get());
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(ev_[2], stream_));
      HIP_CHECK(hipMemcpyAsync(h_status_.get(), d_status_, count, hipMemcpyDeviceToHost, stream_));
      if (fetch_text && total) {
        if (total > cap_htext_) {
          const size_t c = std::max<size_t>(total, cap_htext_ * 2);
          cap_htext_ = 0;
          h_text_.alloc(c);
          cap_htext_ = c;
        }
        HIP_CHECK(hipMemcpyAsync(h_text_.get(), d_text_, total, hipMemcpyDeviceToHost, stream_));
      }
      HIP_CHECK(hipEventRecord(ev_[3], stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
      memcpy(status_.data(), h_status_.get(), count);
      (void)hipEventElapsedTime(&st_.upload_ms, ev_[0], ev_[1]);
      (void)hipEventElapsedTime(&st_.inflate_ms, ev_[1], ev_[2]);
      (void)hipEventElapsedTime(&st_.download_ms, ev_[2], ev_[3]);
    }
    if (fetch_text) {
      if (!h_text_) { h_text_.alloc(16); cap_htext_ = 16; }
      *text = h_text_.get();
    }
    text_n_ = total;
    inf_fill_info(status_, n, total, info);
  }

  bool member_status(uint8_t *status, uint64_t *text_off, uint64_t cap) const override {
    if (status_.size() > cap) return false;
    if (status && !status_.empty()) memcpy(status, status_.data(), status_.size());
    if (text_off) {
      if (text_off_.empty()) text_off[0] = 0;
      else memcpy(text_off, text_off_.data(), text_off_.size() * 8);
    }
    return true;
  }

  bool device_text(const void **d_text, uint64_t *n) override {
    if (d_text) *d_text = d_text_.get();
    if (n) *n = text_n_;
    return true;
  }

  void stats(cfr_inflate_stats *st) const override { *st = st_; }

 private:
  int device_;
  unsigned resident_ = 1;
  Stream stream_;                  // first: the last to go
  Event ev_[4];                    // start, uploaded, inflated, downloaded
  DevBuf<uint8_t> d_in_, d_text_, d_status_, tmp_;
  DevBuf<InfMember> d_table_;
  DevBuf<uint64_t> d_off_;
  DevBuf<uint32_t> d_adv_;
  PinnedBuf<uint8_t> h_status_, h_text_;
  size_t cap_in_ = 0, cap_text_ = 0, cap_status_ = 0, cap_table_ = 0, cap_off_ = 0, cap_hstatus_ = 0, cap_htext_ = 0, cap_tmp_ = 0;
  std::vector<InfMember> members_;
  std::vector<uint64_t> text_off_, sizes_;
  std::vector<uint8_t> status_;
  uint64_t text_n_ = 0;
  cfr_inflate_stats st_{};
};

}  // namespace

Inflate *make_inflate_device(int device) { return new InflateDevice(device); }

}  // namespace cfr
