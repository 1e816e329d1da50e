// cfr_gz.hip — a text in HBM cut into BGZF members, and the records of a read dump made there (gfx950).  What the bytes are:
// cfr_gz_core.hpp; the host twin: cfr_gz.cpp.
//
//   k_dump_len     one lane per read, grid-stride: the bytes of the read's record in one file (0: not selected, or dropped); the lane
//                  behind the last read writes the zero the scan ends on.
//   (hipcub::DeviceScan::ExclusiveSum: the records' offsets; the total goes to the host, which sizes the text.)
//   k_dump_write   one wave per read, the waves stride: the lanes write the record's bytes 64 at a time (gz_record_byte), coalesced.
//   k_gz_deflate   one wave (a workgroup of 64) per block of the text, the workgroups stride.  LDS: the hash table (2^12 words), 64 words
//                  of output bits, the CRC table: 17.25 KiB, 9 workgroups per CU.  The input stays in HBM / L2.  Per window of 64
//                  positions: lookup, barrier, insert by atomic maximum, the choice of tokens as a scalar walk over the window (the
//                  lengths by readlane), the tokens' bit counts prefix-summed over the wave, the bits ORed into the LDS words, the full
//                  words stored to the block's slot.  The slot's stream begins on a 4-byte boundary.  gz_must_store is asked before a
//                  window's words leave: a stored block is then copied over the slot instead.  CRC32: a slice per lane, joined in 6
//                  rounds with the advance matrices.  Lane 0 writes header, trailer and the member's size.
//   k_gzd_encode   dynamic mode's stand-in for k_gz_deflate (described in front of it): tokens to HBM and histograms, the block's codes
//                  built by lane 0, the tokens written in those codes.
//   (ExclusiveSum over the sizes: where each member goes.)
//   k_gz_pack      one workgroup of 256 per member: slot -> packed output.
// Every table entry is checked by gz_match_len before a byte is read at it; nothing outside [block start, block end) is read.  No lane
// keeps an array: no scratch.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstring>
#include <stdexcept>

#include "cfr_hip_util.hpp"
#include "cfr_gz.hpp"

namespace cfr {

namespace {

constexpr int kLanes = 64;
constexpr int kBlock = 256;
constexpr uint32_t kTableSize = 1u << kGzHashBits;

struct DumpIds { const char *bytes; const uint64_t *off; const uint8_t *select; };

__global__ __launch_bounds__(kBlock) void k_dump_len(GzFileView f, DumpIds ids, uint64_t n, uint64_t *len) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kBlock)
    len[i] = i == n ? 0 : gz_record_len(f, ids.off, ids.select, i);
}

__global__ __launch_bounds__(kBlock) void k_dump_write(GzFileView f, DumpIds ids, uint64_t n, const uint64_t *off, uint8_t *text) {
  const uint32_t lane = threadIdx.x & (kLanes - 1);
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kLanes);
  for (uint64_t i = (uint64_t)blockIdx.x * (kBlock / kLanes) + threadIdx.x / kLanes; i < n; i += waves) {
    const uint64_t at = off[i], len = off[i + 1] - at;          // (below kGzRecordLimit)
    for (uint64_t j = lane; j < len; j += kLanes) text[at + j] = gz_record_byte(f, ids.bytes, ids.off, i, j);
  }
}

__global__ __launch_bounds__(kLanes) void k_gz_deflate(const uint8_t *text, uint64_t n_text, uint32_t block_bytes, uint64_t n_blocks, uint32_t stride,
                                                       uint8_t *slots, uint64_t *sizes, const uint32_t *crc_adv, unsigned long long *stored_blocks) {
  __shared__ uint32_t s_table[kTableSize];
  __shared__ uint32_t s_out[kLanes];
  __shared__ uint32_t s_crc[256];
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = lane; i < 256; i += kLanes) s_crc[i] = gz_crc_entry(i);
  if (blockIdx.x == 0 && lane == 0) sizes[n_blocks] = 0;          // the zero the scan ends on
  for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const uint8_t *in = text + b * block_bytes;
    const uint32_t n = (uint32_t)min((uint64_t)block_bytes, n_text - b * block_bytes);
    uint8_t *member = slots + b * stride + 2, *def = member + kGzHeader;
    uint32_t *def32 = reinterpret_cast<uint32_t *>(def);          // (slots and stride are multiples of 16: def is 4-aligned)
    for (uint32_t i = lane; i < kTableSize; i += kLanes) s_table[i] = 0;
    s_out[lane] = lane == 0 ? 3u : 0u;
    __syncthreads();
    uint32_t bitpos = kGzFirstBits, word_base = 0, next_free = 0;
    bool stored = false;
    for (uint32_t base = 0; base < n; base += kGzWindow) {
      const uint32_t p = base + lane;
      const bool can = p + 4 <= n;
      uint32_t mlen = 0, dist = 0, h = 0;
      if (can) {
        h = gz_hash(gz_load32(in + p));
        mlen = gz_match_len(in, n, p, s_table[h], dist);
      }
      __syncthreads();
      if (can) atomicMax(&s_table[h], p + 1);
      // the tokens' first positions: a walk every lane makes alike
      const uint32_t end = min(base + kGzWindow, n);
      uint64_t starts = 0;
      uint32_t pos = max(next_free, base);
      while (pos < end) {
        const uint32_t k = __builtin_amdgcn_readfirstlane(pos - base);
        starts |= 1ull << k;
        const uint32_t l = __builtin_amdgcn_readlane(mlen, k);
        pos += l ? l : 1;
      }
      next_free = pos;
      const bool tok = p < n && ((starts >> lane) & 1);
      uint64_t bits = 0;
      uint32_t nb = 0;
      if (tok) nb = mlen ? gz_match(mlen, dist, bits) : gz_literal(in[p], bits);
      uint32_t incl = nb;
      for (int d = 1; d < kLanes; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, kLanes);
        if ((int)lane >= d) incl += up;
      }
      const uint32_t total = __shfl(incl, kLanes - 1, kLanes);
      const uint32_t new_bitpos = bitpos + total;
      if (gz_must_store(new_bitpos, n)) { stored = true; break; }       // (the same answer in every lane)
      if (tok) {
        const uint32_t rel = bitpos + (incl - nb) - word_base * 32;     // at most 31 + 63 * 31 + ...: word 62 and its neighbour
        const uint64_t v = bits << (rel & 31);
        atomicOr(&s_out[rel >> 5], (uint32_t)v);
        if (v >> 32) atomicOr(&s_out[(rel >> 5) + 1], (uint32_t)(v >> 32));
      }
      __syncthreads();
      const uint32_t full = (new_bitpos >> 5) - word_base;              // whole words: below 64
      const uint32_t mine = s_out[lane], carry = s_out[full & (kLanes - 1)];
      __syncthreads();
      if (lane < full) def32[word_base + lane] = mine;
      s_out[lane] = lane == 0 ? carry : 0u;
      word_base += full;
      bitpos = new_bitpos;
      __syncthreads();
    }
    uint32_t def_bytes;
    if (stored) {
      def_bytes = kGzStoredHead + n;
      if (lane == 0) { gz_put_stored_head(def, n); atomicAdd(stored_blocks, 1ull); }
      for (uint32_t i = lane; i < n; i += kLanes) def[kGzStoredHead + i] = in[i];
    } else {
      bitpos += kGzEndBits;                                             // seven zero bits: nothing to OR in
      def_bytes = (bitpos + 7) >> 3;
      const uint32_t left = def_bytes - word_base * 4;                  // at most 8
      if (lane < left) def[word_base * 4 + lane] = (uint8_t)(s_out[lane >> 2] >> (8 * (lane & 3)));
    }
    // CRC32: lane l owns the slice that ends l * kGzCrcSlice bytes in front of the block's end
    uint32_t crc = 0;
    {
      const uint32_t back = lane * kGzCrcSlice;
      if (back < n) {
        const uint32_t hi = n - back, lo = hi > kGzCrcSlice ? hi - kGzCrcSlice : 0;
        if (lo == 0) crc = 0xffffffffu;
        for (uint32_t i = lo; i < hi; ++i) crc = gz_crc_byte(s_crc, crc, in[i]);
      }
      for (uint32_t k = 0; k < kGzCrcLevels; ++k) {
        const uint32_t other = __shfl_down(crc, 1u << k, kLanes);
        if ((lane & ((2u << k) - 1)) == 0 && lane + (1u << k) < kLanes) crc ^= gz_gf2_times(crc_adv + 32 * k, other);
      }
    }
    if (lane == 0) {
      const uint32_t member_bytes = kGzHeader + def_bytes + kGzTrailer;
      gz_put_header(member, member_bytes);
      gz_put_trailer(def + def_bytes, crc ^ 0xffffffffu, n);
      sizes[b] = member_bytes;
    }
    __syncthreads();                                                    // the next block of this workgroup uses the same LDS
  }
}

// Dynamic mode (cfr_gz_options.codes = 1): one wave per block, the workgroups stride; the block's tokens wait in the workgroup's own
// area of HBM (block_bytes words at blockIdx.x * block_bytes: a block has at most one token per byte) until its codes are known.
//   pass A   k_gz_deflate's window loop without the emission: every token goes to the area as one word and into the histograms in LDS.
//   build    lane 0 alone runs gz_dyn_build and gz_choose on the LDS arrays and, for a dynamic stream, writes the header into the slot
//            with whole words; the bits of the last, unfinished word go on in the staging.  (Serial on purpose: the other
//            workgroups of the CU run meanwhile; measured in DESIGN.md, section 4j.)
//   pass B   64 tokens at a time, one per lane, the end-of-block symbol behind the last: codes from the LDS tables (the block's own, or
//            the fixed code in the same form: then the bytes are those of k_gz_deflate), prefix sum, OR into the staging, whole words out.
//            A token has at most 15 + 5 + 15 + 13 = 48 bits and starts at most 31 + 63 * 48 = 3055 bits into the staging: shifted by up to
//            31 it spans 79 bits, three words, the last of them word 97 at most; 64 tokens and the 31 bits in front of them fill at most
//            96 whole words, and the word carried over is word 96 at most: kStageWords = 128, two words per lane.
//   A stored block is the copy of the input.  CRC32, header, trailer and size as in k_gz_deflate.
// Histograms, tables, hash table and staging are reset for every block a workgroup takes.  A stream that is not stored is shorter than
// 5 + n bytes (gz_choose): nothing is written outside the slot.  LDS: the 17.25 KiB of k_gz_deflate + 5 KiB (22 756 bytes): seven workgroups per CU.
constexpr uint32_t kStageWords = 128;

__global__ __launch_bounds__(kLanes) void k_gzd_encode(const uint8_t *text, uint64_t n_text, uint32_t block_bytes, uint64_t n_blocks, uint32_t stride,
                                                       uint8_t *slots, uint64_t *sizes, const uint32_t *crc_adv, uint32_t *token_area,
                                                       unsigned long long *kinds) {
  __shared__ uint32_t s_table[kTableSize];
  __shared__ uint32_t s_crc[256];
  __shared__ uint32_t s_out[kStageWords];
  __shared__ uint32_t s_lfreq[kGzLitSyms], s_dfreq[kGzDistSyms], s_ltab[kGzLitSyms], s_dtab[kGzDistSyms], s_clfreq[kGzClSyms], s_cltab[kGzClSyms], s_w32[kGzLitSyms];
  __shared__ uint16_t s_w16[kGzLitSyms], s_cnt[16];
  __shared__ uint8_t s_lens[kGzLitSyms + kGzDistSyms], s_cllen[kGzClSyms];
  __shared__ uint32_t s_start[4];                                   // the choice; the stream's bits, whole words and unfinished word behind the header
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = lane; i < 256; i += kLanes) s_crc[i] = gz_crc_entry(i);
  if (blockIdx.x == 0 && lane == 0) sizes[n_blocks] = 0;          // the zero the scan ends on
  uint32_t *tokens = token_area + (uint64_t)blockIdx.x * block_bytes;
  for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const uint8_t *in = text + b * block_bytes;
    const uint32_t n = (uint32_t)min((uint64_t)block_bytes, n_text - b * block_bytes);
    uint8_t *member = slots + b * stride + 2, *def = member + kGzHeader;
    uint32_t *def32 = reinterpret_cast<uint32_t *>(def);          // (slots and stride are multiples of 16: def is 4-aligned)
    for (uint32_t i = lane; i < kTableSize; i += kLanes) s_table[i] = 0;
    for (uint32_t i = lane; i < kGzLitSyms; i += kLanes) s_lfreq[i] = i == kGzEob ? 1u : 0u;
    if (lane < kGzDistSyms) s_dfreq[lane] = 0;
    __syncthreads();
    // ---- pass A
    uint32_t n_tok = 0, next_free = 0;
    for (uint32_t base = 0; base < n; base += kGzWindow) {
      const uint32_t p = base + lane;
      const bool can = p + 4 <= n;
      uint32_t mlen = 0, dist = 0, h = 0;
      if (can) {
        h = gz_hash(gz_load32(in + p));
        mlen = gz_match_len(in, n, p, s_table[h], dist);
      }
      __syncthreads();
      if (can) atomicMax(&s_table[h], p + 1);
      const uint32_t end = min(base + kGzWindow, n);
      uint64_t starts = 0;
      uint32_t pos = max(next_free, base);
      while (pos < end) {
        const uint32_t k = __builtin_amdgcn_readfirstlane(pos - base);
        starts |= 1ull << k;
        const uint32_t l = __builtin_amdgcn_readlane(mlen, k);
        pos += l ? l : 1;
      }
      next_free = pos;
      if (p < n && ((starts >> lane) & 1)) {
        const uint32_t at = n_tok + (uint32_t)__popcll(starts & ((1ull << lane) - 1));     // below n: a token covers a byte at least
        if (mlen) {
          uint32_t eb, ev;
          atomicAdd(&s_lfreq[gz_len_symbol(mlen, eb, ev)], 1u);
          atomicAdd(&s_dfreq[gz_dist_symbol(dist, eb, ev)], 1u);
          tokens[at] = gz_token_match(mlen, dist);
        } else {
          const uint32_t byte = in[p];
          atomicAdd(&s_lfreq[byte], 1u);
          tokens[at] = byte;
        }
      }
      n_tok += (uint32_t)__popcll(starts);
      __syncthreads();                                                  // the next window reads the table behind these insertions
    }
    // ---- the codes, the choice, the header
    if (lane == 0) {
      const GzDynWork w{s_lfreq, s_dfreq, s_ltab, s_dtab, s_clfreq, s_cltab, s_lens, s_cllen, s_w32, s_w16, s_cnt};
      const GzDynPlan plan = gz_dyn_build(w);
      const uint32_t kind = gz_choose(n, plan);
      s_start[0] = kind;
      s_start[1] = kGzFirstBits; s_start[2] = 0; s_start[3] = 3;        // a fixed stream: BFINAL = 1, BTYPE = 01
      if (kind == 2) {
        GzWordSink sink{def, 0, 0};
        gz_put_dyn_header(sink, w, plan);
        s_start[2] = (uint32_t)(sink.p - def) >> 2;
        s_start[1] = s_start[2] * 32 + sink.have;
        s_start[3] = (uint32_t)sink.acc;
      }
      if (kind != 1) atomicAdd(&kinds[kind ? 1 : 0], 1ull);
    }
    __syncthreads();
    const uint32_t kind = s_start[0];
    uint32_t def_bytes;
    if (kind == 0) {
      def_bytes = kGzStoredHead + n;
      if (lane == 0) gz_put_stored_head(def, n);
      for (uint32_t i = lane; i < n; i += kLanes) def[kGzStoredHead + i] = in[i];
    } else {
      // ---- pass B
      if (kind == 1) {
        for (uint32_t i = lane; i < kGzLitSyms; i += kLanes) s_ltab[i] = gz_fixed_entry(i);
        if (lane < kGzDistSyms) s_dtab[lane] = gz_fixed_dist_entry(lane);
      }
      uint32_t bitpos = s_start[1], word_base = s_start[2];
      s_out[lane] = lane == 0 ? s_start[3] : 0u;
      s_out[lane + kLanes] = 0;
      __syncthreads();
      for (uint32_t t0 = 0; t0 <= n_tok; t0 += kLanes) {
        const uint32_t t = t0 + lane;
        uint64_t bits = 0;
        uint32_t nb = 0;
        if (t <= n_tok) nb = gz_token_bits(t < n_tok ? tokens[t] : kGzEob, s_ltab, s_dtab, bits);
        uint32_t incl = nb;
        for (int d = 1; d < kLanes; d <<= 1) {
          const uint32_t up = __shfl_up(incl, d, kLanes);
          if ((int)lane >= d) incl += up;
        }
        const uint32_t new_bitpos = bitpos + __shfl(incl, kLanes - 1, kLanes);
        if (nb) {
          const uint32_t rel = bitpos + (incl - nb) - word_base * 32, sh = rel & 31, word = rel >> 5;
          const uint64_t lo = bits << sh;                                // bits is below 2^48: what falls off the top is hi
          const uint32_t hi = sh > 16 ? (uint32_t)(bits >> (64 - sh)) : 0u;
          atomicOr(&s_out[word], (uint32_t)lo);
          if (lo >> 32) atomicOr(&s_out[word + 1], (uint32_t)(lo >> 32));
          if (hi) atomicOr(&s_out[word + 2], hi);
        }
        __syncthreads();
        const uint32_t full = (new_bitpos >> 5) - word_base;             // whole words: 96 at most
        const uint32_t mine = s_out[lane], mine2 = s_out[lane + kLanes], carry = s_out[full];
        __syncthreads();
        if (lane < full) def32[word_base + lane] = mine;
        if (lane + kLanes < full) def32[word_base + lane + kLanes] = mine2;
        s_out[lane] = lane == 0 ? carry : 0u;
        s_out[lane + kLanes] = 0;
        word_base += full;
        bitpos = new_bitpos;
        __syncthreads();
      }
      def_bytes = (bitpos + 7) >> 3;
      const uint32_t left = def_bytes - word_base * 4;                  // at most 4
      if (lane < left) def[word_base * 4 + lane] = (uint8_t)(s_out[0] >> (8 * lane));
    }
    // CRC32: lane l owns the slice that ends l * kGzCrcSlice bytes in front of the block's end
    uint32_t crc = 0;
    {
      const uint32_t back = lane * kGzCrcSlice;
      if (back < n) {
        const uint32_t hi = n - back, lo = hi > kGzCrcSlice ? hi - kGzCrcSlice : 0;
        if (lo == 0) crc = 0xffffffffu;
        for (uint32_t i = lo; i < hi; ++i) crc = gz_crc_byte(s_crc, crc, in[i]);
      }
      for (uint32_t k = 0; k < kGzCrcLevels; ++k) {
        const uint32_t other = __shfl_down(crc, 1u << k, kLanes);
        if ((lane & ((2u << k) - 1)) == 0 && lane + (1u << k) < kLanes) crc ^= gz_gf2_times(crc_adv + 32 * k, other);
      }
    }
    if (lane == 0) {
      const uint32_t member_bytes = kGzHeader + def_bytes + kGzTrailer;
      gz_put_header(member, member_bytes);
      gz_put_trailer(def + def_bytes, crc ^ 0xffffffffu, n);
      sizes[b] = member_bytes;
    }
    __syncthreads();                                                    // the next block of this workgroup uses the same LDS and tokens
  }
}

__global__ __launch_bounds__(kBlock) void k_gz_pack(const uint8_t *slots, uint32_t stride, const uint64_t *off, uint64_t n_blocks, uint8_t *out) {
  for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const uint8_t *src = slots + b * stride + 2;
    uint8_t *dst = out + off[b];
    const uint32_t len = (uint32_t)(off[b + 1] - off[b]);
    for (uint32_t i = threadIdx.x; i < len; i += kBlock) dst[i] = src[i];
  }
}

template <class T> void grow(DevBuf<T> &b, size_t &cap, size_t need) {      // by doubling; the old contents are not kept
  if (need <= cap) return;
  const size_t c = std::max(need, cap * 2);
  cap = 0;
  b.alloc(c);
  cap = c;
}

class GzDevice : public Gz {
 public:
  GzDevice(int device, const cfr_gz_options &o) : device_(device), block_(gz_block_bytes(o)), stride_(gz_slot_stride(block_)), dynamic_(gz_dynamic(o)) {
    if (!device_exists(device)) throw HipError{"cfr_gz_open: no HIP device " + std::to_string(device), -1};
    max_blocks_ = o.max_blocks > 0 ? (unsigned)o.max_blocks : 0u;
    DeviceScope scope(device);
    stream_.create();
    for (auto &e : ev_) e.create();
    uint32_t adv[32 * kGzCrcLevels];
    gz_crc_advance_tables(adv);
    d_adv_.alloc(32 * kGzCrcLevels);
    d_kinds_.alloc(2);
    h_back_.alloc(3);
    if (dynamic_) {                                        // as many workgroups as the device holds at once: each owns a token area
      int cus = 0, per_cu = 0;
      HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
      HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_gzd_encode, kLanes, 0));
      resident_ = (unsigned)std::max(cus, 1) * (unsigned)std::max(per_cu, 1);
    }
    HIP_CHECK(hipMemcpyAsync(d_adv_, adv, sizeof(adv), hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }
  ~GzDevice() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }

  void compress(const uint8_t *text, uint64_t n, const uint8_t **out, uint64_t *out_n) override {
    if (!out || !out_n || (n && !text)) throw std::invalid_argument("cfr_gz_compress: null argument");
    DeviceScope scope(device_);
    st_ = cfr_gz_stats{};
    grow(d_text_, cap_text_, std::max<uint64_t>(n, 1));
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    if (n) HIP_CHECK(hipMemcpyAsync(d_text_, text, n, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipEventRecord(ev_[1], stream_));
    HIP_CHECK(hipEventRecord(ev_[2], stream_));
    deflate(n, 0);
    add_time(st_.upload_ms, 0, 1);
    *out = h_out_[0].get();
    *out_n = out_n_[0];
  }

  void dump(const char *id_bytes, const uint64_t *id_off, const uint8_t *select, size_t n, const cfr_gz_file *files, int n_files,
            const uint8_t **out, uint64_t *out_n) override {
    gz_check_dump(id_bytes, id_off, select, n, files, n_files, out, out_n);
    if ((uint64_t)n + 1 > (uint64_t)INT_MAX) throw std::invalid_argument("cfr_gz_dump: more than 2^31 - 2 reads in one call: hand over less");
    DeviceScope scope(device_);
    st_ = cfr_gz_stats{};
    // the ids and the selector serve every file
    const uint64_t id_base = id_off[0], id_total = id_off[n] - id_base;
    grow(d_id_off_, cap_id_off_, n + 1);
    grow(d_id_, cap_id_, std::max<uint64_t>(id_off[n], 1));
    grow(d_select_, cap_select_, std::max<size_t>(n, 1));
    grow(d_len_, cap_len_, 2 * (n + 1));
    HIP_CHECK(hipEventRecord(ev_[0], stream_));
    HIP_CHECK(hipMemcpyAsync(d_id_off_, id_off, (n + 1) * 8, hipMemcpyHostToDevice, stream_));
    if (id_total) HIP_CHECK(hipMemcpyAsync(d_id_.get() + id_base, id_bytes + id_base, id_total, hipMemcpyHostToDevice, stream_));
    if (n) HIP_CHECK(hipMemcpyAsync(d_select_, select, n, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipEventRecord(ev_[1], stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    add_time(st_.upload_ms, 0, 1);
    const DumpIds ids{d_id_, d_id_off_, d_select_};
    for (int f = 0; f < n_files; ++f) {
      HIP_CHECK(hipEventRecord(ev_[0], stream_));
      GzFileView v{};
      v.seq = up(d_seq_, cap_seq_, files[f].seq, files[f].seq_off, n);
      v.seq_off = up_off(d_seq_off_, cap_seq_off_, files[f].seq_off, n);
      if (files[f].qual) {
        v.qual = (const char *)up(d_qual_, cap_qual_, (const uint8_t *)files[f].qual, files[f].qual_off, n);
        v.qual_off = up_off(d_qual_off_, cap_qual_off_, files[f].qual_off, n);
        grow(d_hasq_, cap_hasq_, std::max<size_t>(n, 1));
        if (n) HIP_CHECK(hipMemcpyAsync(d_hasq_, files[f].has_qual, n, hipMemcpyHostToDevice, stream_));
        v.has_qual = d_hasq_;
      }
      HIP_CHECK(hipEventRecord(ev_[1], stream_));
      uint64_t *d_len = d_len_, *d_off = d_len + (n + 1);
      const unsigned want = grid_for(n + 1, kBlock);
      hipLaunchKernelGGL(k_dump_len, dim3(cap_grid(want)), dim3(kBlock), 0, stream_, v, ids, (uint64_t)n, d_len);
      HIP_CHECK(hipGetLastError());
      scan(d_len, d_off, n + 1);
      HIP_CHECK(hipMemcpyAsync(h_back_.get(), d_off + n, 8, hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
      const uint64_t total = h_back_.get()[0];
      grow(d_text_, cap_text_, std::max<uint64_t>(total, 1));
      if (n && total) {
        const unsigned blocks = grid_for(n, kBlock / kLanes);
        hipLaunchKernelGGL(k_dump_write, dim3(cap_grid(std::min(blocks, 65536u))), dim3(kBlock), 0, stream_, v, ids, (uint64_t)n, d_off, d_text_.get());
        HIP_CHECK(hipGetLastError());
      }
      HIP_CHECK(hipEventRecord(ev_[2], stream_));
      deflate(total, f);
      add_time(st_.upload_ms, 0, 1);
      add_time(st_.format_ms, 1, 2);
      out[f] = h_out_[f].get();
      out_n[f] = out_n_[f];
    }
  }

  void stats(cfr_gz_stats *st) const override { *st = st_; }

 private:
  unsigned cap_grid(unsigned want) const { return std::max(1u, max_blocks_ ? std::min(want, max_blocks_) : want); }

  void add_time(float &sum, int a, int b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev_[a], ev_[b]) == hipSuccess) sum += ms;
  }

  // the bytes the offsets span, at the place the offsets name (so that the offsets go up as they are)
  const uint8_t *up(DevBuf<uint8_t> &d, size_t &cap, const uint8_t *bytes, const uint64_t *off, size_t n) {
    grow(d, cap, std::max<uint64_t>(off[n], 1));
    if (off[n] > off[0]) HIP_CHECK(hipMemcpyAsync(d.get() + off[0], bytes + off[0], off[n] - off[0], hipMemcpyHostToDevice, stream_));
    return d;
  }
  const uint64_t *up_off(DevBuf<uint64_t> &d, size_t &cap, const uint64_t *off, size_t n) {
    grow(d, cap, n + 1);
    HIP_CHECK(hipMemcpyAsync(d, off, (n + 1) * 8, hipMemcpyHostToDevice, stream_));
    return d;
  }

  void scan(const uint64_t *in, uint64_t *out, size_t count) {
    size_t need = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)count, stream_));
    grow(tmp_, cap_tmp_, need);
    need = cap_tmp_;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp_.get(), need, in, out, (int)count, stream_));
  }

  // d_text_[0, n) -> members in h_out_[slot]; ev_[2] was recorded in front
  void deflate(uint64_t n, int slot) {
    const uint64_t n_blocks = (n + block_ - 1) / block_;
    out_n_[slot] = 0;
    st_.bytes_in += n;
    if (!n_blocks) { if (!h_out_[slot]) { h_out_[slot].alloc(16); cap_out_[slot] = 16; } return; }
    if (n_blocks + 1 > (uint64_t)INT_MAX) throw std::invalid_argument("cfr_gz: more than 2^31 - 2 blocks in one call: hand over less");
    grow(d_slots_, cap_slots_, n_blocks * stride_);
    grow(d_sizes_, cap_sizes_, 2 * (n_blocks + 1));
    grow(d_packed_, cap_packed_, n_blocks * (uint64_t)(kGzHeader + kGzStoredHead + block_ + kGzTrailer));
    uint64_t *d_sizes = d_sizes_, *d_off = d_sizes + (n_blocks + 1);
    HIP_CHECK(hipMemsetAsync(d_kinds_, 0, 16, stream_));
    const unsigned grid = cap_grid((unsigned)std::min<uint64_t>(n_blocks, 1u << 20));
    if (dynamic_) {                                     // the token area: 4 * block_ bytes a workgroup - 256 CUs x 7 x 261 120 = 468 MB at the most
      const unsigned grid_dyn = cap_grid((unsigned)std::min<uint64_t>(n_blocks, resident_));
      grow(d_tokens_, cap_tokens_, (size_t)grid_dyn * block_);
      hipLaunchKernelGGL(k_gzd_encode, dim3(grid_dyn), dim3(kLanes), 0, stream_, (const uint8_t *)d_text_.get(), n, block_, n_blocks, stride_, d_slots_.get(), d_sizes,
                         (const uint32_t *)d_adv_.get(), d_tokens_.get(), d_kinds_.get());
    } else {
      hipLaunchKernelGGL(k_gz_deflate, dim3(grid), dim3(kLanes), 0, stream_, (const uint8_t *)d_text_.get(), n, block_, n_blocks, stride_, d_slots_.get(), d_sizes,
                         (const uint32_t *)d_adv_.get(), d_kinds_.get());
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev_[3], stream_));
    scan(d_sizes, d_off, n_blocks + 1);
    hipLaunchKernelGGL(k_gz_pack, dim3(grid), dim3(kBlock), 0, stream_, (const uint8_t *)d_slots_.get(), stride_, (const uint64_t *)d_off, n_blocks, d_packed_.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev_[4], stream_));
    HIP_CHECK(hipMemcpyAsync(h_back_.get(), d_off + n_blocks, 8, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(h_back_.get() + 1, d_kinds_, 16, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    const uint64_t total = h_back_.get()[0];
    if (total > cap_out_[slot]) {
      const size_t c = std::max<size_t>(total, cap_out_[slot] * 2);
      cap_out_[slot] = 0;
      h_out_[slot].alloc(c);
      cap_out_[slot] = c;
    }
    HIP_CHECK(hipMemcpyAsync(h_out_[slot].get(), d_packed_, total, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipEventRecord(ev_[5], stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    add_time(st_.deflate_ms, 2, 3);
    add_time(st_.pack_ms, 3, 4);
    add_time(st_.download_ms, 4, 5);
    out_n_[slot] = total;
    st_.blocks += n_blocks;
    st_.stored_blocks += h_back_.get()[1];
    st_.dynamic_blocks += (uint32_t)h_back_.get()[2];
    st_.bytes_out += total;
  }

  int device_;
  const uint32_t block_, stride_;
  const bool dynamic_;
  unsigned max_blocks_ = 0, resident_ = 1;
  Stream stream_;                  // first: the last to go
  Event ev_[6];                    // start, uploads done, text made, deflated, packed, downloaded
  DevBuf<uint8_t> d_text_, d_slots_, d_packed_, d_seq_, d_qual_, d_hasq_, d_select_, tmp_;
  DevBuf<char> d_id_;
  DevBuf<uint64_t> d_id_off_, d_seq_off_, d_qual_off_, d_len_, d_sizes_;
  DevBuf<uint32_t> d_adv_, d_tokens_;
  DevBuf<unsigned long long> d_kinds_;   // stored blocks, dynamic blocks
  PinnedBuf<uint64_t> h_back_;     // [0]: a total, [1]: stored blocks, [2]: dynamic blocks
  PinnedBuf<uint8_t> h_out_[kGzMaxFiles];
  size_t cap_out_[kGzMaxFiles] = {0, 0, 0, 0};
  uint64_t out_n_[kGzMaxFiles] = {0, 0, 0, 0};
  size_t cap_text_ = 0, cap_slots_ = 0, cap_packed_ = 0, cap_seq_ = 0, cap_qual_ = 0, cap_hasq_ = 0, cap_select_ = 0, cap_tmp_ = 0, cap_id_ = 0, cap_id_off_ = 0,
         cap_seq_off_ = 0, cap_qual_off_ = 0, cap_len_ = 0, cap_sizes_ = 0, cap_tokens_ = 0;
  cfr_gz_stats st_{};
};

}  // namespace

Gz *make_gz_device(int device, const cfr_gz_options &o) { return new GzDevice(device, o); }

}  // namespace cfr
