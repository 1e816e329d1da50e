// cfr_gz.cpp — the host twin of the device compressor (cfr_gz.hip) and the argument checks both share: the handle behind cfr_gz_*
// with device = -1 (semantics: cfr_gz_core.hpp).  Plain C++: no HIP header, so tools/gz_sanitize.cpp builds it alone.
//
// As on the device: every block is encoded into a slot of a fixed stride with its size beside it, then the members are packed back to
// back.  The blocks are spread over the threads by parallel_slices; a block's bytes do not depend on which thread made it.
#include "cfr_gz.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "cfr_threads.hpp"

namespace cfr {

uint32_t gz_block_bytes(const cfr_gz_options &o) {
  if (o.block_bytes < 0 || (uint32_t)o.block_bytes > kGzBlockMax) throw std::invalid_argument("cfr_gz_open: block_bytes is 0 (the default, 65280) or in [1, 65280]");
  if (o.max_blocks < 0 || o.threads < 0) throw std::invalid_argument("cfr_gz_open: an option below 0");
  return o.block_bytes ? (uint32_t)o.block_bytes : kGzBlockMax;
}

bool gz_dynamic(const cfr_gz_options &o) {
  if (o.codes != 0 && o.codes != 1) throw std::invalid_argument("cfr_gz_open: codes is 0 (fixed Huffman codes) or 1 (dynamic)");
  return o.codes == 1;
}

void gz_check_dump(const char *id_bytes, const uint64_t *id_off, const uint8_t *select, size_t n, const cfr_gz_file *files, int n_files,
                   const uint8_t *const *out, const uint64_t *out_n) {
  if (n_files < 1 || n_files > kGzMaxFiles) throw std::invalid_argument("cfr_gz_dump: n_files is 1 .. 4");
  if (!files || !out || !out_n) throw std::invalid_argument("cfr_gz_dump: null argument");
  if (!id_off) throw std::invalid_argument("cfr_gz_dump: id_off is null (n + 1 entries, also for n = 0)");
  if (n && !select) throw std::invalid_argument("cfr_gz_dump: select is null");
  auto offsets = [n](const uint64_t *off, const void *bytes, const std::string &what) {
    if (!off) throw std::invalid_argument("cfr_gz_dump: " + what + " offsets are null");
    for (size_t i = 0; i < n; ++i)
      if (off[i + 1] < off[i]) throw std::invalid_argument("cfr_gz_dump: " + what + " offsets decrease at read " + std::to_string(i));
    if (!bytes && off[n] > off[0]) throw std::invalid_argument("cfr_gz_dump: " + what + " bytes are null but the offsets span bytes");
  };
  offsets(id_off, id_bytes, "id");
  for (int f = 0; f < n_files; ++f) {
    offsets(files[f].seq_off, files[f].seq, "file " + std::to_string(f) + ": sequence");
    if (!files[f].qual) continue;
    if (n && !files[f].has_qual) throw std::invalid_argument("cfr_gz_dump: file " + std::to_string(f) + ": qual without has_qual");
    offsets(files[f].qual_off, files[f].qual, "file " + std::to_string(f) + ": quality");
  }
}

namespace {

struct CrcTable {
  uint32_t t[256];
  CrcTable() { for (uint32_t i = 0; i < 256; ++i) t[i] = gz_crc_entry(i); }
};

struct BitSink {            // the stream's bits into bytes, least significant bit first
  uint8_t *p;
  uint64_t acc = 0;
  uint32_t have = 0;
  void put(uint64_t bits, uint32_t nb) {
    acc |= bits << have;
    have += nb;
    while (have >= 8) { *p++ = (uint8_t)acc; acc >>= 8; have -= 8; }
  }
  void flush() { if (have) { *p++ = (uint8_t)acc; acc = 0; have = 0; } }
};

// one block into its slot (the member begins at slot + 2); returns the member's bytes.  kind: 0 stored, 1 fixed, 2 dynamic.
// tokens: nullptr in fixed mode, else room for n tokens: they are kept, counted and written once the choice is made.
uint32_t encode_block(const uint8_t *in, uint32_t n, uint8_t *slot, std::vector<uint32_t> &table, const CrcTable &crc_table, uint32_t *tokens, uint32_t &kind) {
  uint8_t *member = slot + 2, *def = member + kGzHeader;
  std::fill(table.begin(), table.end(), 0u);
  uint32_t mlen[kGzWindow], mdist[kGzWindow];
  uint64_t tok_bits[kGzWindow];
  uint32_t tok_nb[kGzWindow];
  uint32_t lfreq[kGzLitSyms] = {0}, dfreq[kGzDistSyms] = {0};
  BitSink sink{def};
  if (!tokens) sink.put(3, kGzFirstBits);
  uint64_t bitpos = kGzFirstBits;
  uint32_t next_free = 0, n_kept = 0;
  bool stored = false;
  for (uint32_t base = 0; base < n; base += kGzWindow) {
    const uint32_t end = std::min(base + kGzWindow, n);
    for (uint32_t p = base; p < end; ++p) {                 // 1. lookup: the table as the earlier windows left it
      mlen[p - base] = 0; mdist[p - base] = 0;
      if (p + 4 <= n) mlen[p - base] = gz_match_len(in, n, p, table[gz_hash(gz_load32(in + p))], mdist[p - base]);
    }
    for (uint32_t p = base; p < end && p + 4 <= n; ++p) {   // 2. insert: ascending, the highest position of a hash stays
      uint32_t &e = table[gz_hash(gz_load32(in + p))];
      e = std::max(e, p + 1);
    }
    uint32_t n_tok = 0, total = 0;                          // 3. choose
    uint32_t pos = std::max(next_free, base);
    while (pos < end) {
      const uint32_t k = pos - base;
      if (tokens) {                                         // dynamic mode: count and keep
        uint32_t eb, ev;
        if (mlen[k]) {
          ++lfreq[gz_len_symbol(mlen[k], eb, ev)];
          ++dfreq[gz_dist_symbol(mdist[k], eb, ev)];
          tokens[n_kept++] = gz_token_match(mlen[k], mdist[k]);
        } else {
          ++lfreq[in[pos]];
          tokens[n_kept++] = in[pos];
        }
      } else {
        tok_nb[n_tok] = mlen[k] ? gz_match(mlen[k], mdist[k], tok_bits[n_tok]) : gz_literal(in[pos], tok_bits[n_tok]);
        total += tok_nb[n_tok++];
      }
      pos += mlen[k] ? mlen[k] : 1;
    }
    next_free = pos;
    if (tokens) continue;
    if (gz_must_store(bitpos + total, n)) { stored = true; break; }
    for (uint32_t t = 0; t < n_tok; ++t) sink.put(tok_bits[t], tok_nb[t]);   // 4. emit
    bitpos += total;
  }
  uint32_t def_bytes = 0;
  if (tokens) {
    ++lfreq[kGzEob];
    uint32_t ltab[kGzLitSyms], dtab[kGzDistSyms], clfreq[kGzClSyms], cltab[kGzClSyms], w32[kGzLitSyms];
    uint8_t lens[kGzLitSyms + kGzDistSyms], cllen[kGzClSyms];
    uint16_t w16[kGzLitSyms], cnt[16];
    const GzDynWork w{lfreq, dfreq, ltab, dtab, clfreq, cltab, lens, cllen, w32, w16, cnt};
    const GzDynPlan plan = gz_dyn_build(w);
    kind = gz_choose(n, plan);
    if (kind) {
      GzWordSink words{def, 0, 0};
      if (kind == 2) gz_put_dyn_header(words, w, plan);
      else {
        words.put(3, kGzFirstBits);
        for (uint32_t s = 0; s < kGzLitSyms; ++s) ltab[s] = gz_fixed_entry(s);
        for (uint32_t d = 0; d < kGzDistSyms; ++d) dtab[d] = gz_fixed_dist_entry(d);
      }
      for (uint32_t t = 0; t <= n_kept; ++t) {              // (the end-of-block symbol behind the last token)
        uint64_t bits;
        const uint32_t nb = gz_token_bits(t < n_kept ? tokens[t] : kGzEob, ltab, dtab, bits);
        words.put(bits & 0xffffffffu, std::min(nb, 32u));
        if (nb > 32) words.put(bits >> 32, nb - 32);
      }
      def_bytes = ((kind == 2 ? plan.dyn_bits : plan.fixed_bits) + 7) >> 3;
      for (uint32_t k = 0; k * 8 < words.have; ++k) words.p[k] = (uint8_t)(words.acc >> (8 * k));
    }
  } else kind = stored ? 0 : 1;
  if (kind == 0) {
    gz_put_stored_head(def, n);
    memcpy(def + kGzStoredHead, in, n);
    def_bytes = kGzStoredHead + n;
  } else if (!tokens) {
    sink.put(0, kGzEndBits);
    sink.flush();
    def_bytes = (uint32_t)((bitpos + kGzEndBits + 7) >> 3);
  }
  uint32_t crc = 0xffffffffu;
  for (uint32_t i = 0; i < n; ++i) crc = gz_crc_byte(crc_table.t, crc, in[i]);
  const uint32_t member_bytes = kGzHeader + def_bytes + kGzTrailer;
  gz_put_header(member, member_bytes);
  gz_put_trailer(def + def_bytes, crc ^ 0xffffffffu, n);
  return member_bytes;
}

float ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

class GzHost : public Gz {
 public:
  explicit GzHost(const cfr_gz_options &o) : block_(gz_block_bytes(o)), stride_(gz_slot_stride(block_)), threads_(o.threads), dynamic_(gz_dynamic(o)) {}

  void compress(const uint8_t *text, uint64_t n, const uint8_t **out, uint64_t *out_n) override {
    if (!out || !out_n || (n && !text)) throw std::invalid_argument("cfr_gz_compress: null argument");
    st_ = cfr_gz_stats{};
    deflate(text, n, out_[0]);
    *out = out_[0].data();
    *out_n = out_[0].size();
  }

  void dump(const char *id_bytes, const uint64_t *id_off, const uint8_t *select, size_t n, const cfr_gz_file *files, int n_files,
            const uint8_t **out, uint64_t *out_n) override {
    gz_check_dump(id_bytes, id_off, select, n, files, n_files, out, out_n);
    st_ = cfr_gz_stats{};
    for (int f = 0; f < n_files; ++f) {
      const auto t0 = std::chrono::steady_clock::now();
      const GzFileView v{files[f].seq, files[f].seq_off, files[f].qual, files[f].qual_off, files[f].has_qual};
      // two passes, as on the device: the records' lengths and their prefix sum (per slice, then over the slices), then the bytes
      int threads = thread_count(n / 4096);
      off_.resize(n + 1);
      std::vector<uint64_t> slice((size_t)threads + 1, 0);
      parallel_slices(n, threads, [&](size_t lo, size_t hi, int tid) {
        uint64_t sum = 0;
        for (size_t i = lo; i < hi; ++i) { off_[i] = sum; sum += gz_record_len(v, id_off, select, i); }
        slice[(size_t)tid + 1] = sum;
      });
      for (int t = 0; t < threads; ++t) slice[(size_t)t + 1] += slice[(size_t)t];
      const uint64_t total = slice[(size_t)threads];
      text_.resize(total);
      parallel_slices(n, threads, [&](size_t lo, size_t hi, int tid) {
        for (size_t i = lo; i < hi; ++i) {
          const uint64_t len = gz_record_len(v, id_off, select, i);
          if (!len) continue;
          uint8_t *o = text_.data() + off_[i] + slice[(size_t)tid];
          const bool q = gz_has_qual(v, i);
          const uint64_t idl = id_off[i + 1] - id_off[i], sl = v.seq_off[i + 1] - v.seq_off[i];
          *o++ = q ? '@' : '>';
          if (idl) memcpy(o, id_bytes + id_off[i], idl);
          o += idl; *o++ = '\n';
          if (sl) memcpy(o, v.seq + v.seq_off[i], sl);
          o += sl; *o++ = '\n';
          if (q) {
            const uint64_t ql = v.qual_off[i + 1] - v.qual_off[i];
            *o++ = '+'; *o++ = '\n';
            if (ql) memcpy(o, v.qual + v.qual_off[i], ql);
            o += ql; *o++ = '\n';
          }
        }
      });
      st_.format_ms += ms_since(t0);
      deflate(text_.data(), total, out_[f]);
      out[f] = out_[f].data();
      out_n[f] = out_[f].size();
    }
  }

  void stats(cfr_gz_stats *st) const override { *st = st_; }

 private:
  int thread_count(size_t pieces) const {
    int threads = threads_ > 0 ? threads_ : (int)std::min(std::max(std::thread::hardware_concurrency(), 1u), 16u);
    if ((size_t)threads > pieces) threads = pieces ? (int)pieces : 1;
    return threads;
  }

  void deflate(const uint8_t *text, uint64_t n, std::vector<uint8_t> &out) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n_blocks = (n + block_ - 1) / block_;
    slots_.resize(n_blocks * stride_);
    sizes_.assign(n_blocks + 1, 0);
    std::vector<uint64_t> kinds_by_thread;                  // per thread: stored, fixed, dynamic
    const int threads = thread_count(n_blocks);
    kinds_by_thread.assign((size_t)threads * 3, 0);
    parallel_slices(n_blocks, threads, [&](size_t lo, size_t hi, int tid) {
      std::vector<uint32_t> table(1u << kGzHashBits), tokens(dynamic_ ? block_ : 0);
      for (size_t b = lo; b < hi; ++b) {
        const uint64_t at = (uint64_t)b * block_;
        uint32_t kind;
        sizes_[b] = encode_block(text + at, (uint32_t)std::min<uint64_t>(block_, n - at), slots_.data() + b * stride_, table, crc_table_,
                                 dynamic_ ? tokens.data() : nullptr, kind);
        ++kinds_by_thread[(size_t)tid * 3 + kind];
      }
    });
    uint64_t total = 0;
    for (uint64_t b = 0; b <= n_blocks; ++b) { const uint64_t s = sizes_[b]; sizes_[b] = total; total += s; }
    out.resize(total);
    parallel_slices(n_blocks, threads, [&](size_t lo, size_t hi, int) {
      for (size_t b = lo; b < hi; ++b) memcpy(out.data() + sizes_[b], slots_.data() + b * stride_ + 2, sizes_[b + 1] - sizes_[b]);
    });
    st_.deflate_ms += ms_since(t0);
    st_.blocks += n_blocks;
    for (int t = 0; t < threads; ++t) {
      st_.stored_blocks += kinds_by_thread[(size_t)t * 3];
      st_.dynamic_blocks += (uint32_t)kinds_by_thread[(size_t)t * 3 + 2];
    }
    st_.bytes_in += n;
    st_.bytes_out += total;
  }

  const uint32_t block_, stride_;
  const int threads_;
  const bool dynamic_;
  const CrcTable crc_table_;
  std::vector<uint8_t> slots_, text_, out_[kGzMaxFiles];
  std::vector<uint64_t> sizes_, off_;
  cfr_gz_stats st_{};
};

}  // namespace

Gz *make_gz_host(const cfr_gz_options &o) { return new GzHost(o); }

}  // namespace cfr
