// cfr_inflate.cpp — the host twin of the device inflater (cfr_inflate.hip) and the header walk both share: the handle behind
// cfr_inflate_* with device = -1 (semantics: cfr_inflate_core.hpp).  Plain C++: no HIP header and no zlib call, so
// tools/inflate_sanitize.cpp builds it alone.
//
// The members are spread over the threads by parallel_slices; a member's text and status do not depend on which thread made them.
#include "cfr_inflate.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>

#include "cfr_threads.hpp"

namespace cfr {

void inf_walk(const uint8_t *members, uint64_t n, std::vector<InfMember> &out, std::vector<uint64_t> &text_off, std::vector<uint8_t> &status) {
  out.clear(); text_off.clear(); status.clear();
  if (n && !members) throw std::invalid_argument("cfr_inflate_bgzf: null argument");
  uint64_t text = 0;
  for (uint64_t o = 0; o < n;) {
    InfMember m;
    if (!inf_frame(members + o, n - o, o, m)) throw std::invalid_argument("cfr_inflate_bgzf: no BGZF member at byte " + std::to_string(o) + " of the input");
    out.push_back(m);
    text_off.push_back(text);
    status.push_back(m.isize > kInfMaxText ? (uint8_t)CFR_INF_BAD_HEADER : (uint8_t)CFR_INF_OK);
    text += inf_text_bytes(m);
    o += m.size;
  }
  text_off.push_back(text);
  if (text >= kInfMaxCallText) throw std::invalid_argument("cfr_inflate_bgzf: 4 GiB of text or more in one call: hand over fewer members");
}

void inf_fill_info(const std::vector<uint8_t> &status, uint64_t bytes_in, uint64_t bytes_out, cfr_inflate_info *info) {
  *info = cfr_inflate_info{};
  info->members = status.size();
  info->bytes_in = bytes_in;
  info->bytes_out = bytes_out;
  for (size_t i = 0; i < status.size(); ++i)
    if (status[i]) {
      if (!info->bad_members++) { info->first_bad = i; info->first_bad_status = status[i]; }
    }
}

namespace {

struct CrcTable {
  uint32_t t[256];
  CrcTable() { for (uint32_t i = 0; i < 256; ++i) t[i] = gz_crc_entry(i); }
};

// the maker's part of inf_member (cfr_inflate_core.hpp), in plain loops
struct HostMachine {
  const uint8_t *in;             // the deflate stream
  uint32_t n_in;
  uint8_t *out;                  // the member's text: isize bytes

  uint32_t peek(uint32_t pos) const {
    const uint32_t b = pos >> 3;
    uint64_t v = 0;
    for (uint32_t k = 0; k < 5; ++k)
      if (b + k < n_in) v |= (uint64_t)in[b + k] << (8 * k);
    return (uint32_t)(v >> (pos & 7));
  }
  void sync() {}
  void set_len(uint8_t *a, uint32_t i, uint32_t n, uint32_t v) { for (uint32_t k = 0; k < n; ++k) a[i + k] = (uint8_t)v; }
  void fixed_lens(uint8_t *lens) {
    for (uint32_t s = 0; s < kInfLitSyms; ++s) lens[s] = (uint8_t)gz_fixed_len(s);
    for (uint32_t d = 0; d < kInfDistSyms; ++d) lens[kInfLitSyms + d] = 5;
  }
  bool build(const uint8_t *lens, uint32_t n, int32_t kind, uint16_t *tab, uint32_t tbits, uint16_t *cnt, uint16_t *sym) {
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++cnt[lens[s]];
    cnt[0] = 0;
    if (!inf_check_set(cnt, kind)) return false;
    uint32_t offs[16], next[16], code = 0;
    offs[0] = offs[1] = 0; next[0] = 0;
    for (uint32_t l = 1; l < 16; ++l) {
      code = (code + cnt[l - 1]) << 1;
      next[l] = code;
      if (l < 15) offs[l + 1] = offs[l] + cnt[l];
    }
    for (uint32_t k = 0; k < (1u << tbits); ++k) tab[k] = 0;
    for (uint32_t s = 0; s < n; ++s) {
      const uint32_t l = lens[s];
      if (!l) continue;
      sym[offs[l]++] = (uint16_t)s;
      const uint32_t c = next[l]++;
      if (l <= tbits)
        for (uint32_t k = gz_rev(c, l); k < (1u << tbits); k += 1u << l) tab[k] = inf_entry(s, l);
    }
    return true;
  }
  void literal(uint32_t at, uint32_t byte) { out[at] = (uint8_t)byte; }
  void flush() {}
  void copy_stored(uint32_t src, uint32_t at, uint32_t n) { if (n) memcpy(out + at, in + src, n); }
  void copy_match(uint32_t at, uint32_t dist, uint32_t n) {
    const uint8_t *src = out + at - dist;
    for (uint32_t i = 0; i < n; ++i) out[at + i] = src[dist >= n ? i : i % dist];
  }
};

uint8_t inflate_member(const uint8_t *members, const InfMember &m, uint8_t *text, const CrcTable &crc_table) {
  uint16_t ltab[1u << kInfLitBits], dtab[1u << kInfDistBits], ctab[1u << kInfClBits], lsym[kInfLitSyms], dsym[kInfDistSyms], csym[kGzClSyms], lcnt[16], dcnt[16], ccnt[16];
  uint8_t lens[kInfLitSyms + kInfDistSyms], cllen[kGzClSyms];
  const InfWork w{ltab, dtab, ctab, lsym, dsym, csym, lcnt, dcnt, ccnt, lens, cllen};
  const uint32_t n_in = m.size - m.head - kGzTrailer;
  HostMachine machine{members + m.off + m.head, n_in, text};
  int32_t st = inf_member(machine, w, n_in * 8, m.isize);
  if (st == CFR_INF_OK) {
    uint32_t crc = 0xffffffffu;
    for (uint32_t i = 0; i < m.isize; ++i) crc = gz_crc_byte(crc_table.t, crc, text[i]);
    if ((crc ^ 0xffffffffu) != m.crc) st = CFR_INF_BAD_CRC;
  }
  if (st != CFR_INF_OK && m.isize) memset(text, 0, m.isize);
  return (uint8_t)st;
}

class InflateHost : public Inflate {
 public:
  explicit InflateHost(int threads) : threads_(threads) {}

  void inflate(const uint8_t *members, uint64_t n, int fetch_text, const uint8_t **text, uint64_t *text_n, cfr_inflate_info *info) override {
    (void)fetch_text;
    if (!text || !text_n || !info) throw std::invalid_argument("cfr_inflate_bgzf: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    st_ = cfr_inflate_stats{};
    inf_walk(members, n, members_, text_off_, status_);
    const uint64_t total = text_off_.back();
    if (!text_ || total != text_n_) {                       // a block of exactly the text's size: an access one byte off is outside it
      text_.reset(new uint8_t[std::max<uint64_t>(total, 1)]);
      text_n_ = total;
    }
    int threads = threads_ > 0 ? threads_ : (int)std::min(std::max(std::thread::hardware_concurrency(), 1u), 16u);
    if ((size_t)threads > members_.size()) threads = members_.empty() ? 1 : (int)members_.size();
    parallel_slices(members_.size(), threads, [&](size_t lo, size_t hi, int) {
      for (size_t i = lo; i < hi; ++i)
        if (!status_[i]) status_[i] = inflate_member(members, members_[i], text_.get() + text_off_[i], crc_table_);
    });
    inf_fill_info(status_, n, total, info);
    *text = text_.get();
    *text_n = total;
    st_.inflate_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
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

  void stats(cfr_inflate_stats *st) const override { *st = st_; }

 private:
  const int threads_;
  const CrcTable crc_table_;
  std::vector<InfMember> members_;
  std::vector<uint64_t> text_off_;
  std::vector<uint8_t> status_;
  std::unique_ptr<uint8_t[]> text_;
  uint64_t text_n_ = 0;
  cfr_inflate_stats st_{};
};

}  // namespace

Inflate *make_inflate_host(int threads) { return new InflateHost(threads); }

}  // namespace cfr
