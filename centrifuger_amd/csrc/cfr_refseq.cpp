// cfr_refseq.cpp — the host twin of the reference-text front end: the grammar of cfr_refseq_core.hpp as the plain byte loop the
// command line used to run (one pass, one thread).  With `protein` it is the only path.  U and T are ASCII here.
// No HIP header is included, so any C++17 compiler builds this file (the sanitizer driver in tools/ does).
#include <chrono>
#include <vector>

#include "cfr_refseq_core.hpp"

namespace cfr {

namespace {

class RefseqHost : public Refseq {
 public:
  explicit RefseqHost(bool protein) : protein_(protein) {}

  void feed(const uint8_t *text, uint64_t len, int at_line_start, int final, cfr_refseq_info *info) override {
    const auto t0 = std::chrono::steady_clock::now();
    memset(info, 0, sizeof(*info));
    records_.clear();
    const uint64_t eff = refseq_effective_len(text, len, at_line_start, final);
    u_.resize((u_.size() + 31) / 32 * 32, 0);
    const uint64_t u_start = u_.size();
    bool in_header = false, line_start = at_line_start != 0;
    uint64_t lead = 0;
    for (uint64_t i = 0; i < eff; ++i) {
      const uint8_t ch = text[i];
      if (in_header) {
        if (ch == '\n') { in_header = false; line_start = true; close_header(text, i); }
        continue;
      }
      if (line_start && ch == '>') {
        in_header = true;
        records_.push_back(cfr_refseq_record{(uint32_t)i, 0, 0, 0});
        continue;
      }
      line_start = ch == '\n';
      if (protein_ ? refseq_kept_aa(ch) : refseq_kept_nt(ch)) {
        u_.push_back(ch);
        if (records_.empty()) ++lead; else ++records_.back().kept;
      } else if (protein_ && ch == '$') {
        u_.resize(u_start);
        throw std::runtime_error("cfr_refseq_feed: a '$' inside a protein sequence is outside this writer");
      }
    }
    if (in_header) close_header(text, eff);          // (a file that ends inside a header line)
    info->n_records = records_.size(); info->consumed = eff; info->lead_kept = lead; info->kept = u_.size() - u_start; info->u_start = u_start;
    info->at_line_start = eff ? (text[eff - 1] == '\n') : (at_line_start != 0);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    info->device_ms = ms;
    feed_ms_ += ms;
  }

  void fetch(cfr_refseq_record *records) override {
    if (records && !records_.empty()) memcpy(records, records_.data(), records_.size() * sizeof(cfr_refseq_record));
  }

  void assemble(const cfr_refseq_segment *segments, uint64_t n_segments, uint64_t n) override {
    const auto t0 = std::chrono::steady_clock::now();
    refseq_check_segments(segments, n_segments, n, u_.size());
    t_.resize(n);
    for (uint64_t k = 0; k < n_segments; ++k) memcpy(t_.data() + segments[k].dst, u_.data() + segments[k].src, segments[k].len);
    std::vector<uint8_t>().swap(u_);
    assemble_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }

  void text(uint8_t *ascii_out) override { if (!t_.empty()) memcpy(ascii_out, t_.data(), t_.size()); }
  uint64_t text_len() const override { return t_.size(); }
  void stats(cfr_refseq_stats *st) const override { st->feed_ms = feed_ms_; st->copy_in_ms = 0.0; st->assemble_ms = assemble_ms_; }
  const uint8_t *host_text() const override { return t_.data(); }

 private:
  void close_header(const uint8_t *text, uint64_t end) {
    cfr_refseq_record &r = records_.back();
    r.header_len = (uint32_t)(end - r.header);
    r.id_len = refseq_id_len(text + r.header, r.header_len);
  }

  bool protein_;
  std::vector<uint8_t> u_, t_;
  std::vector<cfr_refseq_record> records_;
  double feed_ms_ = 0.0, assemble_ms_ = 0.0;
};

}  // namespace

Refseq *make_refseq_host(bool protein) { return new RefseqHost(protein); }

}  // namespace cfr
