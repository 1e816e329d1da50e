// cfr_tokenize_host.cpp — the host twin of the tokeniser: the statement of the grammar in cfr_tokenize_core.hpp, run in plain loops.
// No HIP header is included, so any C++17 compiler builds this file (the sanitizer driver in tools/ does).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "cfr_tokenize_core.hpp"

namespace cfr {

namespace {

class TokenizerHost : public Tokenizer {
 public:
  void tokenize(const uint8_t *text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info) override {
    const auto t0 = std::chrono::steady_clock::now();
    records_.clear(); offsets_.assign(1, 0); bases_.clear(); ids_.clear(); id_off_.assign(1, 0);
    memset(info, 0, sizeof(*info));
    if (len == 0) return;
    info->fastq = text[0] == '@';
    bool virtual_newline = false;
    const uint64_t eff = tok_effective_len(text, len, final, virtual_newline);
    if (eff == 0) return;

    // the line table: every '\n' below eff (the last one may be the tokeniser's own) ends a line
    lstart_.clear(); lcend_.clear(); hdr_line_.clear(); line_rec_.clear();
    uint32_t last_nonempty = 0;
    for (uint64_t s = 0; s < eff;) {
      const void *nl = s < len ? memchr(text + s, '\n', len - s) : nullptr;
      const uint64_t p = nl ? (uint64_t)((const uint8_t *)nl - text) : len;       // (no '\n' left: the virtual one at len)
      uint64_t e = p;
      while (e > s && text[e - 1] == '\r') --e;
      if (!info->fastq) {
        if (e > s && text[s] == '>') hdr_line_.push_back((uint32_t)lstart_.size());
        line_rec_.push_back((uint32_t)hdr_line_.size() - 1);
      }
      lstart_.push_back((uint32_t)s); lcend_.push_back((uint32_t)e);
      if (e > s) last_nonempty = (uint32_t)lstart_.size();
      s = p + 1;
    }
    TokTables t{text, lstart_.data(), lcend_.data(), hdr_line_.data(), line_rec_.data(), (uint32_t)lstart_.size(), (uint32_t)hdr_line_.size(),
                len, eff, info->fastq, final ? 1 : 0};

    // per unit: record, weight, the first candidate that breaks a rule
    const uint32_t units = tok_units(t), cand = tok_candidates(t, last_nonempty);
    std::vector<cfr_read_record> recs(t.fastq ? units : t.H);
    weight_.assign((size_t)units + 1, 0);
    uint32_t first_bad = kTokNone;
    for (uint32_t u = 0; u < units; ++u) {
      const bool ok = t.fastq ? tok_fastq_unit(t, u, cand, recs[u], weight_[u]) : tok_fasta_unit(t, u, cand, recs.data(), weight_[u]);
      if (!ok) first_bad = std::min(first_bad, t.fastq ? u : t.line_rec[u]);
    }
    dst_.resize((size_t)units + 1);
    uint32_t sum = 0;
    for (uint32_t u = 0; u <= units; ++u) { dst_[u] = sum; sum += weight_[u]; }

    const TokSummary s = tok_summary(t, dst_.data(), last_nonempty, first_bad, max_records);
    info->n_records = s.n_records; info->consumed = s.consumed; info->total_bases = s.total_bases;
    info->irregular = s.irregular; info->irregular_at = s.irregular_at;
    records_.assign(recs.begin(), recs.begin() + s.n_records);
    offsets_.resize(s.n_records + 1);
    for (uint32_t r = 0; r <= s.n_records; ++r) offsets_[r] = tok_offset(t, dst_.data(), r);
    bases_.resize(s.total_bases);
    const uint32_t u_end = t.fastq ? (uint32_t)s.n_records : (s.n_records < t.H ? t.hdr_line[s.n_records] : t.L);
    for (uint32_t u = 0; u < u_end; ++u)
      if (weight_[u]) memcpy(bases_.data() + dst_[u], text + t.lstart[t.fastq ? 4 * u + 1 : u], weight_[u]);
    id_off_.resize(s.n_records + 1);                        // the ids are kept: the caller's text may be gone when they are asked for
    for (uint32_t r = 0; r < s.n_records; ++r) {
      const uint8_t *id = text + records_[r].header + 1;
      ids_.insert(ids_.end(), id, id + records_[r].id_len);
      id_off_[r + 1] = ids_.size();
    }
    info->device_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }

  void fetch(cfr_read_record *records, uint64_t *offsets, uint8_t *bases) override {
    if (records && !records_.empty()) memcpy(records, records_.data(), records_.size() * sizeof(cfr_read_record));
    if (offsets) memcpy(offsets, offsets_.data(), offsets_.size() * 8);
    if (bases && !bases_.empty()) memcpy(bases, bases_.data(), bases_.size());
  }

  bool fetch_ids(char *ids, uint64_t cap, uint64_t *id_off, uint64_t *need) override {
    *need = ids_.size();
    if (ids && ids_.size() > cap) return false;
    if (ids && !ids_.empty()) memcpy(ids, ids_.data(), ids_.size());
    if (id_off) memcpy(id_off, id_off_.data(), id_off_.size() * 8);
    return true;
  }

 private:
  std::vector<uint32_t> lstart_, lcend_, hdr_line_, line_rec_, weight_, dst_;
  std::vector<cfr_read_record> records_;
  std::vector<uint64_t> offsets_, id_off_;
  std::vector<uint8_t> bases_, ids_;
};

}  // namespace

Tokenizer *make_tokenizer_host() { return new TokenizerHost(); }

}  // namespace cfr
