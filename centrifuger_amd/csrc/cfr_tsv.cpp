// cfr_tsv.cpp — the host twin of the device formatter (cfr_tsv.hip) and the argument checks both share: the handle behind cfr_tsv_*
// with device = -1 (semantics: cfr_tsv_core.hpp).  Plain C++: no HIP header, so tools/tsv_sanitize.cpp builds it alone.
//
// Two passes, as on the device: the lengths of the reads' rows and their prefix sum (per slice of the batch, then over the slices),
// then every thread writes its slice at its offset - so the twin and the kernels agree on row_offsets as well as on the text.
#include "cfr_tsv.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <thread>

#include "cfr_threads.hpp"

namespace cfr {

void TsvTables::set_names(const std::vector<std::string> &seq_names) {
  names.clear();
  name_off.assign(1, 0);
  for (const std::string &s : seq_names) {
    const size_t k = strlen(s.c_str());          // (cfr_format_tsv prints the name as a C string)
    names.insert(names.end(), s.data(), s.data() + k);
    name_off.push_back(names.size());
  }
}

void TsvTables::set_rank_strings(const char *(*rank_string)(uint8_t)) {
  rank_text.clear();
  rank_off.assign(1, 0);
  for (uint32_t r = 0; r < kTsvRankStrings; ++r) {
    const char *s = rank_string((uint8_t)r);
    rank_text.insert(rank_text.end(), s, s + strlen(s));
    rank_off.push_back((uint32_t)rank_text.size());
  }
}

void tsv_check_ids(size_t n, const char *id_bytes, const uint64_t *id_offsets) {
  if (!id_offsets) throw std::invalid_argument("cfr_tsv_format: id_offsets is null (n + 1 entries, also for n = 0)");
  for (size_t i = 0; i < n; ++i)
    if (id_offsets[i + 1] < id_offsets[i]) throw std::invalid_argument("cfr_tsv_format: id_offsets decreases at read " + std::to_string(i));
  if (!id_bytes && id_offsets[n] > 0)throw std::invalid_argument("cfr_tsv_format: id_bytes is null but the offsets span bytes");
}

void tsv_check_args(const cfr_result *results, const cfr_match *matches, size_t n_slots, size_t n, const char *id_bytes, const uint64_t *id_offsets,
                    const char *text, uint64_t cap, const uint64_t *len) {
  if (!len) throw std::invalid_argument("cfr_tsv_format: len is null");
  if (!text && cap) throw std::invalid_argument("cfr_tsv_format: text is null with a capacity");
  if (n && !results) throw std::invalid_argument("cfr_tsv_format: results is null");
  if (!matches && n_slots) throw std::invalid_argument("cfr_tsv_format: matches is null with match slots");
  tsv_check_ids(n, id_bytes, id_offsets);
  for (size_t i = 0; i < n; ++i) {
    const cfr_result &r = results[i];
    if (r.n_match <= 0) continue;
    if (r.match_begin > n_slots || (uint64_t)r.n_match > n_slots - r.match_begin)
      throw std::invalid_argument("cfr_tsv_format: the matches of read " + std::to_string(i) + " end behind the " + std::to_string(n_slots) + " match slots");
  }
}

bool Tsv::format_resident(const cfr_result *, const cfr_match *, size_t, const TsvIds &, bool, char *, uint64_t, uint64_t *, uint64_t *) {
  throw std::invalid_argument("cfr_tsv: results in device memory need a device handle");
}

namespace {

class TsvHost : public Tsv {
 public:
  TsvHost(const TsvTables &t, int threads) : t_(t), threads_(threads) {}
  bool format(const cfr_result *results, const cfr_match *matches, size_t n_slots, size_t n, const char *id_bytes, const uint64_t *id_offsets,
              char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets) override {
    tsv_check_args(results, matches, n_slots, n, id_bytes, id_offsets, text, cap, len);
    const auto t0 = std::chrono::steady_clock::now();
    const TsvView v = t_.view();
    const TsvIds ids{id_bytes, id_offsets, nullptr};
    int threads = threads_ > 0 ? threads_ : (int)std::min(std::max(std::thread::hardware_concurrency(), 1u), 16u);
    if ((size_t)threads > n) threads = n ? (int)n : 1;
    off_.resize(n + 1);
    std::vector<uint64_t> slice((size_t)threads + 1, 0);
    // pass 1: off_[i] = the bytes of the slice's reads in front of read i
    parallel_slices(n, threads, [&](size_t lo, size_t hi, int tid) {
      uint64_t sum = 0;
      for (size_t i = lo; i < hi; ++i) {
        off_[i] = sum;
        uint64_t id_len;
        (void)tsv_id(ids, i, id_len);
        sum += tsv_read_len(v, results[i], (results[i].n_match > 0 ? matches + results[i].match_begin : nullptr), id_len);
      }
      slice[(size_t)tid + 1] = sum;
    });
    for (int t = 0; t < threads; ++t) slice[(size_t)t + 1] += slice[(size_t)t];
    const uint64_t total = slice[(size_t)threads];
    *len = total;
    const auto t1 = std::chrono::steady_clock::now();
    len_ms_ = std::chrono::duration<float, std::milli>(t1 - t0).count();
    write_ms_ = 0.f;
    if (total > cap) return false;
    // pass 2: the slices' offsets added, the rows written
    parallel_slices(n, threads, [&](size_t lo, size_t hi, int tid) {
      for (size_t i = lo; i < hi; ++i) {
        off_[i] += slice[(size_t)tid];
        uint64_t id_len;
        const char *id = tsv_id(ids, i, id_len);
        TsvBytes o{text + off_[i]};
        tsv_rows(v, results[i], (results[i].n_match > 0 ? matches + results[i].match_begin : nullptr), id, id_len, o);
      }
    });
    off_[n] = total;
    if (row_offsets) memcpy(row_offsets, off_.data(), (n + 1) * 8);
    write_ms_ = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
    return true;
  }
  void stats(cfr_tsv_stats *st) const override {
    memset(st, 0, sizeof(*st));
    st->len_ms = len_ms_; st->write_ms = write_ms_;
  }

 private:
  TsvTables t_;
  int threads_;
  std::vector<uint64_t> off_;
  float len_ms_ = 0.f, write_ms_ = 0.f;
};

}  // namespace

Tsv *make_tsv_host(const TsvTables &t, int threads) { return new TsvHost(t, threads); }

}  // namespace cfr
