// cfr_tsv.hpp — the handle behind cfr_tsv_*: the rows of a batch as one text (semantics: cfr_tsv_core.hpp).  Two makers of one
// interface: the host twin (cfr_tsv.cpp: plain C++, no HIP header, so that a sanitizer build of it stands alone) and the device form
// (cfr_tsv.hip).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "cfr_tsv_core.hpp"

namespace cfr {

// the tables of a TsvView with their owner (host memory); the device form uploads them once
struct TsvTables {
  std::vector<char> names;
  std::vector<uint64_t> name_off;      // seq_cnt + 1
  std::vector<uint8_t> rank;           // node_cnt
  std::vector<char> rank_text;
  std::vector<uint32_t> rank_off;      // kTsvRankStrings + 1
  TsvView view() const {
    return TsvView{names.data(), name_off.data(), rank.data(), rank_text.data(), rank_off.data(), name_off.empty() ? 0 : (uint64_t)name_off.size() - 1, (uint64_t)rank.size()};
  }
  void set_names(const std::vector<std::string> &seq_names);
  void set_rank_strings(const char *(*rank_string)(uint8_t));
};

constexpr int kTsvBlock = 256;                         // reads of one block of k_tsv_write
constexpr uint32_t kTsvTileDefault = 80 * 1024 - 64;   // bytes of a block's span that are staged in LDS
constexpr uint32_t kTsvTileMax = 160 * 1024 - 64;

class Tsv {
 public:
  virtual ~Tsv() {}
  // host arrays in and out; false: the text needs more than cap bytes (*len says how many).  Throws std::invalid_argument for an
  // argument the handle refuses (tsv_check_args).
  virtual bool format(const cfr_result *results, const cfr_match *matches, size_t n_slots, size_t n, const char *id_bytes, const uint64_t *id_offsets,
                      char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets) = 0;
  // device form only: results and matches in HBM (match_begin counts from d_matches), ids in HBM (by offsets or by records) or - host_ids -
  // bytes and offsets on the host, uploaded by the call; text and row_offsets on the host
  virtual bool format_resident(const cfr_result *d_results, const cfr_match *d_matches, size_t n, const TsvIds &ids, bool host_ids,
                               char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets);
  virtual void stats(cfr_tsv_stats *st) const = 0;
};

// the argument checks of cfr_tsv_format, before anything is launched: throws std::invalid_argument that names the read
void tsv_check_args(const cfr_result *results, const cfr_match *matches, size_t n_slots, size_t n, const char *id_bytes, const uint64_t *id_offsets,
                    const char *text, uint64_t cap, const uint64_t *len);
void tsv_check_ids(size_t n, const char *id_bytes, const uint64_t *id_offsets);

Tsv *make_tsv_host(const TsvTables &t, int threads);                               // cfr_tsv.cpp
Tsv *make_tsv_device(int device, const TsvTables &t, const cfr_tsv_options &o);    // cfr_tsv.hip; throws HipError{.., -1} without that GPU

}  // namespace cfr
