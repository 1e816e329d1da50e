// cfr_kreport.hpp — the handle behind cfr_kreport_* and the launchers of the kernels in cfr_kreport.hip.  Semantics, plain types and
// the per-read code shared by host and device: cfr_kreport_core.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "cfr_kreport_core.hpp"

namespace cfr {

constexpr uint32_t kKreportSlots = 1024;      // slots of the block's LDS table in k_kreport_accumulate (a power of two)

// ---- the device side (cfr_kreport.hip); all throw HipError.  The launchers enqueue on `st` and do not wait. ----
// reads [0, n): slot of match k of read i = results[i].match_begin - match_base + k in d_matches; writes d_bin[i] and d_score[i]
void kreport_launch_fold(const PromoteTables &T, const KreportOptions &opt, const cfr_result *d_results, const cfr_match *d_matches, size_t n,
                         uint64_t match_base, uint32_t *d_bin, uint64_t *d_score, hipStream_t st, unsigned max_blocks = 0);
// d_count[b] += the reads of bin b, d_maxscore[b] = max(itself, their scores); bins >= n_bins (dropped reads) are skipped.
// max_blocks > 0: at most that many blocks; slots: of the LDS table, a power of two in [64, 2048], 0 = kKreportSlots
void kreport_launch_accumulate(const uint32_t *d_bin, const uint64_t *d_score, size_t n, uint64_t *d_count, uint64_t *d_maxscore, uint32_t n_bins,
                               hipStream_t st, unsigned max_blocks = 0, uint32_t slots = 0);

class KreportDevice {               // the tables of a taxonomy and the bins in one GPU's HBM, buffers for add()
 public:
  virtual ~KreportDevice() {}
  virtual void add(const cfr_result *results, const cfr_match *matches, size_t n, uint64_t extent) = 0;
  virtual void download(uint64_t *count, uint64_t *maxscore) = 0;      // node_cnt + 1 entries each
  virtual float fold_ms() const = 0;         // device time of k_kreport_fold of the last add()
  virtual float accumulate_ms() const = 0;   // ... of k_kreport_accumulate
};
KreportDevice *make_kreport_device(int device, const Taxonomy &t, const std::vector<uint32_t> &depth, uint64_t one_node, const KreportOptions &opt,
                                   unsigned max_blocks, uint32_t slots);

// cfr_kreport_*: <prefix>.2.cfr and the script's options; device = -1: the host twin alone
class Kreport {
 public:
  Kreport(const std::string &prefix, const KreportOptions &opt, int device, unsigned max_blocks = 0, uint32_t slots = 0, int threads = 0);
  ~Kreport();
  void add_results(const cfr_result *results, const cfr_match *matches, size_t n);
  void add_tsv(const std::string &path);             // plain or gz, "-": stdin
  void add_count_table(const std::string &path);
  // only the "Couldn't find parent" lines of these reads, nothing counted: for reads that a device image counts (cfr_device_index_set_kreport)
  void scan_warnings(const cfr_result *results, const cfr_match *matches, size_t n) { read_warnings(results, matches, n); }
  void add_counts(const uint64_t *own, const uint64_t *own_score, size_t n);     // bins downloaded from a device image
  // own / clade counts and scores per bin (node_cnt + 1 entries; the last one is "unclassified") and the script's $seq_count.
  // In the fraction modes (--no-lca, --is-count-table) the counts are truncated towards zero, as the script prints them.
  void counts(std::vector<uint64_t> &own, std::vector<uint64_t> &clade, std::vector<uint64_t> &own_score, std::vector<uint64_t> &clade_score, double &seq_count);
  const std::vector<uint64_t> &warnings() const { return warnings_; }      // tax ids of the "Couldn't find parent" lines so far, in the script's order
  void write(const char *path);                       // null or "-": stdout; throws std::runtime_error with the script's message when nothing was counted, and makes no file
  uint64_t bins() const { return tax_.node_cnt + 1; }
  float fold_ms() const { return dev_ ? dev_->fold_ms() : (float)host_ms_; }
  float accumulate_ms() const { return dev_ ? dev_->accumulate_ms() : 0.f; }
  float parse_ms() const { return (float)parse_ms_; }

 private:
  PromoteTables tables() const;
  void read_warnings(const cfr_result *results, const cfr_match *matches, size_t n);
  struct Rollup;
  void rollup(Rollup &r);
  Taxonomy tax_;
  KreportOptions opt_;
  std::vector<uint32_t> depth_;
  uint64_t one_node_ = 0;
  std::vector<uint64_t> count_, score_;              // the host's bins (the device's stay in HBM and are added in by rollup)
  std::vector<double> frac_;                         // the fraction modes' bins
  double frac_seq_ = 0;
  bool frac_mode_ = false;
  std::vector<uint64_t> warnings_;
  std::unique_ptr<KreportDevice> dev_;
  double host_ms_ = 0, parse_ms_ = 0;
  int threads_ = 0;
};

}  // namespace cfr
