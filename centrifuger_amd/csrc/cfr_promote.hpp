// cfr_promote.hpp — the handle behind cfr_promote_* and the launchers of the kernels in cfr_promote.hip.  Semantics, plain types and
// the per-read code shared by host and device: cfr_promote_core.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "cfr_promote_core.hpp"

namespace cfr {

// ---- the device side (cfr_promote.hip); all throw HipError.  The launchers enqueue on `st` and do not wait. ----
void promote_launch_table(const PromoteTables &T, const PromoteLevel &L, uint32_t *d_promo, hipStream_t st);
// reads [0, n): slot of match k of read i = results[i].match_begin - match_base + k in d_matches; d_src as promote_read_rank's src (may be null)
void promote_launch_reads(const PromoteTables &T, const PromoteLevel &L, const uint32_t *d_promo, cfr_result *d_results, cfr_match *d_matches,
                          size_t n, uint64_t match_base, uint64_t *d_src, hipStream_t st, unsigned max_blocks = 0);   // max_blocks > 0: at most that many blocks (the lanes stride over the reads)
class PromoteDevice {               // the tables of a taxonomy and the table of a level in one GPU's HBM, buffers for apply()
 public:
  virtual ~PromoteDevice() {}
  virtual void apply(cfr_result *results, cfr_match *matches, size_t n, uint64_t extent, uint64_t *src_slot) = 0;
  virtual float table_ms() const = 0;   // device time of k_promote_table (once, at construction)
  virtual float reads_ms() const = 0;   // ... of the per-read kernel of the last apply()
};
PromoteDevice *make_promote_device(int device, const Taxonomy &t, const std::vector<uint32_t> &depth, uint64_t one_node, const PromoteLevel &L);

// cfr_promote_*: <prefix>.2.cfr and a level; device = -1: the host twin alone
class Promote {
 public:
  Promote(const std::string &prefix, const std::string &level, int device);
  ~Promote();
  void apply(cfr_result *results, cfr_match *matches, size_t n, uint64_t *src_slot, int threads = 0);
  // the "Couldn't find parent of taxID" lines the script prints for these reads in lca mode (none in rank mode), in its order
  void lca_warnings(const cfr_result *results, const cfr_match *matches, size_t n, std::vector<uint64_t> &taxids) const;
  const Taxonomy &tax() const { return tax_; }
  const PromoteLevel &level() const { return level_; }
  float table_ms() const { return dev_ ? dev_->table_ms() : 0.f; }
  float reads_ms() const { return dev_ ? dev_->reads_ms() : (float)host_ms_; }

 private:
  PromoteTables tables() const;
  Taxonomy tax_;
  PromoteLevel level_;
  std::vector<uint32_t> depth_, promo_;
  uint64_t one_node_ = 0;
  std::unique_ptr<PromoteDevice> dev_;
  double host_ms_ = 0;
};

}  // namespace cfr
