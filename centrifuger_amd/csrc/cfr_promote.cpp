// cfr_promote.cpp — the host twin of centrifuger-promote and the handle behind cfr_promote_* (semantics: cfr_promote_core.hpp).
#include "cfr_promote.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

#include "cfr_device.hpp"
#include "cfr_quant.hpp"
#include "cfr_threads.hpp"

namespace cfr {

PromoteLevel promote_parse_level(const char *level) {
  PromoteLevel L;
  if (!strcmp(level, "lca")) { L.lca = 1; return L; }
  for (int r = 0; r < 31; ++r) if (!strcmp(quant_rank_string((uint8_t)r), level)) L.rank_mask |= 1u << r;
  return L;
}

// steps from every node to its root (the tax_depth of the device image); a parent outside the tree ends the walk like a root
std::vector<uint32_t> promote_depths(const std::vector<uint64_t> &par) {
  std::vector<uint32_t> depth(par.size(), 0xffffffffu);
  std::vector<uint64_t> path;
  for (uint64_t x0 = 0; x0 < par.size(); ++x0) {
    path.clear();
    uint64_t x = x0;
    while (depth[x] == 0xffffffffu && par[x] != x && par[x] < par.size() && path.size() <= par.size()) { path.push_back(x); x = par[x]; }
    uint32_t d = depth[x] == 0xffffffffu ? 0u : depth[x];
    if (depth[x] == 0xffffffffu) depth[x] = 0;
    for (size_t k = path.size(); k-- > 0;) depth[path[k]] = ++d;
  }
  return depth;
}

Promote::Promote(const std::string &prefix, const std::string &level, int device) {
  load_taxonomy(prefix + ".2.cfr", tax_);
  const uint64_t nc = tax_.node_cnt;
  if (nc >= 0xffffffffull) throw FormatError{"cfr_promote: a taxonomy of 2^32 nodes or more"};
  for (uint64_t i = 0; i < nc; ++i)
    if (tax_.parent[i] >= nc) throw FormatError{"cfr_promote: " + prefix + ".2.cfr: the parent of node " + std::to_string(i) + " is outside the tree"};
  level_ = promote_parse_level(level.c_str());
  depth_ = promote_depths(tax_.parent);
  one_node_ = nc;
  for (uint64_t i = 0; i < nc; ++i) if (tax_.orig_taxid[i] == 1) one_node_ = i;
  if (device >= 0) {
    dev_.reset(make_promote_device(device, tax_, depth_, one_node_, level_));
  } else if (!level_.lca) {
    const PromoteTables T = tables();
    promo_.resize(nc);
    for (uint64_t i = 0; i < nc; ++i) promo_[i] = promote_walk(T, level_, i);
  }
}

Promote::~Promote() {}

PromoteTables Promote::tables() const {
  return PromoteTables{tax_.parent.data(), tax_.orig_taxid.data(), tax_.seq_to_tax.data(), tax_.rank.data(), depth_.data(),
                       tax_.node_cnt, tax_.seq_cnt, tax_.root, one_node_};
}

void Promote::apply(cfr_result *results, cfr_match *matches, size_t n, uint64_t *src_slot, int threads) {
  if (n == 0) return;
  if (dev_) {
    uint64_t extent = 0;
    for (size_t i = 0; i < n; ++i) if (results[i].n_match > 0) extent = std::max<uint64_t>(extent, results[i].match_begin + (uint64_t)results[i].n_match);
    dev_->apply(results, matches, n, extent, src_slot);
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (threads <= 0) threads = (int)std::min(std::max(std::thread::hardware_concurrency(), 1u), 16u);
  const PromoteTables T = tables();
  // (reads own disjoint slot ranges: slices do not meet)
  parallel_slices(n, n < 4096 ? 1 : threads, [&](size_t lo, size_t hi, int) {
    for (size_t i = lo; i < hi; ++i) {
      if (level_.lca) promote_read_lca(T, results[i], matches, results[i].match_begin, src_slot);
      else promote_read_rank(T, promo_.data(), results[i], matches, results[i].match_begin, src_slot);
    }
  });
  host_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// lca() prints its line for an id without a parent entry: the first argument always, the second when it is above 1 (:67-87).  The
// first argument is the fold so far - the first row's id, or a result (a node, or the literal 1).
void Promote::lca_warnings(const cfr_result *results, const cfr_match *matches, size_t n, std::vector<uint64_t> &out) const {
  if (!level_.lca) return;
  const PromoteTables T = tables();
  const uint64_t nc = T.node_cnt;
  for (size_t i = 0; i < n; ++i) {
    const int32_t nm = results[i].n_match;
    if (nm <= 1) continue;
    const cfr_match *m = matches + results[i].match_begin;
    bool any = one_node_ >= nc;
    for (int32_t j = 0; j < nm && !any; ++j) any = promote_match_node(T, m[j]) >= nc;
    if (!any) continue;                      // (every id is a node, and so is every result: nothing to print)
    uint64_t node = promote_match_node(T, m[0]);
    uint64_t taxid = node < nc ? T.orig[node] : m[0].taxid;
    for (int32_t j = 1; j < nm; ++j) {
      const uint64_t nb = promote_match_node(T, m[j]);
      const uint64_t tb = nb < nc ? T.orig[nb] : m[j].taxid;
      if (taxid == 0) { taxid = tb; node = nb; continue; }
      if (tb == 0 || tb == taxid) continue;
      if (node >= nc) out.push_back(taxid);
      if (nb >= nc && tb > 1) out.push_back(tb);
      uint64_t x = nc;
      if (node < nc && nb < nc) x = promote_lca_nodes(T, node, nb);
      if (x < nc) { node = x; taxid = T.orig[x]; }
      else { node = one_node_; taxid = 1; }
    }
  }
}

}  // namespace cfr
