// cfr_tax_fold.hpp — Taxonomy::LCA (Taxonomy.hpp:733-836) as a fold over the ids, with the depth table of the device image.  Written
// once, for the kernels of the tail (cfr_kernels.hip.inc: d_tax_lca, tail_emit_small, k_adjust_tail, k_tail_heavy) and for the host
// (cfr_tail.cpp: tax_lca_fold, which the tests compare with the literal restatement tax_lca and with the oracle).
//
// The taxonomy may be a forest: every node that is its own parent is the top of a tree, and tax_root is the first of them.  The
// reference ends EVERY path with tax_root, whichever top the walk stopped under, and leaves the top itself out of the path.  So:
//   * an id equal to tax_root takes no part;
//   * the first id that is not tax_root is the backbone, even when it is its own parent (a second top);
//   * every later id that is its own parent is skipped;
//   * two paths that have not met below depth 0 meet in tax_root - whether they stand on two tops or on the same second top.
// depth[x] = steps from x to the top of its tree (0 for a top), so a climb that counts dcur down to 0 ends on every forest.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#ifndef CFR_HD
#define CFR_HD __host__ __device__
#endif
#else
#ifndef CFR_HD
#define CFR_HD
#endif
#endif

namespace cfr {

struct TaxFold {
  uint64_t cur;        // the fold so far (tax_root while have is false)
  uint32_t dcur;       // depth[cur]; 0 once the fold has reached tax_root
  bool have;           // an id has been taken
};

CFR_HD inline TaxFold tax_fold_begin(uint64_t tax_root) { return TaxFold{tax_root, 0u, false}; }

// cur (depth dcur) and x (depth dx) -> their meeting point in cur / dcur.  steps (may be null) counts the loop iterations: at most
// dcur + dx, since every iteration takes one step up on at least one side.
CFR_HD inline void tax_fold_join(const uint64_t *parent, uint64_t tax_root, uint64_t &cur, uint32_t &dcur, uint64_t x, uint32_t dx,
                                 uint32_t *steps = nullptr) {
  while (dx > dcur) { x = parent[x]; --dx; if (steps) ++*steps; }
  while (dcur > dx) { cur = parent[cur]; --dcur; if (steps) ++*steps; }
  while (cur != x && dcur > 0) { cur = parent[cur]; x = parent[x]; --dcur; if (steps) ++*steps; }
  if (dcur == 0) cur = tax_root;
}

// one more id (a node of the tree) into the fold
CFR_HD inline void tax_fold_add(const uint64_t *parent, const uint32_t *depth, uint64_t tax_root, TaxFold &F, uint64_t x,
                                uint32_t *steps = nullptr) {
  if (x == tax_root) return;
  const bool top = x == parent[x];
  if (!F.have) { F.cur = x; F.dcur = top ? 0u : depth[x]; F.have = true; return; }
  if (top) return;
  tax_fold_join(parent, tax_root, F.cur, F.dcur, x, depth[x], steps);
}

CFR_HD inline uint64_t tax_fold_result(const TaxFold &F, uint64_t tax_root) { return F.have ? F.cur : tax_root; }

}  // namespace cfr
