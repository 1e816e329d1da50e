// cfr_promote_core.hpp — centrifuger-promote: every read's assignments rewritten to a chosen rank, or folded into their lowest common
// ancestor ("lca").  The statement of record is the reference's Perl script (centrifuger-promote:44-149); this header restates it on
// compact tax ids, once, for the host twin (cfr_promote.cpp) and for the kernels (cfr_promote.hip).
//
// A level is "lca" or a rank string; a rank code matches when Taxonomy::GetTaxRankString of it equals the string, and a string that
// matches no code promotes nothing.  The node of a match: kind 1: its id (node_cnt and above: a tax id the tree does not hold);
// kind 0: SeqIdToTaxId of the sequence, the root where that is no node (what GetOrigTaxId prints for it, Taxonomy.hpp:633-639).  The
// tax id of a match that has a node is the node's original id, otherwise the taxid field.
//
// Rank mode (PromoteTaxId, :44-58; OutputPromotedLines, :102-124), per match with node c:
//   no node: the match stays as it is.  Otherwise walk from c towards the root: stop at the first node whose rank matches, give up at
//   a node whose original id is <= 1.  No result, or one whose original id is <= 1: c itself.  The match becomes kind 1, id = that
//   node, taxid = its original id (so its TSV name is the node's rank string, the script's $newLevel).
//   A later match whose resulting tax id already appeared in the read is dropped; survivors keep their order and move to the front.
// lca mode (lca, :60-89; :125-141): the script's lca() folded over the read's tax ids in order - the tree's LCA, and the literal tax
//   id 1 when one of the two is no node ("Couldn't find parent"), when the walk from the second meets a node with an original id <= 1
//   first, or when the two share no ancestor.  The read keeps one match: the first one untouched when the result is its tax id,
//   otherwise kind 1 with the node of the result.
// An unclassified read (n_match <= 0) is untouched in both modes.
//
// One difference, on input no fixture has: the script recurses forever on a tree whose root has an original id above 1 and a rank that
// does not match (PromoteTaxId(parent of the root) is the root again).  Here every walk also stops at a node that is its own parent.
//
// Device design: k_promote_table runs once per (taxonomy, level), one lane per node, and writes promo[node] = the node it promotes
// to; the per-read kernel then makes ONE gather per match instead of a walk.  lca mode needs no table: it equalises depths
// (tax_depth) and climbs both sides in lock step.
// This header holds the plain types and the per-read code only (what the device image needs too); the handle classes and the kernel
// launchers are in cfr_promote.hpp.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "cfr_index.hpp"

#if defined(__HIPCC__)
#define CFR_HD __host__ __device__
#else
#define CFR_HD
#endif

namespace cfr {

// the taxonomy side tables as the device image holds them (cfr_device.hpp: tax_parent, tax_orig, tax_rank, tax_depth, seq_to_tax)
struct PromoteTables {
  const uint64_t *parent, *orig, *seq_to_tax;
  const uint8_t *rank;
  const uint32_t *depth;       // steps from a node to its root
  uint64_t node_cnt, seq_cnt, root;
  uint64_t one_node;           // the node whose original id is 1, node_cnt when there is none
};

struct PromoteLevel {
  uint32_t lca = 0;            // 1: "lca"
  uint32_t rank_mask = 0;      // bit r: GetTaxRankString(r) equals the level (r < 31; codes above print "no rank", as code 0 does)
};
PromoteLevel promote_parse_level(const char *level);
std::vector<uint32_t> promote_depths(const std::vector<uint64_t> &parent);

CFR_HD inline bool promote_rank_matches(const PromoteLevel &L, uint8_t rank) { return ((L.rank_mask >> (rank < 31 ? rank : 0)) & 1u) != 0; }

// PromoteTaxId over compact ids: the node `c` promotes to (c itself when the walk finds nothing, or something with an original id <= 1)
CFR_HD inline uint32_t promote_walk(const PromoteTables &T, const PromoteLevel &L, uint64_t c) {
  uint64_t v = c;
  for (uint64_t guard = 0; guard <= T.node_cnt; ++guard) {
    const uint64_t o = T.orig[v];
    if (o == 0) break;
    if (promote_rank_matches(L, T.rank[v])) return o <= 1 ? (uint32_t)c : (uint32_t)v;
    if (o <= 1) break;
    const uint64_t p = T.parent[v];
    if (p == v || p >= T.node_cnt) break;
    v = p;
  }
  return (uint32_t)c;
}

CFR_HD inline uint64_t promote_match_node(const PromoteTables &T, const cfr_match &m) {
  if (m.kind != 0) return m.id < T.node_cnt ? m.id : T.node_cnt;
  const uint64_t c = m.id < T.seq_cnt ? T.seq_to_tax[m.id] : T.node_cnt;
  return c < T.node_cnt ? c : T.root;
}

// rank mode for one read, in place; promo: the table of k_promote_table.  src (may be null): src[kept slot] = the slot it came from
CFR_HD inline void promote_read_rank(const PromoteTables &T, const uint32_t *promo, cfr_result &r, cfr_match *m, uint64_t base, uint64_t *src) {
  const int32_t nm = r.n_match;
  if (nm <= 0) return;
  int32_t kept = 0;
  for (int32_t j = 0; j < nm; ++j) {
    cfr_match out = m[base + j];
    const uint64_t c = promote_match_node(T, out);
    if (c < T.node_cnt) {
      const uint64_t p = promo[c];
      out.id = p; out.taxid = T.orig[p]; out.kind = 1; out.pad = 0;
    }
    bool dup = false;
    for (int32_t q = 0; q < kept; ++q) if (m[base + q].taxid == out.taxid) { dup = true; break; }
    if (dup) continue;
    m[base + kept] = out;
    if (src) src[base + kept] = base + (uint64_t)j;
    ++kept;
  }
  r.n_match = kept;
}

// the script's lca(a, b) for two nodes; T.node_cnt = the literal tax id 1
CFR_HD inline uint64_t promote_lca_nodes(const PromoteTables &T, uint64_t a, uint64_t b) {
  uint32_t da = T.depth[a], db = T.depth[b];
  for (; da > db; --da) { if (T.orig[a] == 0) return T.node_cnt; a = T.parent[a]; }     // (a's path ends at an id below 1: `while ($a ge 1)`)
  for (; db > da; --db) { if (T.orig[b] <= 1) return T.node_cnt; b = T.parent[b]; }     // (`while ($b > 1)`)
  while (a != b) {
    if (da == 0 || T.orig[a] == 0 || T.orig[b] <= 1) return T.node_cnt;                 // (two trees: no common ancestor)
    a = T.parent[a]; b = T.parent[b]; --da;
  }
  return T.orig[a] > 1 ? a : T.node_cnt;
}

// lca mode for one read, in place
CFR_HD inline void promote_read_lca(const PromoteTables &T, cfr_result &r, cfr_match *m, uint64_t base, uint64_t *src) {
  const int32_t nm = r.n_match;
  if (nm <= 0) return;
  const cfr_match first = m[base];
  uint64_t node = promote_match_node(T, first);
  const uint64_t first_taxid = node < T.node_cnt ? T.orig[node] : first.taxid;
  uint64_t taxid = first_taxid;
  for (int32_t j = 1; j < nm; ++j) {
    const cfr_match mb = m[base + j];
    const uint64_t nb = promote_match_node(T, mb);
    const uint64_t tb = nb < T.node_cnt ? T.orig[nb] : mb.taxid;
    if (taxid == 0) { taxid = tb; node = nb; continue; }
    if (tb == 0 || tb == taxid) continue;
    uint64_t x = T.node_cnt;
    if (node < T.node_cnt && nb < T.node_cnt) x = promote_lca_nodes(T, node, nb);
    if (x < T.node_cnt) { node = x; taxid = T.orig[x]; }
    else { node = T.one_node; taxid = 1; }
  }
  if (taxid != first_taxid) {
    cfr_match out;
    out.id = node; out.taxid = taxid; out.kind = 1; out.pad = 0;
    m[base] = out;
  }
  if (src) src[base] = base;
  r.n_match = 1;
}

}  // namespace cfr
