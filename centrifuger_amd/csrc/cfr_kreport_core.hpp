// cfr_kreport_core.hpp — centrifuger-kreport: the Kraken-style report of a classification, reads counted per taxon.  The statement
// of record is the reference's Perl script (centrifuger-kreport, all of it); this header restates its per-read rules on compact tax
// ids, once, for the host twin (cfr_kreport.cpp) and for the kernels (cfr_kreport.hip).
//
// Bins.  node_cnt + 1 of them: the compact nodes, then one for "unclassified" (tax id 0).  Every read that survives the filters
// lands in exactly one bin and adds 1 to seq_count; with --report-score-data its score is maximised into the bin.
//
// A read is a row group of the TSV (the script groups by numMatches: a row with m > 1 swallows the next m - 1 lines; here that is
// n_match), its score and hit length are those of its first row (cfr_result::score, ::hit_length).  Per read (:102-132):
//   dropped when hit_length < min_length or score < min_score (each only when the option was given).  An unclassified read
//   (n_match <= 0) is one row with tax id 0: it goes through the same filters and lands in the "unclassified" bin.
//   The first tax id becomes 1 when it is no node of the tree (isTaxIDInTree, :186-200; every node of the image has its parent in
//   the image, so the walk of a node never fails).  Then lca() (:202-227) is folded over the further tax ids.  It is line for line
//   the lca() of centrifuger-promote, and so is the fold here (promote_lca_nodes, cfr_promote_core.hpp).
//   Whether the "becomes 1" step changes a result: it does.  Promote's fold keeps an unknown first id u when every further id is u
//   or 0 (`return $a if $a eq $b`), kreport has replaced it by 1 before.  In every other case an unknown first id gives 1 from the
//   first real lca() call on.  The step also prints a line of its own on stderr (kreport_read_warnings).
//   The bin of the fold's result: tax id 0 -> "unclassified"; a node -> that node; the literal 1 -> the node of tax id 1.
//
// Deliberate differences from the script:
//   * One input file or stdin.  The script's `<>` over several files takes the second file's header for a data row; the command
//     line refuses more than one file.
//   * An index whose taxonomy has no node with original id 1 is refused (FormatError): the script prints a nameless line and Perl
//     warnings there.
//   * A row group whose first tax id is 0 and that holds a tax id the tree lacks can end the script's fold on that unknown id
//     (lca(0, u) = u); the script then counts the read in seq_count and prints it nowhere.  Here such a read goes to the node of
//     tax id 1, like every other id the tree lacks.  The classifier writes no such group (a classified read has no tax id 0 row).
//   * A file that ends inside a row group is refused (FormatError).  In the script the inner `<>` returns undef there (Perl warnings,
//     lca(taxid, undef) gives 1), and the next `<>`, its file list used up, goes on to read standard input: run from a terminal it
//     waits for ever.  Nothing of that is worth matching.
//   * A header line that names no taxID, score, hitLength or numMatches column is refused; the script would read column 0 for it.
//
// --no-lca and --is-count-table add fractions in file order and print them truncated; the result depends on the order of the
// sum, so both run on the host, one thread, in cfr_kreport.cpp and never here.
#pragma once

#include "cfr_promote_core.hpp"

namespace cfr {

struct KreportOptions {
  bool has_min_score = false, has_min_length = false;
  uint64_t min_score = 0;
  int64_t min_length = 0;
  bool no_lca = false, show_zeros = false, score_data = false;
};

constexpr uint32_t kKreportDropped = 0xffffffffu;

// the bin of one read (kKreportDropped: filtered out); T.one_node < T.node_cnt is the caller's to check
CFR_HD inline uint32_t kreport_read_bin(const PromoteTables &T, const KreportOptions &opt, const cfr_result &r, const cfr_match *m, uint64_t base) {
  if (opt.has_min_length && (int64_t)r.hit_length < opt.min_length) return kKreportDropped;
  if (opt.has_min_score && r.score < opt.min_score) return kKreportDropped;
  const int32_t nm = r.n_match;
  if (nm <= 0) return (uint32_t)T.node_cnt;
  const cfr_match first = m[base];
  uint64_t node = promote_match_node(T, first);
  uint64_t taxid = node < T.node_cnt ? T.orig[node] : first.taxid;
  if (node >= T.node_cnt && taxid >= 1) { node = T.one_node; taxid = 1; }      // isTaxIDInTree failed (or the literal 1)
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
  if (taxid == 0) return (uint32_t)T.node_cnt;
  return (uint32_t)(node < T.node_cnt ? node : T.one_node);
}

}  // namespace cfr
