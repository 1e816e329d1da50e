// cfr_kreport.cpp — the host twin of centrifuger-kreport, its file readers, the clade roll-up and the report writer: the handle behind
// cfr_kreport_* (semantics: cfr_kreport_core.hpp).
#include "cfr_kreport.hpp"

#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <unordered_map>

#include "cfr_device.hpp"
#include "cfr_quant.hpp"
#include "cfr_threads.hpp"

namespace cfr {

namespace {

constexpr size_t kChunkReads = 1u << 20;      // reads handed to add_results at a time by add_tsv

// a line reader over zlib (plain files pass through), "-": stdin; lines of any length, without their newline
class Lines {
 public:
  explicit Lines(const std::string &path) : buf_(1u << 20) {
    gz_ = path == "-" ? gzdopen(0, "rb") : gzopen(path.c_str(), "rb");
    if (!gz_) throw IoError{"cfr_kreport: cannot open " + path};
    gzbuffer(gz_, 1u << 20);
    stdin_ = path == "-";
  }
  ~Lines() { if (gz_) { if (stdin_) (void)gzclose_r(gz_); else gzclose(gz_); } }
  bool next(std::string &line) {
    line.clear();
    bool any = false;                          // (a last line without a newline is a line)
    for (;;) {
      if (at_ == have_) {
        const int got = gzread(gz_, buf_.data(), (unsigned)buf_.size());
        if (got < 0) throw IoError{"cfr_kreport: read error"};
        if (got == 0) return any;
        at_ = 0; have_ = (size_t)got;
      }
      const char *nl = (const char *)memchr(buf_.data() + at_, '\n', have_ - at_);
      const size_t end = nl ? (size_t)(nl - buf_.data()) : have_;
      line.append(buf_.data() + at_, end - at_);
      any = true;
      at_ = nl ? end + 1 : have_;
      if (nl) return true;
    }
  }

 private:
  gzFile gz_ = nullptr;
  bool stdin_ = false;
  std::vector<char> buf_;
  size_t at_ = 0, have_ = 0;
};

// column k of a tab-separated line ("" behind the last one)
inline void column(const std::string &l, int k, const char *&b, const char *&e) {
  const char *p = l.data(), *end = l.data() + l.size();
  for (; k > 0 && p < end; --k) { const char *t = (const char *)memchr(p, '\t', (size_t)(end - p)); p = t ? t + 1 : end; if (!t) { b = e = end; return; } }
  const char *t = (const char *)memchr(p, '\t', (size_t)(end - p));
  b = p; e = t ? t : end;
}
inline uint64_t to_u64(const char *b, const char *e) {
  uint64_t v = 0;
  for (; b < e && *b >= '0' && *b <= '9'; ++b) v = v * 10 + (uint64_t)(*b - '0');
  return v;
}
inline int64_t to_i64(const char *b, const char *e) {
  const bool neg = b < e && *b == '-';
  const int64_t v = (int64_t)to_u64(b + (neg ? 1 : 0), e);
  return neg ? -v : v;
}

const char *rank_code(const char *rank) {
  static const char *const table[][2] = {{"species", "S"}, {"genus", "G"}, {"family", "F"}, {"order", "O"}, {"class", "C"}, {"phylum", "P"},
                                         {"kingdom", "K"}, {"superkingdom", "D"}, {"domain", "D"}, {"acellular root", "D"}};
  for (const auto &t : table) if (!strcmp(rank, t[0])) return t[1];
  return "-";
}

}  // namespace

struct Kreport::Rollup {
  std::vector<uint64_t> own, clade, own_score, clade_score;
  std::vector<double> own_d, clade_d;          // the fraction modes
  double seq = 0;
  std::vector<uint64_t> child_begin, child;    // children of every node in compact order, as the script's child_lists
};

Kreport::Kreport(const std::string &prefix, const KreportOptions &opt, int device, unsigned max_blocks, uint32_t slots, int threads) : opt_(opt), threads_(threads) {
  load_taxonomy(prefix + ".2.cfr", tax_);
  const uint64_t nc = tax_.node_cnt;
  if (nc >= 0xfffffffeull) throw FormatError{"cfr_kreport: a taxonomy of 2^32 nodes or more"};
  for (uint64_t i = 0; i < nc; ++i)
    if (tax_.parent[i] >= nc) throw FormatError{"cfr_kreport: " + prefix + ".2.cfr: the parent of node " + std::to_string(i) + " is outside the tree"};
  depth_ = promote_depths(tax_.parent);
  one_node_ = nc;
  for (uint64_t i = 0; i < nc; ++i) if (tax_.orig_taxid[i] == 1) one_node_ = i;
  if (one_node_ >= nc) throw FormatError{"cfr_kreport: " + prefix + ".2.cfr holds no node with tax id 1: the report is the tree below that node"};
  count_.assign(nc + 1, 0); score_.assign(nc + 1, 0); frac_.assign(nc + 1, 0.0);
  if (device >= 0) dev_.reset(make_kreport_device(device, tax_, depth_, one_node_, opt_, max_blocks, slots));
}

Kreport::~Kreport() {}

PromoteTables Kreport::tables() const {
  return PromoteTables{tax_.parent.data(), tax_.orig_taxid.data(), tax_.seq_to_tax.data(), tax_.rank.data(), depth_.data(),
                       tax_.node_cnt, tax_.seq_cnt, tax_.root, one_node_};
}

// The script's lines on stderr for these reads, in its order: isTaxIDInTree prints one for a first tax id above 1 that is no node;
// lca() prints one for its first argument when that is no node (only an unknown id handed through by a leading 0) and one for its
// second when that is no node and above 1 (:210-220).  A dropped read prints nothing.
void Kreport::read_warnings(const cfr_result *results, const cfr_match *matches, size_t n) {
  const PromoteTables T = tables();
  const uint64_t nc = T.node_cnt;
  for (size_t i = 0; i < n; ++i) {
    const cfr_result &r = results[i];
    const int32_t nm = r.n_match;
    if (nm <= 0) continue;
    if (opt_.has_min_length && (int64_t)r.hit_length < opt_.min_length) continue;
    if (opt_.has_min_score && r.score < opt_.min_score) continue;
    const cfr_match *m = matches + r.match_begin;
    bool any = false;
    for (int32_t j = 0; j < nm && !any; ++j) any = promote_match_node(T, m[j]) >= nc;
    if (!any) continue;                      // (every id is a node, and so is every result: nothing to print)
    uint64_t node = promote_match_node(T, m[0]);
    uint64_t taxid = node < nc ? T.orig[node] : m[0].taxid;
    if (node >= nc && taxid > 1) warnings_.push_back(taxid);
    if (node >= nc && taxid >= 1) { node = one_node_; taxid = 1; }
    for (int32_t j = 1; j < nm; ++j) {
      const uint64_t nb = promote_match_node(T, m[j]);
      const uint64_t tb = nb < nc ? T.orig[nb] : m[j].taxid;
      if (taxid == 0) { taxid = tb; node = nb; continue; }
      if (tb == 0 || tb == taxid) continue;
      if (node >= nc) warnings_.push_back(taxid);
      if (nb >= nc && tb > 1) warnings_.push_back(tb);
      uint64_t x = nc;
      if (node < nc && nb < nc) x = promote_lca_nodes(T, node, nb);
      if (x < nc) { node = x; taxid = T.orig[x]; }
      else { node = one_node_; taxid = 1; }
    }
  }
}

void Kreport::add_results(const cfr_result *results, const cfr_match *matches, size_t n) {
  if (opt_.no_lca) throw std::runtime_error("cfr_kreport_add_results: --no-lca adds fractions row by row in file order: it takes a file (cfr_kreport_add_tsv)");
  if (n == 0) return;
  read_warnings(results, matches, n);
  if (dev_) {
    uint64_t extent = 0;
    for (size_t i = 0; i < n; ++i) if (results[i].n_match > 0) extent = std::max<uint64_t>(extent, results[i].match_begin + (uint64_t)results[i].n_match);
    dev_->add(results, matches, n, extent);
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const int threads = threads_ > 0 ? threads_ : (int)std::min(std::max(std::thread::hardware_concurrency(), 1u), 16u);
  const int nth = n < 4096 ? 1 : threads;
  const PromoteTables T = tables();
  const size_t nb = (size_t)T.node_cnt + 1;
  // per-thread bins, summed: the first thread writes into the handle's own
  std::vector<std::vector<uint64_t>> cnt((size_t)nth - 1, std::vector<uint64_t>(nb, 0)), sc((size_t)nth - 1, std::vector<uint64_t>(nb, 0));
  parallel_slices(n, nth, [&](size_t lo, size_t hi, int tid) {
    uint64_t *c = tid ? cnt[(size_t)tid - 1].data() : count_.data(), *s = tid ? sc[(size_t)tid - 1].data() : score_.data();
    for (size_t i = lo; i < hi; ++i) {
      const uint32_t b = kreport_read_bin(T, opt_, results[i], matches, results[i].match_begin);
      if (b == kKreportDropped) continue;
      ++c[b];
      if (results[i].score > s[b]) s[b] = results[i].score;
    }
  });
  for (size_t t = 0; t + 1 < (size_t)nth; ++t)
    for (size_t b = 0; b < nb; ++b) { count_[b] += cnt[t][b]; score_[b] = std::max(score_[b], sc[t][b]); }
  host_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void Kreport::add_counts(const uint64_t *own, const uint64_t *own_score, size_t n) {
  if (n != count_.size()) throw std::runtime_error("cfr_kreport_add_counts: the arrays hold node_cnt + 1 entries");
  for (size_t b = 0; b < n; ++b) { count_[b] += own[b]; if (own_score) score_[b] = std::max(score_[b], own_score[b]); }
}

void Kreport::add_tsv(const std::string &path) {
  const auto t0 = std::chrono::steady_clock::now();
  double inner_ms = 0;
  Lines in(path);
  std::string line;
  if (!in.next(line)) { parse_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); return; }
  // the header maps names to positions (a later column with the same name wins, as in the script's hash)
  int c_tax = -1, c_score = -1, c_len = -1, c_num = -1;
  {
    int k = 0;
    size_t p = 0;
    for (;;) {
      const size_t t = line.find('\t', p);
      const std::string name = line.substr(p, t == std::string::npos ? std::string::npos : t - p);
      if (name == "taxID") c_tax = k; else if (name == "score") c_score = k; else if (name == "hitLength") c_len = k; else if (name == "numMatches") c_num = k;
      if (t == std::string::npos) break;
      p = t + 1; ++k;
    }
  }
  if (c_tax < 0 || c_score < 0 || c_len < 0 || c_num < 0)
    throw FormatError{"cfr_kreport: " + path + ": the header line names no taxID, score, hitLength or numMatches column"};
  std::unordered_map<uint64_t, uint32_t> to_compact;
  const uint64_t nc = tax_.node_cnt;
  for (uint64_t i = 0; i < nc; ++i) to_compact[tax_.orig_taxid[i]] = (uint32_t)i;       // (a later duplicate wins, as in the script's hashes)
  auto node_of = [&](uint64_t taxid) -> uint64_t {
    if (!taxid) return nc;
    const auto it = to_compact.find(taxid);
    return it == to_compact.end() ? nc : it->second;
  };
  std::vector<cfr_result> results;
  std::vector<cfr_match> matches;
  auto flush = [&]() {
    if (results.empty()) return;
    const auto a = std::chrono::steady_clock::now();
    add_results(results.data(), matches.data(), results.size());
    inner_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    results.clear(); matches.clear();
  };
  uint64_t remaining = 0;                      // rows the open group still swallows
  const char *b, *e;
  while (in.next(line)) {
    column(line, c_tax, b, e);
    const uint64_t taxid = to_u64(b, e);
    if (remaining) {                           // swallowed unfiltered: only its tax id counts
      matches.push_back(cfr_match{node_of(taxid), taxid, 1, 0});
      --remaining;
      continue;
    }
    column(line, c_score, b, e);
    const uint64_t score = to_u64(b, e);
    column(line, c_len, b, e);
    const int64_t len = to_i64(b, e);
    column(line, c_num, b, e);
    const uint64_t num = to_u64(b, e);
    if (opt_.has_min_length && len < opt_.min_length) continue;
    if (opt_.has_min_score && score < opt_.min_score) continue;
    if (opt_.no_lca) {                         // one thread, row order: the sum of the fractions depends on it
      if (!num) throw FormatError{"cfr_kreport: " + path + ": a row with numMatches 0 (the script divides by it)"};
      uint64_t node = node_of(taxid);
      if (node >= nc && taxid > 1) warnings_.push_back(taxid);
      const size_t bin = taxid == 0 ? (size_t)nc : (size_t)(node < nc ? node : one_node_);
      frac_[bin] += 1.0 / (double)num;
      frac_seq_ += 1.0 / (double)num;
      frac_mode_ = true;
      continue;
    }
    if (results.size() >= kChunkReads) flush();
    cfr_result r{};
    r.score = score;
    r.hit_length = (int32_t)std::max<int64_t>(std::min<int64_t>(len, INT32_MAX), INT32_MIN);
    r.n_match = (int32_t)std::min<uint64_t>(std::max<uint64_t>(num, 1), INT32_MAX);
    r.match_begin = matches.size();
    results.push_back(r);
    matches.push_back(cfr_match{node_of(taxid), taxid, 1, 0});
    remaining = (uint64_t)r.n_match - 1;
  }
  if (remaining) throw FormatError{"cfr_kreport: " + path + " ends inside a row group: " + std::to_string(remaining) + " more rows were announced by numMatches"};
  flush();
  parse_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - inner_ms;
}

// rows of `taxID count`, split on white space; a later row for an id replaces the earlier one, seq_count takes every row (:77-81)
void Kreport::add_count_table(const std::string &path) {
  const auto t0 = std::chrono::steady_clock::now();
  Lines in(path);
  std::string line;
  std::unordered_map<uint64_t, uint32_t> to_compact;
  const uint64_t nc = tax_.node_cnt;
  for (uint64_t i = 0; i < nc; ++i) to_compact[tax_.orig_taxid[i]] = (uint32_t)i;
  while (in.next(line)) {
    const char *p = line.c_str();
    while (*p == ' ' || *p == '\t' || *p == '\r') ++p;
    if (!*p) continue;
    const char *q = p;
    while (*q && *q != ' ' && *q != '\t' && *q != '\r') ++q;
    const uint64_t taxid = to_u64(p, q);
    const double count = strtod(q, nullptr);
    frac_mode_ = true;
    frac_seq_ += count;
    if (taxid == 0) { frac_[nc] = count; continue; }
    const auto it = to_compact.find(taxid);
    if (it != to_compact.end()) frac_[it->second] = count;      // (an id the tree lacks is counted and printed nowhere)
  }
  parse_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Clade sums on the host: dfs_summation(1) adds every child's finished clade to its parent in child order, which one pass over the
// post-order of the tree below node 1 does in the same order (that matters for the doubles of the fraction modes only).  Node 1's
// own parent entry is forced to 0 by the script, so node 1 is nobody's child.
void Kreport::rollup(Rollup &r) {
  const uint64_t nc = tax_.node_cnt;
  r.own = count_; r.own_score = score_;
  if (dev_) {
    std::vector<uint64_t> c(nc + 1), s(nc + 1);
    dev_->download(c.data(), s.data());
    for (uint64_t b = 0; b <= nc; ++b) { r.own[b] += c[b]; r.own_score[b] = std::max(r.own_score[b], s[b]); }
  }
  r.seq = frac_seq_;
  for (uint64_t b = 0; b <= nc; ++b) r.seq += (double)r.own[b];
  r.child_begin.assign(nc + 1, 0);
  auto is_child = [&](uint64_t i) { return i != one_node_ && tax_.parent[i] != i; };
  // (child_begin[p + 1] counts p's children; p < nc was checked when the handle was opened)
  for (uint64_t i = 0; i < nc; ++i) if (is_child(i)) ++r.child_begin[tax_.parent[i] + 1];
  for (uint64_t i = 0; i < nc; ++i) r.child_begin[i + 1] += r.child_begin[i];
  r.child.resize(r.child_begin[nc]);
  {
    std::vector<uint64_t> at(r.child_begin.begin(), r.child_begin.end() - 1);
    for (uint64_t i = 0; i < nc; ++i) if (is_child(i)) r.child[at[tax_.parent[i]]++] = i;
  }
  r.clade = r.own; r.clade_score = r.own_score;
  if (frac_mode_) { r.own_d.resize(nc + 1); for (uint64_t b = 0; b <= nc; ++b) r.own_d[b] = frac_[b] + (double)r.own[b]; r.clade_d = r.own_d; }
  // post-order below node 1, iteratively: (node, next child)
  std::vector<std::pair<uint64_t, uint64_t>> stack;
  std::vector<uint8_t> seen(nc, 0);
  stack.emplace_back(one_node_, r.child_begin[one_node_]);
  seen[one_node_] = 1;
  while (!stack.empty()) {
    auto &top = stack.back();
    if (top.second < r.child_begin[top.first + 1]) {
      const uint64_t c = r.child[top.second++];
      if (!seen[c]) { seen[c] = 1; stack.emplace_back(c, r.child_begin[c]); }
      continue;
    }
    const uint64_t v = top.first;
    stack.pop_back();
    if (stack.empty()) break;
    const uint64_t p = stack.back().first;
    r.clade[p] += r.clade[v];
    r.clade_score[p] = std::max(r.clade_score[p], r.clade_score[v]);
    if (frac_mode_) r.clade_d[p] += r.clade_d[v];
  }
}

void Kreport::counts(std::vector<uint64_t> &own, std::vector<uint64_t> &clade, std::vector<uint64_t> &own_score, std::vector<uint64_t> &clade_score,
                     double &seq_count) {
  Rollup r;
  rollup(r);
  if (frac_mode_) {
    for (size_t b = 0; b < r.own.size(); ++b) { r.own[b] = (uint64_t)r.own_d[b]; r.clade[b] = (uint64_t)r.clade_d[b]; }
  }
  own = std::move(r.own); clade = std::move(r.clade); own_score = std::move(r.own_score); clade_score = std::move(r.clade_score);
  seq_count = r.seq;
}

void Kreport::write(const char *path) {
  Rollup r;
  rollup(r);
  if (!(r.seq > 0)) throw std::runtime_error("No sequence matches with given settings");      // (before the file is made)
  const bool to_stdout = !path || !strcmp(path, "-");
  FILE *out = to_stdout ? stdout : fopen(path, "wb");
  if (!out) throw IoError{std::string("cfr_kreport_write: cannot write ") + path};
  struct Close { FILE *f; bool own; ~Close() { if (own) fclose(f); } } close{out, !to_stdout};
  const uint64_t nc = tax_.node_cnt;
  const bool fr = frac_mode_;
  auto clade_of = [&](uint64_t b) { return fr ? r.clade_d[b] : (double)r.clade[b]; };
  auto line = [&](uint64_t b, const char *code, uint64_t taxid, uint32_t depth, const char *name, bool unclassified) {
    // count * 100 / seq_count in doubles (the integers of the default mode are exact in them)
    fprintf(out, "%6.2f\t%lld\t%lld\t%s\t%llu\t", clade_of(b) * 100 / r.seq, fr ? (long long)r.clade_d[b] : (long long)r.clade[b],
            fr ? (long long)r.own_d[b] : (long long)r.own[b], code, (unsigned long long)taxid);
    for (uint32_t d = 0; d < depth; ++d) fputs("  ", out);
    fputs(name, out);
    if (opt_.score_data) fprintf(out, "\t%llu", unclassified ? 0ull : (unsigned long long)r.clade_score[b]);
    fputc('\n', out);
  };
  line(nc, "U", 0, 0, "unclassified", true);
  // pre-order from node 1, children by clade count, largest first; the sort is stable like Perl's, so ties keep compact order
  struct Frame { uint64_t node; uint32_t depth; };
  std::vector<Frame> stack{{one_node_, 0}};
  std::vector<uint8_t> seen(nc, 0);
  std::vector<uint64_t> kids;
  while (!stack.empty()) {
    const Frame f = stack.back();
    stack.pop_back();
    if (seen[f.node]) continue;
    seen[f.node] = 1;
    if (clade_of(f.node) == 0 && !opt_.show_zeros) continue;
    line(f.node, rank_code(quant_rank_string(tax_.rank[f.node])), tax_.orig_taxid[f.node], f.depth, tax_.tax_name[f.node].c_str(), false);
    kids.assign(r.child.begin() + (ptrdiff_t)r.child_begin[f.node], r.child.begin() + (ptrdiff_t)r.child_begin[f.node + 1]);
    std::stable_sort(kids.begin(), kids.end(), [&](uint64_t a, uint64_t b) { return clade_of(a) > clade_of(b); });
    for (size_t k = kids.size(); k-- > 0;) stack.push_back(Frame{kids[k], f.depth + 1});
  }
  fflush(out);
}

}  // namespace cfr
