// cfr_quant.cpp — the host twin of centrifuger-quant: reader, coalesce, EM and the four reports.
//
// Steps and where the reference has them:
//   rows -> read assignments        Quantifier::LoadReadAssignments   Quantifier.hpp:515-622   (add_tsv / add_results)
//   equal target lists merged       CoalesceAssignments               :490-513                 (QuantCoalescer + the sort in finish_coalesce)
//   genome length per tax id        ConvertSeqLengthToTaxLength,      Taxonomy.hpp:1111-1213   (the constructor)
//                                   InferAllTaxLength
//   covered subtree, EM             Quantification, EMupdate,         Quantifier.hpp:123-281,  (run)
//                                   EstimateAbundanceWithEM           640-743
//   reports                         Output, OutputKreportDFS          :353-399, 746-818        (write)
// Every double sum is written in the reference's order of operations; this file is compiled with -ffp-contract=off (the
// reference is built with -O3 -msse4.2: no fused multiply-add, no reassociation), so the bits agree.  The weight of a read is
// 4^-d with d <= 11 and the counts are integers, so the coalesce step sums integers (weights in units of 2^-22) and is exact in
// any order - that is what lets it run with atomics on the device.
#include "cfr_quant.hpp"
#include "cfr_threads.hpp"

#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <thread>
#include <unistd.h>

namespace cfr {

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

enum { R_UNKNOWN = 0, R_STRAIN = 1, R_SPECIES, R_GENUS, R_FAMILY, R_ORDER, R_CLASS, R_PHYLUM, R_KINGDOM, R_DOMAIN, R_SUPER_KINGDOM = 24, R_ACELLULAR_ROOT = 30 };
}  // namespace

const char *quant_rank_string(uint8_t rank) {   // Taxonomy::GetTaxRankString (Taxonomy.hpp:497-532), in the order of the rank enum (:25-59)
  static const char *const names[31] = {"no rank", "strain", "species", "genus", "family", "order", "class", "phylum", "kingdom", "domain",
      "forma", "infraclass", "infraorder", "parvorder", "subclass", "subfamily", "subgenus", "subkingdom", "suborder", "subphylum",
      "subspecies", "subtribe", "superclass", "superfamily", "superkingdom", "superorder", "superphylum", "tribe", "varietas", "life",
      "acellular root"};
  return rank < 31 ? names[rank] : "no rank";
}

bool quant_next_seq_same_genome(const char *a, const char *b) {
  uint64_t id[2];
  for (int i = 0; i < 2; ++i) {
    const char *s = i ? b : a;
    int j;
    id[i] = 0;
    for (j = 0; s[j]; ++j) if (s[j] >= '0' && s[j] <= '9') break;
    for (; s[j]; ++j) {
      if (s[j] >= '0' && s[j] <= '9') id[i] = id[i] * 10 + s[j] - '0';
      else break;
    }
    if (j < 3 || s[2] != '_') return false;   // the prefix should look like ab_
  }
  return id[1] == id[0] + 1;
}

uint32_t quant_weight_exp(uint64_t hit_length, uint64_t read_length) {
  int diff = (int)(read_length - hit_length);
  if (diff < int(read_length * 0.01)) return 0;
  diff -= int(read_length * 0.01);
  if (diff > 10) diff = 11;
  return (uint32_t)diff;
}

// ---- Tree_Plain (compactds/Tree_Plain.hpp): first child / next sibling, `root` doubles as "none"; AddEdge appends to the
// end of the sibling chain, so children come out in the order their edges were added ----
struct Quant::PlainTree {
  struct Node { size_t parent, sibling, child, last_child; };
  std::vector<Node> nodes;
  size_t root = 0;
  void init(size_t n, size_t r) { root = r; nodes.assign(n, Node{r, r, r, r}); }
  void add_edge(size_t c, size_t parent) {
    nodes[c].parent = parent;
    size_t last = nodes[parent].last_child;
    if (last == root) nodes[parent].child = c; else nodes[last].sibling = c;
    nodes[parent].last_child = c;
  }
  std::vector<size_t> children(size_t v) const {
    std::vector<size_t> ret;
    for (size_t c = nodes[v].child; c != root; c = nodes[c].sibling) ret.push_back(c);
    return ret;
  }
};

namespace {
using Tree = std::vector<std::vector<size_t>>;   // children of every node, in Tree_Plain::GetChildren order

// GenerateTreeAbundance (Quantifier.hpp:123-133)
double tree_abundance(size_t tag, double *abund, const Tree &ch) {
  double sum = abund[tag];
  for (size_t c : ch[tag]) sum += tree_abundance(c, abund, ch);
  return abund[tag] = sum;
}

// RedistributeAbundToChildren (Quantifier.hpp:136-182) with treeEdgeWeight == NULL: expandedChildSum stays 0
void redistribute(size_t tag, double *abund, const Tree &ch, const uint64_t *len) {
  const std::vector<size_t> &children = ch[tag];
  const size_t csize = children.size();
  double childrenSum = 0, weightedChildrenSum = 0;
  for (size_t i = 0; i < csize; ++i) childrenSum += abund[children[i]];
  double excess = abund[tag] - childrenSum;
  if (excess < 0) excess = 0;
  if (childrenSum == 0) return;
  const double expandedChildSum = 0;
  for (size_t i = 0; i < csize; ++i)
    weightedChildrenSum += abund[children[i]] / (len ? len[children[i]] : (uint64_t)1) * ((excess - expandedChildSum) / csize + 0.0);
  if (weightedChildrenSum == 0) weightedChildrenSum = 1;
  for (size_t i = 0; i < csize; ++i) {
    abund[children[i]] += excess * (abund[children[i]] / (len ? len[children[i]] : (uint64_t)1) * ((excess - expandedChildSum) / csize + 0.0)) / weightedChildrenSum;
    redistribute(children[i], abund, ch, len);
  }
}

// ---- host coalesce: a hash map keyed on the list ----
class HostCoalescer : public QuantCoalescer {
 public:
  void add(const QuantRecords &r) override {
    std::string key;
    for (size_t i = 0; i < r.n(); ++i) {
      const uint32_t *w = r.words.data() + r.off[i];
      const uint32_t nt = w[0], meta = w[1 + nt];
      key.assign((const char *)(w + 1), (size_t)nt * 4);
      auto it = map_.find(key);
      if (it == map_.end()) { it = map_.emplace(key, acc_.size() / 3).first; acc_.insert(acc_.end(), 3, 0); }
      uint64_t *a = acc_.data() + it->second * 3;
      a[0] += quant_weight_units(meta); a[1] += 1; a[2] += (meta >> 8) & 1;
    }
  }
  void finish(QuantAssignments &out) override {
    out = QuantAssignments();
    for (const auto &kv : map_) {
      const uint32_t *t = (const uint32_t *)kv.first.data();
      out.targets.insert(out.targets.end(), t, t + kv.first.size() / 4);
      out.begin.push_back(out.targets.size());
      const uint64_t *a = acc_.data() + kv.second * 3;
      out.weight_units.push_back(a[0]); out.count.push_back(a[1]); out.uniq.push_back(a[2]);
    }
  }
 private:
  std::unordered_map<std::string, size_t> map_;
  std::vector<uint64_t> acc_;
};

class HostEStep : public QuantEStep {
 public:
  explicit HostEStep(const QuantCsr &c) : c_(c) {}
  // the loop of EMupdate as it stands (Quantifier.hpp:196-208): readCount[t] receives its terms in (assignment, slot) order
  void run(const double *abund, bool init, double *read_count) override {
    memset(read_count, 0, sizeof(double) * c_.n_nodes);
    const size_t na = c_.a_begin.size() - 1;
    for (size_t i = 0; i < na; ++i) {
      const uint32_t *t = c_.a_target.data() + c_.a_begin[i];
      const size_t cnt = c_.a_begin[i + 1] - c_.a_begin[i];
      if (init) {
        for (size_t j = 0; j < cnt; ++j) read_count[t[j]] += c_.a_weight[i] / (double)cnt;
      } else {
        double sum = 0;
        for (size_t j = 0; j < cnt; ++j) sum += abund[t[j]];
        for (size_t j = 0; j < cnt; ++j) read_count[t[j]] += c_.a_weight[i] * abund[t[j]] / sum;
      }
    }
  }
 private:
  const QuantCsr &c_;
};

// ---- TSV rows ----
struct Row { const char *id; size_t id_len; uint64_t taxid, score, second, hit, len; };

inline bool parse_uint(const char *&p, const char *e, uint64_t &v) {
  while (p < e && (*p == '\t' || *p == ' ')) ++p;
  if (p >= e || *p < '0' || *p > '9') return false;
  v = 0;
  while (p < e && *p >= '0' && *p <= '9') v = v * 10 + (uint64_t)(*p++ - '0');
  return true;
}
// readID \t seqID \t taxID \t score \t 2ndBestScore \t hitLength \t queryLength [\t ...]
inline bool parse_row(const char *b, const char *e, Row &r) {
  const char *t1 = (const char *)memchr(b, '\t', e - b);
  if (!t1 || t1 == b) return false;
  const char *t2 = (const char *)memchr(t1 + 1, '\t', e - t1 - 1);
  if (!t2) return false;
  r.id = b; r.id_len = t1 - b;
  const char *p = t2 + 1;
  return parse_uint(p, e, r.taxid) && parse_uint(p, e, r.score) && parse_uint(p, e, r.second) && parse_uint(p, e, r.hit) && parse_uint(p, e, r.len);
}

struct Group { std::string id; std::vector<uint32_t> targets; uint32_t meta = 0; };
struct Chunk {
  int groups = 0;          // 0: no kept row; 1: `first` only, still open; >= 2: first, mid..., last (open)
  Group first, last;
  QuantRecords mid;
};
}  // namespace

QuantCoalescer *make_host_coalescer() { return new HostCoalescer(); }
QuantEStep *make_host_estep(const QuantCsr &c) { return new HostEStep(c); }

// the node-major order of the terms: for every node its (assignment, slot) occurrences as the sequential loop meets them
void quant_csr_finish(QuantCsr &csr) {
  const size_t ns = csr.n_nodes;
  csr.n_slots = csr.a_target.size();
  csr.node_begin.assign(ns + 1, 0);
  for (uint32_t t : csr.a_target) ++csr.node_begin[t + 1];
  for (size_t i = 0; i < ns; ++i) csr.node_begin[i + 1] += csr.node_begin[i];
  csr.slot_pos.resize(csr.n_slots);
  std::vector<uint64_t> fill(csr.node_begin.begin(), csr.node_begin.end() - 1);
  for (size_t s = 0; s < csr.n_slots; ++s) csr.slot_pos[s] = fill[csr.a_target[s]]++;
}

// Quantifier::Init (Quantifier.hpp:443-457), CentrifugerInspect.cpp:84-90: .3.cfr is pairs of size_t (seqId, length); a later pair
// replaces an earlier one
std::map<uint64_t, uint64_t> read_seq_lengths(const std::string &prefix) {
  std::map<uint64_t, uint64_t> seq_length;
  FILE *fp = fopen((prefix + ".3.cfr").c_str(), "rb");
  if (!fp) throw IoError{"cannot open " + prefix + ".3.cfr"};
  uint64_t tmp[2];
  while (fread(tmp, 8, 2, fp) == 2) seq_length[tmp[0]] = tmp[1];
  fclose(fp);
  return seq_length;
}

// the genome length of every tax id: node_cnt + 1 entries (the last one, for ids the tree does not hold, stays 0)
void tax_genome_lengths(const Taxonomy &tax, const std::map<uint64_t, uint64_t> &seq_length, std::vector<uint64_t> &taxid_length) {
  const size_t nc = tax.node_cnt;
  // ConvertSeqLengthToTaxLength (Taxonomy.hpp:1111-1150).  The names go through MapID::Add (MapID.hpp:30-42): a name seen twice
  // keeps its first id and takes none of its own.
  std::map<std::string, size_t> name_id;
  std::vector<std::string> names;
  for (const std::string &s : tax.seq_name)
    if (name_id.find(s) == name_id.end()) { size_t id = name_id.size(); name_id[s] = id; names.push_back(s); }
  std::sort(names.begin(), names.end());
  auto seq_tax = [&](size_t id) { return id < tax.seq_cnt ? tax.seq_to_tax[id] : (uint64_t)nc; };
  auto seq_len = [&](size_t id) { auto it = seq_length.find(id); return it == seq_length.end() ? (uint64_t)0 : it->second; };
  taxid_length.assign(nc + 1, 0);
  for (size_t i = 0, j; i < names.size(); i = j) {
    const size_t id = name_id[names[i]];
    uint64_t len = seq_len(id);
    const uint64_t taxid = seq_tax(id);
    for (j = i + 1; j < names.size(); ++j) {
      const size_t next = name_id[names[j]];
      if (seq_tax(next) != taxid || !quant_next_seq_same_genome(names[j - 1].c_str(), names[j].c_str())) break;
      len += seq_len(next);
    }
    if (taxid < nc && len > taxid_length[taxid]) taxid_length[taxid] = len;
  }
  // InferAllTaxLength(taxidLength, true) (Taxonomy.hpp:1156-1213)
  {
    std::vector<uint64_t> count(nc, 0), new_len(nc, 0);
    std::vector<char> preset(nc, 0);
    for (size_t i = 0; i < nc; ++i) if (taxid_length[i] != 0) { preset[i] = 1; count[i] = 1; }
    for (size_t i = 0; i < nc; ++i) {
      if (!preset[i]) continue;
      if (i == tax.parent[i] || !tax.leaf[i]) continue;
      size_t p = tax.parent[i];
      for (size_t guard = 0; guard <= nc; ++guard) {
        ++count[p];
        new_len[p] += taxid_length[i];
        if (p == tax.parent[p]) break;
        p = tax.parent[p];
      }
    }
    for (size_t i = 0; i < nc; ++i) {
      uint64_t sum = new_len[i];
      if (preset[i]) sum += taxid_length[i];
      taxid_length[i] = count[i] == 0 ? sum : sum / count[i];
    }
  }
}

Quant::Quant(const std::string &prefix, const QuantOptions &o) : opt_(o) {
  load_taxonomy(prefix + ".2.cfr", tax_);
  const size_t nc = tax_.node_cnt;
  if (nc >= 0xffffffffull) throw FormatError{"cfr_quant: a taxonomy of 2^32 nodes or more"};
  for (size_t i = 0; i < tax_.orig_taxid.size(); ++i) to_compact_[tax_.orig_taxid[i]] = (uint32_t)i;   // MapID::Load (MapID.hpp:83-99): a later duplicate wins

  tax_genome_lengths(tax_, read_seq_lengths(prefix), taxid_length_);
  abund_.assign(nc + 1, 0); read_count_.assign(nc + 1, 0); uniq_count_.assign(nc + 1, 0);
  coalescer_.reset(opt_.device >= 0 ? make_device_coalescer(opt_.device, opt_.table_slots) : make_host_coalescer());
}

Quant::~Quant() {}

void Quant::flush(bool all) {
  const size_t batch = 1u << 20;
  if (pending_.n() == 0 || (!all && pending_.n() < batch && pending_.words.size() < (48u << 20))) return;
  const double t0 = now_ms();
  coalescer_->add(pending_);
  coalesce_ms += now_ms() - t0;
  pending_.clear();
}

void Quant::add_results(const cfr_result *r, const cfr_match *m, size_t n) {
  if (coalesced_) throw std::runtime_error("cfr_quant: assignments were already coalesced");
  const uint64_t min_len = (uint64_t)(int64_t)opt_.min_length;
  std::vector<uint32_t> t;
  for (size_t i = 0; i < n; ++i) {
    if (r[i].n_match <= 0) continue;
    const uint64_t hit = (uint64_t)(int64_t)r[i].hit_length, len = (uint64_t)(int64_t)r[i].query_length;
    if (hit < min_len || r[i].score < opt_.min_score) continue;
    t.clear();
    for (int k = 0; k < r[i].n_match; ++k) {
      const uint64_t taxid = m[r[i].match_begin + k].taxid;
      if (taxid != 0) t.push_back(compact(taxid));
    }
    if (t.empty()) continue;
    if (t.size() > kQuantMaxTargets) throw FormatError{"cfr_quant: a read with more than 65535 targets"};
    pending_.push(t.data(), (uint32_t)t.size(), quant_weight_exp(hit, len) | (r[i].score > r[i].secondary_score ? 256u : 0u));
    flush(false);
  }
}

void Quant::add_tsv(const std::string &path) {
  if (coalesced_) throw std::runtime_error("cfr_quant: assignments were already coalesced");
  const double t_start = now_ms(), c_start = coalesce_ms;
  gzFile gz = path == "-" ? gzdopen(dup(0), "rb") : gzopen(path.c_str(), "rb");   // (zlib hands plain files through as they are)
  if (!gz) throw IoError{"cannot open " + path};
  gzbuffer(gz, 1u << 20);
  int threads = opt_.threads > 0 ? opt_.threads : (int)std::min(std::thread::hardware_concurrency(), 16u);
  if (threads < 1) threads = 1;
  const uint64_t min_len = (uint64_t)(int64_t)opt_.min_length, min_score = opt_.min_score;
  const size_t block = 64u << 20;
  std::vector<char, NoInitAlloc<char>> buf(block + 1);
  size_t have = 0;            // bytes carried over: the start of a line whose end is not read yet
  bool header = true, eof = false;
  Group open;                  // the group the rows read so far leave open (prevReadId and `assign` of LoadReadAssignments)
  bool have_open = false;
  auto close_open = [&]() {
    if (!have_open) return;
    if (open.targets.size() > kQuantMaxTargets) throw FormatError{"cfr_quant: more than 65535 consecutive rows of one read id"};
    pending_.push(open.targets.data(), (uint32_t)open.targets.size(), open.meta);
    have_open = false;
  };
  std::string err;
  while (!eof) {
    if (have == buf.size() - 1) buf.resize(buf.size() * 2);            // one line longer than the block
    while (have < buf.size() - 1) {
      int got = gzread(gz, buf.data() + have, (unsigned)std::min<size_t>(buf.size() - 1 - have, 1u << 30));
      if (got < 0) { gzclose(gz); throw IoError{"read error in " + path}; }
      if (got == 0) { eof = true; break; }
      have += (size_t)got;
    }
    size_t end = have;         // parse [0, end): whole lines only, except at the end of the file
    if (!eof) { while (end > 0 && buf[end - 1] != '\n') --end; if (end == 0) continue; }
    size_t begin = 0;
    if (header) {              // the first line of the file is the header, whatever it holds (Quantifier.hpp:535-541)
      const char *nl = (const char *)memchr(buf.data(), '\n', end);
      begin = nl ? (size_t)(nl - buf.data()) + 1 : end;
      header = false;
    }
    // line-aligned chunks, one per thread
    const int nchunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)threads, (end - begin) / (1u << 16) + 1));
    std::vector<size_t> cut(nchunk + 1, end);
    cut[0] = begin;
    for (int c = 1; c < nchunk; ++c) {
      size_t p = begin + (end - begin) / nchunk * c;
      if (p < cut[c - 1]) p = cut[c - 1];
      const char *nl = p < end ? (const char *)memchr(buf.data() + p, '\n', end - p) : nullptr;
      cut[c] = nl ? (size_t)(nl - buf.data()) + 1 : end;
    }
    std::vector<Chunk> chunks(nchunk);
    auto parse = [&](int c) {
      Chunk &ch = chunks[c];
      const char *p = buf.data() + cut[c], *e = buf.data() + cut[c + 1];
      Group cur;
      const char *cur_id = nullptr; size_t cur_len = 0;
      auto close = [&]() {
        cur.id.assign(cur_id, cur_len);
        if (ch.groups == 1) ch.first = cur;
        else if (cur.targets.size() > kQuantMaxTargets) ch.groups = -1000000;
        else ch.mid.push(cur.targets.data(), (uint32_t)cur.targets.size(), cur.meta);
      };
      while (p < e) {
        const char *nl = (const char *)memchr(p, '\n', e - p);
        const char *le = nl ? nl : e;
        Row r;
        if (parse_row(p, le, r) && !(r.hit < min_len || r.score < min_score || r.taxid == 0)) {
          if (!cur_id || r.id_len != cur_len || memcmp(r.id, cur_id, cur_len)) {
            if (cur_id) close();
            ++ch.groups;
            cur.targets.clear();
            cur.meta = quant_weight_exp(r.hit, r.len) | (r.score > r.second ? 256u : 0u);
            cur_id = r.id; cur_len = r.id_len;
          }
          cur.targets.push_back(compact(r.taxid));
        }
        p = nl ? nl + 1 : e;
      }
      if (cur_id) { cur.id.assign(cur_id, cur_len); if (ch.groups == 1) ch.first = cur; else ch.last = cur; }
    };
    parallel_slices((size_t)nchunk, nchunk, [&](size_t, size_t, int c) { parse(c); });   // one chunk per thread
    // stitch: the result is that of one reader walking the rows in order
    for (Chunk &ch : chunks) {
      if (ch.groups < 0) { gzclose(gz); throw FormatError{"cfr_quant: more than 65535 consecutive rows of one read id"}; }
      if (ch.groups == 0) continue;
      if (have_open && open.id == ch.first.id) open.targets.insert(open.targets.end(), ch.first.targets.begin(), ch.first.targets.end());
      else { close_open(); open = std::move(ch.first); have_open = true; }
      if (ch.groups == 1) continue;
      close_open();
      for (size_t i = 0; i < ch.mid.n(); ++i) {
        const uint32_t *w = ch.mid.words.data() + ch.mid.off[i];
        pending_.push(w + 1, w[0], w[1 + w[0]]);
      }
      open = std::move(ch.last); have_open = true;
      flush(false);
    }
    memmove(buf.data(), buf.data() + end, have - end);
    have -= end;
  }
  gzclose(gz);
  close_open();
  flush(false);
  reader_ms += (now_ms() - t_start) - (coalesce_ms - c_start);
}

void Quant::finish_coalesce() {
  if (coalesced_) return;
  flush(true);
  const double t0 = now_ms();
  QuantAssignments raw;
  coalescer_->finish(raw);
  // operator< of _readAssignment (Quantifier.hpp:50-63): by size, then by the targets in order
  std::vector<size_t> order(raw.n());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    const size_t la = raw.begin[a + 1] - raw.begin[a], lb = raw.begin[b + 1] - raw.begin[b];
    if (la != lb) return la < lb;
    const uint32_t *x = raw.targets.data() + raw.begin[a], *y = raw.targets.data() + raw.begin[b];
    for (size_t i = 0; i < la; ++i) if (x[i] != y[i]) return x[i] < y[i];
    return false;
  });
  assign_ = QuantAssignments();
  for (size_t k : order) {
    assign_.targets.insert(assign_.targets.end(), raw.targets.begin() + raw.begin[k], raw.targets.begin() + raw.begin[k + 1]);
    assign_.begin.push_back(assign_.targets.size());
    assign_.weight_units.push_back(raw.weight_units[k]); assign_.count.push_back(raw.count[k]); assign_.uniq.push_back(raw.uniq[k]);
  }
  coalesce_ms += now_ms() - t0;
  coalesced_ = true;
}

const QuantAssignments &Quant::assignments() { finish_coalesce(); return assign_; }

// Taxonomy::ConvertToGeneralTree (Taxonomy.hpp:1086-1108).  Its second loop is there to "connect the disjoint trees to the root".
// One deliberate difference, which shows on a forest only: the reference's loop also meets the root itself (its parent field is the
// root and it is no child of its own) and adds the edge root -> root; Tree_Plain uses the root's index as its "no child" mark, so the
// next top that is added finds "no child yet" and REPLACES the root's child list - the root then counts the second tree alone (107.3
// of 210 reads in tests/tax_worlds.py's orphan_subtree).  Here the root is left out of that loop, so every top hangs below the root
// beside the root's own children, which is what the loop's comment says it is for.  On a single-rooted taxonomy nothing changes (the
// self-edge ends up behind the last child, where the children walk stops anyway): the reports stay the reference's byte for byte.
void Quant::general_tree(PlainTree &tree) const {
  const size_t nc = tax_.node_cnt;
  tree.init(nc, tax_.root);
  for (size_t i = 0; i < nc; ++i) if (i != tax_.parent[i]) tree.add_edge(i, tax_.parent[i]);
  std::vector<size_t> rc = tree.children(tree.root);
  std::vector<char> is_root_child(nc, 0);
  for (size_t c : rc) is_root_child[c] = 1;
  for (size_t i = 0; i < nc; ++i) if (i != tree.root && tree.nodes[i].parent == tree.root && !is_root_child[i]) tree.add_edge(i, tree.root);
}

int Quant::run() {
  finish_coalesce();
  const double t0 = now_ms();
  const size_t nc = tax_.node_cnt, na = assign_.n();
  std::fill(abund_.begin(), abund_.end(), 0.0); std::fill(read_count_.begin(), read_count_.end(), 0.0); std::fill(uniq_count_.begin(), uniq_count_.end(), 0.0);
  PlainTree all;
  general_tree(all);
  // the covered subtree: the root is 0, then every target and its ancestors in order of first appearance (Quantifier.hpp:656-686)
  std::vector<uint32_t> to_sub(nc, 0xffffffffu);
  std::vector<size_t> inverse{all.root};
  to_sub[all.root] = 0;
  QuantCsr csr;
  csr.a_begin.assign(1, 0);
  for (size_t i = 0; i < na; ++i) {
    const size_t cnt = assign_.begin[i + 1] - assign_.begin[i];
    const double count = (double)assign_.count[i], uniq = (double)assign_.uniq[i];
    for (size_t j = 0; j < cnt; ++j) {
      const uint64_t ctid = assign_.targets[assign_.begin[i] + j];
      if (ctid == nc) {   // a tax id the tree does not hold counts for the root; the root may then stand in a list twice
        csr.a_target.push_back(0);
        read_count_[all.root] += count / cnt;
        uniq_count_[all.root] += uniq;
        continue;
      }
      read_count_[ctid] += count / cnt;
      uniq_count_[ctid] += uniq;
      uint64_t p = ctid;
      while (to_sub[p] == 0xffffffffu) { to_sub[p] = (uint32_t)inverse.size(); inverse.push_back(p); p = tax_.parent[p]; }
      csr.a_target.push_back(to_sub[ctid]);
    }
    csr.a_begin.push_back(csr.a_target.size());
    csr.a_weight.push_back((double)assign_.weight_units[i] / (double)(1ull << kQuantWeightShift));
  }
  Tree all_ch(nc);
  for (size_t i = 0; i < nc; ++i) all_ch[i] = all.children(i);
  tree_abundance(all.root, read_count_.data(), all_ch);
  tree_abundance(all.root, uniq_count_.data(), all_ch);

  const size_t ns = inverse.size();
  PlainTree sub;
  sub.init(ns, 0);
  // (a covered top other than the root hangs below the root here too, as in general_tree: with the taxonomy's own parent it would be
  //  its own child and the EM's tree passes, which start at the root, would never see its tree)
  for (size_t i = 1; i < ns; ++i) {
    const uint64_t par = tax_.parent[inverse[i]];
    sub.add_edge(i, par == inverse[i] ? 0 : to_sub[par]);
  }
  Tree ch(ns);
  for (size_t i = 0; i < ns; ++i) ch[i] = sub.children(i);
  std::vector<uint64_t> len(ns, 0);
  for (size_t i = 0; i < nc; ++i) if (to_sub[i] != 0xffffffffu) len[to_sub[i]] = taxid_length_[i] + taxid_length_[tax_.root] / 10;

  csr.n_nodes = ns;
  quant_csr_finish(csr);
  std::unique_ptr<QuantEStep> estep(opt_.device >= 0 ? make_device_estep(opt_.device, csr) : make_host_estep(csr));

  // EstimateAbundanceWithEM (Quantifier.hpp:236-281)
  std::vector<double> rc(ns, 0), abund(ns, 0), next(ns, 0);
  estep->run(nullptr, true, rc.data());
  tree_abundance(0, rc.data(), ch);
  redistribute(0, rc.data(), ch, len.data());
  const double factor = rc[0];
  for (size_t i = 0; i < ns; ++i) abund[i] = rc[i] / factor;
  int rounds = 0;
  for (int t = 0; t < 1000; ++t) {
    // EMupdate (Quantifier.hpp:186-234): E-step through the seam, M-step and the tree passes here
    estep->run(abund.data(), false, rc.data());
    double sum = 0;
    for (size_t i = 0; i < ns; ++i) sum += rc[i] / (double)len[i];
    for (size_t i = 0; i < ns; ++i) next[i] = rc[i] / (double)len[i] / sum;
    tree_abundance(0, next.data(), ch);
    redistribute(0, next.data(), ch, nullptr);
    double delta = 0;
    for (size_t i = 0; i < ns; ++i) { const double d = abund[i] - next[i]; delta += d > 0 ? d : -d; }
    abund = next;
    ++rounds;
    if (delta < 1e-6 && delta < 0.1 / (double)ns) break;
  }
  for (size_t i = 0; i < ns; ++i) abund_[inverse[i]] = abund[i];
  em_ms = now_ms() - t0;
  return rounds;
}

bool Quant::canonical(size_t ctid) const {   // Taxonomy::IsCanonicalRankNum (Taxonomy.hpp:435-443): subspecies is not one of them
  const uint8_t r = tax_.rank[ctid];
  return r == R_STRAIN || r == R_SPECIES || r == R_GENUS || r == R_FAMILY || r == R_ORDER || r == R_CLASS || r == R_PHYLUM || r == R_KINGDOM ||
         r == R_SUPER_KINGDOM || r == R_DOMAIN || r == R_ACELLULAR_ROOT;
}

// GetTaxLineagePathString (Quantifier.hpp:300-350) over Taxonomy::GetTaxLineagePath (Taxonomy.hpp:977-993)
int Quant::lineage(size_t ctid, int style, bool use_name, bool canonical_only, std::string &out) const {
  std::vector<size_t> path;
  if (ctid >= tax_.node_cnt) path.push_back(tax_.root);
  else {
    size_t guard = 0;
    do { path.push_back(ctid); ctid = tax_.parent[ctid]; } while (ctid != tax_.parent[ctid] && ++guard <= tax_.node_cnt);
  }
  std::reverse(path.begin(), path.end());
  const int n = (int)path.size();
  out.clear();
  for (int i = 0; i < n; ++i) {
    if (canonical_only && !canonical(path[i])) continue;
    if (style == 1 && use_name) {
      if (canonical(path[i])) {
        const uint8_t r = tax_.rank[path[i]];
        out += (r == R_SUPER_KINGDOM || r == R_ACELLULAR_ROOT) ? 'd' : quant_rank_string(r)[0];
        out += "__";
      } else out += "__";
    }
    if (use_name) out += tax_.tax_name[path[i]];
    else out += std::to_string(tax_.orig_taxid[path[i]]);
    if (i < n - 1) out += "|";
  }
  return n;
}

// OutputKreportDFS (Quantifier.hpp:353-399)
void Quant::kreport_dfs(const PlainTree &tree, size_t ctid, int depth, int dist, char prev, FILE *fp) const {
  char r[25];
  if (read_count_[ctid] < 1e-6) return;
  const uint8_t rank = tax_.rank[ctid];
  if (canonical(ctid) && rank != R_STRAIN) {
    r[0] = (rank == R_SUPER_KINGDOM || rank == R_ACELLULAR_ROOT) ? 'D' : (char)(quant_rank_string(rank)[0] - 'a' + 'A');
    r[1] = '\0';
    dist = 0;
  } else if (prev == '\0') { r[0] = 'R'; r[1] = '\0'; }
  else snprintf(r, sizeof(r), "%c%d", prev, dist);
  double children_count = 0;
  const std::vector<size_t> children = tree.children(ctid);
  for (size_t c : children) children_count += read_count_[c];
  fprintf(fp, "%.2lf\t%.0lf\t%.0lf\t%s\t%lu\t", abund_[ctid] * 100, read_count_[ctid], read_count_[ctid] - children_count, r, (unsigned long)tax_.orig_taxid[ctid]);
  for (int i = 0; i < depth; ++i) fprintf(fp, "  ");
  fprintf(fp, "%s\n", tax_.tax_name[ctid].c_str());
  for (size_t c : children) kreport_dfs(tree, c, depth + 1, dist + 1, r[0], fp);
}

// Quantifier::Output (Quantifier.hpp:746-818)
void Quant::write(FILE *fp, int format) const {
  const size_t nc = tax_.node_cnt;
  std::string ids, names;
  if (format == 1) {
    fprintf(fp, "#clade_name\tNCBI_tax_id\trelative_abundance\tadditional_species\n");
    for (size_t i = 0; i < nc; ++i) {
      if (read_count_[i] < 1e-6 || !canonical(i)) continue;
      lineage(i, format, false, true, ids); lineage(i, format, true, true, names);
      fprintf(fp, "%s\t%s\t%.5lf\t\n", names.c_str(), ids.c_str(), abund_[i] * 100.0);
    }
  } else if (format == 2) {
    fprintf(fp, "@@TAXID\tRANK\tTAXPATH\tTAXPATHSN\tPERCENTAGE\n");
    for (size_t i = 0; i < nc; ++i) {
      if (read_count_[i] < 1e-6 || !canonical(i)) continue;
      lineage(i, format, false, true, ids); lineage(i, format, true, true, names);
      fprintf(fp, "%lu\t%s\t%s\t%s\t%.5lf\n", (unsigned long)tax_.orig_taxid[i], quant_rank_string(tax_.rank[i]), ids.c_str(), names.c_str(), abund_[i] * 100.0);
    }
  } else if (format == 3) {
    PlainTree tree;
    general_tree(tree);
    kreport_dfs(tree, tree.root, 0, 0, '\0', fp);
  } else {
    fprintf(fp, "name\ttaxID\ttaxRank\tgenomeSize\tnumReads\tnumUniqueReads\tabundance\n");
    for (size_t i = 0; i < nc; ++i) {
      if (read_count_[i] < 1e-6) continue;
      fprintf(fp, "%s\t%lu\t%s\t%lu\t%d\t%d\t%.7lf\n", tax_.tax_name[i].c_str(), (unsigned long)tax_.orig_taxid[i], quant_rank_string(tax_.rank[i]),
              (unsigned long)taxid_length_[i], (int)(read_count_[i] + 1e-3), (int)(uniq_count_[i] + 1e-3), abund_[i]);
    }
  }
}

}  // namespace cfr
