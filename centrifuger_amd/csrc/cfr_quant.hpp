// cfr_quant.hpp — abundance estimation (centrifuger-quant): the host twin and the seam to the device kernels.
//
// A restatement of Quantifier (Quantifier.hpp:186-818) and of the taxonomy helpers it calls (Taxonomy.hpp:372-406, 977-993,
// 1084-1213; compactds/Tree_Plain.hpp:109-168), in the reference's order of floating-point operations.  cfr_quant.cpp holds the
// reader, the host coalesce, the EM and the four report writers; cfr_quant.hip holds the device coalesce and the E-step.
#pragma once

#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "cfr_index.hpp"

namespace cfr {

// the taxonomy of <prefix>.2.cfr alone (cfr_index.cpp): quantification never opens .1.cfr
void load_taxonomy(const std::string &path, Taxonomy &t);
// <prefix>.3.cfr (sequence id -> length) and Taxonomy::ConvertSeqLengthToTaxLength (Taxonomy.hpp:1111-1213): the genome length of
// every tax id, node_cnt + 1 entries.  Shared by the quantifier and by centrifuger-inspect --size-table.
std::map<uint64_t, uint64_t> read_seq_lengths(const std::string &prefix);
void tax_genome_lengths(const Taxonomy &t, const std::map<uint64_t, uint64_t> &seq_length, std::vector<uint64_t> &taxid_length);

// Flat read assignments, one record per read: n_targets | targets[n_targets] (compact tax ids, node_cnt = not in the tree) |
// meta (bits 0..7: d of the weight 4^-d, 0..11; bit 8: score > secondScore).  off[i] = first word of record i, off[n] = words used.
struct QuantRecords {
  std::vector<uint32_t> words;
  std::vector<uint32_t> off{0};
  size_t n() const { return off.size() - 1; }
  void clear() { words.clear(); off.assign(1, 0); }
  void push(const uint32_t *targets, uint32_t nt, uint32_t meta) {
    words.push_back(nt);
    words.insert(words.end(), targets, targets + nt);
    words.push_back(meta);
    off.push_back((uint32_t)words.size());
  }
};
constexpr uint32_t kQuantMaxTargets = 65535;   // longest target list a record may hold (the classifier prints at most -k rows per read)
constexpr int kQuantWeightShift = 22;           // weights are summed in units of 2^-22: 4^-11 is one unit
inline uint64_t quant_weight_units(uint32_t meta) { return 1ull << (kQuantWeightShift - 2 * (int)(meta & 0xff)); }

// coalesced assignments: list i = targets[begin[i] .. begin[i + 1])
struct QuantAssignments {
  std::vector<uint64_t> begin{0};
  std::vector<uint32_t> targets;
  std::vector<uint64_t> weight_units, count, uniq;
  size_t n() const { return begin.size() - 1; }
};

// records in, distinct target lists out (in no particular order; Quant sorts them)
class QuantCoalescer {
 public:
  virtual ~QuantCoalescer() {}
  virtual void add(const QuantRecords &r) = 0;
  virtual void finish(QuantAssignments &out) = 0;
};
QuantCoalescer *make_host_coalescer();

// E-step of EMupdate (Quantifier.hpp:196-208) over the transposed CSR of the assignments; see cfr_quant.hip
class QuantEStep {
 public:
  virtual ~QuantEStep() {}
  // init = true: the start of EstimateAbundanceWithEM (weight / targetCnt, Quantifier.hpp:243-249); abund is not read then
  virtual void run(const double *abund, bool init, double *read_count) = 0;
};
struct QuantCsr {                  // built once per quantification by the host
  uint64_t n_nodes = 0, n_slots = 0;
  std::vector<uint64_t> a_begin;   // assignment -> its first slot (n_assign + 1)
  std::vector<uint32_t> a_target;  // slot -> subtree node
  std::vector<double> a_weight;    // assignment -> weight
  std::vector<uint64_t> slot_pos;  // slot -> position of its term in the node-major order
  std::vector<uint64_t> node_begin;// node -> first position (n_nodes + 1)
};
// fills n_slots, node_begin and slot_pos from n_nodes, a_begin and a_target (every target < n_nodes)
void quant_csr_finish(QuantCsr &c);
QuantEStep *make_host_estep(const QuantCsr &c);

// the device side (cfr_quant.hip); both throw HipError
QuantCoalescer *make_device_coalescer(int device, uint64_t table_slots);
QuantEStep *make_device_estep(int device, const QuantCsr &c);
struct QuantDeviceStats { uint64_t grow_count = 0, table_slots = 0; double coalesce_ms = 0; };
QuantDeviceStats device_coalescer_stats(const QuantCoalescer *c);

struct QuantOptions { uint64_t min_score = 0; int32_t min_length = 0; int32_t device = -1; uint64_t table_slots = 0; int32_t threads = 0; };

class Quant {
 public:
  Quant(const std::string &prefix, const QuantOptions &o);
  ~Quant();
  void add_tsv(const std::string &path);
  void add_results(const cfr_result *r, const cfr_match *m, size_t n);
  const QuantAssignments &assignments();          // coalesces what was added, sorted as CoalesceAssignments leaves it
  int run();                                      // Quantification(); returns the EM rounds
  void write(FILE *fp, int format) const;         // Output()
  uint64_t node_cnt() const { return tax_.node_cnt; }
  const std::vector<double> &abund() const { return abund_; }
  const std::vector<double> &read_count() const { return read_count_; }
  const std::vector<double> &uniq_count() const { return uniq_count_; }
  const std::vector<uint64_t> &taxid_length() const { return taxid_length_; }
  double reader_ms = 0, coalesce_ms = 0, em_ms = 0;
  QuantDeviceStats device_stats() const { return opt_.device >= 0 ? device_coalescer_stats(coalescer_.get()) : QuantDeviceStats(); }

 private:
  struct PlainTree;
  void flush(bool all);
  void finish_coalesce();
  uint32_t compact(uint64_t taxid) const {
    auto it = to_compact_.find(taxid);
    return it == to_compact_.end() ? (uint32_t)tax_.node_cnt : it->second;
  }
  void general_tree(PlainTree &t) const;
  void kreport_dfs(const PlainTree &tree, size_t ctid, int depth, int dist, char prev, FILE *fp) const;
  int lineage(size_t ctid, int style, bool use_name, bool canonical_only, std::string &out) const;
  bool canonical(size_t ctid) const;

  QuantOptions opt_;
  Taxonomy tax_;
  std::unordered_map<uint64_t, uint32_t> to_compact_;
  std::vector<uint64_t> taxid_length_;
  std::vector<double> abund_, read_count_, uniq_count_;
  QuantRecords pending_;
  std::unique_ptr<QuantCoalescer> coalescer_;
  QuantAssignments assign_;
  bool coalesced_ = false;
  // TSV reader state that crosses chunk and file borders within one add_tsv call lives in add_tsv itself
};

// Taxonomy::IsNextSeqNameFromTheSameGenome (Taxonomy.hpp:372-406)
bool quant_next_seq_same_genome(const char *a, const char *b);
// CalculateAssignmentWeight (Quantifier.hpp:283-293) as the exponent d of 4^-d
uint32_t quant_weight_exp(uint64_t hit_length, uint64_t read_length);
const char *quant_rank_string(uint8_t rank);

}  // namespace cfr
