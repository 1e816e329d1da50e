// cfr_build.hpp — the index writer: what centrifuger-build's FMBuilder / Builder produce (FMBuilder.hpp:209-313,
// Builder.hpp:86-313), built on one MI355X.  Not on the classification path; it exists so that indexes of the sizes the
// path is measured on (several Gbp; n >= 2^32) can be manufactured on the GPU box in a minute instead of the reference
// builder's half hour, and so that the on-disk contract is exercised from the writing side.
//
//   cfr_build_sa.hip  : the suffix array in HBM (prefix doubling over 32-mer-sorted groups, radix sorts by hipCUB) and what
//                       is read off it: BWT, firstISA, sampled sequence ids, selected rows, ftab
//   cfr_build.cpp     : run-block compression, wavelet trees, rank9 counters, taxonomy, the four .cfr files; C-ABI entry
#pragma once

#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace cfr {

struct SaProducts {
  uint64_t n = 0, first_isa = 0;
  std::vector<uint8_t> bwt;              // n codes 0..3: B[i] = T[SA[i]-1], T[n-1] at the row of position 0 (FMBuilder.hpp:244-250)
  std::vector<uint32_t> sampled_ids;     // sequence id of SA[k * rate] with the fuzzy boundary (Builder.hpp:27-51)
  std::vector<uint64_t> rows_of;         // rows of the requested text positions (for selectedSA, Builder.hpp:224-234)
  std::vector<uint64_t> ftab;            // 4^w pairs (first row, count) over suffixes of >= w characters (FMBuilder.hpp:256-283)
  double seconds_sa = 0, seconds_products = 0;
  int rounds = 0;
  uint8_t last_code = 0;                 // the code of T[n-1], read from the packed text
};

// text: n upper-case A,C,G,T (host; read once, front to back).  psum: G+1 sequence start offsets.  want_pos: text positions
// whose rows are wanted.  Throws HipError (cfr_device.hpp) on device failure / unsupported size / other characters.
void build_sa_products(const uint8_t *text, uint64_t n, int device, uint32_t sample_rate, uint32_t ftab_width,
                       const std::vector<uint64_t> &psum, const std::vector<uint64_t> &want_pos, SaProducts &out,
                       const std::function<void(const std::string &)> &log);

// The same with the text already packed in the memory of `device` (2 bits per symbol, the first symbol of a word in its top bits,
// (n + 31) / 32 + 4 words with the tail zero: what cfr_refseq_assemble wrote).  The call owns `packed` from its first line on.
void build_sa_products_packed(uint64_t *packed, uint64_t n, int device, uint32_t sample_rate, uint32_t ftab_width,
                              const std::vector<uint64_t> &psum, const std::vector<uint64_t> &want_pos, SaProducts &out,
                              const std::function<void(const std::string &)> &log);

// Suffix array of a text of byte codes (protein indexes: 21 codes, '$' = 0 closes every sequence), n < 2^32: prefix doubling with
// hipCUB radix sorts in HBM (cfr_build_sa.hip).  Same order as above: plain lexicographic, a proper prefix first.
void build_sa_bytes(const uint8_t *codes, uint64_t n, int device, std::vector<uint32_t> &sa, double *seconds, int *rounds);

struct TaxNode { uint64_t taxid, parent; std::string rank; };
// The compact tax ids of an index (Taxonomy::Init, Taxonomy.hpp:146-232): the ids on the paths from the conversion table's ids to the
// root, numbered in ascending original id.  Made once per build by compact_taxonomy(); the selection and the writer of .2.cfr share it.
struct TaxCompact {
  std::vector<uint64_t> order;             // original id of every compact id
  std::map<uint64_t, uint64_t> cid;        // original id -> compact id
  std::vector<uint64_t> parent;            // compact parent (a top is its own parent)
  std::vector<uint8_t> rank, leaf;
  std::vector<std::string> name;           // scientific name with '_' for blanks, "" without one
};
struct BuildInput {
  std::vector<std::string> names;          // sequence names, conversion-table order = sequence ids; the last n_extra are extra names (no tax id)
  std::vector<uint64_t> taxids;            // original tax id of every conversion-table sequence
  std::vector<uint64_t> present_taxids;    // further ids the conversion table mentions (their lineages stay in the tree)
  uint64_t n_extra = 0;
  std::vector<uint64_t> genome_seq, lens;  // the genomes of the text, text order: sequence id and length (ACGT only)
  const uint8_t *text = nullptr;           // the genomes back to back, upper-case ACGT (BuildOptions::protein: the proteins back to back, letters of
                                           // "ARNDCEQGHILKMFPSTWYV" only; lens are residue counts, the writer puts '$' behind every protein)
  std::vector<TaxNode> nodes;              // nodes.dmp
  std::vector<std::pair<uint64_t, std::string>> tax_names;   // names.dmp, scientific names
  // ---- set by select_genomes / cfr_build_index_assembled only
  // the nucleotide text packed in the memory of BuildOptions::device (see build_sa_products_packed): called once, when the suffix sort
  // begins, and hands the memory over; `text` is not read then
  std::function<uint64_t *()> take_packed_text;
  bool taxid_as_seqid = false;             // --concat-tax-genome (Taxonomy::SetTaxIdAsSeqId): sequence id = compact tax id, node_cnt = "uncategorized";
                                           // genome_seq holds such ids, names / taxids still describe the conversion table (they shape the tree)
  std::shared_ptr<const TaxCompact> compact;   // made by build_index_files when absent
};
std::shared_ptr<const TaxCompact> compact_taxonomy(const BuildInput &in);

// ---- selection: from the records of the reference files to the genomes of the text (Builder::Build, Builder.hpp:104-211)
struct SelectPiece { uint64_t src, len; };                 // symbols of the stream U (cfr_refseq_core.hpp)
struct SelectRecord { std::string id, file; std::vector<SelectPiece> pieces; };   // one FASTA record: its id, its file, its kept symbols in U
struct SelectOptions { bool file_level = false, concat = false, ignore_uncategorized = false, protein = false; uint64_t subset_tax = 0; int ftab_chars = 10; };
struct SelectSegment { uint64_t src, len, dst; };
// in: names / taxids (the conversion table, or the file list with base names), nodes, tax_names.  Adds the extra names, fills genome_seq, lens,
// n_extra, taxid_as_seqid, compact; segments (sorted by dst, covering [0, n)) say where the text's symbols lie in U.  Warnings go to stderr in
// the reference's words; throws std::runtime_error with the reference's "found 0 genomes" message when nothing is left.
void select_genomes(BuildInput &in, const SelectOptions &so, const std::vector<SelectRecord> &records, std::vector<SelectSegment> &segments, uint64_t &n);
// Utils::GetFileBaseName(path, "fna|fa|fasta|faa"): no directory, no last extension, and not one of these four behind it either
std::string file_base_name(const std::string &path);
struct BuildOptions { int ftab_chars = 10, offrate = 4, device = 0, threads = 0; uint64_t rbbwt_b = 0; bool verbose = false, protein = false; };
struct BuildReport { uint64_t n = 0, block_size = 0, first_isa = 0; double seconds_sa = 0, seconds_total = 0; int rounds = 0; };

// Writes <prefix>.{1,2,3,4}.cfr.  Throws HipError / IoError / std::runtime_error.
void build_index_files(const BuildInput &in, const BuildOptions &opt, const std::string &prefix, BuildReport *report);

}  // namespace cfr
