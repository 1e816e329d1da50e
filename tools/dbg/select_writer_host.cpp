// tools/dbg/select_writer_host.cpp — the selection and the HOST half of the nucleotide index writer without a GPU: compiles cfr_build.cpp
// and the front end's host twin (cfr_refseq.cpp) with g++ and supplies a naive suffix sort, with everything the device reads off the
// suffix array, in place of csrc/cfr_build_sa.hip.  It reads what centrifuger-build reads - FASTA files, nodes.dmp / names.dmp, a
// conversion table or a two-column file list - feeds the files to the twin in chunks, lets select_genomes turn the records into genomes
// and segments, assembles the text and writes <prefix>.*.cfr, to be compared with what the reference builder wrote for the same input
// (tests/test_build_select_cpu.py).  Test infrastructure: never part of libcfr_hip.so.
//   g++ -O2 -std=c++17 -I centrifuger_amd/csrc -o select_writer_host tools/dbg/select_writer_host.cpp centrifuger_amd/csrc/cfr_build.cpp \
//       centrifuger_amd/csrc/cfr_refseq.cpp -lpthread
//   select_writer_host OUT FTABCHARS nodes.dmp names.dmp TABLE FILE_LEVEL CONCAT SUBSET_TAX IGNORE_UNCATEGORIZED CHUNK_LOG2 FASTA...
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>

#include "cfr_build.hpp"
#include "cfr_refseq_core.hpp"

namespace cfr {
// what cfr_build_sa.hip delivers, from a comparison sort: the same order (a proper prefix first), the same products
void build_sa_products(const uint8_t *text, uint64_t n, int, uint32_t rate, uint32_t w, const std::vector<uint64_t> &psum, const std::vector<uint64_t> &want,
                       SaProducts &out, const std::function<void(const std::string &)> &) {
  auto code = [&](uint64_t p) -> uint8_t { return (uint8_t)(strchr("ACGT", text[p]) - "ACGT"); };
  std::vector<uint64_t> sa(n), isa(n);
  for (uint64_t i = 0; i < n; ++i) sa[i] = i;
  std::sort(sa.begin(), sa.end(), [&](uint64_t a, uint64_t b) {
    const uint64_t la = n - a, lb = n - b;
    const int c = memcmp(text + a, text + b, std::min(la, lb));
    return c ? c < 0 : la < lb;
  });
  out.n = n;
  out.bwt.resize(n);
  out.sampled_ids.clear();
  const uint64_t entries = 1ull << (2 * w);
  std::vector<uint64_t> first(entries, ~0ull), count(entries, 0);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t p = sa[i];
    isa[p] = i;
    if (p == 0) { out.first_isa = i; out.bwt[i] = code(n - 1); } else out.bwt[i] = code(p - 1);
    if (i % rate == 0) {
      const uint64_t adj = p + w + 1 < n ? p + w + 1 : p;          // the fuzzy boundary of Builder.hpp:27-51
      out.sampled_ids.push_back((uint32_t)((std::upper_bound(psum.begin(), psum.end(), adj) - psum.begin()) - 1));
    }
    if (p + w <= n) {
      uint64_t key = 0;
      for (uint32_t k = 0; k < w; ++k) key |= (uint64_t)code(p + k) << (2 * k);
      if (!count[key]++) first[key] = i;
    }
  }
  out.ftab.assign(entries * 2, 0);
  for (uint64_t k = 0; k < entries; ++k) { out.ftab[2 * k] = count[k] ? first[k] : 0; out.ftab[2 * k + 1] = count[k]; }
  out.rows_of.clear();
  for (uint64_t p : want) out.rows_of.push_back(isa[p]);
  out.last_code = code(n - 1);
}
void build_sa_products_packed(uint64_t *, uint64_t, int, uint32_t, uint32_t, const std::vector<uint64_t> &, const std::vector<uint64_t> &, SaProducts &,
                              const std::function<void(const std::string &)> &) { throw std::runtime_error("a packed text needs the device"); }
void build_sa_bytes(const uint8_t *, uint64_t, int, std::vector<uint32_t> &, double *, int *) { throw std::runtime_error("protein texts: tools/dbg/prot_writer_host.cpp"); }
}  // namespace cfr

int main(int argc, char **argv) {
  if (argc < 12) { fprintf(stderr, "usage: OUT FTABCHARS nodes.dmp names.dmp TABLE FILE_LEVEL CONCAT SUBSET_TAX IGNORE_UNCATEGORIZED CHUNK_LOG2 FASTA...\n"); return 2; }
  cfr::BuildInput in;
  cfr::SelectOptions so;
  so.ftab_chars = atoi(argv[2]); so.file_level = atoi(argv[6]) != 0; so.concat = atoi(argv[7]) != 0; so.subset_tax = strtoull(argv[8], nullptr, 10);
  so.ignore_uncategorized = atoi(argv[9]) != 0;
  const size_t chunk = (size_t)1 << atoi(argv[10]);
  {
    std::ifstream f(argv[5]);
    std::string nm; unsigned long long t;
    while (f >> nm >> t) { in.names.push_back(so.file_level ? cfr::file_base_name(nm) : nm); in.taxids.push_back(t); }
  }
  {
    std::ifstream f(argv[3]);
    std::string ln;
    while (std::getline(f, ln)) {
      unsigned long long a, b; char rk[256];
      if (sscanf(ln.c_str(), "%llu\t|\t%llu\t|\t%255[^\t]", &a, &b, rk) == 3) in.nodes.push_back(cfr::TaxNode{a, b, rk});
    }
    std::ifstream g(argv[4]);
    while (std::getline(g, ln)) {
      if (ln.find("scientific name") == std::string::npos) continue;
      unsigned long long a; char nm[1024];
      if (sscanf(ln.c_str(), "%llu\t|\t%1023[^\t]", &a, nm) == 2) in.tax_names.emplace_back(a, nm);
    }
  }
  std::unique_ptr<cfr::Refseq> rs(cfr::make_refseq_host(false));
  std::vector<cfr::SelectRecord> records;
  for (int a = 11; a < argc; ++a) {
    std::ifstream f(argv[a], std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::stringstream ss; ss << f.rdbuf();
    const std::string data = ss.str();
    size_t at = 0, first = records.size();
    int line_start = 1;
    for (;;) {
      const size_t take = std::min(chunk, data.size() - at);
      const int final = at + chunk >= data.size();
      cfr_refseq_info info;
      rs->feed((const uint8_t *)data.data() + at, take, line_start, final, &info);
      std::vector<cfr_refseq_record> recs(info.n_records);
      rs->fetch(recs.data());
      uint64_t src = info.u_start;
      if (info.lead_kept && records.size() > first) records.back().pieces.push_back(cfr::SelectPiece{src, info.lead_kept});
      src += info.lead_kept;
      for (const auto &r : recs) {
        records.push_back(cfr::SelectRecord{data.substr(at + r.header + 1, r.id_len), argv[a], {}});
        if (r.kept) records.back().pieces.push_back(cfr::SelectPiece{src, r.kept});
        src += r.kept;
      }
      at += info.consumed;
      line_start = info.at_line_start;
      if (final) break;
    }
  }
  std::vector<cfr::SelectSegment> segs;
  uint64_t n = 0;
  try {
    cfr::select_genomes(in, so, records, segs, n);
  } catch (const std::exception &e) {
    fprintf(stderr, "ERROR: %s\n", e.what());
    return 1;
  }
  std::vector<cfr_refseq_segment> cs;
  for (const auto &g : segs) cs.push_back(cfr_refseq_segment{g.src, g.len, g.dst});
  rs->assemble(cs.data(), cs.size(), n);
  in.text = rs->host_text();
  cfr::BuildOptions opt;
  opt.ftab_chars = so.ftab_chars;
  cfr::BuildReport rep;
  cfr::build_index_files(in, opt, argv[1], &rep);
  printf("%llu genomes, %llu symbols, %llu segments, %llu extra names\n", (unsigned long long)in.genome_seq.size(), (unsigned long long)n, (unsigned long long)cs.size(), (unsigned long long)in.n_extra);
  return 0;
}
