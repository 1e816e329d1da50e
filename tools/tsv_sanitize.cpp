// tsv_sanitize.cpp — a stand-alone driver of the batch formatter's host twin (csrc/cfr_tsv.cpp) for sanitizer builds:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/tsv_sanitize.cpp \
//       centrifuger_amd/csrc/cfr_tsv.cpp -o tsv_sanitize -lpthread && ./tsv_sanitize corpus.bin
// corpus.bin (tests/tsv_cases.py write_corpus; little-endian): <u64 names> <u64 ranks>, every name as <u32 length> <bytes>, the rank
// codes; then batches of <u64 n> <u64 slots> <u64 id bytes> <u64 text bytes>, n cfr_result, slots cfr_match, n + 1 id offsets, the id
// bytes and the text the twin must make.  Every array goes into a heap block of exactly its size and the text into one of exactly
// the announced length - so a read or write one byte off is a report - with 1 and 3 threads; then once more with one byte less,
// which must be refused with the length set.
// Exit status 0: no report, every text is the expected one.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../centrifuger_amd/csrc/cfr_tsv.hpp"

static const char *rank_string(uint8_t r) {      // the strings of cfr::tax_rank_string (csrc/cfr_dust.cpp), which the expected texts were made with
  static const char *names[] = {"no rank", "strain", "species", "genus", "family", "order", "class", "phylum", "kingdom", "domain", "forma",
                                "infraclass", "infraorder", "parvorder", "subclass", "subfamily", "subgenus", "subkingdom", "suborder",
                                "subphylum", "subspecies", "subtribe", "superclass", "superfamily", "superkingdom", "superorder", "superphylum",
                                "tribe", "varietas", "life", "acellular root"};
  return names[r];
}

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> static T *block(FILE *f, size_t count, bool &ok) {      // exactly count entries (one byte when there are none)
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  ok = ok && get(f, p, count * sizeof(T));
  return p;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t head[2];
  if (!get(f, head, 16)) { fprintf(stderr, "tsv_sanitize: short corpus file\n"); return 1; }
  cfr::TsvTables t;
  std::vector<std::string> names;
  for (uint64_t i = 0; i < head[0]; ++i) {
    uint32_t k = 0;
    if (!get(f, &k, 4)) return 1;
    std::string s(k, '\0');
    if (!get(f, &s[0], k)) return 1;
    names.push_back(s);
  }
  t.set_names(names);
  t.rank.resize(head[1]);
  if (!get(f, t.rank.data(), head[1])) return 1;
  t.set_rank_strings(rank_string);
  size_t n_batches = 0;
  for (;;) {
    uint64_t h[4];
    if (fread(h, 1, 32, f) != 32) break;
    bool ok = true;
    cfr_result *res = block<cfr_result>(f, h[0], ok);
    cfr_match *mat = block<cfr_match>(f, h[1], ok);
    uint64_t *ido = block<uint64_t>(f, h[0] + 1, ok);
    char *idb = block<char>(f, h[2], ok), *want = block<char>(f, h[3], ok);
    if (!ok) { fprintf(stderr, "tsv_sanitize: short corpus file (batch %zu)\n", n_batches); return 1; }
    for (int threads : {1, 3}) {
      std::unique_ptr<cfr::Tsv> tsv(cfr::make_tsv_host(t, threads));
      char *text = (char *)malloc(h[3] ? h[3] : 1);
      uint64_t *off = (uint64_t *)malloc((h[0] + 1) * 8);
      uint64_t len = 0;
      if (!tsv->format(res, mat, h[1], h[0], h[2] ? idb : nullptr, ido, text, h[3], &len, off) || len != h[3] || memcmp(text, want, h[3]) || off[0] != 0 || off[h[0]] != len) {
        fprintf(stderr, "tsv_sanitize: batch %zu, %d threads: not the expected text\n", n_batches, threads);
        return 1;
      }
      if (h[3]) {
        len = 0;
        char *less = (char *)malloc(h[3] - 1 ? h[3] - 1 : 1);
        if (tsv->format(res, mat, h[1], h[0], h[2] ? idb : nullptr, ido, less, h[3] - 1, &len, nullptr) || len != h[3]) {
          fprintf(stderr, "tsv_sanitize: batch %zu: a buffer one byte short was not refused\n", n_batches);
          return 1;
        }
        free(less);
      }
      // a refusal throws before anything is read behind the arrays
      if (h[0]) {
        bool threw = false;
        try { tsv->format(res, mat, 0, h[0], idb, nullptr, text, h[3], &len, nullptr); } catch (const std::invalid_argument &) { threw = true; }
        if (!threw) { fprintf(stderr, "tsv_sanitize: batch %zu: null id_offsets were not refused\n", n_batches); return 1; }
      }
      free(text); free(off);
    }
    free(res); free(mat); free(ido); free(idb); free(want);
    ++n_batches;
  }
  fclose(f);
  printf("tsv_sanitize: %zu batches, no report\n", n_batches);
  return 0;
}
