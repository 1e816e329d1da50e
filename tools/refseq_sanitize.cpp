// refseq_sanitize.cpp — a stand-alone driver of the reference-text front end's host twin (csrc/cfr_refseq.cpp) for sanitizer builds:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/refseq_sanitize.cpp \
//       centrifuger_amd/csrc/cfr_refseq.cpp -o refseq_sanitize && ./refseq_sanitize corpus.bin
// corpus.bin: records of <u32 little-endian length> <u8 protein> <bytes> (tests/test_refseq_host_cpu.py writes it).  Every text is fed as
// one file in chunks of 2^20, 4096, 1024, 256 and 64 bytes, each chunk from a heap block of exactly its length, the records fetched into a
// block of exactly their size; then everything kept is assembled in feed order and, record by record, backwards, and read back into a
// block of exactly n bytes - so a read or write one byte off is a report.  A header line longer than a chunk ends that text's run at
// that chunk size (RefseqCapacity), nothing else may throw.
// Exit status 0: no report and every result is consistent in itself.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../centrifuger_amd/csrc/cfr_refseq_core.hpp"

static int fail(const char *what, size_t text_no, size_t chunk) {
  fprintf(stderr, "refseq_sanitize: %s (text %zu, chunks of %zu bytes)\n", what, text_no, chunk);
  return 1;
}

static int one(const uint8_t *src, size_t len, bool protein, size_t chunk, size_t text_no, size_t *calls) {
  std::unique_ptr<cfr::Refseq> h(cfr::make_refseq_host(protein));
  std::vector<cfr_refseq_segment> runs;          // the kept run of every chunk
  size_t at = 0;
  int line_start = 1;
  for (;;) {
    const size_t take = len - at < chunk ? len - at : chunk;
    const int final = at + chunk >= len;
    uint8_t *text = (uint8_t *)malloc(take ? take : 1);
    memcpy(text, src + at, take);
    cfr_refseq_info info;
    try {
      h->feed(text, take, line_start, final, &info);
    } catch (const cfr::RefseqCapacity &) {
      free(text);
      return 0;
    }
    ++*calls;
    int bad = 0;
    if (info.consumed > take || (!final && info.consumed == 0) || info.kept > info.consumed || info.lead_kept > info.kept || info.u_start % 32) bad = fail("summary out of range", text_no, chunk);
    cfr_refseq_record *rec = (cfr_refseq_record *)malloc(info.n_records * sizeof(cfr_refseq_record) + 1);
    h->fetch(rec);
    uint64_t sum = info.lead_kept;
    for (uint64_t r = 0; r < info.n_records && !bad; ++r) {
      if ((uint64_t)rec[r].header + rec[r].header_len > info.consumed || rec[r].header_len == 0 || rec[r].id_len + 1 > rec[r].header_len || text[rec[r].header] != '>')
        bad = fail("record out of range", text_no, chunk);
      sum += rec[r].kept;
    }
    if (!bad && sum != info.kept) bad = fail("the records' symbols do not add up", text_no, chunk);
    free(rec);
    free(text);
    if (bad) return 1;
    if (info.kept) runs.push_back(cfr_refseq_segment{info.u_start, info.kept, 0});
    at += info.consumed;
    line_start = info.at_line_start;
    if (final) break;
  }
  if (runs.empty()) return 0;
  for (int backwards = 0; backwards < 2; ++backwards) {
    std::unique_ptr<cfr::Refseq> g;
    if (backwards) {              // (assemble frees U: feed again, whole)
      g.reset(cfr::make_refseq_host(protein));
      cfr_refseq_info info;
      g->feed(src, len, 1, 1, &info);
      runs.assign(1, cfr_refseq_segment{info.u_start, info.kept, 0});
    }
    cfr::Refseq &r = backwards ? *g : *h;
    std::vector<cfr_refseq_segment> segs;
    uint64_t n = 0;
    if (!backwards) for (auto s : runs) { s.dst = n; n += s.len; segs.push_back(s); }
    else for (uint64_t k = runs[0].len; k-- > 0;) { segs.push_back(cfr_refseq_segment{runs[0].src + k, 1, n}); ++n; }
    r.assemble(segs.data(), segs.size(), n);
    if (r.text_len() != n) return fail("text_len differs from n", text_no, chunk);
    uint8_t *out = (uint8_t *)malloc(n);
    r.text(out);
    for (uint64_t k = 0; k < n; ++k) if (!(protein ? cfr::refseq_kept_aa(out[k]) : cfr::refseq_kept_nt(out[k]))) { free(out); return fail("a symbol outside the alphabet", text_no, chunk); }
    free(out);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> text;
  size_t n_texts = 0, n_calls = 0;
  for (;;) {
    uint8_t head[5];
    if (fread(head, 1, 5, f) != 5) break;
    const size_t len = (size_t)head[0] | ((size_t)head[1] << 8) | ((size_t)head[2] << 16) | ((size_t)head[3] << 24);
    text.resize(len);
    if (len && fread(text.data(), 1, len, f) != len) { fclose(f); return fail("short corpus file", n_texts, 0); }
    for (size_t chunk : {(size_t)1 << 20, (size_t)4096, (size_t)1024, (size_t)256, (size_t)64})
      if (one(text.data(), len, head[4] != 0, chunk, n_texts, &n_calls)) { fclose(f); return 1; }
    ++n_texts;
  }
  fclose(f);
  printf("refseq_sanitize: %zu texts, %zu chunks, no report\n", n_texts, n_calls);
  return 0;
}
