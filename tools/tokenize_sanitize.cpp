// tokenize_sanitize.cpp — a stand-alone driver of the tokeniser's host twin (csrc/cfr_tokenize_host.cpp) for sanitizer builds:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/tokenize_sanitize.cpp \
//       centrifuger_amd/csrc/cfr_tokenize_host.cpp -o tokenize_sanitize && ./tokenize_sanitize corpus.bin
// corpus.bin: records of <u32 little-endian length> <u8 sweep> <bytes> (tests/test_tokenize_sanitized_cpu.py writes it).  Every text is
// tokenised with final = 0 and 1 and with a cap of 0 and 2 records, from a heap block of exactly its length, and fetched into blocks of
// exactly the announced sizes - so a read or write one byte off is a report.  sweep != 0: also every truncation of the text.
// Exit status 0: no report and every result is consistent in itself.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../centrifuger_amd/csrc/cfr_tokenize_core.hpp"

static int fail(const char *what, size_t text_no, size_t len) {
  fprintf(stderr, "tokenize_sanitize: %s (text %zu, %zu bytes)\n", what, text_no, len);
  return 1;
}

static int one(cfr::Tokenizer &tok, const uint8_t *src, size_t len, size_t text_no) {
  uint8_t *text = (uint8_t *)malloc(len ? len : 1);
  memcpy(text, src, len);
  int bad = 0;
  for (int final = 0; final < 2 && !bad; ++final)
    for (uint64_t cap = 0; cap <= 2 && !bad; cap += 2) {
      cfr_token_info info;
      tok.tokenize(text, len, final, cap, &info);
      if (info.consumed > len || (cap && info.n_records > cap) || info.total_bases > len) { bad = fail("summary out of range", text_no, len); break; }
      if (info.irregular && info.irregular_at >= len) { bad = fail("irregular_at out of range", text_no, len); break; }
      cfr_read_record *rec = (cfr_read_record *)malloc(info.n_records * sizeof(cfr_read_record) + 1);
      uint64_t *off = (uint64_t *)malloc((info.n_records + 1) * 8);
      uint8_t *bases = (uint8_t *)malloc(info.total_bases + 1);
      tok.fetch(rec, off, bases);
      if (off[0] != 0 || off[info.n_records] != info.total_bases) bad = fail("offsets do not span the bases", text_no, len);
      for (uint64_t r = 0; r < info.n_records && !bad; ++r) {
        if (off[r] > off[r + 1]) bad = fail("offsets decrease", text_no, len);
        if (rec[r].header + rec[r].header_len > len || rec[r].id_len + 1 > rec[r].header_len || rec[r].qual > len) bad = fail("record out of range", text_no, len);
      }
      free(rec); free(off); free(bases);
    }
  free(text);
  return bad;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::unique_ptr<cfr::Tokenizer> tok(cfr::make_tokenizer_host());
  std::vector<uint8_t> text;
  size_t n_texts = 0, n_calls = 0;
  for (;;) {
    uint8_t head[5];
    if (fread(head, 1, 5, f) != 5) break;
    const size_t len = (size_t)head[0] | ((size_t)head[1] << 8) | ((size_t)head[2] << 16) | ((size_t)head[3] << 24);
    text.resize(len);
    if (len && fread(text.data(), 1, len, f) != len) { fclose(f); return fail("short corpus file", n_texts, len); }
    if (one(*tok, text.data(), len, n_texts)) { fclose(f); return 1; }
    ++n_calls;
    if (head[4]) for (size_t cut = 1; cut < len; ++cut, ++n_calls) if (one(*tok, text.data(), cut, n_texts)) { fclose(f); return 1; }
    ++n_texts;
  }
  fclose(f);
  printf("tokenize_sanitize: %zu texts, %zu lengths, no report\n", n_texts, n_calls);
  return 0;
}
