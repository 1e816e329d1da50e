// inflate_sanitize.cpp — a stand-alone driver of the inflater's host twin (csrc/cfr_inflate.cpp) for sanitizer builds:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/inflate_sanitize.cpp \
//       centrifuger_amd/csrc/cfr_inflate.cpp -o inflate_sanitize -lpthread && ./inflate_sanitize corpus.bin
// corpus.bin (tests/inflate_cases.py write_corpus; little-endian) is a sequence of items:
//   'M' <u64 bytes> members <u64 text bytes> the expected text <u64 n> n expected statuses (one byte each)
// The members - malformed ones among them: the decoder's input is untrusted - go into a heap block of exactly their size, and the twin
// keeps its text in a block of exactly the sum of the ISIZEs: a read or a store one byte off either is a report.  Every item is
// inflated with 1 and with 3 threads, as a whole and member by member; text and statuses must be the expected ones every time.
// Exit status 0: no report, every item came out as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../centrifuger_amd/csrc/cfr_inflate.hpp"

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static uint8_t *block(FILE *f, size_t n, bool &ok) {       // exactly n bytes (one when there are none)
  uint8_t *p = (uint8_t *)malloc(n ? n : 1);
  ok = ok && get(f, p, n);
  return p;
}

static void check(cfr::Inflate &h, const uint8_t *members, uint64_t n, const uint8_t *want, uint64_t want_n, const uint8_t *status, uint64_t n_status,
                  const std::string &what) {
  const uint8_t *text = nullptr;
  uint64_t text_n = 0;
  cfr_inflate_info info;
  h.inflate(members, n, 1, &text, &text_n, &info);
  if (text_n != want_n || (want_n && memcmp(text, want, want_n))) throw std::runtime_error(what + ": not the expected text");
  if (info.members != n_status) throw std::runtime_error(what + ": not the expected number of members");
  std::vector<uint8_t> got(n_status + 1);
  std::vector<uint64_t> off(n_status + 1);
  if (!h.member_status(got.data(), off.data(), n_status)) throw std::runtime_error(what + ": member_status refuses its own count");
  if (n_status && memcmp(got.data(), status, n_status)) throw std::runtime_error(what + ": not the expected statuses");
  if (off[n_status] != want_n) throw std::runtime_error(what + ": the text offsets do not end at the text's size");
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  size_t n_items = 0, n_members = 0;
  try {
    std::unique_ptr<cfr::Inflate> h[2] = {std::unique_ptr<cfr::Inflate>(cfr::make_inflate_host(1)), std::unique_ptr<cfr::Inflate>(cfr::make_inflate_host(3))};
    for (int kind; (kind = fgetc(f)) != EOF;) {
      if (kind != 'M') throw std::runtime_error("an item of unknown kind");
      uint64_t n = 0, text_n = 0, n_status = 0;
      bool ok = get(f, &n, 8);
      uint8_t *members = ok ? block(f, n, ok) : nullptr;
      ok = ok && get(f, &text_n, 8);
      uint8_t *text = ok ? block(f, text_n, ok) : nullptr;
      ok = ok && get(f, &n_status, 8);
      uint8_t *status = ok ? block(f, n_status, ok) : nullptr;
      if (!ok) throw std::runtime_error("short corpus file");
      const std::string what = "item " + std::to_string(n_items);
      for (auto &hh : h) check(*hh, members, n, text, text_n, status, n_status, what);
      // member by member, each in a block of its own
      std::vector<cfr::InfMember> table;
      std::vector<uint64_t> off;
      std::vector<uint8_t> pre;
      cfr::inf_walk(members, n, table, off, pre);
      for (size_t m = 0; m < table.size(); ++m) {
        uint8_t *one = (uint8_t *)malloc(table[m].size);
        memcpy(one, members + table[m].off, table[m].size);
        check(*h[0], one, table[m].size, text + off[m], off[m + 1] - off[m], status + m, 1, what + ", member " + std::to_string(m));
        free(one);
      }
      n_members += table.size();
      free(members); free(text); free(status);
      ++n_items;
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "inflate_sanitize: %s\n", e.what());
    return 1;
  }
  fclose(f);
  printf("inflate_sanitize: %zu items, %zu members, every text and status as expected\n", n_items, n_members);
  return 0;
}
