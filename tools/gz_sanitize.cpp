// gz_sanitize.cpp — a stand-alone driver of the compressor's host twin (csrc/cfr_gz.cpp) for sanitizer builds:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/gz_sanitize.cpp \
//       centrifuger_amd/csrc/cfr_gz.cpp -o gz_sanitize -lpthread && ./gz_sanitize corpus.bin
// corpus.bin (tests/gz_cases.py write_corpus; little-endian) is a sequence of items:
//   'T' <u32 block_bytes> <u64 n> text
//   'D' <u32 block_bytes> <u64 n reads> <u32 files> <u64 id bytes> ids, n + 1 id offsets, n select bytes; per file <u64 seq bytes>
//       <u64 qual bytes, or 2^64 - 1 for none> seq, n + 1 offsets, [qual, n + 1 offsets, n has_qual bytes], <u64 expected bytes> the text
// Every input goes into a heap block of exactly its size - so a read one byte off is a report - and is compressed with 1 and with 3
// threads: both must give the same bytes, and the members are undone here (stored blocks copied, fixed-Huffman blocks decoded by a
// small inflater of this file's own) and compared with the text.
//   ./gz_sanitize corpus.bin dynamic   the same items with cfr_gz_options.codes = 1; the inflater reads dynamic blocks (BTYPE 10) too.
// Exit status 0: no report, every text came back.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../centrifuger_amd/csrc/cfr_gz.hpp"

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> static T *block(FILE *f, size_t count, bool &ok) {      // exactly count entries (one byte when there are none)
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  ok = ok && get(f, p, count * sizeof(T));
  return p;
}

static bool same(const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb) { return na == nb && (na == 0 || memcmp(a, b, na) == 0); }

// ---- members back into text: only what the twin writes (one final block per member, stored or fixed Huffman) ----
struct Bits {
  const uint8_t *p, *end;
  uint32_t at = 0;
  int bit() {
    if (p >= end) throw std::runtime_error("the stream ends early");
    const int b = (*p >> at) & 1;
    if (++at == 8) { at = 0; ++p; }
    return b;
  }
  uint32_t low_first(int n) { uint32_t v = 0; for (int i = 0; i < n; ++i) v |= (uint32_t)bit() << i; return v; }
  uint32_t high_first(int n) { uint32_t v = 0; for (int i = 0; i < n; ++i) v = (v << 1) | (uint32_t)bit(); return v; }
};

// a Huffman code from its lengths (RFC 1951, 3.2.2), decoded bit by bit
struct Code {
  uint16_t count[16] = {0}, symbol[288] = {0};
  Code(const uint8_t *len, int n) {
    for (int s = 0; s < n; ++s) ++count[len[s]];
    count[0] = 0;
    uint16_t offs[16] = {0};
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; ++s) if (len[s]) symbol[offs[len[s]]++] = (uint16_t)s;
  }
  uint32_t decode(Bits &in) const {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
      code |= in.bit();
      const int c = count[l];
      if (code - c < first) return symbol[index + (code - first)];
      index += c; first += c; first <<= 1; code <<= 1;
    }
    throw std::runtime_error("a code that no symbol has");
  }
};

// lit == nullptr: the fixed code
static void inflate_codes(Bits &in, std::string &out, const Code *lit, const Code *dist);
static void inflate_fixed(Bits &in, std::string &out) { inflate_codes(in, out, nullptr, nullptr); }

static void inflate_dynamic(Bits &in, std::string &out) {
  static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  const uint32_t hlit = in.low_first(5) + 257, hdist = in.low_first(5) + 1, hclen = in.low_first(4) + 4;
  if (hlit > 286 || hdist > 30) throw std::runtime_error("HLIT / HDIST out of range");
  uint8_t cl[19] = {0}, len[286 + 30] = {0};
  for (uint32_t i = 0; i < hclen; ++i) cl[order[i]] = (uint8_t)in.low_first(3);
  const Code clc(cl, 19);
  for (uint32_t i = 0; i < hlit + hdist;) {
    const uint32_t sym = clc.decode(in);
    if (sym < 16) { len[i++] = (uint8_t)sym; continue; }
    uint32_t rep;
    uint8_t v = 0;
    if (sym == 16) { if (!i) throw std::runtime_error("a repeat with nothing in front"); v = len[i - 1]; rep = 3 + in.low_first(2); }
    else if (sym == 17) rep = 3 + in.low_first(3);
    else rep = 11 + in.low_first(7);
    if (i + rep > hlit + hdist) throw std::runtime_error("a repeat runs over the end of the lengths");
    while (rep--) len[i++] = v;
  }
  if (!len[256]) throw std::runtime_error("no end-of-block code");
  const Code lit(len, (int)hlit), dist(len + hlit, (int)hdist);
  inflate_codes(in, out, &lit, &dist);
}

static void inflate_codes(Bits &in, std::string &out, const Code *lit, const Code *dist) {
  static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  static const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  const size_t first = out.size();
  for (;;) {
    uint32_t sym;
    if (lit) sym = lit->decode(in);
    else {
      uint32_t code = in.high_first(7);
      if (code <= 0x17) sym = 256 + code;
      else {
        code = (code << 1) | (uint32_t)in.bit();
        if (code >= 0x30 && code <= 0xbf) sym = code - 0x30;
        else if (code >= 0xc0 && code <= 0xc7) sym = 280 + (code - 0xc0);
        else { code = (code << 1) | (uint32_t)in.bit(); sym = 144 + (code - 0x190); }
      }
    }
    if (sym < 256) { out.push_back((char)sym); continue; }
    if (sym == 256) return;
    if (sym > 285) throw std::runtime_error("a length symbol above 285");
    const uint32_t len = len_base[sym - 257] + in.low_first(len_extra[sym - 257]);
    const uint32_t dc = dist ? dist->decode(in) : in.high_first(5);
    if (dc > 29) throw std::runtime_error("a distance code above 29");
    const uint32_t distance = dist_base[dc] + in.low_first(dist_extra[dc]);
    if (distance > out.size() - first) throw std::runtime_error("a distance that reaches in front of the block");
    for (uint32_t k = 0; k < len; ++k) out.push_back(out[out.size() - distance]);
  }
}

static uint32_t crc32_of(const char *p, size_t n) {
  uint32_t table[256], c = 0xffffffffu;
  for (uint32_t i = 0; i < 256; ++i) table[i] = cfr::gz_crc_entry(i);
  for (size_t i = 0; i < n; ++i) c = cfr::gz_crc_byte(table, c, (uint8_t)p[i]);
  return c ^ 0xffffffffu;
}

static bool g_dynamic = false;             // argv[2] == "dynamic": codes = 1, and BTYPE 10 is expected
static size_t g_dynamic_members = 0;

static std::string undo(const uint8_t *m, uint64_t n, uint32_t block_bytes) {
  std::string out;
  uint64_t at = 0;
  while (at < n) {
    if (n - at < 26 || m[at] != 0x1f || m[at + 1] != 0x8b || m[at + 3] != 4 || m[at + 12] != 'B' || m[at + 13] != 'C') throw std::runtime_error("not a BGZF member");
    const uint32_t size = (uint32_t)(m[at + 16] | (m[at + 17] << 8)) + 1;
    if (size > 65536 || at + size > n) throw std::runtime_error("BSIZE reaches behind the output");
    const size_t before = out.size();
    Bits in{m + at + 18, m + at + size - 8};
    if (in.bit() != 1) throw std::runtime_error("BFINAL is not set");
    const uint32_t type = in.low_first(2);
    if (type == 0) {
      const uint8_t *s = m + at + 19;
      const uint32_t len = (uint32_t)(s[0] | (s[1] << 8));
      if ((uint32_t)(s[2] | (s[3] << 8)) != (~len & 0xffffu) || 23 + len + 8 != size) throw std::runtime_error("a bad stored block");
      out.append((const char *)s + 4, len);
    } else if (type == 1 || (type == 2 && g_dynamic)) {
      if (type == 1) inflate_fixed(in, out); else { inflate_dynamic(in, out); ++g_dynamic_members; }
      if (in.p + (in.at ? 1 : 0) != in.end) throw std::runtime_error("bytes between the stream and the trailer");
    } else throw std::runtime_error("a block type the twin does not write");
    const uint8_t *t = m + at + size - 8;
    const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    if (isize != out.size() - before || isize > block_bytes || crc != crc32_of(out.data() + before, isize)) throw std::runtime_error("CRC32 / ISIZE");
    at += size;
  }
  return out;
}

int main(int argc, char **argv) {
  if (argc != 2 && !(argc == 3 && !strcmp(argv[2], "dynamic"))) { fprintf(stderr, "usage: %s corpus.bin [dynamic]\n", argv[0]); return 2; }
  g_dynamic = argc == 3;
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  size_t n_items = 0;
  try {
    for (int kind; (kind = fgetc(f)) != EOF;) {
      uint32_t bb = 0;
      uint64_t n = 0;
      if (!get(f, &bb, 4) || !get(f, &n, 8)) throw std::runtime_error("short corpus file");
      cfr_gz_options o{};
      o.block_bytes = (int32_t)bb;
      o.codes = g_dynamic ? 1 : 0;
      std::unique_ptr<cfr::Gz> g[2];
      o.threads = 1; g[0].reset(cfr::make_gz_host(o));
      o.threads = 3; g[1].reset(cfr::make_gz_host(o));
      bool ok = true;
      if (kind == 'T') {
        uint8_t *text = block<uint8_t>(f, n, ok);
        if (!ok) throw std::runtime_error("short corpus file");
        const uint8_t *out[2];
        uint64_t out_n[2];
        for (int k = 0; k < 2; ++k) g[k]->compress(text, n, &out[k], &out_n[k]);
        if (!same(out[0], out_n[0], out[1], out_n[1])) throw std::runtime_error("1 and 3 threads give different bytes");
        const std::string back = undo(out[0], out_n[0], bb);
        if (!same((const uint8_t *)back.data(), back.size(), text, n)) throw std::runtime_error("text item " + std::to_string(n_items) + " does not come back");
        free(text);
      } else if (kind == 'D') {
        uint32_t n_files = 0;
        uint64_t id_bytes = 0;
        if (!get(f, &n_files, 4) || !get(f, &id_bytes, 8) || n_files < 1 || n_files > 4) throw std::runtime_error("short corpus file");
        char *ids = block<char>(f, id_bytes, ok);
        uint64_t *id_off = block<uint64_t>(f, n + 1, ok);
        uint8_t *select = block<uint8_t>(f, n, ok);
        cfr_gz_file files[4];
        std::vector<void *> owned{ids, id_off, select};
        std::vector<std::string> want;
        for (uint32_t k = 0; k < n_files; ++k) {
          uint64_t sizes[2];
          if (!get(f, sizes, 16)) throw std::runtime_error("short corpus file");
          files[k] = cfr_gz_file{nullptr, nullptr, nullptr, nullptr, nullptr};
          files[k].seq = block<uint8_t>(f, sizes[0], ok);
          files[k].seq_off = block<uint64_t>(f, n + 1, ok);
          owned.push_back((void *)files[k].seq); owned.push_back((void *)files[k].seq_off);
          if (sizes[1] != ~0ull) {
            files[k].qual = block<char>(f, sizes[1], ok);
            files[k].qual_off = block<uint64_t>(f, n + 1, ok);
            files[k].has_qual = block<uint8_t>(f, n, ok);
            owned.push_back((void *)files[k].qual); owned.push_back((void *)files[k].qual_off); owned.push_back((void *)files[k].has_qual);
          }
          uint64_t len = 0;
          ok = ok && get(f, &len, 8);
          if (!ok) throw std::runtime_error("short corpus file");
          want.emplace_back(len, '\0');
          if (!get(f, &want.back()[0], len)) throw std::runtime_error("short corpus file");
        }
        const uint8_t *out[2][4];
        uint64_t out_n[2][4];
        for (int k = 0; k < 2; ++k) g[k]->dump(ids, id_off, select, n, files, (int)n_files, out[k], out_n[k]);
        for (uint32_t k = 0; k < n_files; ++k) {
          if (!same(out[0][k], out_n[0][k], out[1][k], out_n[1][k])) throw std::runtime_error("1 and 3 threads give different bytes");
          if (undo(out[0][k], out_n[0][k], bb) != want[k]) throw std::runtime_error("dump item " + std::to_string(n_items) + ", file " + std::to_string(k) + ": not the expected text");
        }
        for (void *p : owned) free(p);
      } else throw std::runtime_error("an item of unknown kind");
      ++n_items;
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "gz_sanitize: %s\n", e.what());
    return 1;
  }
  fclose(f);
  if (g_dynamic) printf("gz_sanitize: %zu members with dynamic codes\n", g_dynamic_members);
  printf("gz_sanitize: %zu items, every text came back\n", n_items);
  return 0;
}
