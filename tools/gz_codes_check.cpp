// gz_codes_check.cpp — a stand-alone driver of the code build of the compressor's dynamic mode (csrc/cfr_gz_core.hpp: gz_code_lengths,
// gz_canonical, gz_dyn_build, gz_put_dyn_header), for sanitizer builds; it includes the core header and nothing else of the library:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/gz_codes_check.cpp
//       -o gz_codes_check && ./gz_codes_check
// Histograms over 286, 30 and 19 symbols with the limits 15, 15 and 7: Fibonacci frequencies (Huffman's deepest tree), one used symbol,
// two, all equal, one symbol with 65280 beside ones, and nothing but the end-of-block symbol.  For every one:
//   no length above the limit; the Kraft sum is exactly 1; length 0 exactly for the symbols that took no part (with fewer than two
//   used symbols the lowest unused ones take part); a more frequent symbol never has the longer code; the canonical codes are
//   those of RFC 1951, 3.2.2, restated here.
// For pairs of them as literal/length and distance histograms: the header gz_put_dyn_header writes is read back by a parser of this
// file's own and gives the lengths, HLIT / HDIST / HCLEN are trimmed, and its size is what gz_dyn_build said.
// Every workspace is a heap block of exactly its size, so that a step past its end is a report.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../centrifuger_amd/csrc/cfr_gz_core.hpp"

using namespace cfr;

static void need(bool ok, const std::string &what) { if (!ok) throw std::runtime_error(what); }

template <class T> struct Heap {                // exactly n entries
  T *p;
  explicit Heap(size_t n) : p((T *)malloc(n * sizeof(T))) { memset(p, 0xa5, n * sizeof(T)); }
  ~Heap() { free(p); }
  Heap(const Heap &) = delete;
};

static std::vector<uint32_t> fibonacci(uint32_t n) {      // capped at 65536: the sums stay inside 32 bits
  std::vector<uint32_t> f(n);
  uint64_t a = 1, b = 1;
  for (uint32_t i = 0; i < n; ++i) { f[i] = (uint32_t)(a < 65536 ? a : 65536); const uint64_t c = a + b; a = b; b = c < (1ull << 40) ? c : (1ull << 40); }
  return f;
}

struct Histogram { std::string name; std::vector<uint32_t> freq; };

static std::vector<Histogram> histograms(uint32_t n) {
  std::vector<Histogram> h;
  h.push_back({"fibonacci", fibonacci(n)});
  { auto f = fibonacci(n); std::vector<uint32_t> r(f.rbegin(), f.rend()); h.push_back({"fibonacci, descending", r}); }
  { std::vector<uint32_t> f(n, 0); f[n / 2] = 7; h.push_back({"one used symbol", f}); }
  { std::vector<uint32_t> f(n, 0); f[0] = 9; h.push_back({"symbol 0 alone", f}); }
  { std::vector<uint32_t> f(n, 0); f[1] = 3; f[n - 1] = 1000; h.push_back({"two used symbols", f}); }
  h.push_back({"all equal", std::vector<uint32_t>(n, 5)});
  { std::vector<uint32_t> f(n, 1); f[n / 3] = 65280; h.push_back({"one heavy symbol", f}); }
  { std::vector<uint32_t> f(n, 0); f[n - 1] = 1; h.push_back({"the last symbol once", f}); }
  return h;
}

// lengths of one histogram, checked; returns them
static std::vector<uint8_t> check_lengths(const Histogram &h, uint32_t limit) {
  const uint32_t n = (uint32_t)h.freq.size();
  Heap<uint32_t> freq(n), w32(n), tab(n);
  Heap<uint16_t> w16(n), cnt(16);
  Heap<uint8_t> len(n);
  memcpy(freq.p, h.freq.data(), n * 4);
  gz_code_lengths(freq.p, n, limit, len.p, w32.p, w16.p, cnt.p);
  const std::string at = h.name + " over " + std::to_string(n) + " symbols: ";
  uint32_t used = 0;
  for (uint32_t s = 0; s < n; ++s) used += h.freq[s] != 0;
  std::vector<uint32_t> part(h.freq);                                     // the frequencies that take part: zlib's rule
  for (uint32_t s = 0, u = used; u < 2 && s < n; ++s) if (!part[s]) { part[s] = 1; ++u; }
  uint64_t kraft = 0;
  for (uint32_t s = 0; s < n; ++s) {
    if (len.p[s] > limit) need(false, at + "a length above the limit");
    if ((len.p[s] == 0) != (part[s] == 0)) need(false, at + "length 0 and frequency 0 do not go together at symbol " + std::to_string(s));
    if (len.p[s]) kraft += 1ull << (limit - len.p[s]);
  }
  need(kraft == 1ull << limit, at + "the Kraft sum is not 1");
  bool monotone = true;
  for (uint32_t a = 0; a < n; ++a)
    for (uint32_t b = 0; b < n; ++b) monotone = monotone && !(part[a] > part[b] && part[b] && len.p[a] > len.p[b]);
  need(monotone, at + "a more frequent symbol has the longer code");
  // canonical codes, restated: count the lengths, first code of every length, codes in symbol order
  gz_canonical(len.p, n, tab.p, cnt.p);
  uint32_t count[17] = {0}, next[17] = {0};
  for (uint32_t s = 0; s < n; ++s) ++count[len.p[s]];
  count[0] = 0;
  for (uint32_t l = 1, code = 0; l <= 15; ++l) { code = (code + count[l - 1]) << 1; next[l] = code; }
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = len.p[s];
    if (!l) { if (tab.p[s]) need(false, at + "a code for a symbol without a length"); continue; }
    const uint32_t code = next[l]++;
    uint32_t rev = 0;
    for (uint32_t k = 0; k < l; ++k) rev |= ((code >> k) & 1) << (l - 1 - k);
    if (tab.p[s] != (rev | (l << 16))) need(false, at + "not the canonical code at symbol " + std::to_string(s));
  }
  return std::vector<uint8_t>(len.p, len.p + n);
}

struct Reader {
  const uint8_t *p;
  size_t n_bits, at = 0;
  uint32_t bits(uint32_t k) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < k; ++i, ++at) {
      need(at < n_bits, "the header ends early");
      v |= (uint32_t)((p[at >> 3] >> (at & 7)) & 1) << i;
    }
    return v;
  }
};

// the header of (lfreq, dfreq) written and read back
static void check_header(const Histogram &l, const Histogram &d) {
  const std::string at = "header of (" + l.name + ", " + d.name + "): ";
  Heap<uint32_t> lfreq(kGzLitSyms), dfreq(kGzDistSyms), ltab(kGzLitSyms), dtab(kGzDistSyms), clfreq(kGzClSyms), cltab(kGzClSyms), w32(kGzLitSyms);
  Heap<uint8_t> lens(kGzLitSyms + kGzDistSyms), cllen(kGzClSyms);
  Heap<uint16_t> w16(kGzLitSyms), cnt(16);
  memcpy(lfreq.p, l.freq.data(), kGzLitSyms * 4);
  memcpy(dfreq.p, d.freq.data(), kGzDistSyms * 4);
  if (!lfreq.p[kGzEob]) lfreq.p[kGzEob] = 1;                                 // the encoder always counts it
  const GzDynWork w{lfreq.p, dfreq.p, ltab.p, dtab.p, clfreq.p, cltab.p, lens.p, cllen.p, w32.p, w16.p, cnt.p};
  const GzDynPlan plan = gz_dyn_build(w);
  // what the lengths must be: the code build on each histogram alone
  Histogram l1{l.name, std::vector<uint32_t>(lfreq.p, lfreq.p + kGzLitSyms)};
  const std::vector<uint8_t> want_l = check_lengths(l1, kGzLitLimit), want_d = check_lengths(d, kGzDistLimit);
  uint64_t body = 0;
  for (uint32_t s = 0; s < kGzLitSyms; ++s) body += (uint64_t)lfreq.p[s] * (want_l[s] + (s > kGzEob ? gz_len_extra(s) : 0));
  for (uint32_t s = 0; s < kGzDistSyms; ++s) body += (uint64_t)dfreq.p[s] * (want_d[s] + gz_dist_extra(s));
  need(body < plan.dyn_bits, at + "dyn_bits is smaller than the body");
  const size_t head_bits = plan.dyn_bits - body;
  const size_t words = (head_bits + 31) / 32;
  Heap<uint8_t> out(words * 4);
  GzWordSink sink{out.p, 0, 0};
  gz_put_dyn_header(sink, w, plan);
  need((size_t)(sink.p - out.p) * 8 + sink.have == head_bits, at + "the header's size is not the one gz_dyn_build counted");
  for (uint32_t k = 0; k * 8 < sink.have; ++k) sink.p[k] = (uint8_t)(sink.acc >> (8 * k));
  Reader r{out.p, head_bits};
  need(r.bits(1) == 1 && r.bits(2) == 2, at + "BFINAL / BTYPE");
  const uint32_t hlit = r.bits(5) + 257, hdist = r.bits(5) + 1, hclen = r.bits(4) + 4;
  need(hlit == plan.hlit && hdist == plan.hdist && hclen == plan.hclen, at + "HLIT / HDIST / HCLEN are not the plan's");
  need(hlit <= kGzLitSyms && hdist <= kGzDistSyms && hclen <= kGzClSyms, at + "HLIT / HDIST / HCLEN out of range");
  uint8_t cl[19] = {0};
  static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (uint32_t i = 0; i < hclen; ++i) { need(gz_cl_order(i) == order[i], at + "gz_cl_order"); cl[order[i]] = (uint8_t)r.bits(3); }
  need(hclen == 4 || cl[order[hclen - 1]], at + "HCLEN is not trimmed");
  uint64_t kraft = 0;
  for (uint32_t s = 0; s < 19; ++s) { need(cl[s] <= kGzClLimit, at + "a code-length code above 7 bits"); if (cl[s]) kraft += 1u << (7 - cl[s]); }
  need(kraft == 128, at + "the code-length code's Kraft sum is not 1");
  uint32_t count[9] = {0}, next[9] = {0};
  for (uint32_t s = 0; s < 19; ++s) ++count[cl[s]];
  count[0] = 0;
  for (uint32_t k = 1, code = 0; k <= 7; ++k) { code = (code + count[k - 1]) << 1; next[k] = code; }
  uint32_t code_of[19];
  for (uint32_t s = 0; s < 19; ++s) code_of[s] = cl[s] ? next[cl[s]]++ : 0;
  std::vector<uint8_t> seq;
  while (seq.size() < hlit + hdist) {
    uint32_t code = 0, k = 0, sym = 19;
    while (sym == 19) {
      code = (code << 1) | r.bits(1);
      need(++k <= 7, at + "no code of the code-length code matches");
      for (uint32_t s = 0; s < 19; ++s) if (cl[s] == k && code_of[s] == code) sym = s;
    }
    if (sym < 16) { seq.push_back((uint8_t)sym); continue; }
    uint32_t rep;
    uint8_t v = 0;
    if (sym == 16) { need(!seq.empty(), at + "a repeat with nothing in front"); v = seq.back(); rep = 3 + r.bits(2); }
    else if (sym == 17) rep = 3 + r.bits(3);
    else rep = 11 + r.bits(7);
    seq.insert(seq.end(), rep, v);
  }
  need(seq.size() == hlit + hdist, at + "a repeat runs over the end of the lengths");
  need(r.at == head_bits, at + "bits left between the header and the body");
  for (uint32_t s = 0; s < kGzLitSyms; ++s)
    if ((s < hlit ? seq[s] : 0) != want_l[s]) need(false, at + "literal/length code, symbol " + std::to_string(s));
  for (uint32_t s = 0; s < kGzDistSyms; ++s)
    if ((s < hdist ? seq[hlit + s] : 0) != want_d[s]) need(false, at + "distance code, symbol " + std::to_string(s));
  need(hlit == 257 || seq[hlit - 1], at + "HLIT is not trimmed");
  need(seq[hlit + hdist - 1], at + "HDIST is not trimmed");
}

int main() {
  size_t checks = 0;
  try {
    const uint32_t sizes[3] = {kGzLitSyms, kGzDistSyms, kGzClSyms}, limits[3] = {kGzLitLimit, kGzDistLimit, kGzClLimit};
    for (int k = 0; k < 3; ++k)
      for (const Histogram &h : histograms(sizes[k])) { check_lengths(h, limits[k]); ++checks; }
    for (const Histogram &l : histograms(kGzLitSyms))
      for (const Histogram &d : histograms(kGzDistSyms)) { check_header(l, d); ++checks; }
    // no distance at all: the distance code is the two forced symbols
    check_header(histograms(kGzLitSyms)[0], Histogram{"no distance", std::vector<uint32_t>(kGzDistSyms, 0)});
    ++checks;
  } catch (const std::exception &e) {
    fprintf(stderr, "gz_codes_check: %s\n", e.what());
    return 1;
  }
  printf("gz_codes_check: %zu checks, every one held\n", checks);
  return 0;
}
