// cfr_gz_core.hpp — a text cut into BGZF members (the bgzip / htslib framing of gzip), and the records of a read dump, stated once
// for the host twin (cfr_gz.cpp) and for the kernels (cfr_gz.hip).  Both give the same bytes.
//
// Framing.  The text is cut into blocks of block_bytes (1 .. 65280) of input; each block becomes one complete gzip member:
//   the 18-byte header (FLG.FEXTRA, one extra subfield 'B' 'C' of 2 bytes: BSIZE = member size - 1),
//   one deflate stream with BFINAL set,
//   CRC32 and ISIZE of the block's input.
// The stream is either fixed-Huffman (BTYPE 01) or, when that would not be smaller than 5 + n bytes, one stored block (BTYPE 00)
// (in dynamic mode, below, it may also have the block's own codes: BTYPE 10):
// a member is at most 18 + 5 + 65280 + 8 = 65311 bytes.  The 28-byte end-of-file member (kGzEof) is written once by whoever closes a file.
//
// The encoder of one block of n bytes, in[0, n):
//   A table of 2^12 entries, all empty.  The positions are taken in windows of 64: window w is [64 w, 64 w + 64).
//   1. lookup   every position p of the window with p + 4 <= n hashes its 4 bytes and reads the table as the windows BEFORE this one
//               left it.  The entry is a candidate c only if c < p, c < n and p - c <= 32768 (gz_match_len checks this before it
//               reads a byte at c).  The match is extended over in[] to at most min(258, n - p) bytes; fewer than 4 equal bytes: no match.
//   2. insert   every such p then enters the table under its hash; of several positions of one window with one hash the HIGHEST stays
//               (on the device an atomic maximum, on the host the ascending order) - nothing depends on who comes first.
//   3. choose   from the first position that no earlier match covers: a position with a match emits it and skips its length, any
//               other emits its byte as a literal and skips 1 - to the end of the window.  A match may reach into later windows.
//   4. emit     the chosen tokens' codes, back to back in position order (gz_literal, gz_match: RFC 1951, 3.2.6).
//   Behind the last window: the end-of-block code (7 zero bits).
//   Stored: gz_must_store is asked with the bit count after every window, BEFORE the window's bits are written: the answer only ever
//   turns from no to yes, and the last question is the one about the whole stream - so the block is stored exactly when the finished
//   stream would take 5 + n bytes or more, and an encoder never writes at or behind byte 5 + n of its stream.
// A match at a distance below the window's first position is never found inside its own window (a run of one byte: the first window is
// literals, the second window's first position matches at distance 1).  Matches of length 3 are legal deflate but not looked for.
//
// Dynamic mode (cfr_gz_options.codes = 1) keeps steps 1 - 3: the tokens of a block are the same.  They are kept instead of written and
// counted (286 literal/length symbols with the end-of-block symbol once, 30 distance symbols); gz_dyn_build makes both codes
// (gz_code_lengths: limits 15 and 15, and 7 for the code-length code; gz_canonical) and sizes the header (gz_cl_next: how the lengths
// are run-length coded); gz_choose takes the smallest of stored, fixed and dynamic in whole bytes BEFORE a bit is written - equal sizes
// go to stored, then to fixed - so a member that does not come out dynamic (BTYPE 10) has exactly fixed mode's bytes, and a member
// never grows; then the header (gz_put_dyn_header) and the tokens in the block's codes (gz_token_bits: up to 48 bits a token).
// Each of these is described where it stands, below.
//
// CRC32 (the gzip polynomial, reflected): byte-wise with the 256-entry table of gz_crc_entry.  The device cuts a block into slices of
// kGzCrcSlice bytes counted from the block's END, one per lane; the slice that holds byte 0 starts from 0xffffffff, the others from 0,
// and the states are joined with the matrices "advance by kGzCrcSlice * 2^k zero bytes" (gz_crc_advance_tables): the same value.
//
// Read dumps (ResultWriter::OutputRead / OutputExtraRead): a record is  >id \n seq \n  without a quality string and
// @id \n seq \n + \n qual \n  with one.  A record of kGzRecordLimit (8192) bytes or more is left out of its file - gzprintf formats into
// a buffer of 8192 bytes and writes nothing when the text and its NUL do not fit (tests/test_gz_host_cpu.py pins the boundary against zlib).
#pragma once

#include <cstdint>

#include "../../include/cfr_hip.h"

#ifndef CFR_HD
#if defined(__HIPCC__)
#define CFR_HD __host__ __device__
#else
#define CFR_HD
#endif
#endif

// in front of the counted loops of the serial code build: unrolled and inlined into k_gzd_encode they take it from 109 to 159 registers
// (the compiler's kernel-resource-usage remarks) and gain lane 0 nothing.  Loops without a plain induction step go without it: g++
// does not take the annotation there.  Undefined again at the end of this file.
#define CFR_GZ_ROLLED _Pragma("GCC unroll 1")

namespace cfr {

constexpr uint32_t kGzBlockMax = 65280;        // htslib's BGZF_BLOCK_SIZE: bytes of input per member
constexpr uint32_t kGzHeader = 18, kGzTrailer = 8, kGzStoredHead = 5;
constexpr uint32_t kGzWindow = 64;
constexpr uint32_t kGzHashBits = 12;
constexpr uint32_t kGzMinMatch = 4, kGzMaxMatch = 258, kGzMaxDist = 32768;
constexpr uint32_t kGzCrcSlice = 1024;         // 64 slices cover a block
constexpr uint32_t kGzCrcLevels = 6;           // advance by kGzCrcSlice << k bytes, k < 6
constexpr uint64_t kGzRecordLimit = 8192;
constexpr uint32_t kGzEofBytes = 28;

// a member's slot: 2 bytes of padding (so that the deflate stream begins on a 4-byte boundary), then the member
CFR_HD inline uint32_t gz_slot_stride(uint32_t block_bytes) { return (2 + kGzHeader + kGzStoredHead + block_bytes + kGzTrailer + 15u) & ~15u; }

CFR_HD inline uint32_t gz_load32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
CFR_HD inline uint32_t gz_hash(uint32_t v) { return (v * 2654435761u) >> (32 - kGzHashBits); }

// the match of position p (p < n) with table entry `entry` (0: empty, else candidate + 1): its length (0: none) and distance
CFR_HD inline uint32_t gz_match_len(const uint8_t *in, uint32_t n, uint32_t p, uint32_t entry, uint32_t &dist) {
  if (entry == 0) return 0;
  const uint32_t c = entry - 1;
  if (c >= p || c >= n || p - c > kGzMaxDist) return 0;
  uint32_t lim = n - p;                         // (c < p: c + lim < n as well)
  if (lim > kGzMaxMatch) lim = kGzMaxMatch;
  uint32_t k = 0;
  bool differ = false;
  while (k + 8 <= lim) {
    uint64_t a, b;
    __builtin_memcpy(&a, in + c + k, 8);
    __builtin_memcpy(&b, in + p + k, 8);
    if (a != b) { k += (uint32_t)__builtin_ctzll(a ^ b) >> 3; differ = true; break; }
    k += 8;
  }
  if (!differ) while (k < lim && in[c + k] == in[p + k]) ++k;
  if (k < kGzMinMatch) return 0;
  dist = p - c;
  return k;
}

// the low nbits of v in reverse order (Huffman codes go out most significant bit first)
CFR_HD inline uint32_t gz_rev(uint32_t v, uint32_t nbits) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  v = (v >> 16) | (v << 16);
  return v >> (32 - nbits);
}

// the fixed code of literal/length symbol sym (0 .. 285), ready to OR in: its bit count is returned
CFR_HD inline uint32_t gz_symbol(uint32_t sym, uint64_t &bits) {
  uint32_t code, nb;
  if (sym < 144) { code = 0x30 + sym; nb = 8; }
  else if (sym < 256) { code = 0x190 + (sym - 144); nb = 9; }
  else if (sym < 280) { code = sym - 256; nb = 7; }
  else { code = 0xc0 + (sym - 280); nb = 8; }
  bits = gz_rev(code, nb);
  return nb;
}
CFR_HD inline uint32_t gz_literal(uint32_t byte, uint64_t &bits) { return gz_symbol(byte, bits); }

// the length symbol (257 .. 285) of a match length 3 .. 258, and the distance symbol (0 .. 29) of a distance 1 .. 32768, each with the
// count and the value of the extra bits that follow its code (RFC 1951, 3.2.5)
CFR_HD inline uint32_t gz_len_symbol(uint32_t len, uint32_t &eb, uint32_t &ev) {
  const uint32_t l = len - 3;
  eb = 0; ev = 0;
  if (len == 258) return 285;
  if (l < 8) return 257 + l;
  eb = (31u - (uint32_t)__builtin_clz(l)) - 2;
  ev = l & ((1u << eb) - 1);
  return 257 + 4 * (eb + 1) + ((l >> eb) & 3);
}
CFR_HD inline uint32_t gz_dist_symbol(uint32_t dist, uint32_t &eb, uint32_t &ev) {
  const uint32_t d = dist - 1;
  eb = 0; ev = 0;
  if (d < 4) return d;
  eb = (31u - (uint32_t)__builtin_clz(d)) - 1;
  ev = d & ((1u << eb) - 1);
  return 2 * (eb + 1) + ((d >> eb) & 1);
}

// <length, distance>: length 3 .. 258, distance 1 .. 32768; at most 8 + 5 + 5 + 13 = 31 bits
CFR_HD inline uint32_t gz_match(uint32_t len, uint32_t dist, uint64_t &bits) {
  uint32_t eb, ev, deb, dev;
  const uint32_t sym = gz_len_symbol(len, eb, ev), dc = gz_dist_symbol(dist, deb, dev);
  uint64_t b;
  uint32_t nb = gz_symbol(sym, b);
  b |= (uint64_t)ev << nb;
  nb += eb;
  b |= (uint64_t)gz_rev(dc, 5) << nb;
  nb += 5;
  b |= (uint64_t)dev << nb;
  nb += deb;
  bits = b;
  return nb;
}

constexpr uint32_t kGzFirstBits = 3;           // BFINAL = 1, BTYPE = 01: the value 3 in 3 bits
constexpr uint32_t kGzEndBits = 7;             // symbol 256

// bits: the stream's bits so far, the end-of-block code not counted.  true: a stream that goes on from here takes 5 + n bytes or more.
CFR_HD inline bool gz_must_store(uint64_t bits, uint32_t n) { return ((bits + kGzEndBits + 7) >> 3) >= (uint64_t)kGzStoredHead + n; }

// ---- dynamic mode (cfr_gz_options.codes = 1): the block's own Huffman codes (BTYPE 10) ----
// The tokens are kept instead of written, one u32 each: a literal is its byte, a match is kGzTokMatch | (len - 3) << 15 | (dist - 1).
constexpr uint32_t kGzLitSyms = 286, kGzDistSyms = 30, kGzClSyms = 19, kGzEob = 256;
constexpr uint32_t kGzLitLimit = 15, kGzDistLimit = 15, kGzClLimit = 7;
constexpr uint32_t kGzTokMatch = 1u << 31;
CFR_HD inline uint32_t gz_token_match(uint32_t len, uint32_t dist) { return kGzTokMatch | ((len - 3) << 15) | (dist - 1); }
CFR_HD inline uint32_t gz_token_len(uint32_t tok) { return ((tok >> 15) & 0xff) + 3; }
CFR_HD inline uint32_t gz_token_dist(uint32_t tok) { return (tok & 0x7fff) + 1; }
// the extra bits behind a length symbol / a distance symbol
CFR_HD inline uint32_t gz_len_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
CFR_HD inline uint32_t gz_dist_extra(uint32_t dc) { return dc < 4 ? 0 : (dc >> 1) - 1; }
// the bit count of a symbol in the fixed code
CFR_HD inline uint32_t gz_fixed_len(uint32_t sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
// the order in which the lengths of the code-length code are sent (RFC 1951, 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
CFR_HD inline uint32_t gz_cl_order(uint32_t i) { return (uint32_t)((i < 12 ? 0x22caa324e804a30ull >> (5 * i) : 0x3c2e1346cull >> (5 * (i - 12))) & 31); }

// a[0, m) ascending, in place (heap sort: no array of its own)
CFR_HD inline void gz_sift(uint32_t *a, uint32_t i, uint32_t m) {
  const uint32_t v = a[i];
  CFR_GZ_ROLLED for (uint32_t c = 2 * i + 1; c < m; c = 2 * i + 1) {
    if (c + 1 < m && a[c + 1] > a[c]) ++c;
    if (a[c] <= v) break;
    a[i] = a[c];
    i = c;
  }
  a[i] = v;
}
CFR_HD inline void gz_sort(uint32_t *a, uint32_t m) {
  CFR_GZ_ROLLED for (uint32_t i = m / 2; i-- > 0;) gz_sift(a, i, m);
  CFR_GZ_ROLLED for (uint32_t e = m; e-- > 1;) {
    const uint32_t t = a[0]; a[0] = a[e]; a[e] = t;
    gz_sift(a, 0, e);
  }
}

// Code lengths of at most `limit` bits for n_sym symbols (n_sym <= 512, every frequency below 2^23), by Huffman's algorithm and a
// repair of the Kraft sum:
//   the used symbols (frequency above 0) are sorted by (frequency, symbol number); with fewer than two of them the lowest unused symbols
//   join with frequency 1 (zlib's rule), so every code has two lengths above 0 at least and is complete: its Kraft sum is exactly 1;
//   Huffman's depths are found in place on the sorted frequencies (Moffat and Katajainen, "In-place calculation of minimum-redundancy
//   codes", 1995): they do not grow along the sorted order;
//   depths above the limit are cut to it, which puts the Kraft sum above 1; while it is, a code of `limit` bits is taken out and the
//   longest code shorter than the limit gives way to two codes one bit longer - that takes 2^-limit off the sum and keeps the number
//   of codes; the lengths, longest first, then go to the symbols in sorted order, so a more frequent symbol never has the longer code.
// The repair never runs dry: some depth was cut, so the tree has an internal node at depth limit - 1, and the codes shorter than the limit
// sum to 1 - 2 * 2^-limit at most - a sum that every step only lowers; while the whole sum is above 1, three codes of `limit` bits or more
// make up the rest.  And a shorter code to move exists: n_sym <= 2^limit codes of `limit` bits alone do not exceed 1.  (zlib's own move.)
// len[s] = 0 for every symbol that did not take part.  Workspace: w32[n_sym], w16[n_sym], cnt[16].
CFR_HD inline void gz_code_lengths(const uint32_t *freq, uint32_t n_sym, uint32_t limit, uint8_t *len, uint32_t *w32, uint16_t *w16, uint16_t *cnt) {
  uint32_t m = 0;
  CFR_GZ_ROLLED for (uint32_t s = 0; s < n_sym; ++s) {
    len[s] = 0;
    if (freq[s]) w32[m++] = (freq[s] << 9) | s;
  }
  CFR_GZ_ROLLED for (uint32_t s = 0; m < 2 && s < n_sym; ++s)
    if (!freq[s]) w32[m++] = (1u << 9) | s;
  gz_sort(w32, m);
  CFR_GZ_ROLLED for (uint32_t i = 0; i < m; ++i) { w16[i] = (uint16_t)(w32[i] & 511); w32[i] >>= 9; }
  uint32_t *a = w32;
  const int n = (int)m;
  a[0] += a[1];                                  // the internal nodes' weights, then their parents, in the place the leaves leave
  CFR_GZ_ROLLED for (int root = 0, leaf = 2, next = 1; next < n - 1; ++next) {
    if (leaf >= n || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; } else a[next] = a[leaf++];
    if (leaf >= n || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; } else a[next] += a[leaf++];
  }
  a[n - 2] = 0;                                  // the internal nodes' depths
  CFR_GZ_ROLLED for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
  CFR_GZ_ROLLED for (int avail = 1, used = 0, depth = 0, root = n - 2, next = n - 1; avail > 0;) {   // the leaves' depths: a[0] is the deepest
    while (root >= 0 && (int)a[root] == depth) { ++used; --root; }
    CFR_GZ_ROLLED while (avail > used) { a[next--] = (uint32_t)depth; --avail; }
    avail = 2 * used; ++depth; used = 0;
  }
  CFR_GZ_ROLLED for (uint32_t l = 0; l <= limit; ++l) cnt[l] = 0;
  CFR_GZ_ROLLED for (uint32_t i = 0; i < m; ++i) ++cnt[a[i] < limit ? a[i] : limit];
  uint32_t kraft = 0;                            // in units of 2^-limit
  CFR_GZ_ROLLED for (uint32_t l = 1; l <= limit; ++l) kraft += (uint32_t)cnt[l] << (limit - l);
  for (; kraft > (1u << limit); --kraft) {
    --cnt[limit];
    CFR_GZ_ROLLED for (uint32_t l = limit - 1; l > 0; --l)
      if (cnt[l]) { --cnt[l]; cnt[l + 1] += 2; break; }
  }
  uint32_t i = 0;
  CFR_GZ_ROLLED for (uint32_t l = limit; l > 0; --l)
    CFR_GZ_ROLLED for (uint32_t c = 0; c < cnt[l]; ++c) len[w16[i++]] = (uint8_t)l;
}

// canonical codes (RFC 1951, 3.2.2) of the lengths: tab[s] = the code's bits, reversed and ready to OR in, | length << 16; 0: no code.
CFR_HD inline void gz_canonical(const uint8_t *len, uint32_t n_sym, uint32_t *tab, uint16_t *cnt) {
  CFR_GZ_ROLLED for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
  CFR_GZ_ROLLED for (uint32_t s = 0; s < n_sym; ++s) ++cnt[len[s]];
  uint32_t code = 0, prev = 0;
  CFR_GZ_ROLLED for (uint32_t l = 1; l < 16; ++l) {           // cnt[l] becomes the next code of length l
    code = (code + prev) << 1;
    prev = cnt[l];
    cnt[l] = (uint16_t)code;
  }
  CFR_GZ_ROLLED for (uint32_t s = 0; s < n_sym; ++s) {
    const uint32_t l = len[s];
    tab[s] = l ? gz_rev(cnt[l]++, l) | (l << 16) : 0u;
  }
}
// the fixed code in the same form
CFR_HD inline uint32_t gz_fixed_entry(uint32_t sym) { uint64_t b; const uint32_t nb = gz_symbol(sym, b); return (uint32_t)b | (nb << 16); }
CFR_HD inline uint32_t gz_fixed_dist_entry(uint32_t dc) { return gz_rev(dc, 5) | (5u << 16); }

// a kept token in the codes of ltab / dtab: at most 15 + 5 + 15 + 13 = 48 bits
CFR_HD inline uint32_t gz_token_bits(uint32_t tok, const uint32_t *ltab, const uint32_t *dtab, uint64_t &bits) {
  if (!(tok & kGzTokMatch)) { const uint32_t e = ltab[tok]; bits = e & 0xffff; return e >> 16; }
  uint32_t eb, ev, deb, dev;
  const uint32_t le = ltab[gz_len_symbol(gz_token_len(tok), eb, ev)], de = dtab[gz_dist_symbol(gz_token_dist(tok), deb, dev)];
  uint64_t b = le & 0xffff;
  uint32_t nb = le >> 16;
  b |= (uint64_t)ev << nb;
  nb += eb;
  b |= (uint64_t)(de & 0xffff) << nb;
  nb += de >> 16;
  b |= (uint64_t)dev << nb;
  nb += deb;
  bits = b;
  return nb;
}

// The lengths of the two codes are sent as ONE sequence seq[0, total) (literal/length code first) in the code-length alphabet, by this
// greedy rule, from position i on:
//   a zero with 11 or more equal neighbours from i: symbol 18 for as many as fit (up to 138); with 3 .. 10: symbol 17;
//   a length above 0 that equals the one in front of it and has 3 or more from i: symbol 16 for up to 6 of them;
//   anything else is sent as itself - so a new length is sent once before a 16 can follow, and remainders of 1 or 2 go as themselves.
// Returns the position behind what the symbol covers.
CFR_HD inline uint32_t gz_cl_next(const uint8_t *seq, uint32_t total, uint32_t i, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
  const uint32_t v = seq[i];
  uint32_t run = 1;
  while (i + run < total && run < 138 && seq[i + run] == v) ++run;
  if (v == 0 && run >= 11) { sym = 18; eb = 7; ev = run - 11; return i + run; }
  if (v == 0 && run >= 3) { sym = 17; eb = 3; ev = run - 3; return i + run; }
  if (v != 0 && run >= 3 && i > 0 && seq[i - 1] == v) {
    if (run > 6) run = 6;
    sym = 16; eb = 2; ev = run - 3;
    return i + run;
  }
  sym = v; eb = 0; ev = 0;
  return i + 1;
}

// everything the code build of one block works on: LDS on the device, the stack on the host
struct GzDynWork {
  uint32_t *lfreq, *dfreq;        // kGzLitSyms, kGzDistSyms: the histograms (the end-of-block symbol counted)
  uint32_t *ltab, *dtab;          // the same sizes: the codes, as gz_canonical leaves them
  uint32_t *clfreq, *cltab;       // kGzClSyms each
  uint8_t *lens;                  // kGzLitSyms + kGzDistSyms: the two codes' lengths, then the sequence that is sent
  uint8_t *cllen;                 // kGzClSyms
  uint32_t *w32;                  // kGzLitSyms
  uint16_t *w16, *cnt;            // kGzLitSyms, 16
};
struct GzDynPlan { uint32_t hlit, hdist, hclen, fixed_bits, dyn_bits; };

// From the histograms: both codes, the header's shape and the two streams' sizes in bits (first three bits and end-of-block included).
// HLIT and HDIST end at the highest symbol with a code, HCLEN at the last length above 0 in gz_cl_order, 4 at least.
CFR_HD inline GzDynPlan gz_dyn_build(const GzDynWork &w) {
  GzDynPlan p;
  gz_code_lengths(w.lfreq, kGzLitSyms, kGzLitLimit, w.lens, w.w32, w.w16, w.cnt);
  gz_code_lengths(w.dfreq, kGzDistSyms, kGzDistLimit, w.lens + kGzLitSyms, w.w32, w.w16, w.cnt);
  gz_canonical(w.lens, kGzLitSyms, w.ltab, w.cnt);
  gz_canonical(w.lens + kGzLitSyms, kGzDistSyms, w.dtab, w.cnt);
  uint32_t extra = 0, fixed = 0, dyn = 0;
  CFR_GZ_ROLLED for (uint32_t s = 0; s < kGzLitSyms; ++s) {
    const uint32_t f = w.lfreq[s];
    fixed += f * gz_fixed_len(s);
    dyn += f * w.lens[s];
    if (s > kGzEob) extra += f * gz_len_extra(s);
  }
  CFR_GZ_ROLLED for (uint32_t d = 0; d < kGzDistSyms; ++d) {
    const uint32_t f = w.dfreq[d];
    fixed += f * 5;
    dyn += f * w.lens[kGzLitSyms + d];
    extra += f * gz_dist_extra(d);
  }
  p.hlit = kGzLitSyms;
  while (p.hlit > kGzEob + 1 && !w.lens[p.hlit - 1]) --p.hlit;
  p.hdist = kGzDistSyms;
  while (p.hdist > 1 && !w.lens[kGzLitSyms + p.hdist - 1]) --p.hdist;
  CFR_GZ_ROLLED for (uint32_t d = 0; d < p.hdist; ++d) w.lens[p.hlit + d] = w.lens[kGzLitSyms + d];      // one sequence (moved down in ascending order: read before overwritten)
  const uint32_t total = p.hlit + p.hdist;
  CFR_GZ_ROLLED for (uint32_t s = 0; s < kGzClSyms; ++s) w.clfreq[s] = 0;
  uint32_t head = 3 + 5 + 5 + 4;
  CFR_GZ_ROLLED for (uint32_t i = 0; i < total;) {
    uint32_t sym, eb, ev;
    i = gz_cl_next(w.lens, total, i, sym, eb, ev);
    ++w.clfreq[sym];
    head += eb;
  }
  gz_code_lengths(w.clfreq, kGzClSyms, kGzClLimit, w.cllen, w.w32, w.w16, w.cnt);
  gz_canonical(w.cllen, kGzClSyms, w.cltab, w.cnt);
  p.hclen = kGzClSyms;
  while (p.hclen > 4 && !w.cllen[gz_cl_order(p.hclen - 1)]) --p.hclen;
  head += 3 * p.hclen;
  CFR_GZ_ROLLED for (uint32_t s = 0; s < kGzClSyms; ++s) head += w.clfreq[s] * w.cllen[s];
  p.fixed_bits = kGzFirstBits + fixed + extra;
  p.dyn_bits = head + dyn + extra;
  return p;
}

// 0: stored, 1: fixed, 2: dynamic - the smallest in whole bytes; equal sizes go to stored, then to fixed.  So a block that does not
// come out dynamic has the bytes fixed mode gives it (there gz_must_store's last answer is the same comparison), a dynamic stream is
// shorter than 5 + n bytes, and no encoder writes at or behind byte 5 + n of its stream.
CFR_HD inline uint32_t gz_choose(uint32_t n, const GzDynPlan &p) {
  const uint32_t stored = kGzStoredHead + n, fixed = (p.fixed_bits + 7) >> 3, dyn = (p.dyn_bits + 7) >> 3;
  if (stored <= fixed && stored <= dyn) return 0;
  return fixed <= dyn ? 1 : 2;
}

// the stream's bits into 32-bit words at p (4-byte aligned; little-endian as gz_match_len's loads are), least significant bit first
struct GzWordSink {
  uint8_t *p;
  uint64_t acc;
  uint32_t have;                  // below 32 between calls
  CFR_HD void put(uint64_t bits, uint32_t nb) {           // nb <= 32
    acc |= bits << have;
    have += nb;
    if (have >= 32) {
      const uint32_t word = (uint32_t)acc;
      __builtin_memcpy(__builtin_assume_aligned(p, 4), &word, 4);
      p += 4; acc >>= 32; have -= 32;
    }
  }
};

// BFINAL = 1 and BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code's lengths, the sequence: p.dyn_bits minus body and end-of-block
CFR_HD inline void gz_put_dyn_header(GzWordSink &sink, const GzDynWork &w, const GzDynPlan &p) {
  sink.put(5, 3);
  sink.put(p.hlit - 257, 5);
  sink.put(p.hdist - 1, 5);
  sink.put(p.hclen - 4, 4);
  CFR_GZ_ROLLED for (uint32_t i = 0; i < p.hclen; ++i) sink.put(w.cllen[gz_cl_order(i)], 3);
  const uint32_t total = p.hlit + p.hdist;
  CFR_GZ_ROLLED for (uint32_t i = 0; i < total;) {
    uint32_t sym, eb, ev;
    i = gz_cl_next(w.lens, total, i, sym, eb, ev);
    sink.put(w.cltab[sym] & 0xffff, w.cltab[sym] >> 16);
    sink.put(ev, eb);
  }
}

// the 18 bytes in front of the stream / the 8 behind it
CFR_HD inline void gz_put_header(uint8_t *m, uint32_t member_bytes) {
  const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
  for (int i = 0; i < 16; ++i) m[i] = h[i];
  m[16] = (uint8_t)((member_bytes - 1) & 0xff);
  m[17] = (uint8_t)((member_bytes - 1) >> 8);
}
CFR_HD inline void gz_put_trailer(uint8_t *t, uint32_t crc, uint32_t n) {
  for (int i = 0; i < 4; ++i) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(n >> (8 * i)); }
}
CFR_HD inline void gz_put_stored_head(uint8_t *d, uint32_t n) {
  d[0] = 1;
  d[1] = (uint8_t)(n & 0xff); d[2] = (uint8_t)(n >> 8);
  d[3] = (uint8_t)(~n & 0xff); d[4] = (uint8_t)((~n >> 8) & 0xff);
}

CFR_HD inline uint32_t gz_crc_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  return c;
}
CFR_HD inline uint32_t gz_crc_byte(const uint32_t *table, uint32_t crc, uint8_t b) { return table[(crc ^ b) & 0xff] ^ (crc >> 8); }
// mat (32 words: the images of the 32 state bits) applied to a state
CFR_HD inline uint32_t gz_gf2_times(const uint32_t *mat, uint32_t v) {
  uint32_t s = 0;
  for (int j = 0; j < 32; ++j) s ^= mat[j] & (0u - ((v >> j) & 1u));
  return s;
}
// out[k * 32 .. +32): the state advanced over kGzCrcSlice << k zero bytes, k < kGzCrcLevels
inline void gz_crc_advance_tables(uint32_t *out) {
  uint32_t m[32], t[32];
  for (int j = 0; j < 32; ++j) {                // one zero byte
    uint32_t c = 1u << j;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    m[j] = c;
  }
  uint32_t bytes = 1;
  for (uint32_t level = 0;;) {
    if (bytes >= kGzCrcSlice) {
      for (int j = 0; j < 32; ++j) out[level * 32 + j] = m[j];
      if (++level == kGzCrcLevels) return;
    }
    for (int j = 0; j < 32; ++j) t[j] = gz_gf2_times(m, m[j]);
    for (int j = 0; j < 32; ++j) m[j] = t[j];
    bytes *= 2;
  }
}

// ---- the records of a read dump ----
// one file of a dump: sequences (or barcode / UMI strings) and, where a read has one, its quality string
struct GzFileView {
  const uint8_t *seq;
  const uint64_t *seq_off;      // n + 1
  const char *qual;             // nullptr: no read of this file has a quality string
  const uint64_t *qual_off;     // n + 1
  const uint8_t *has_qual;      // n
};
CFR_HD inline bool gz_has_qual(const GzFileView &f, uint64_t i) { return f.qual && f.qual_off && f.has_qual && f.has_qual[i]; }
// the bytes of read i's record in file f; 0: not selected, or the record is one that gzprintf drops
CFR_HD inline uint64_t gz_record_len(const GzFileView &f, const uint64_t *id_off, const uint8_t *select, uint64_t i) {
  if (!select[i]) return 0;
  const uint64_t id = id_off[i + 1] - id_off[i], s = f.seq_off[i + 1] - f.seq_off[i];
  const uint64_t len = gz_has_qual(f, i) ? 1 + id + 1 + s + 3 + (f.qual_off[i + 1] - f.qual_off[i]) + 1 : 1 + id + 1 + s + 1;
  return len >= kGzRecordLimit ? 0 : len;
}
// byte j of that record (j below its length)
CFR_HD inline uint8_t gz_record_byte(const GzFileView &f, const char *id_bytes, const uint64_t *id_off, uint64_t i, uint64_t j) {
  const bool q = gz_has_qual(f, i);
  if (j == 0) return q ? '@' : '>';
  j -= 1;
  const uint64_t id = id_off[i + 1] - id_off[i];
  if (j < id) return (uint8_t)id_bytes[id_off[i] + j];
  if (j == id) return '\n';
  j -= id + 1;
  const uint64_t s = f.seq_off[i + 1] - f.seq_off[i];
  if (j < s) return f.seq[f.seq_off[i] + j];
  if (j == s) return '\n';
  j -= s + 1;
  if (j == 0) return '+';
  if (j == 1) return '\n';
  j -= 2;
  const uint64_t ql = f.qual_off[i + 1] - f.qual_off[i];
  return j < ql ? (uint8_t)f.qual[f.qual_off[i] + j] : (uint8_t)'\n';
}

}  // namespace cfr

#undef CFR_GZ_ROLLED
