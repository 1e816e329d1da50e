// cfr_gz_core.hpp — a text cut into BGZF members (the bgzip / htslib framing of gzip), and the records of a read dump, stated once
// for the host twin (cfr_gz.cpp) and for the kernels (cfr_gz.hip).  Both give the same bytes.
//
// Framing.  The text is cut into blocks of block_bytes (1 .. 65280) of input; each block becomes one complete gzip member:
//   the 18-byte header (FLG.FEXTRA, one extra subfield 'B' 'C' of 2 bytes: BSIZE = member size - 1),
//   one deflate stream with BFINAL set,
//   CRC32 and ISIZE of the block's input.
// The stream is either fixed-Huffman (BTYPE 01) or, when that would not be smaller than 5 + n bytes, one stored block (BTYPE 00):
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

// <length, distance>: length 3 .. 258, distance 1 .. 32768; at most 8 + 5 + 5 + 13 = 31 bits
CFR_HD inline uint32_t gz_match(uint32_t len, uint32_t dist, uint64_t &bits) {
  uint32_t sym, eb = 0, ev = 0;
  const uint32_t l = len - 3;
  if (len == 258) sym = 285;
  else if (l < 8) sym = 257 + l;
  else {
    eb = (31u - (uint32_t)__builtin_clz(l)) - 2;
    sym = 257 + 4 * (eb + 1) + ((l >> eb) & 3);
    ev = l & ((1u << eb) - 1);
  }
  uint64_t b;
  uint32_t nb = gz_symbol(sym, b);
  b |= (uint64_t)ev << nb;
  nb += eb;
  const uint32_t d = dist - 1;
  uint32_t dc, deb = 0, dev = 0;
  if (d < 4) dc = d;
  else {
    deb = (31u - (uint32_t)__builtin_clz(d)) - 1;
    dc = 2 * (deb + 1) + ((d >> deb) & 1);
    dev = d & ((1u << deb) - 1);
  }
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
