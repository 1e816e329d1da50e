// cfr_inflate_core.hpp — BGZF members back into text: the framing, all of deflate (RFC 1951) within one member and the status a member
// gets, stated once for the host twin (cfr_inflate.cpp) and for the kernel (cfr_inflate.hip).  Both give the same text and statuses.
//
// Framing (the rule of the command line's BGZF reader, restated so that the library does not depend on it): a member starts with
// 1f 8b 08 and FLG.FEXTRA set; the extra field (XLEN bytes from byte 12) holds a subfield 'B' 'C' of length 2 anywhere in it:
// BSIZE = member size - 1.  The deflate stream is the bytes [12 + XLEN, size - 8); the trailer is CRC32 and ISIZE.  Input that does
// not frame is no member at all (inf_frame: false; the call is refused).  A framed member with ISIZE above 65536 is refused as a
// member (CFR_INF_BAD_HEADER) and owns no text.  ISIZE = 0 (the 28-byte end-of-file member) is legal anywhere and gives no text.
//
// Deflate: any number of blocks; stored (LEN / NLEN checked), fixed and dynamic; code lengths up to 15 (7 for the code-length code);
// the repeat codes 16 / 17 / 18, a run may cross from the literal/length lengths into the distance lengths; distances up to 32768 but
// never in front of the member's first byte; copies that overlap their source read src[i % distance]; length 258.  Code sets are
// judged as zlib judges them (inf_check_set): over-subscribed sets are refused; incomplete sets are refused except a set whose only
// code has length 1 (zlib allows that for the distance code - and for a literal/length code that is the end-of-block symbol alone);
// a distance set without any code is legal as long as no distance is used; HLIT above 286, HDIST above 30 and a literal/length set
// without the end-of-block symbol are refused.
//
// The status of a member is the FIRST rule violated in decode order (inf_member states the order): every check stands in front of
// the access it guards.  The bit reader is m.peek(pos): 32 bits of the stream from bit pos on, ZERO behind the stream's last byte -
// so a lookup never reads memory behind the member, and a code or field counts only when all its bits lie inside the stream
// (pos + bits <= total_bits, checked before pos moves: CFR_INF_INPUT).  A code that no symbol has is CFR_INF_BAD_SYMBOL when 15 real
// bits were there and CFR_INF_INPUT otherwise.  A literal or a copy is stored only after out + length <= ISIZE held
// (CFR_INF_OUTPUT_LONG).  Behind the last block: fewer bytes than ISIZE is CFR_INF_OUTPUT_SHORT; whole bytes left between the stream
// and the trailer are CFR_INF_BAD_HEADER (BSIZE does not fit the stream; zlib would leave them unused).  The CRC32 of the text is
// compared with the trailer only when everything before it held (CFR_INF_BAD_CRC).  A member with a status loses its text - its
// ISIZE bytes of the output are zero - and nothing else does.
//
// Decode tables (InfWork: LDS on the device, the stack on the host), per code: cnt[l] codes of length l, sym[] the symbols sorted by
// (length, symbol) - the canonical order - and a first-level table of 2^bits entries (10 / 9 / 7 bits for literal/length, distance,
// code-length code) indexed by the next bits of the stream: symbol | length << 9, 0 where no code of at most `bits` bits fits.  A 0
// sends inf_decode on the canonical walk over cnt[] and sym[], bit by bit: the overflow path of the codes longer than the table, and
// the place where an unused code of an incomplete set is found out.
//
// CRC32: gz_crc_entry / gz_crc_byte / gz_gf2_times / gz_crc_advance_tables and the slice-per-lane join of cfr_gz_core.hpp as they are.
#pragma once

#include <cstdint>

#include "cfr_gz_core.hpp"

namespace cfr {

constexpr uint32_t kInfMaxText = 65536;          // ISIZE above this is refused
constexpr uint32_t kInfLitBits = 10, kInfDistBits = 9, kInfClBits = 7;
constexpr uint32_t kInfLitSyms = 288, kInfDistSyms = 32;     // the fixed code has codes for 286 / 287 and 30 / 31: using one is an error
constexpr uint32_t kInfNoSym = 0xffffu;
constexpr uint64_t kInfMaxCallText = 1ull << 32;

// one member as the host walk leaves it
struct InfMember {
  uint64_t off;                  // of the member in the input
  uint32_t size, head;           // BSIZE + 1; 12 + XLEN: where the deflate stream begins
  uint32_t isize, crc;           // the trailer (isize as it stands there, also above 65536)
};
CFR_HD inline uint32_t inf_text_bytes(const InfMember &m) { return m.isize > kInfMaxText ? 0 : m.isize; }

// b: where a member is due, left bytes from there on; false: no BGZF member
CFR_HD inline bool inf_frame(const uint8_t *b, uint64_t left, uint64_t off, InfMember &m) {
  if (left < 18 || b[0] != 0x1f || b[1] != 0x8b || b[2] != 8 || !(b[3] & 4)) return false;
  const uint64_t xlen = (uint64_t)b[10] | ((uint64_t)b[11] << 8);
  if (12 + xlen > left) return false;
  for (uint64_t o = 12; o + 4 <= 12 + xlen;) {
    const uint64_t slen = (uint64_t)b[o + 2] | ((uint64_t)b[o + 3] << 8);
    if (b[o] == 'B' && b[o + 1] == 'C' && slen == 2 && o + 6 <= 12 + xlen) {
      const uint64_t size = ((uint64_t)b[o + 4] | ((uint64_t)b[o + 5] << 8)) + 1;
      if (size < 12 + xlen + 8 || size > left) return false;
      m.off = off; m.size = (uint32_t)size; m.head = (uint32_t)(12 + xlen);
      m.crc = gz_load32(b + size - 8); m.isize = gz_load32(b + size - 4);
      return true;
    }
    o += 4 + slen;
  }
  return false;
}

// length symbol 257 .. 285 / distance symbol 0 .. 29: the value without its extra bits (their counts: gz_len_extra, gz_dist_extra)
CFR_HD inline uint32_t inf_len_base(uint32_t sym) {
  const uint32_t s = sym - 257;
  if (s < 8) return 3 + s;
  if (sym == 285) return 258;
  return 3 + ((4 + (s & 3)) << ((s >> 2) - 1));
}
CFR_HD inline uint32_t inf_dist_base(uint32_t dc) { return dc < 4 ? 1 + dc : 1 + ((2 + (dc & 1)) << ((dc >> 1) - 1)); }

CFR_HD inline uint16_t inf_entry(uint32_t sym, uint32_t len) { return (uint16_t)(sym | (len << 9)); }

// kind of a code set: the code-length code, literal/length, distance
enum InfKind : int32_t { kInfCl = 0, kInfLit = 1, kInfDist = 2 };
// cnt[1 .. 15]: codes per length.  true: zlib builds a table from it.
CFR_HD inline bool inf_check_set(const uint16_t *cnt, int32_t kind) {
  uint32_t max = 0;
  int32_t left = 1;
  for (uint32_t l = 1; l < 16; ++l) {
    left = left * 2 - (int32_t)cnt[l];
    if (left < 0) return false;                 // over-subscribed
    if (cnt[l]) max = l;
  }
  if (max == 0) return kind == kInfDist;         // no code at all: only a block without matches may say so
  return left == 0 || (kind != kInfCl && max == 1);
}

// the symbol the bits (least significant first) begin with, its length in len; kInfNoSym: no code of the set
CFR_HD inline uint32_t inf_decode(const uint16_t *tab, uint32_t tbits, const uint16_t *cnt, const uint16_t *sym, uint32_t bits, uint32_t &len) {
  const uint32_t e = tab[bits & ((1u << tbits) - 1)];
  if (e) { len = e >> 9; return e & 511; }
  int32_t code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l < 16; ++l) {
    code |= (int32_t)((bits >> (l - 1)) & 1);
    const int32_t c = cnt[l];
    if (code - c < first) { len = l; return sym[index + (code - first)]; }
    index += c; first += c; first <<= 1; code <<= 1;
  }
  len = 0;
  return kInfNoSym;
}

// everything the decoder of one member works on
struct InfWork {
  uint16_t *ltab, *dtab, *ctab;          // 2^kInfLitBits, 2^kInfDistBits, 2^kInfClBits
  uint16_t *lsym, *dsym, *csym;          // kInfLitSyms, kInfDistSyms, kGzClSyms
  uint16_t *lcnt, *dcnt, *ccnt;          // 16 each
  uint8_t *lens;                         // kInfLitSyms + kInfDistSyms: the lengths as they are sent, literal/length code first
  uint8_t *cllen;                        // kGzClSyms
};

// The maker's part, M:
//   uint32_t peek(uint32_t pos)                                    32 bits of the stream from bit pos, zero behind its end
//   void sync()                                                    what one lane wrote to the work arrays is there for every lane
//   void set_len(uint8_t *a, uint32_t i, uint32_t n, uint32_t v)   a[i, i + n) = v (n <= 138)
//   void fixed_lens(uint8_t *lens)                                 the lengths of the fixed code: 288 + 32
//   bool build(lens, n, kind, tab, tbits, cnt, sym)                cnt, sym and tab of a code set; false: inf_check_set refuses it
//   void literal(uint32_t out, uint32_t byte)                      text[out] = byte (may be held back until flush)
//   void flush()
//   void copy_stored(uint32_t src_byte, uint32_t out, uint32_t n)  n bytes of the stream to the text
//   void copy_match(uint32_t out, uint32_t dist, uint32_t n)       text[out + i] = text[out - dist + i % dist]
// Every argument is checked here before the call.

#define CFR_INF_NEED(nbits) do { if (pos + (nbits) > total_bits) return CFR_INF_INPUT; } while (0)

// the header of a dynamic block from pos on: both code sets built
template <class M> CFR_HD inline int32_t inf_dyn_header(M &m, const InfWork &w, uint32_t &pos, uint32_t total_bits, uint32_t &hlit, uint32_t &hdist) {
  CFR_INF_NEED(14);
  uint32_t b = m.peek(pos);
  pos += 14;
  hlit = (b & 31) + 257; hdist = ((b >> 5) & 31) + 1;
  const uint32_t hclen = ((b >> 10) & 15) + 4;
  if (hlit > kGzLitSyms || hdist > kGzDistSyms) return CFR_INF_BAD_CODE_SET;
  CFR_INF_NEED(3 * hclen);
  m.set_len(w.cllen, 0, kGzClSyms, 0);
  m.sync();
  for (uint32_t i = 0; i < hclen; ++i) {
    m.set_len(w.cllen, gz_cl_order(i), 1, m.peek(pos) & 7);
    pos += 3;
  }
  if (!m.build(w.cllen, kGzClSyms, kInfCl, w.ctab, kInfClBits, w.ccnt, w.csym)) return CFR_INF_BAD_CODE_SET;
  const uint32_t n = hlit + hdist;
  uint32_t prev = 0;
  for (uint32_t i = 0; i < n;) {
    b = m.peek(pos);
    uint32_t l;
    const uint32_t sym = inf_decode(w.ctab, kInfClBits, w.ccnt, w.csym, b, l);
    if (sym == kInfNoSym) return pos + 15 <= total_bits ? CFR_INF_BAD_SYMBOL : CFR_INF_INPUT;
    CFR_INF_NEED(l);
    pos += l;
    if (sym < 16) { m.set_len(w.lens, i, 1, sym); prev = sym; ++i; continue; }
    const uint32_t eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
    CFR_INF_NEED(eb);
    const uint32_t rep = (sym == 18 ? 11 : 3) + ((b >> l) & ((1u << eb) - 1));       // (l + eb <= 14 bits of b)
    pos += eb;
    if (sym == 16 && i == 0) return CFR_INF_BAD_CODE_SET;
    if (sym != 16) prev = 0;
    if (i + rep > n) return CFR_INF_BAD_CODE_SET;
    m.set_len(w.lens, i, rep, prev);
    i += rep;
  }
  m.sync();
  if (w.lens[kGzEob] == 0) return CFR_INF_BAD_CODE_SET;
  if (!m.build(w.lens, hlit, kInfLit, w.ltab, kInfLitBits, w.lcnt, w.lsym)) return CFR_INF_BAD_CODE_SET;
  if (!m.build(w.lens + hlit, hdist, kInfDist, w.dtab, kInfDistBits, w.dcnt, w.dsym)) return CFR_INF_BAD_CODE_SET;
  return CFR_INF_OK;
}

// One member's deflate stream of total_bits bits into isize bytes of text (isize <= kInfMaxText): the status before the CRC.
template <class M> CFR_HD inline int32_t inf_member(M &m, const InfWork &w, uint32_t total_bits, uint32_t isize) {
  uint32_t pos = 0, out = 0;
  for (;;) {
    CFR_INF_NEED(3);
    uint32_t b = m.peek(pos);
    pos += 3;
    const uint32_t last = b & 1, type = (b >> 1) & 3;
    if (type == 3) return CFR_INF_BAD_BLOCK_TYPE;
    if (type == 0) {
      pos = (pos + 7) & ~7u;
      CFR_INF_NEED(32);
      b = m.peek(pos);
      pos += 32;
      const uint32_t len = b & 0xffffu;
      if (len != ((~b >> 16) & 0xffffu)) return CFR_INF_BAD_STORED_LEN;
      CFR_INF_NEED(8 * len);
      if (out + len > isize) return CFR_INF_OUTPUT_LONG;
      m.copy_stored(pos >> 3, out, len);
      out += len;
      pos += 8 * len;
    } else {
      if (type == 1) {
        m.fixed_lens(w.lens);
        m.sync();
        m.build(w.lens, kInfLitSyms, kInfLit, w.ltab, kInfLitBits, w.lcnt, w.lsym);
        m.build(w.lens + kInfLitSyms, kInfDistSyms, kInfDist, w.dtab, kInfDistBits, w.dcnt, w.dsym);
      } else {
        uint32_t hlit, hdist;
        const int32_t st = inf_dyn_header(m, w, pos, total_bits, hlit, hdist);
        if (st != CFR_INF_OK) return st;
      }
      for (;;) {
        b = m.peek(pos);
        uint32_t l;
        const uint32_t sym = inf_decode(w.ltab, kInfLitBits, w.lcnt, w.lsym, b, l);
        if (sym == kInfNoSym) return pos + 15 <= total_bits ? CFR_INF_BAD_SYMBOL : CFR_INF_INPUT;
        CFR_INF_NEED(l);
        pos += l;
        if (sym < kGzEob) {
          if (out + 1 > isize) return CFR_INF_OUTPUT_LONG;
          m.literal(out, sym);
          ++out;
          continue;
        }
        if (sym == kGzEob) break;
        if (sym > 285) return CFR_INF_BAD_SYMBOL;
        uint32_t eb = gz_len_extra(sym);
        CFR_INF_NEED(eb);
        const uint32_t len = inf_len_base(sym) + ((b >> l) & ((1u << eb) - 1));       // (l + eb <= 20 bits of b)
        pos += eb;
        b = m.peek(pos);
        const uint32_t dc = inf_decode(w.dtab, kInfDistBits, w.dcnt, w.dsym, b, l);
        if (dc == kInfNoSym) return pos + 15 <= total_bits ? CFR_INF_BAD_SYMBOL : CFR_INF_INPUT;
        CFR_INF_NEED(l);
        pos += l;
        if (dc > 29) return CFR_INF_BAD_SYMBOL;
        eb = gz_dist_extra(dc);
        CFR_INF_NEED(eb);
        const uint32_t dist = inf_dist_base(dc) + ((b >> l) & ((1u << eb) - 1));      // (l + eb <= 28 bits of b)
        pos += eb;
        if (dist > out) return CFR_INF_BAD_SYMBOL;                                     // in front of the member's first byte
        if (out + len > isize) return CFR_INF_OUTPUT_LONG;
        m.copy_match(out, dist, len);
        out += len;
      }
    }
    if (last) break;
  }
  m.flush();
  if (out < isize) return CFR_INF_OUTPUT_SHORT;
  if (((pos + 7) >> 3) != (total_bits >> 3)) return CFR_INF_BAD_HEADER;                // whole bytes between the stream and the trailer
  return CFR_INF_OK;
}

#undef CFR_INF_NEED

}  // namespace cfr
