// cfr_refseq_core.hpp — the grammar of the reference text the index writer reads (FASTA of genomes or proteins), stated once for the
// host twin (cfr_refseq.cpp) and for the kernels (cfr_refseq.hip), and the handle behind cfr_refseq_*.
//
// Bytes    A chunk is a run of bytes of ONE file.  A chunk never begins inside a header line; `at_line_start` says whether its first
//          byte begins a line (the first chunk of a file: yes).
// Header   A '>' at a line start opens a header that runs to the next '\n' (the '\n' is part of the line, not of header_len).  A '>'
//          anywhere else is a byte like any other.  The id is the header behind its '>' up to the first ' ', '\t' or '\r'.
// Kept     In the other lines only upper-case A, C, G, T are kept (SequenceCompactor::Compact: no capitalisation, no replacement); with
//          `protein` the letters of "ARNDCEQGHILKMFPSTWYV", and a '$' is an error.  Everything else - '\n', '\r', lower case, N - is dropped.
// Records  One per header of the chunk: {header offset, header_len, id_len, kept = the kept symbols up to the next header or the chunk's
//          end}.  Kept symbols before the chunk's first header (`lead_kept`) continue the last record of the previous chunk of the file;
//          in a file's first chunk they belong to no record.
// Ends     A chunk that ends inside a header line: with `final` the header still opens its record (header_len runs to the chunk's end);
//          without it the chunk is looked at up to that '>' only (`consumed`), and the caller continues there.  A header line that
//          fills a whole chunk that is not final cannot be cut: RefseqCapacity.
//
// State    What a byte is depends on one thing: whether its line began with '>'.  Before every byte the reader is in one of three
//          states - kLs (the byte begins a line), kSeq (inside a sequence line), kHdr (inside a header line) - and a run of bytes is a
//          map from the state before it to the state behind it (refseq_map_*: three 2-bit fields).  A run that holds a '\n' is a
//          constant map, decided by the byte behind its last '\n'; composing the maps of the blocks in order (a scan) gives every
//          block the state it starts in, and ballots over the 64 lanes of a wave do the same for the bytes inside it.
//
// Stream   The kept symbols of all chunks go to one stream U in feed order; every chunk starts at a multiple of 32 symbols (the
//          device keeps U as 2-bit words and no word is shared between chunks).  cfr_refseq_assemble copies segments of U into the text T
//          of the index; the host twin keeps U and T as ASCII.
#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>

#include "../../include/cfr_hip.h"

#ifndef CFR_HD
#if defined(__HIPCC__)
#define CFR_HD __host__ __device__
#else
#define CFR_HD
#endif
#endif

namespace cfr {

struct RefseqCapacity : std::runtime_error { using std::runtime_error::runtime_error; };      // CFR_ERR_CAPACITY behind the C-ABI

enum : uint32_t { kLs = 0, kSeq = 1, kHdr = 2 };
// marks of a byte: dropped, kept, inside a header line, the '>' that opens one
enum : uint8_t { kMarkDrop = 0, kMarkKept = 1, kMarkHdr = 2, kMarkOpen = 3 };

constexpr uint32_t kRefMapIdentity = kLs | (kSeq << 2) | (kHdr << 4);
CFR_HD inline uint32_t refseq_map_const(uint32_t s) { return s * 0x15u; }
CFR_HD inline uint32_t refseq_map_apply(uint32_t m, uint32_t s) { return (m >> (2 * s)) & 3u; }
// first a, then b
CFR_HD inline uint32_t refseq_map_then(uint32_t a, uint32_t b) {
  return refseq_map_apply(b, refseq_map_apply(a, kLs)) | (refseq_map_apply(b, refseq_map_apply(a, kSeq)) << 2) | (refseq_map_apply(b, refseq_map_apply(a, kHdr)) << 4);
}
// the map of a run of bytes: has_nl: it holds a '\n'; nl_last: its last byte is one; after_gt: the byte behind its last '\n' is '>';
// first_gt: its first byte is '>'
CFR_HD inline uint32_t refseq_map_of(bool has_nl, bool nl_last, bool after_gt, bool first_gt) {
  if (has_nl) return refseq_map_const(nl_last ? kLs : after_gt ? kHdr : kSeq);
  return (first_gt ? kHdr : kSeq) | (kSeq << 2) | (kHdr << 4);
}

CFR_HD inline bool refseq_kept_nt(uint32_t ch) { return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'; }
inline bool refseq_kept_aa(uint8_t ch) { return ch > 0 && ch != '$' && strchr("ARNDCEQGHILKMFPSTWYV", ch) != nullptr; }

// the id of a header of n bytes (h[0] is its '>'; n excludes the '\n')
CFR_HD inline uint32_t refseq_id_len(const uint8_t *h, uint32_t n) {
  uint32_t e = 1;
  while (e < n && h[e] != ' ' && h[e] != '\t' && h[e] != '\r') ++e;
  return e - 1;
}

// the bytes of a chunk that are looked at (see Ends above); throws RefseqCapacity for a header line longer than a chunk
inline uint64_t refseq_effective_len(const uint8_t *text, uint64_t len, int at_line_start, int final) {
  if (len == 0 || final) return len;
  const void *nl = memrchr(text, '\n', len);
  const uint64_t tail = nl ? (uint64_t)((const uint8_t *)nl - text) + 1 : 0;
  const bool tail_starts_line = nl ? true : at_line_start != 0;
  if (tail < len && tail_starts_line && text[tail] == '>') {
    if (tail == 0) throw RefseqCapacity("cfr_refseq_feed: a header line is longer than the chunk");
    return tail;
  }
  return len;
}

// the handle behind cfr_refseq_*
class Refseq {
 public:
  virtual ~Refseq() {}
  virtual void feed(const uint8_t *text, uint64_t len, int at_line_start, int final, cfr_refseq_info *info) = 0;
  virtual void fetch(cfr_refseq_record *records) = 0;
  // segments sorted by dst, covering [0, n) exactly, every one inside U (checked: std::invalid_argument); U is freed
  virtual void assemble(const cfr_refseq_segment *segments, uint64_t n_segments, uint64_t n) = 0;
  virtual void text(uint8_t *ascii_out) = 0;               // the n symbols of T as ASCII
  virtual uint64_t text_len() const = 0;                   // n of the last assemble
  virtual void stats(cfr_refseq_stats *st) const = 0;
  virtual int device() const { return -1; }
  // host twin: T as ASCII, valid while the handle lives; device handle: nullptr
  virtual const uint8_t *host_text() const { return nullptr; }
  // device handle: hands the packed T (2 bits per symbol, first symbol in the top bits, (n + 31) / 32 + 4 words, the tail zero) to the
  // caller, who frees it with hipFree; host twin: nullptr
  virtual uint64_t *release_device_text() { return nullptr; }
};
Refseq *make_refseq_host(bool protein);                    // cfr_refseq.cpp
Refseq *make_refseq_device(int device);                    // cfr_refseq.hip; throws HipError{.., -1} without that GPU

// shared checks of assemble(); u_len: the symbols U holds
inline void refseq_check_segments(const cfr_refseq_segment *s, uint64_t ns, uint64_t n, uint64_t u_len) {
  uint64_t at = 0;
  for (uint64_t k = 0; k < ns; ++k) {
    if (s[k].len == 0 || s[k].dst != at) throw std::invalid_argument("cfr_refseq_assemble: segments must be sorted by dst, not empty, and cover [0, n) exactly");
    if (s[k].src > u_len || s[k].len > u_len - s[k].src) throw std::invalid_argument("cfr_refseq_assemble: a segment lies outside the fed symbols");
    at += s[k].len;
  }
  if (at != n) throw std::invalid_argument("cfr_refseq_assemble: segments must be sorted by dst, not empty, and cover [0, n) exactly");
}

}  // namespace cfr
