// cfr_tsv_core.hpp — the rows of the classification TSV for one read (ResultWriter::Output, ResultWriter.hpp:199-242), stated once
// for the host twin (cfr_tsv.cpp) and for the kernels (cfr_tsv.hip).  The bytes are those of cfr_format_tsv:
//
//   n_match > 0   one row per match:  <id> \t <name> \t <taxID> \t <score> \t <2ndBestScore> \t <hitLength> \t <queryLength> \t <numMatches> \n
//                 name: kind 0 - the sequence name of match.id ("" for an id outside the table); otherwise the rank string of node
//                 match.id (rank string 0 for a node outside the table, and for a rank code the strings do not reach).
//   n_match <= 0  <id> \t unclassified \t 0 \t 0 \t 0 \t 0 \t <queryLength> \t 1 \n
//   taxID, score, 2ndBestScore are %lu (up to 20 digits); hitLength, queryLength, numMatches are %d (a leading '-').
//
// Not here: the barcode, UMI and expandedTaxIDs columns (their callers format on the host).
//
// One walk over a read's rows, tsv_rows, feeds a sink: TsvCount only adds up, TsvBytes stores.  The length of a read's rows and the
// rows themselves therefore cannot disagree - the device sizes its text by the first and writes it by the second.  A number keeps no
// digit buffer: its digit count comes from comparisons with the powers of ten, its digits leave most significant first.
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

constexpr uint32_t kTsvRankStrings = 31;       // the strings of cfr::tax_rank_string (Taxonomy.hpp:497-533); a code beyond them prints string 0

// what a row is made from besides the read: everything is an array, on the host or in HBM
struct TsvView {
  const char *names;             // the sequence names back to back, no terminators
  const uint64_t *name_off;      // seq_cnt + 1: name s = names[name_off[s] .. name_off[s + 1])
  const uint8_t *rank;           // node_cnt rank codes
  const char *rank_text;         // the rank strings back to back
  const uint32_t *rank_off;      // kTsvRankStrings + 1
  uint64_t seq_cnt, node_cnt;
};

// where the ids of a batch are: n + 1 offsets into bytes, or - the tokeniser's own tables - the records of the text the reads came from
struct TsvIds {
  const char *bytes;
  const uint64_t *off;           // nullptr: by records
  const cfr_read_record *rec;    // id of read i = bytes[rec[i].header + 1 .. + rec[i].id_len)
};
CFR_HD inline const char *tsv_id(const TsvIds &ids, uint64_t i, uint64_t &len) {
  if (ids.off) { len = ids.off[i + 1] - ids.off[i]; return ids.bytes + ids.off[i]; }
  len = ids.rec[i].id_len;
  return ids.bytes + ids.rec[i].header + 1;
}

CFR_HD inline uint64_t tsv_pow10(uint32_t k) {           // k <= 19
  static constexpr uint64_t kPow10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull,
                                          10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull,
                                          1000000000000000ull, 10000000000000000ull, 100000000000000000ull, 1000000000000000000ull,
                                          10000000000000000000ull};
  return kPow10[k];
}
CFR_HD inline uint32_t tsv_digits32(uint32_t v) {
  return v < 100000u ? (v < 100u ? (v < 10u ? 1u : 2u) : (v < 1000u ? 3u : (v < 10000u ? 4u : 5u)))
                     : (v < 10000000u ? (v < 1000000u ? 6u : 7u) : (v < 100000000u ? 8u : (v < 1000000000u ? 9u : 10u)));
}
CFR_HD inline uint32_t tsv_digits64(uint64_t v) {
  if (v < 10000000000ull) {
    if (!(v >> 32)) return tsv_digits32((uint32_t)v);
    return 10u;                                   // [2^32, 10^10)
  }
  uint32_t d = 11;
  while (d < 20 && v >= tsv_pow10(d)) ++d;
  return d;
}

struct TsvCount {
  uint64_t n = 0;
  static constexpr bool kStores = false;
  CFR_HD void ch(char) { ++n; }
  CFR_HD void skip(uint64_t k) { n += k; }
  CFR_HD void bytes(const char *, uint64_t k) { n += k; }
};
struct TsvBytes {
  char *p;
  static constexpr bool kStores = true;
  CFR_HD void ch(char c) { *p++ = c; }
  CFR_HD void skip(uint64_t) {}
  CFR_HD void bytes(const char *s, uint64_t k) { for (uint64_t i = 0; i < k; ++i) p[i] = s[i]; p += k; }
};

// v as decimal digits.  Three groups of at most 9 digits - v = (hi * 10^9 + mid) * 10^9 + lo - so that every division but the two
// by the constant 10^9 is a 32-bit one; one loop emits all groups (a single copy of it in a kernel keeps the registers down).
template <class Out> CFR_HD inline void tsv_u64(Out &o, uint64_t v) {
  const uint32_t d = tsv_digits64(v);
  if (!Out::kStores) { o.skip(d); return; }
  uint32_t hi = 0, mid, lo;
  if (!(v >> 32)) { const uint32_t w = (uint32_t)v; mid = w / 1000000000u; lo = w - mid * 1000000000u; }
  else {
    const uint64_t q = v / 1000000000ull;
    lo = (uint32_t)(v - q * 1000000000ull);
    hi = (uint32_t)(q / 1000000000ull);
    mid = (uint32_t)(q - (uint64_t)hi * 1000000000ull);
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t g = d > 18 ? 0u : (d > 9 ? 1u : 2u); g < 3; ++g) {
    uint32_t w = g == 0 ? hi : (g == 1 ? mid : lo);
    uint32_t k = g == 0 ? d - 18 : (g == 1 && d <= 18 ? d - 9 : (g == 2 && d <= 9 ? d : 9u));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (; k > 0; --k) {
      const uint32_t p = (uint32_t)tsv_pow10(k - 1), q = w / p;
      o.ch((char)('0' + (int)q));
      w -= q * p;
    }
  }
}

// the rows of one read; m: the read's first match (read only when n_match > 0).  The six numbers of a row go through one loop, and the
// row of an unclassified read is the same walk with a fixed middle: one copy of the digit code per caller.
template <class Out> CFR_HD inline void tsv_rows(const TsvView &v, const cfr_result &r, const cfr_match *m, const char *id, uint64_t id_len, Out &o) {
  static constexpr char kUn[] = "\tunclassified\t0\t0\t0\t0\t", kEnd[] = "\t1\n";
  const bool un = r.n_match <= 0;
  const int32_t rows = un ? 1 : r.n_match;
  for (int32_t j = 0; j < rows; ++j) {
    uint64_t taxid = 0;
    o.bytes(id, id_len);
    if (un) o.bytes(kUn, sizeof(kUn) - 1);
    else {
      const cfr_match mm = m[j];
      const char *name;
      uint64_t name_len;
      if (mm.kind == 0) {
        if (mm.id < v.seq_cnt) { name = v.names + v.name_off[mm.id]; name_len = v.name_off[mm.id + 1] - v.name_off[mm.id]; }
        else { name = v.names; name_len = 0; }
      } else {
        uint32_t rk = mm.id < v.node_cnt ? v.rank[mm.id] : 0u;
        if (rk >= kTsvRankStrings) rk = 0;
        name = v.rank_text + v.rank_off[rk];
        name_len = v.rank_off[rk + 1] - v.rank_off[rk];
      }
      o.ch('\t');
      o.bytes(name, name_len);
      taxid = mm.taxid;
    }
    // fields 0..5: taxID, score, 2ndBestScore (%lu), hitLength, queryLength, numMatches (%d); an unclassified read prints field 4 alone
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int f = un ? 4 : 0; f < (un ? 5 : 6); ++f) {
      if (!un) o.ch('\t');
      uint64_t val;
      if (f < 3) val = f == 0 ? taxid : (f == 1 ? r.score : r.secondary_score);
      else {
        const int32_t s = f == 3 ? r.hit_length : (f == 4 ? r.query_length : r.n_match);
        if (s < 0) { o.ch('-'); val = (uint64_t)(-(int64_t)s); }
        else val = (uint64_t)s;
      }
      tsv_u64(o, val);
    }
    if (un) o.bytes(kEnd, sizeof(kEnd) - 1);
    else o.ch('\n');
  }
}

// the length in bytes of the rows of read i
CFR_HD inline uint64_t tsv_read_len(const TsvView &v, const cfr_result &r, const cfr_match *m, uint64_t id_len) {
  TsvCount c;
  tsv_rows(v, r, m, (const char *)nullptr, id_len, c);
  return c.n;
}

}  // namespace cfr
