// cfr_tokenize_core.hpp — the tokeniser of raw FASTA/FASTQ text behind cfr_tokenize: the grammar it accepts ("regular" text), stated
// once for the host twin (cfr_tokenize_host.cpp) and for the kernels (cfr_tokenize.hip).
//
// The sequential reader of the command line (SeqReader::read_record in cfr_cli.cpp, kseq's grammar: multi-line FASTQ, a sequence that
// ends at any line starting with '>', '@' or '+', quality read until it is as long as the sequence) cannot be decided per line.  The
// tokeniser accepts the subset that can, and REFUSES the rest rather than guessing:
//
// Lines    Text is cut at '\n'.  A line's content excludes the '\n' and every trailing '\r'.  A last line without '\n' is a line only
//          when the caller says that the text ends there (`final`); otherwise the text is looked at up to its last '\n' only.
//          "Starts with c": the content is not empty and its first byte is c.
// Format   text[0] is '>' (FASTA) or '@' (FASTQ).
// FASTQ    Record r is lines 4r .. 4r+3.  Line 4r starts with '@'; line 4r+1 is empty or starts with none of '>', '@', '+'; line 4r+2
//          starts with '+'; the contents of lines 4r+1 and 4r+3 are equally long.  The first byte of a quality line is never looked at:
//          that is the point of counting lines.  Candidates: without `final` the floor(L/4) records whose four lines are there; with
//          `final` the records up to the one that holds the last line that is not empty (trailing empty lines are ignored) - and when
//          that record lacks one of its four lines it is truncated, which breaks the rules.
// FASTA    A record is a line starting with '>' plus the lines up to the next such line; those lines are empty or start with neither
//          '@' nor '+'.  The sequence is their contents back to back, bytes as they are.  Candidates: every record with `final`, every
//          record but the last without it (nothing shows that the last one has ended).
// Id       From the byte after the header character to the first ' ' or '\t'; a trailing "/1" or "/2" is removed when the id has at
//          least two bytes.
// Irregular  The first candidate that breaks a rule is the irregular record: the candidates before it are delivered, `irregular_at` is
//          the offset of its header line, and the caller continues there with the sequential reader.  Every irregular case is one where
//          the sequential grammar might read something else.
// Safety   Whatever is delivered is a prefix of what the sequential grammar reads from the same text.
//
// Both sides work on the same tables: lstart[j] / lcend[j] (first byte and end of content of line j), for FASTA hdr_line[r] (the line
// of record r's header) and line_rec[j] (the record line j belongs to), then per unit - a FASTQ record, a FASTA line - one
// cfr_read_record and one weight (the sequence bytes the unit contributes).  An exclusive sum of the weights gives every unit's place in
// the flat buffer, and at record starts the offsets.  The functions below are the per-unit rules and the summary; the host twin calls them
// in loops, the device from k_tok_records and k_tok_offsets.  Offsets inside one call fit 32 bits (len < 2^32).
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/cfr_hip.h"

#ifndef CFR_HD
#if defined(__HIPCC__)
#define CFR_HD __host__ __device__
#else
#define CFR_HD
#endif
#endif

namespace cfr {

constexpr uint32_t kTokNone = 0xffffffffu;       // "no irregular record"

struct TokTables {
  const uint8_t *text;
  const uint32_t *lstart, *lcend;                // L entries each
  const uint32_t *hdr_line, *line_rec;           // FASTA: H and L entries
  uint32_t L, H;                                 // lines, FASTA header lines
  uint64_t len, eff;                             // the caller's length; the bytes looked at (all of them in complete lines)
  int32_t fastq, final;
};
// what the device reads back and the twin fills in directly (cfr_token_info without the clock)
struct TokSummary { uint64_t n_records, consumed, total_bases, irregular_at; int32_t irregular, pad; };

CFR_HD inline uint32_t tok_len(const TokTables &t, uint32_t j) { return t.lcend[j] - t.lstart[j]; }
CFR_HD inline bool tok_starts(const TokTables &t, uint32_t j, uint8_t c) { return tok_len(t, j) > 0 && t.text[t.lstart[j]] == c; }

// h: a header line's content, n >= 1 bytes
CFR_HD inline uint32_t tok_id_len(const uint8_t *h, uint32_t n) {
  uint32_t e = 1;
  while (e < n && h[e] != ' ' && h[e] != '\t') ++e;
  uint32_t idn = e - 1;
  if (idn >= 2 && h[e - 2] == '/' && (h[e - 1] == '1' || h[e - 1] == '2')) idn -= 2;
  return idn;
}

// units that get a lane: FASTQ records that have at least one line, FASTA lines
CFR_HD inline uint32_t tok_units(const TokTables &t) { return t.fastq ? (t.final ? (uint32_t)(((uint64_t)t.L + 3) / 4) : t.L / 4) : t.L; }
// candidates (see above); last_nonempty = 1 + the last line whose content is not empty, 0 when there is none
CFR_HD inline uint32_t tok_candidates(const TokTables &t, uint32_t last_nonempty) {
  if (t.fastq) return t.final ? (uint32_t)(((uint64_t)last_nonempty + 3) / 4) : t.L / 4;
  return t.final ? t.H : (t.H ? t.H - 1 : 0);
}

// FASTQ unit r < tok_units: its record and weight; false when r is a candidate that breaks a rule
CFR_HD inline bool tok_fastq_unit(const TokTables &t, uint32_t r, uint32_t cand, cfr_read_record &rec, uint32_t &weight) {
  rec.header = 0; rec.qual = 0; rec.header_len = 0; rec.id_len = 0;
  weight = 0;
  if (r >= cand) return true;                    // trailing empty lines
  const uint32_t j = 4 * r;
  rec.header = t.lstart[j];
  rec.header_len = tok_len(t, j);
  if (rec.header_len) rec.id_len = tok_id_len(t.text + t.lstart[j], rec.header_len);
  if ((uint64_t)j + 3 >= t.L) return false;      // truncated
  const uint32_t n1 = tok_len(t, j + 1);
  rec.qual = t.lstart[j + 3];
  weight = n1;
  bool ok = tok_starts(t, j, '@') && tok_starts(t, j + 2, '+') && tok_len(t, j + 3) == n1;
  if (n1) { const uint8_t c = t.text[t.lstart[j + 1]]; ok = ok && c != '>' && c != '@' && c != '+'; }
  return ok;
}

// FASTA unit j (a line): header lines write their record, the others weigh their content; false when the line breaks a rule of a candidate
CFR_HD inline bool tok_fasta_unit(const TokTables &t, uint32_t j, uint32_t cand, cfr_read_record *records, uint32_t &weight) {
  const uint32_t n = tok_len(t, j), r = t.line_rec[j];
  const uint8_t c = n ? t.text[t.lstart[j]] : 0;
  if (c == '>') {
    cfr_read_record rec;
    rec.header = t.lstart[j]; rec.qual = 0; rec.header_len = n; rec.id_len = tok_id_len(t.text + t.lstart[j], n);
    records[r] = rec;
    weight = 0;
    return true;
  }
  weight = n;
  return !((c == '@' || c == '+') && r < cand);
}

// offsets[r] of record r <= n_records; dst: the exclusive sum of the weights, tok_units + 1 entries
CFR_HD inline uint64_t tok_offset(const TokTables &t, const uint32_t *dst, uint32_t r) {
  if (t.fastq) return dst[r];
  return r < t.H ? dst[t.hdr_line[r]] : dst[t.L];
}

CFR_HD inline TokSummary tok_summary(const TokTables &t, const uint32_t *dst, uint32_t last_nonempty, uint32_t first_bad, uint64_t max_records) {
  const uint32_t cand = tok_candidates(t, last_nonempty);
  uint32_t n = first_bad < cand ? first_bad : cand;
  if (max_records && max_records < n) n = (uint32_t)max_records;
  TokSummary s;
  s.n_records = n;
  s.total_bases = tok_offset(t, dst, n);
  if (t.fastq) {
    if (t.final) s.consumed = n == cand ? t.len : t.lstart[4 * n];
    else s.consumed = (uint64_t)4 * n < t.L ? t.lstart[4 * n] : t.eff;
  } else {
    s.consumed = n < t.H ? t.lstart[t.hdr_line[n]] : t.len;
  }
  s.irregular = first_bad != kTokNone;
  s.irregular_at = !s.irregular ? 0 : t.fastq ? t.lstart[4 * first_bad] : t.lstart[t.hdr_line[first_bad]];
  s.pad = 0;
  return s;
}

// the bytes the tables are made from: everything with `final` (plus a '\n' of the tokeniser's own when the text does not end with one),
// otherwise the text up to its last '\n'
inline uint64_t tok_effective_len(const uint8_t *text, uint64_t len, int final, bool &virtual_newline) {
  virtual_newline = false;
  if (len == 0) return 0;
  if (final) { virtual_newline = text[len - 1] != '\n'; return len + (virtual_newline ? 1 : 0); }
  const void *nl = memrchr(text, '\n', len);
  return nl ? (uint64_t)((const uint8_t *)nl - text) + 1 : 0;
}

// the handle behind cfr_tokenizer_*
class Tokenizer {
 public:
  virtual ~Tokenizer() {}
  virtual void tokenize(const uint8_t *text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info) = 0;
  virtual void fetch(cfr_read_record *records, uint64_t *offsets, uint8_t *bases) = 0;
  virtual void stats(cfr_token_stats *st) const { st->copy_in_ms = 0.0; st->kernel_ms = 0.0; }     // (the host twin has one clock: device_ms)
  virtual bool device_reads(const void **d_bases, const void **d_offsets) { (void)d_bases; (void)d_offsets; return false; }
  // the text and the record table of the last call in HBM (the id of record r: id_len bytes at text + header + 1); false on the host twin
  virtual bool device_records(const void **d_text, const void **d_records) { (void)d_text; (void)d_records; return false; }
  // tokenize with the text in the handle's own device memory (copied device to device into the handle's buffer); false on the host twin
  virtual bool tokenize_resident(const void *d_text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info) {
    (void)d_text; (void)len; (void)final; (void)max_records; (void)info; return false;
  }
  // the ids of the last call's records back to back, and n_records + 1 offsets; false: the ids take *need bytes, more than cap
  virtual bool fetch_ids(char *ids, uint64_t cap, uint64_t *id_off, uint64_t *need) = 0;
};
Tokenizer *make_tokenizer_host();                 // cfr_tokenize_host.cpp
Tokenizer *make_tokenizer_device(int device);     // cfr_tokenize.hip; throws HipError{.., -1} without that GPU

}  // namespace cfr
