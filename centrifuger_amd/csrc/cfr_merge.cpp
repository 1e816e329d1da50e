// cfr_merge.cpp — merging of overlapping read pairs, the pre-step `--merge-readpair` puts in front of SDUST and Query
// (ClassifyReads_Thread, CentrifugerClass.cpp:256-335).  A literal restatement of ReadPairMerger::Merge / IsMateOverlap
// (ReadPairMerger.hpp:13-233): host side, per pair; the anchor the device kernels (k_merge_decide / k_merge_write) are tested
// against.  Bytes are compared as they are ('N' equals 'N', lower case never equals the complemented mate); qualities are
// compared as signed char; lengths are int as in the reference (mates below 2^31 bases).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cfr_tail.hpp"

namespace cfr {

// int((flen - j) * similarityThreshold) for L = flen - j below 100, from the reference's own expression in double
// (ReadPairMerger.hpp:26-30, 36); from 100 on the threshold is int(L * 0.85).  The device reads this table from constant memory.
void merge_threshold_table(int32_t t[kMergeThrTable]) {
  for (int L = 0; L < kMergeThrTable; ++L) {
    double similarityThreshold = 0.95;
    if (L >= 100) similarityThreshold = 0.85;
    else if (L >= 50) similarityThreshold = 0.85 + (L - 50) / 50.0 * 0.1;
    t[L] = int(L * similarityThreshold);
  }
}

namespace {

inline char comp_char(uint8_t c) {   // _compChar (ReadPairMerger.hpp:105-111): everything that is not upper-case ACGT becomes 'N'
  switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return 'N'; }
}

// IsMateOverlap (ReadPairMerger.hpp:13-82), loop for loop
int is_mate_overlap(const char *fr, int flen, const char *sr, int slen, int minOverlap, int &offset, bool checkTandem) {
  int i, j, k = 0;
  int offsetCnt = 0;
  int overlapSize = -1;
  for (j = 0; j < flen - minOverlap; ++j) {
    int matchCnt = 0;
    bool flag = true;
    double similarityThreshold = 0.95;
    if (flen - j >= 100) similarityThreshold = 0.85;
    else if (flen - j >= 50) similarityThreshold = 0.85 + (flen - j - 50) / 50.0 * 0.1;
    const int need = int((flen - j) * similarityThreshold);
    for (k = 0; j + k < flen && k < slen; ++k) {
      if (fr[j + k] == sr[k]) ++matchCnt;
      if (matchCnt + (flen - (j + k) - 1) < need) { flag = false; break; }
    }
    if (flag) {
      offset = j;
      ++offsetCnt;
      overlapSize = k;
    }
  }
  if (offsetCnt != 1) return -1;
  if (checkTandem && overlapSize <= minOverlap * 2) {
    for (i = 1; i <= overlapSize / 2; ++i) {   // i: the repeat size
      bool tandem = true;
      for (j = i; j + i - 1 < overlapSize; j += i) {
        for (k = j; k <= j + i - 1; ++k)
          if (sr[k - j] != sr[k]) break;
        if (k <= j + i - 1) { tandem = false; break; }
      }
      if (tandem) return -1;
    }
  }
  return overlapSize;
}

}  // namespace

// ReadPairMerger::Merge (ReadPairMerger.hpp:132-233).  rm / qm: room for len1 + len2 bytes (qm and the qualities may be null
// together: FASTA).  Returns the kind (0 none, 1 overlap, 2 read-through); *mlen = length of the merged read (kinds 1, 2).
int merge_pair(const uint8_t *r1u, const int8_t *q1, int len1, const uint8_t *r2u, const int8_t *q2, int len2, uint8_t *rmu, int8_t *qm,
               int *mlen, int *overlap, int *off, MergeScratch &ws) {
  const char *r1 = (const char *)r1u;
  char *rm = (char *)rmu;
  ws.rcr2.resize((size_t)len2 + 1);
  char *rcr2 = ws.rcr2.data();
  for (int i = 0; i < len2; ++i) rcr2[i] = comp_char(r2u[len2 - 1 - i]);
  const int8_t *rcq2 = nullptr;
  if (q2) {
    ws.rcq2.resize((size_t)len2 + 1);
    for (int i = 0; i < len2; ++i) ws.rcq2[i] = q2[len2 - 1 - i];
    rcq2 = ws.rcq2.data();
  }
  const int64_t tenth = ((int64_t)len1 + (int64_t)len2) / 10;      // (both passes use the same value, ReadPairMerger.hpp:154-159)
  const int minOverlap = tenth > 31 ? 31 : (int)tenth;
  int offset = -1;
  *mlen = 0;

  // read through: the fragment is shorter than the reads
  int overlapSize = is_mate_overlap(rcr2, len2, r1, len1, minOverlap, offset, false);
  if (overlapSize >= 0) {
    memcpy(rm, r1, (size_t)overlapSize);
    if (q1) {
      memcpy(qm, q1, (size_t)overlapSize);
      for (int i = 0; i < overlapSize; ++i)
        if (rcq2[i + offset] > q1[i] || rm[i] == 'N') {
          rm[i] = rcr2[i + offset];
          qm[i] = rcq2[i + offset];
        }
    }
    *mlen = overlapSize; *overlap = overlapSize; *off = offset;
    return 2;
  }

  // simple overlap
  overlapSize = is_mate_overlap(r1, len1, rcr2, len2, minOverlap, offset, true);
  if (overlapSize >= 0) {
    int i;
    for (i = 0; i < len2; ++i) {
      rm[offset + i] = rcr2[i];
      if (rcq2) qm[offset + i] = rcq2[i];
    }
    const int len = offset + i;   // r2 may be a substring of r1
    for (i = 0; i < len1 && i < len; ++i)
      if (i < offset || (q1 && q1[i] >= qm[i] - 14) || rm[i] == 'N') {
        rm[i] = r1[i];
        if (q1) qm[i] = q1[i];
      }
    *mlen = len; *overlap = overlapSize; *off = offset;
    return 1;
  }
  *overlap = overlapSize; *off = offset;
  return 0;
}

}  // namespace cfr
