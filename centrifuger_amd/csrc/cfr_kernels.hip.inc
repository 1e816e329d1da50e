// cfr_kernels.hip.inc — device code of the path (included by cfr_device.hip only).
//
// Integer / bit-manipulation work, HBM-latency bound: no MFMA, no GEMM shapes.  Every FM-index
// step is ONE 64-byte occ record (see cfr_device.hpp); lanes of a wave64 each own a chain.
//
// Map of the file
//   rank / access on the two images   occ_count, rl_rank1 .. rb_access, k_occ_expand (image expansion at load)
//   FM-index steps                    fm_extend, fm_search_core, fm_backward_search, fm_locate, k_build_ftabx, k_build_loc_memo
//   probe kernels (parity entries)    k_rank_probe, k_bs_probe, k_locate
//   path kernels                      k_caps, k_search_chains (v1), k_adjust_select, k_compact_hits, k_enum_rows
//   device tail                       tail_fold_small / tail_fold_general / tail_fold_hash, tail_emit, k_tail, k_adjust_tail
//   SDUST pre-step                    k_dust
//   text-mode tables                  k_lf_init, k_lf_jump, k_text_fill
//   search, v2 (the shipped kernel)   k_pack_reads, k_search_chains_v2
// The default batch runs k_pack_reads once, then per sub-batch k_caps + scan, k_search_chains_v2, k_adjust_tail.
#pragma once

namespace cfr {

constexpr uint64_t kSelFlag = 1ull << 63;
// text-space hits (virt_text_pos below): sp = kVirtRow | delta << kVirtDeltaShift | first row of the entry range (< 2^36).
// delta has 26 bits (bits 36..61): a search only moves to the text when what is left of it cannot exceed that (kVirtDeltaMax
// characters; longer exact matches - contigs of > 67 Mbp - stay on the BWT, where the reference's own loop has no limit either).
// With kVirtInline (bit 62) the hit carries its rows' text positions itself, in place of the first row and of the mask: the one
// or two rows a search of k_search_chains_v2 ended with, which it holds in registers at that point (virt_text_pos below).
constexpr uint32_t kVirtDeltaShift = 36;
constexpr uint64_t kVirtRowMask = (1ull << kVirtDeltaShift) - 1ull;
constexpr uint32_t kVirtDeltaMax = (1u << 26) - 1u;
constexpr uint64_t kVirtInline = 1ull << 62;

// 16-byte gather from an address that is only guaranteed 4-byte alignment (offset arrays, u32 tables, the second half of a
// 2-bit text pair): one global_load_dwordx4 on gfx950, and well defined because the type says what the alignment is.
struct __attribute__((packed, aligned(4))) U128a4 { uint64_t x, y; };
__device__ __forceinline__ ulonglong2 ld16(const void *p) {
  const U128a4 t = *reinterpret_cast<const U128a4 *>(p);
  return make_ulonglong2(t.x, t.y);
}

// The same load with the non-temporal hint (global_load_dwordx4 ... nt): the line is not kept in L2 at the expense of others.
// For the random gathers of the search (K-mer table, occurrence records, suffix array, text): nothing of them is reused, and
// without the hint they push the reads' own packed blocks out of L2 between two visits of a lane (CFR_GATHER_NT, see DESIGN.md).
typedef uint32_t cfr_u32x4 __attribute__((ext_vector_type(4)));
typedef cfr_u32x4 cfr_u32x4a4 __attribute__((aligned(4)));
__device__ __forceinline__ ulonglong2 ld16_nt(const void *p) {
  const cfr_u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const cfr_u32x4a4 *>(p));
  return make_ulonglong2((uint64_t)t.x | ((uint64_t)t.y << 32), (uint64_t)t.z | ((uint64_t)t.w << 32));
}
#ifndef CFR_GATHER_NT
#define CFR_GATHER_NT 0
#endif
__device__ __forceinline__ ulonglong2 ld16_gather(const void *p) { return CFR_GATHER_NT == 1 ? ld16_nt(p) : ld16(p); }

// ---- alphabet: only upper-case A,C,G,T are symbols (Alphabet::IsIn, Alphabet.hpp:169-176) ----
__device__ __forceinline__ uint32_t base_code(uint32_t ch) {
  uint32_t k = (ch >> 1) & 3u;
  k ^= k >> 1;                                        // A0 C1 G2 T3
  return (ch == ((0x54474341u >> (8u * k)) & 0xffu)) ? k : 4u;
}

// A search string is a read, or its reverse complement read through the same bytes
// (Classifier::ReverseComplement, Classifier.hpp:99-111: non-ACGT -> 'N', i.e. "not a symbol").
struct SeqView {
  const uint8_t *s;
  int32_t len;
  int32_t rc;
  __device__ __forceinline__ uint32_t code(int32_t j) const {
    uint32_t c = base_code(rc ? s[len - 1 - j] : s[j]);
    return (rc && c < 4u) ? 3u - c : c;
  }
};

// ---- occ record access -----------------------------------------------------------------------
// #c in B[0 .. p + incl)  ==  Sequence_RunBlock::Rank(c, p, incl)  (Sequence_RunBlock.hpp:378-416)
__device__ __forceinline__ const uint64_t *occ_rec(const DevView &v, uint64_t p) { return v.occ + (p >> 7) * 8; }

__device__ __forceinline__ uint64_t occ_count(uint64_t mid, uint64_t lo, uint64_t hi, uint32_t c, uint64_t p, uint32_t incl) {
  const uint32_t q = (uint32_t)p & 127u, h = q >> 6, e = (q & 63u) + incl;           // e in [0,64]
  const uint64_t m = ((c & 1u) ? lo : ~lo) & ((c & 2u) ? hi : ~hi);                  // bit k: symbol k == c
  mid &= ~kSelFlag;
  if (h == 0) return mid - (e >= 64 ? 0ull : (uint64_t)__popcll(m >> e));
  return mid + (e == 0 ? 0ull : (uint64_t)__popcll(m << (64 - e)));
}

// ---- run-block image: rank lines, wavelet trees, run-block rank/access --------------------------------
// DS_Rank9::Query (DS_Rank.hpp:255-273) on a line array: #1 in [0, i + incl), i clamped to n-1 like the reference
__device__ __forceinline__ uint64_t rl_rank1(const RankLines &L, uint64_t i, uint32_t incl) {
  if (i >= L.nbits) i = L.nbits - 1;
  const uint64_t e = i + incl;
  const uint64_t line = e / 448u;
  const uint32_t off = (uint32_t)(e - line * 448u);
  const uint64_t *p = L.lines + line * 8;
  const ulonglong2 q0 = ld16(p), q1 = ld16(p + 2), q2 = ld16(p + 4), q3 = ld16(p + 6);
  const uint64_t w[7] = {q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
  uint64_t cnt = q0.x;
  const uint32_t full = off >> 6, rem = off & 63u;
#pragma unroll
  for (uint32_t k = 0; k < 7; ++k) {
    if (k < full) cnt += (uint64_t)__popcll(w[k]);
    else if (k == full && rem) cnt += (uint64_t)__popcll(w[k] & ((1ull << rem) - 1));
  }
  return cnt;
}
// Bitvector_Plain::Access (Bitvector_Plain.hpp:128-131)
__device__ __forceinline__ uint32_t rl_access(const RankLines &L, uint64_t i) {
  const uint64_t line = i / 448u;
  const uint32_t off = (uint32_t)(i - line * 448u);
  return (uint32_t)((L.lines[line * 8 + 1 + (off >> 6)] >> (off & 63u)) & 1u);
}
// Bitvector::Rank0 / Rank (Bitvector.hpp:45-57): Rank0 does not re-clamp i
__device__ __forceinline__ uint64_t rl_rank(const RankLines &L, uint32_t type, uint64_t i, uint32_t incl) {
  const uint64_t r1 = rl_rank1(L, i, incl);
  return type ? r1 : i + incl - r1;
}
// Sequence_WaveletTree::Rank (Sequence_WaveletTree.hpp:235-264); node 0 = root (high code bit), 1+hi = leaf
__device__ __forceinline__ uint64_t wt_rank(const RankLines *T, uint32_t c, uint64_t i, uint32_t incl) {
  if (!incl) { if (i == 0) return 0; --i; }
  const uint32_t hi = c >> 1, lo = c & 1u;
  i = rl_rank(T[0], hi, i, 1);
  if (i == 0) return 0;
  --i;
  return rl_rank(T[1 + hi], lo, i, 1);
}
// Sequence_WaveletTree::RankAndTest (:268-293)
__device__ __forceinline__ uint64_t wt_rank_and_test(const RankLines *T, uint32_t c, uint64_t i, bool &is_c) {
  const uint32_t hi = c >> 1, lo = c & 1u;
  is_c = hi == rl_access(T[0], i);
  i = rl_rank(T[0], hi, i, 1);
  if (i == 0) return 0;
  --i;
  if (is_c && lo != rl_access(T[1 + hi], i)) is_c = false;
  return rl_rank(T[1 + hi], lo, i, 1);
}
// Sequence_WaveletTree::Access (:215-232)
__device__ __forceinline__ uint32_t wt_access(const RankLines *T, uint64_t i) {
  const uint32_t hi = rl_access(T[0], i);
  i = rl_rank(T[0], hi, i, 1) - 1;
  return (hi << 1) | rl_access(T[1 + hi], i);
}
// Sequence_RunBlock::Rank (Sequence_RunBlock.hpp:378-416)
__device__ __forceinline__ uint64_t rb_rank(const RbView &r, uint64_t n, uint32_t c, uint64_t i, uint32_t incl) {
  if (!incl) { if (i == 0) return 0; --i; }
  const uint64_t bi = i / r.b;
  const uint32_t type = rl_access(r.use, bi);
  const uint64_t ranki = r.b < n ? rl_rank(r.use, type, bi, 1) : 1;
  const uint64_t other = (bi + 1) - ranki;
  uint64_t ret;
  if (type == 0) ret = wt_rank(r.plain, c, (ranki - 1) * r.b + i % r.b, 1);
  else {
    bool in_run;
    const uint64_t rbr = wt_rank_and_test(r.runs, c, ranki - 1, in_run);
    ret = in_run ? (rbr - 1) * r.b + i % r.b + 1 : rbr * r.b;
  }
  if (other == 0) return ret;
  if (type == 0) ret += wt_rank(r.runs, c, other - 1, 1) * r.b;
  else ret += wt_rank(r.plain, c, other * r.b - 1, 1);
  return ret;
}
// Sequence_RunBlock::Access (:360-376)
__device__ __forceinline__ uint32_t rb_access(const RbView &r, uint64_t i) {
  const uint64_t bi = i / r.b;
  const uint32_t type = rl_access(r.use, bi);
  if (type == 0) return wt_access(r.plain, i - r.b * rl_rank(r.use, 1, bi, 1));
  return wt_access(r.runs, (i - r.b * rl_rank(r.use, 0, bi, 1)) / r.b);
}

// ---- flat occ image from the run-block image, on the device (index load: the compressed components are uploaded as
// they are and expanded here; no sequential decode on the host).  One lane per 64-symbol half-record: the two bit planes
// + the half's symbol counts; a scan over the counts gives every record its mid[] (k_occ_fill_mid).
// Padding beyond n is symbol 0 and is counted, so that occ_count() stays consistent inside the last record.
__global__ void k_occ_expand(RbView r, uint64_t n, uint64_t halves, uint64_t *occ, uint64_t *cnt) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < halves; k += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t lo = 0, hi = 0;
    const uint64_t base = k << 6;
    for (uint32_t j = 0; j < 64; ++j) {
      const uint64_t p = base + j;
      if (p >= n) break;
      const uint32_t sym = rb_access(r, p);
      lo |= (uint64_t)(sym & 1u) << j;
      hi |= (uint64_t)(sym >> 1) << j;
    }
    uint64_t *rec = occ + (k >> 1) * 8;
    rec[4 + 2 * (k & 1)] = lo;
    rec[5 + 2 * (k & 1)] = hi;
    const uint64_t c3 = (uint64_t)__popcll(lo & hi), c2 = (uint64_t)__popcll(~lo & hi), c1 = (uint64_t)__popcll(lo & ~hi);
    cnt[k] = c1;
    cnt[halves + 1 + k] = c2;
    cnt[2 * (halves + 1) + k] = c3;
  }
}
// pre[] = exclusive prefix sums of the three count arrays (each halves+1 long); symbol 0 is what is left of 64 per half
__global__ void k_occ_fill_mid(uint64_t halves, const uint64_t *pre, uint64_t *occ) {
  const uint64_t nrec = halves >> 1;
  for (uint64_t rI = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; rI < nrec; rI += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t k = 2 * rI + 1;                      // symbols before the record's midpoint = before half k
    const uint64_t c1 = pre[k], c2 = pre[halves + 1 + k], c3 = pre[2 * (halves + 1) + k];
    uint64_t *rec = occ + rI * 8;
    rec[0] = 64 * k - c1 - c2 - c3;
    rec[1] = c1;
    rec[2] = c2;
    rec[3] = c3;
  }
}
__global__ void k_occ_flag_selected(const uint64_t *rows, uint64_t cnt, uint64_t *occ, uint64_t flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) atomicOr((unsigned long long *)(occ + (rows[i] >> 7) * 8), (unsigned long long)flag);
}

// ---- protein image: Sequence_RunBlockOneTree::Rank / Access (Sequence_RunBlockOneTree.hpp:382-435) answered from the
// decoded string: bit planes of the 5-bit plain codes + per-block counts
__device__ __forceinline__ uint64_t prot_match(const uint64_t *pl, uint32_t c) {
  uint64_t m = ~0ull;
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) m &= ((c >> k) & 1u) ? pl[k] : ~pl[k];
  return m;
}
__device__ __forceinline__ uint64_t prot_rank(const ProtView &P, uint32_t c, uint64_t p, uint32_t incl) {
  const uint64_t e = p + incl, blk = e >> 6;
  const uint32_t r = (uint32_t)e & 63u;
  if (P.rec) {                                              // one 128-byte record: count and planes from the same line
    const uint64_t *rec = P.rec + blk * 16;
    uint64_t cnt1 = reinterpret_cast<const uint32_t *>(rec)[c];
    if (r) cnt1 += (uint64_t)__popcll(prot_match(rec + 11, c) & ((1ull << r) - 1));
    return cnt1;
  }
  uint64_t cnt = P.counts[blk * 32 + c];
  if (r) cnt += (uint64_t)__popcll(prot_match(P.planes + blk * 8, c) & ((1ull << r) - 1));
  return cnt;
}
__device__ __forceinline__ uint32_t prot_access(const ProtView &P, uint64_t p) {
  const uint64_t *pl = P.rec ? P.rec + (p >> 6) * 16 + 11 : P.planes + (p >> 6) * 8;
  const uint32_t j = (uint32_t)p & 63u;
  uint32_t c = 0;
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) c |= (uint32_t)((pl[k] >> j) & 1ull) << k;
  return c;
}

__device__ __forceinline__ uint64_t occ_rank(const DevView &v, uint32_t c, uint64_t p, uint32_t incl) {
  if (v.prot.enabled) return prot_rank(v.prot, c, p, incl);
  if (v.rb.enabled) return rb_rank(v.rb, v.n, c, p, incl);
  const uint64_t *rec = occ_rec(v, p);
  const uint32_t h = ((uint32_t)p >> 6) & 1u;
  const uint64_t mid = rec[c];
  const ulonglong2 pl = ld16(rec + 4 + 2 * h);
  return occ_count(mid, pl.x, pl.y, c, p, incl);
}

// FMIndex::Rank (FMIndex.hpp:352-362): the text's last char sits at row firstISA instead of a '$' row
__device__ __forceinline__ uint64_t fm_fix(const DevView &v, uint32_t c, uint64_t p, uint32_t incl) {
  return (c == v.last_code && (p < v.first_isa || (!incl && p == v.first_isa))) ? 1ull : 0ull;
}
__device__ __forceinline__ uint64_t fm_rank(const DevView &v, uint32_t c, uint64_t p, uint32_t incl) {
  return occ_rank(v, c, p, incl) + fm_fix(v, c, p, incl);
}
__device__ __forceinline__ uint32_t bwt_access(const DevView &v, uint64_t p) {
  if (v.prot.enabled) return prot_access(v.prot, p);
  if (v.rb.enabled) return rb_access(v.rb, p);
  const uint64_t *rec = occ_rec(v, p);
  const uint32_t h = ((uint32_t)p >> 6) & 1u, j = (uint32_t)p & 63u;
  const ulonglong2 pl = ld16(rec + 4 + 2 * h);
  return (uint32_t)((pl.x >> j) & 1u) | ((uint32_t)((pl.y >> j) & 1u) << 1);
}

// FMIndex::BackwardExtend (FMIndex.hpp:364-379).  Single-row ranges use Access, literally (Appendix B item 4).
__device__ __forceinline__ void fm_extend(const DevView &v, uint32_t c, uint64_t sp, uint64_t ep, uint64_t &nsp, uint64_t &nep) {
  if (v.prot.enabled) {
    nsp = v.prot.C[c] + fm_rank(v, c, sp, 0);
    if (sp != ep) nep = v.prot.C[c] + fm_rank(v, c, ep, 1) - 1;
    else nep = nsp + (prot_access(v.prot, ep) == c ? 0ull : ~0ull);
    return;
  }
  if (v.rb.enabled) {   // literal form on the compressed components
    nsp = v.C[c] + fm_rank(v, c, sp, 0);
    if (sp != ep) nep = v.C[c] + fm_rank(v, c, ep, 1) - 1;
    else nep = nsp + (rb_access(v.rb, ep) == c ? 0ull : ~0ull);
    return;
  }
  const uint64_t *rs = occ_rec(v, sp);
  const uint32_t hs = ((uint32_t)sp >> 6) & 1u;
  const uint64_t mid_s = rs[c];
  const ulonglong2 ps = ld16(rs + 4 + 2 * hs);
  if (sp != ep) {
    const uint64_t *re = occ_rec(v, ep);
    const uint32_t he = ((uint32_t)ep >> 6) & 1u;
    const uint64_t mid_e = re[c];
    const ulonglong2 pe = ld16(re + 4 + 2 * he);
    nsp = v.C[c] + occ_count(mid_s, ps.x, ps.y, c, sp, 0) + fm_fix(v, c, sp, 0);
    nep = v.C[c] + occ_count(mid_e, pe.x, pe.y, c, ep, 1) + fm_fix(v, c, ep, 1) - 1;
  } else {
    nsp = v.C[c] + occ_count(mid_s, ps.x, ps.y, c, sp, 0) + fm_fix(v, c, sp, 0);
    const uint32_t j = (uint32_t)sp & 63u;
    const uint32_t sym = (uint32_t)((ps.x >> j) & 1u) | ((uint32_t)((ps.y >> j) & 1u) << 1);
    nep = nsp + (sym == c ? 0ull : ~0ull);
  }
}

// FMIndex::BackwardSearch (FMIndex.hpp:487-510) incl. GetBackwardSearchInitialRange (:388-422), from an
// arbitrary code source (a read, or the bits of a K-mer key when the wide table is being derived).
// sp/ep are left untouched when m < width (like the reference).  start_l/max_l bound the walk.
template <class CodeAt>
__device__ __forceinline__ uint32_t fm_search_core(const DevView &v, const CodeAt &code_at, uint32_t m, uint64_t &sp, uint64_t &ep) {
  const uint32_t w = v.ftab_width;
  if (m < w) return 0;
  uint32_t l = 0;
  if (w > 0) {
    uint64_t key = 0;
    for (uint32_t i = 0; i < w; ++i) {
      const uint32_t c = code_at(i);
      if (c > 3u) { sp = 1; ep = 0; return i; }
      key = (key << 2) | c;
    }
    const ulonglong2 e = ld16(v.ftab + 2 * key);
    if (e.y == 0) { sp = 1; ep = 0; return w - 1; }
    sp = e.x;
    ep = e.x + e.y - 1;
    l = w;
  } else {
    sp = 0;
    ep = v.n - 1;
  }
  while (l < m) {
    const uint32_t c = code_at(l);
    if (c > 3u) break;
    uint64_t nsp, nep;
    fm_extend(v, c, sp, ep, nsp, nep);
    if (nsp > nep || nep > v.n) break;
    sp = nsp;
    ep = nep;
    ++l;
  }
  return l;
}

// 8-byte form of a derived K-mer entry (images where the 16-byte table does not fit): l in bits 59..63, count - 1 in bits
// 39..58, sp in bits 0..38.  l = 31 is the ESCAPE: the state does not fit (more than 2^20 rows, or a search that stopped
// inside the table with a reportable length) and the plain path (on-disk ftab + extends) answers.  An entry with l < K
// carries no range: such a search ends without a hit (guaranteed by the encoder: l < min_hit_len or the range was empty).
constexpr uint32_t kFtabx8Escape = 31u;
// 16-byte entries: (sp, count << 8 | l) - or, bit 63 of the second word set, (sp, text position of the one row << 16 | 1 << 8 | l): k_ftabx_textpos
constexpr uint64_t kFtabxTextPos = 1ull << 63;
__device__ __forceinline__ uint64_t ftabx16_count(uint64_t y) { return (y & kFtabxTextPos) ? 1ull : y >> 8; }
__device__ __forceinline__ uint64_t ftabx16_textpos(uint64_t y) { return (y >> 16) & ((1ull << 40) - 1ull); }
__device__ __forceinline__ uint64_t ftabx8_encode(uint32_t l, uint64_t sp, uint64_t ep, uint32_t K, int32_t min_hit_len) {
  if (l < K) return (sp <= ep && (int32_t)l >= min_hit_len) ? (uint64_t)kFtabx8Escape << 59 : (uint64_t)l << 59;
  const uint64_t c1 = ep - sp;
  if (c1 >= (1ull << 20) || sp >= (1ull << 39)) return (uint64_t)kFtabx8Escape << 59;
  return ((uint64_t)l << 59) | (c1 << 39) | sp;
}
__device__ __forceinline__ bool ftabx8_decode(uint64_t e, uint32_t K, uint32_t &l, uint64_t &sp, uint64_t &ep) {   // false: escape
  l = (uint32_t)(e >> 59);
  if (l == kFtabx8Escape) return false;
  if (l < K) { sp = 1; ep = 0; }
  else { sp = e & ((1ull << 39) - 1); ep = sp + ((e >> 39) & 0xfffffull); }
  return true;
}

__device__ __forceinline__ uint32_t fm_backward_search(const DevView &v, const SeqView &s, uint32_t m, uint64_t &sp, uint64_t &ep) {
  const uint32_t K = v.ftabx_width;
  if (v.ftabx && m >= K) {
    // derived K-mer table: valid when the first K characters are all symbols; otherwise the plain walk decides
    uint64_t key = 0;
    bool ok = true;
    for (uint32_t i = 0; i < K; ++i) {
      const uint32_t c = s.code((int32_t)(m - 1 - i));
      if (c > 3u) { ok = false; break; }
      key = (key << 2) | c;
    }
    uint32_t l = 0;
    if (ok) {
      if (v.ftabx_e8) ok = ftabx8_decode(v.ftabx[key], K, l, sp, ep) && l >= K;   // (a search that stopped inside the table: the plain walk
      else {                                                                          //  below returns its exact range - this function is also the probe)
        const ulonglong2 e = ld16(v.ftabx + 2 * key);
        l = (uint32_t)(e.y & 0xffu);
        sp = e.x;
        ep = e.x + ftabx16_count(e.y) - 1;      // empty 10-mer bucket is stored as sp = 1, cnt = 0 -> ep = 0
      }
    }
    if (ok) {
      if (l < K) return l;
      while (l < m) {
        const uint32_t c = s.code((int32_t)(m - 1 - l));
        if (c > 3u) break;
        uint64_t nsp, nep;
        fm_extend(v, c, sp, ep, nsp, nep);
        if (nsp > nep || nep > v.n) break;
        sp = nsp;
        ep = nep;
        ++l;
      }
      return l;
    }
  }
  return fm_search_core(v, [&](uint32_t i) { return s.code((int32_t)(m - 1 - i)); }, m, sp, ep);
}

// ---- protein path: translated search (Classifier::TranslatedSearch, Classifier.hpp:463-506) ----------------------------
// Classifier::DnaToAa (:131-241): an if/else ladder - a character that is none of the letters a level tests takes that
// level's last branch; only 'N' gives '?'
__device__ __forceinline__ char dna_to_aa(uint32_t a, uint32_t b, uint32_t c) {
  if (a == 'N' || b == 'N' || c == 'N') return '?';
  const bool ag = c == 'A' || c == 'G';
  if (a == 'A') {
    if (b == 'A') return ag ? 'K' : 'N';
    if (b == 'C') return 'T';
    if (b == 'G') return ag ? 'R' : 'S';
    return c == 'G' ? 'M' : 'I';
  } else if (a == 'C') {
    if (b == 'A') return ag ? 'Q' : 'H';
    if (b == 'C') return 'P';
    if (b == 'G') return 'R';
    return 'L';
  } else if (a == 'G') {
    if (b == 'A') return ag ? 'E' : 'D';
    if (b == 'C') return 'A';
    if (b == 'G') return 'G';
    return 'V';
  }
  if (b == 'A') return ag ? '_' : 'Y';
  if (b == 'C') return 'S';
  if (b == 'G') return c == 'A' ? '_' : (c == 'G' ? 'W' : 'C');
  return ag ? 'L' : 'F';
}
// one frame of one strand of a read, as the amino-acid string TranslatedSearch hands to GetHitsFromRead
struct AaView {
  const uint8_t *s;
  int32_t len, rc, frame, k;       // k = number of amino acids
  __device__ __forceinline__ uint32_t base(int32_t x) const {      // character x of the strand (ReverseComplement: non-ACGT -> 'N')
    if (!rc) return s[x];
    const uint32_t ch = s[len - 1 - x];
    return ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : 'N';
  }
  __device__ __forceinline__ uint32_t code(const ProtView &P, int32_t j) const {   // plain code of amino acid j, > 31 = not a symbol
    const int32_t x = frame + 3 * j;
    return P.code_of[(uint8_t)dna_to_aa(base(x), base(x + 1), base(x + 2))];
  }
};
// FMIndex::BackwardSearch (FMIndex.hpp:487-510) with the general ftab key (initW << bits | code, :388-422)
template <class CodeAt>
__device__ __forceinline__ uint32_t prot_backward_search(const DevView &v, const CodeAt &code_at, uint32_t m, uint64_t &sp, uint64_t &ep) {
  const uint32_t w = v.ftab_width;
  if (m < w) return 0;
  uint32_t l = 0;
  if (w > 0) {
    uint64_t key = 0;
    for (uint32_t i = 0; i < w; ++i) {
      const uint32_t c = code_at(i);
      if (c > 31u) { sp = 1; ep = 0; return i; }
      key = (key << v.prot.bits) | c;
    }
    const ulonglong2 e = ld16(v.ftab + 2 * key);
    if (e.y == 0) { sp = 1; ep = 0; return w - 1; }
    sp = e.x;
    ep = e.x + e.y - 1;
    l = w;
  } else {
    sp = 0;
    ep = v.n - 1;
  }
  while (l < m) {
    const uint32_t c = code_at(l);
    if (c > 31u) break;
    uint64_t nsp, nep;
    fm_extend(v, c, sp, ep, nsp, nep);
    if (nsp > nep || nep > v.n) break;
    sp = nsp;
    ep = nep;
    ++l;
  }
  return l;
}

// derived K-mer table of a protein index: key = the first K codes as a base-sigma number (first character most significant),
// entry = (sp, count << 8 | l) exactly like the nucleotide table
__global__ void k_build_ftabx_prot(DevView v, uint32_t K, uint64_t entries, uint64_t *table) {
  for (uint64_t key = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; key < entries; key += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t codes[12];
    uint64_t x = key;
    for (uint32_t i = K; i-- > 0;) { codes[i] = (uint32_t)(x % v.prot.sigma); x /= v.prot.sigma; }
    uint64_t sp = 0, ep = 0;
    const uint32_t l = prot_backward_search(v, [&](uint32_t i) { return codes[i]; }, K, sp, ep);
    const uint64_t cnt = ep - sp + 1;            // (1,0) -> 0
    table[2 * key] = sp;
    table[2 * key + 1] = (cnt << 8) | l;
  }
}
// FMIndex::BackwardSearch of a protein index through the derived table when the first K characters are all symbols
template <class CodeAt>
__device__ __forceinline__ uint32_t prot_backward_search_x(const DevView &v, const CodeAt &code_at, uint32_t m, uint64_t &sp, uint64_t &ep) {
  const uint32_t K = v.ftabx_width;
  if (v.ftabx && m >= K) {
    uint64_t key = 0;
    bool ok = true;
    for (uint32_t i = 0; i < K; ++i) {
      const uint32_t c = code_at(i);
      if (c >= v.prot.sigma) { ok = false; break; }
      key = key * v.prot.sigma + c;
    }
    if (ok) {
      const ulonglong2 e = ld16(v.ftabx + 2 * key);
      uint32_t l = (uint32_t)(e.y & 0xffu);
      sp = e.x;
      ep = e.x + (e.y >> 8) - 1;
      if (l < K) return l;
      while (l < m) {
        const uint32_t c = code_at(l);
        if (c > 31u) break;
        uint64_t nsp, nep;
        fm_extend(v, c, sp, ep, nsp, nep);
        if (nsp > nep || nep > v.n) break;
        sp = nsp;
        ep = nep;
        ++l;
      }
      return l;
    }
  }
  return prot_backward_search(v, code_at, m, sp, ep);
}

// eight codes of a translated chain from byte `at` on (any alignment): two aligned words, funnelled
__device__ __forceinline__ uint64_t prot_codes8(const uint8_t *codes, uint64_t at) {
  const uint64_t *w = reinterpret_cast<const uint64_t *>(codes) + (at >> 3);
  const uint32_t sh = ((uint32_t)at & 7u) * 8u;
  const uint64_t a = w[0], b = w[1];
  return sh ? (a >> sh) | (b << (64u - sh)) : a;
}

// The whole BackwardSearch of one translated string, with text mode (round 3).  codes / at0: the chain's code stream
// (k_translate_prot), code i of this search at byte at0 + i.  As long as the range is wide the search runs on the BWT (table,
// extends); once it has matched text_min_l characters and holds <= 4 rows it continues on the text like the nucleotide kernel:
// the rows' suffix positions are fetched (SA), then rounds of 8 characters compare the read's codes with the text bytes left of
// every live position; rows that match the round's maximum survive (order kept).  The hit is then in text-position space
// (virt_text_pos: entry range, surviving rows, characters matched since the entry).  Exactness as for nucleotides: B[r] =
// T[SA[r] - 1], LF keeps the order of rows with equal symbol, a '$' in the text (code 0) never equals a read's code, the row of
// text position 0 drops out of a multi-row range (FMIndex::Rank's fix-up) and a single row at position 0 goes back to the BWT
// step (the reference's Access path decides, SURVEY.md Appendix B item 4); no round crosses position 0.
struct ProtHit { uint64_t sp, ep; int32_t pad; };
// codes8(at): the eight codes from byte `at` of the chain's stream on (k_search_prot: the global stream k_translate_prot wrote)
template <class Codes8>
__device__ __forceinline__ uint32_t prot_search_full(const DevView &v, const Codes8 &codes8, uint64_t at0, uint32_t m, ProtHit &H) {
  uint64_t c8 = codes8(at0);
  uint32_t c8_first = 0;
  auto code_at = [&](uint32_t q) -> uint32_t {
    if (q - c8_first >= 8u) { c8_first = q & ~7u; c8 = codes8(at0 + c8_first); }
    return (uint32_t)(c8 >> (8u * (q - c8_first))) & 0xffu;
  };
  uint64_t sp = 0, ep = 0;
  H.pad = 0;
  uint32_t l = 0;
  const uint32_t K = v.ftabx_width, w = v.ftab_width;
  bool started = false;
  if (v.ftabx && m >= K) {
    uint64_t key = 0;
    bool ok = true;
    for (uint32_t i = 0; i < K; ++i) {
      const uint32_t c = code_at(i);
      if (c >= v.prot.sigma) { ok = false; break; }
      key = key * v.prot.sigma + c;
    }
    if (ok) {
      const ulonglong2 e = ld16(v.ftabx + 2 * key);
      l = (uint32_t)(e.y & 0xffu);
      sp = e.x;
      ep = e.x + (e.y >> 8) - 1;
      if (l < K) { H.sp = sp; H.ep = ep; return l; }
      started = true;
    }
  }
  if (!started) {                                          // on-disk ftab (FMIndex.hpp:388-422)
    if (m < w) { H.sp = 0; H.ep = 0; return 0; }
    if (w > 0) {
      uint64_t key = 0;
      for (uint32_t i = 0; i < w; ++i) {
        const uint32_t c = code_at(i);
        if (c > 31u) { H.sp = 1; H.ep = 0; return i; }
        key = (key << v.prot.bits) | c;
      }
      const ulonglong2 e = ld16(v.ftab + 2 * key);
      if (e.y == 0) { H.sp = 1; H.ep = 0; return w - 1; }
      sp = e.x;
      ep = e.x + e.y - 1;
      l = w;
    } else { sp = 0; ep = v.n - 1; }
  }
  const bool text_ok = v.text8 != nullptr && v.sa32 != nullptr && v.steps.pos != nullptr;
  bool no_text = false;                                    // set when a single row at text position 0 went back to the BWT
  while (l < m) {
    if (text_ok && !no_text && l >= v.text_min_l && m - l <= kVirtDeltaMax && ep - sp < 4 && !(sp == ep && sp == v.first_isa)) {   // (m - l: kVirtDeltaMax, virt_text_pos)
      // ---- text mode
      uint32_t R = (uint32_t)(ep - sp) + 1u, mask = (1u << R) - 1u;
      uint32_t tp[4], idx[4] = {0, 1, 2, 3};
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) tp[k] = k < R ? v.sa32[sp + k] : 0u;
      const uint32_t l0 = l;
      bool back_to_bwt = false;
      while (l < m) {
        if (R == 1 && tp[0] == 0) { back_to_bwt = true; break; }
        uint32_t Lc = m - l < 8u ? m - l : 8u;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) if (k < R && tp[k] && tp[k] < Lc) Lc = tp[k];
        // the next 8 codes of the read (byte j = code l + j)
        const uint64_t rc8 = codes8(at0 + l);
        uint32_t e[4] = {0, 0, 0, 0}, J = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) if (k < R && tp[k]) {
          // text bytes left of position tp[k], nearest first: byte j = T[tp - 1 - j]  (16 zero bytes lie in front of the text)
          const uint64_t t8 = __builtin_bswap64(prot_codes8(v.text8 - 16, (uint64_t)tp[k] + 16 - 8));
          const uint64_t x = t8 ^ rc8;
          uint32_t ek = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
          if (ek > Lc) ek = Lc;
          e[k] = ek;
          if (ek > J) J = ek;
        }
        uint32_t cntR = 0, nmask = 0, ntp[4] = {0, 0, 0, 0}, nidx[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) if (k < R && e[k] >= J) {
#pragma unroll
          for (uint32_t q = 0; q < 4; ++q) if (q == cntR) { ntp[q] = tp[k] - J; nidx[q] = idx[k]; }
          nmask |= 1u << idx[k];
          ++cntR;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) { tp[k] = ntp[k]; idx[k] = nidx[k]; }
        R = cntR;
        mask = nmask;
        l += J;
        if (J < Lc) break;                                 // every row mismatched at character J: the search ends
      }
      if (!back_to_bwt) {
        H.sp = kVirtRow | ((uint64_t)(l - l0) << kVirtDeltaShift) | sp;
        H.ep = H.sp + (R - 1u);
        H.pad = (int32_t)mask;
        return l;
      }
      // single row at text position 0: take the step on the BWT (that row is firstISA) and stay there
      // (the rows matched so far were one row: its entry-range index is idx[0]; l characters are matched)
      sp = ep = v.first_isa;
      no_text = true;
      continue;
    }
    const uint32_t c = code_at(l);
    if (c > 31u) break;
    uint64_t nsp, nep;
    fm_extend(v, c, sp, ep, nsp, nep);
    if (nsp > nep || nep > v.n) break;
    sp = nsp;
    ep = nep;
    ++l;
  }
  H.sp = sp;
  H.ep = ep;
  return l;
}

// one entry of the derived table per K-mer key (first-read character in the most significant pair, like the ftab)
template <bool E8>
__global__ void k_build_ftabx(DevView v, uint32_t K, uint64_t *table) {
  const uint64_t entries = 1ull << (2 * K);
  for (uint64_t key = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; key < entries; key += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t sp = 0, ep = 0;
    const uint32_t l = fm_search_core(v, [&](uint32_t i) { return (uint32_t)((key >> (2 * (K - 1 - i))) & 3u); }, K, sp, ep);
    if (E8) { table[key] = ftabx8_encode(l, sp, ep, K, v.min_hit_len); continue; }
    const uint64_t cnt = ep - sp + 1;            // (1,0) -> 0
    table[2 * key] = sp;
    table[2 * key + 1] = (cnt << 8) | l;
  }
}

// FMIndex::GetSampledSA (FMIndex.hpp:203-231).  The reference's 1/1024 filter bitmap + std::map
// is an accelerator for "is row i a selectedSA key"; here the per-record flag plays that role.
__device__ __forceinline__ bool sel_lookup(const DevView &v, uint64_t row, uint64_t &val) {
  uint64_t lo = 0, hi = v.sel_cnt;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (v.sel_rows[mid] < row) lo = mid + 1; else hi = mid;
  }
  if (lo < v.sel_cnt && v.sel_rows[lo] == row) { val = v.sel_vals[lo]; return true; }
  return false;
}
__device__ __forceinline__ uint64_t sampled_read(const DevView &v, uint64_t idx) {   // FixedSizeElemArray::Read
  const uint64_t bit = idx * v.sampled_bits;
  const uint64_t w0 = v.sampled[bit >> 6], w1 = v.sampled[(bit >> 6) + 1];
  const uint32_t sh = (uint32_t)bit & 63u;
  uint64_t x = w0 >> sh;
  if (sh) x |= w1 << (64 - sh);
  return v.sampled_bits >= 64 ? x : (x & ((1ull << v.sampled_bits) - 1));
}

// ---- derived suffix array: u32 entries (n < 2^32) or 36-bit packed entries (entry i at bits [36 i, 36 i + 36))
struct __attribute__((packed, aligned(4))) U64a4 { uint64_t x; };
__device__ __forceinline__ uint64_t ld36(const uint32_t *tab, uint64_t i) {
  const uint64_t bit = 36ull * i;
  const uint64_t x = reinterpret_cast<const U64a4 *>(tab + (bit >> 5))->x;       // bits (bit & 31) + 36 <= 64
  return (x >> ((uint32_t)bit & 31u)) & 0xfffffffffull;
}
// Into a zero-filled table (neighbours share words): one 8-byte atomic OR, two for the entries that straddle two words.  (One plain unaligned 4-byte store for the bytes an entry owns
// alone plus one OR for the shared nibble was measured: the list ranking of an 8 Gbp text took 1.94 s instead of 1.27.)
__device__ __forceinline__ void st36_zeroed(uint32_t *tab, uint64_t i, uint64_t val) {
  const uint64_t bit = 36ull * i;
  const uint32_t b = (uint32_t)bit & 63u;
  unsigned long long *t64 = reinterpret_cast<unsigned long long *>(tab) + (bit >> 6);
  atomicOr(t64, (unsigned long long)(val << b));
  if (b > 28u) atomicOr(t64 + 1, (unsigned long long)(val >> (64u - b)));       // half of the entries straddle two 8-byte words
}
__device__ __forceinline__ uint64_t sa_entry(const DevView &v, uint64_t row) { return v.sa32 ? (uint64_t)v.sa32[row] : ld36(v.sa36, row); }

// Round 5: a K-mer that occurs ONCE and whose search goes on behind the table (l = K, one row) would fetch that row's suffix-array entry
// as its very next step (text mode: K >= text_min_l) - a dependent random gather that the table can carry instead: such an entry holds
// the row's TEXT POSITION in the count's place, bit 63 of its second word says so (count = 1; the low 16 bits stay as they were).
// cfg2: 2.3 of the 2.9 suffix-array fetches per read are of this kind.  Filled in after the suffix array exists.
__global__ void k_ftabx_textpos(DevView v, uint32_t K, uint64_t *table) {
  const uint64_t entries = 1ull << (2 * K);
  for (uint64_t key = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; key < entries; key += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t y = table[2 * key + 1];
    if (y != ((1ull << 8) | (uint64_t)K)) continue;              // one row, all K characters matched
    const uint64_t sp = table[2 * key];
    if (sp == v.first_isa) continue;                             // (the row of text position 0 takes the BWT step, SURVEY.md Appendix B item 4)
    table[2 * key + 1] = kFtabxTextPos | (sa_entry(v, sp) << 16) | y;
  }
}

// BackwardToSampledSA(row) as a function of the text position p = SA[row]: the walk moves left through the text and stops at
// the first position whose row stores a value (position 0, a selectedSA position, a sampled row); every such stop between a
// breakpoint and p carries the breakpoint's value (premise verified by k_memo_check at load), so the answer is the value of
// the last breakpoint at or left of p.  Two-level: a bucket table narrows the binary search to the breakpoints of one bucket.
__device__ __forceinline__ uint64_t steps_value(const StepView &S, uint64_t p) {
  if (p >= S.n) p = S.n - 1;
  const uint64_t b = p >> S.shift;
  uint64_t lo = S.bucket[b], hi = S.bucket[b + 1];       // last breakpoint <= bucket start, .. <= next bucket start: the answer lies in [lo, hi]
  while (lo < hi) { const uint64_t mid = (lo + hi + 1) >> 1; if (S.pos[mid] <= p) lo = mid; else hi = mid - 1; }
  return S.val[lo];
}
// ---- text-space hits.  A search that finished on the text (k_search_chains_v2) has no BWT range: its hit carries VIRTUAL rows,
//   sp  = kVirtRow | delta << 36 | sp0     sp0 = first row of the range the search had when it moved to the text (< 2^36),
//   ep  = sp + R - 1                       delta = characters matched after that point, R = rows that survived,
//   pad = bit k set: row sp0 + k survived  (k < 24: at most kWideRows rows enter the text)
// so that everything downstream keeps reading ep - sp + 1 as the number of rows and sp == ep as "unique hit".  The rows LF would
// have led to are ISA[SA[sp0 + k] - delta] (same order: rows with equal BWT symbol keep their order under LF), and
// BackwardToSampledSA of such a row only depends on its text position SA[sp0 + k] - delta: no inverse suffix array is needed.
// With kVirtInline in sp the search wrote those text positions themselves (it held them in registers when it ended), and no
// suffix-array entry is fetched: bits 0..35 of sp = position of the first surviving row, pad = position of the second one (a
// two-row hit is only written this way where positions have 32 bits); delta is still there, nobody reads it.  One list can hold
// both forms: hits of 3 or more rows, two-row hits of a 36-bit image and the lookup stage of the two-launch search write the mask.
__device__ __forceinline__ uint64_t virt_text_pos(const DevView &v, const cfr_hit &H, uint64_t row) {
  if (H.sp & kVirtInline) return row == H.sp ? (H.sp & kVirtRowMask) : (uint64_t)(uint32_t)H.pad;
  uint32_t m = (uint32_t)H.pad;
  for (uint32_t q = (uint32_t)(row - H.sp); q; --q) m &= m - 1u;               // the (row - sp)-th surviving row
  const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
  return sa_entry(v, (H.sp & kVirtRowMask) + k) - ((H.sp >> kVirtDeltaShift) & (uint64_t)kVirtDeltaMax);
}
// what FMIndex::BackwardToSampledSA returns for a row of hit H, by ONE table access: a virtual row through its text position,
// a real row by the locate memo (when the image has one at every row) or through its suffix-array entry
__device__ __forceinline__ uint64_t locate_row(const DevView &v, const cfr_hit &H, uint64_t row) {
  if (H.sp & kVirtRow) return steps_value(v.steps, virt_text_pos(v, H, row));
  if (v.loc_memo && v.memo_shift == 0) return (uint64_t)v.loc_memo[row];
  return steps_value(v.steps, sa_entry(v, row));
}

// FMIndex::BackwardToSampledSA (FMIndex.hpp:514-524): LF-walk until a row whose SA value is stored.
// One record (32 B header + 16 B half) per LF step; branch order of GetSampledSA kept.
template <bool USE_MEMO = true>
__device__ __forceinline__ uint64_t fm_locate(const DevView &v, uint64_t i, uint32_t &steps) {
  steps = 0;
  if (i & kVirtRow) return steps_value(v.steps, i & ~kVirtRow);               // a row of a text-space hit, resolved to its text position (k_enum_rows)
  if (USE_MEMO && !(v.loc_memo && v.memo_shift == 0) && v.steps.pos && (v.sa32 || v.sa36)) return steps_value(v.steps, sa_entry(v, i));
  for (;;) {
    if (USE_MEMO && v.loc_memo && (i & ((1ull << v.memo_shift) - 1)) == 0) return v.loc_memo[i >> v.memo_shift];
    if (i == v.first_isa) return v.adjusted_sa0;
    if (i % v.sample_rate == 0) return sampled_read(v, i / v.sample_rate);
    if (v.prot.enabled) {   // no selectedSA in a protein index; rows below the end-marker count store their sequence id (FMIndex.hpp:224-228)
      if (i < v.prot.endmarker_n) {
        const uint64_t bit = i * v.prot.endmarker_bits;
        const uint64_t w0 = v.prot.endmarker[bit >> 6], w1 = v.prot.endmarker[(bit >> 6) + 1];
        const uint32_t sh = (uint32_t)bit & 63u;
        uint64_t x = w0 >> sh;
        if (sh) x |= w1 << (64 - sh);
        return v.prot.endmarker_bits >= 64 ? x : (x & ((1ull << v.prot.endmarker_bits) - 1));
      }
      const uint32_t c = prot_access(v.prot, i);
      i = v.prot.C[c] + fm_rank(v, c, i, 1) - 1;
      ++steps;
      continue;
    }
    if (v.rb.enabled) {   // filter bitmap + map lookup, then LF on the compressed components (FMIndex.hpp:215-223, 382-386)
      if (v.rb.sel_filter && ((v.rb.sel_filter[(i / v.rb.filter_rate) >> 6] >> ((i / v.rb.filter_rate) & 63u)) & 1ull)) {
        uint64_t val;
        if (sel_lookup(v, i, val)) return val;
      }
      const uint32_t c = rb_access(v.rb, i);
      i = v.C[c] + fm_rank(v, c, i, 1) - 1;
      ++steps;
      continue;
    }
    const uint64_t *rec = occ_rec(v, i);
    const uint32_t h = ((uint32_t)i >> 6) & 1u, j = (uint32_t)i & 63u;
    const ulonglong2 m01 = ld16(rec);
    const ulonglong2 m23 = ld16(rec + 2);
    const ulonglong2 pl = ld16(rec + 4 + 2 * h);
    if (m01.x & kSelFlag) {
      uint64_t val;
      if (sel_lookup(v, i, val)) return val;
    }
    const uint32_t c = (uint32_t)((pl.x >> j) & 1u) | ((uint32_t)((pl.y >> j) & 1u) << 1);   // Access(i)
    const uint64_t mid = c == 0 ? m01.x : c == 1 ? m01.y : c == 2 ? m23.x : m23.y;
    i = v.C[c] + occ_count(mid, pl.x, pl.y, c, i, 1) + fm_fix(v, c, i, 1) - 1;              // LF (FMIndex.hpp:382-386)
    ++steps;
  }
}

// Classifier::CalculateHitScore (Classifier.hpp:243-252)
__device__ __forceinline__ uint64_t hit_score(const DevView &v, int32_t l) {
  if (l < v.min_hit_len) return 0;
  const uint64_t d = (uint64_t)(int64_t)(l - v.score_adjust);
  return d * d;
}

// =============================================================================== probe kernels
__global__ void k_rank_probe(DevView v, const char *chars, const uint64_t *pos, const uint8_t *incl, size_t n,
                             uint64_t *out_rank, char *out_access) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (v.prot.enabled) {
    const uint32_t pc = v.prot.code_of[(uint8_t)chars[i]];
    if (out_rank) out_rank[i] = pc < 32 ? fm_rank(v, pc, pos[i], incl[i] ? 1u : 0u) : 0;
    if (out_access) out_access[i] = v.prot.list[prot_access(v.prot, pos[i])];
    return;
  }
  const uint32_t c = base_code((uint8_t)chars[i]);
  if (out_rank) out_rank[i] = c < 4 ? fm_rank(v, c, pos[i], incl[i] ? 1u : 0u) : 0;
  if (out_access) out_access[i] = "ACGT"[bwt_access(v, pos[i])];
}

__global__ void k_bs_probe(DevView v, const uint8_t *bases, const uint64_t *offs, const uint32_t *m, size_t n,
                           uint64_t *out_l, uint64_t *out_sp, uint64_t *out_ep) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SeqView s{bases + offs[i], (int32_t)(offs[i + 1] - offs[i]), 0};
  uint64_t sp = 0, ep = 0;
  if (v.prot.enabled) {          // the probe string is an amino-acid string
    const uint32_t mm = m[i];
    out_l[i] = prot_backward_search(v, [&](uint32_t q) { return (uint32_t)v.prot.code_of[s.s[mm - 1 - q]]; }, mm, sp, ep);
    out_sp[i] = sp;
    out_ep[i] = ep;
    return;
  }
  out_l[i] = fm_backward_search(v, s, m[i], sp, ep);
  out_sp[i] = sp;
  out_ep[i] = ep;
}

__global__ void k_locate(DevView v, const uint64_t *rows, size_t n, uint64_t *out_val, uint32_t *out_steps) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t steps;
  if (out_steps) {          // probe form: the reference's walk length is part of the answer, so no memo shortcut
    out_val[i] = fm_locate<false>(v, rows[i], steps);
    out_steps[i] = steps;
  } else {
    out_val[i] = fm_locate<true>(v, rows[i], steps);
  }
}

// derived locate memo: memo[j] = BackwardToSampledSA(j << shift), computed with the plain walk
__global__ void k_build_loc_memo(DevView v, uint32_t shift, uint64_t entries, uint32_t *memo) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < entries; j += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t steps;
    memo[j] = (uint32_t)fm_locate<false>(v, j << shift, steps);
  }
}

// =============================================================================== path kernels
// per-read hit capacity: each strand chain of a read of length L holds at most L/(minHitLen+1)+1 hits
__device__ __forceinline__ uint32_t chain_cap(const DevView &v, uint32_t len) { return len / (uint32_t)(v.min_hit_len + 1) + 1u; }

__global__ void k_caps(DevView v, const uint64_t *offs1, const uint64_t *offs2, size_t n, uint64_t *cap) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t c = 2ull * chain_cap(v, (uint32_t)(offs1[i + 1] - offs1[i]));
  if (offs2) c += 2ull * chain_cap(v, (uint32_t)(offs2[i + 1] - offs2[i]));
  cap[i] = c;
}

// Classifier::GetHitsFromRead (Classifier.hpp:274-293): one lane per (read, mate, strand) chain.
// chain = CPR*i + 2*mate + rc (CPR = 2 single-end, 4 paired); raw hits go to raw[hit_off[i] + sub-offset ...).
template <int CPR>
__global__ void k_search_chains(DevView v, const uint8_t *bases1, const uint64_t *offs1, const uint8_t *bases2,
                                const uint64_t *offs2, size_t n, const uint64_t *hit_off, cfr_hit *raw,
                                uint32_t *chain_cnt) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t / CPR;
  if (i >= n) return;
  const uint32_t mate = CPR == 4 ? (uint32_t)(t >> 1) & 1u : 0u, rc = (uint32_t)t & 1u;
  const uint32_t len1 = (uint32_t)(offs1[i + 1] - offs1[i]);
  const uint32_t len = mate ? (uint32_t)(offs2[i + 1] - offs2[i]) : len1;
  SeqView s{mate ? bases2 + offs2[i] : bases1 + offs1[i], (int32_t)len, (int32_t)rc};
  const uint32_t cap1 = chain_cap(v, len1);
  cfr_hit *out = raw + hit_off[i] + (mate ? 2ull * cap1 : 0ull) + (rc ? (uint64_t)chain_cap(v, len) : 0ull);
  uint32_t cnt = 0;
  uint64_t sp = 0, ep = 0;
  int32_t remaining = (int32_t)len;
  while (remaining >= v.min_hit_len) {
    const int32_t l = (int32_t)fm_backward_search(v, s, (uint32_t)remaining, sp, ep);
    if (l >= v.min_hit_len && sp <= ep) {
      cfr_hit h;
      h.sp = sp; h.ep = ep; h.l = l; h.strand = 0; h.offset = (int32_t)len - remaining; h.pad = 0;
      out[cnt++] = h;
    }
    remaining -= l + 1;
  }
  chain_cnt[t] = cnt;
}

// Classifier::AdjustHitBoundaryFromStrandHits (Classifier.hpp:303-401) on the two raw lists of one mate.
// F = hits of r (strandHits[1]), R = hits of rc (strandHits[0]).
__device__ __forceinline__ void adjust_boundaries(const DevView &v, const uint8_t *r, int32_t len, cfr_hit *F, int32_t nF, cfr_hit *R, int32_t nR) {
  if (!nF || !nR) return;
  SeqView fwd{r, len, 0}, rev{r, len, 1};
  uint64_t sp = 0, ep = 0;
  int32_t j = nR - 1;
  bool fixF = false, fixR = false;
  for (int32_t i = 0; i < nF; ++i) {
    const int32_t right = len - F[i].offset - 1;
    const int32_t left = right - F[i].l + 1;
    for (; j >= 0; --j) {
      const int32_t rcLeft = R[j].offset;
      const int32_t rcRight = rcLeft + R[j].l - 1;
      if (rcLeft >= right) continue;
      if (left >= rcRight) break;
      if (left == rcLeft && right == rcRight) break;
      if (left < rcLeft && rcRight < right) break;
      if (rcLeft < left && right < rcRight) break;
      if (rcRight > right) {
        const int32_t l = (int32_t)fm_backward_search(v, fwd, (uint32_t)(rcRight + 1), sp, ep);
        if (rcRight - l + 1 == left && sp <= ep) {
          cfr_hit h; h.sp = sp; h.ep = ep; h.l = l; h.strand = 1; h.offset = len - rcRight - 1; h.pad = 0;
          F[i] = h;
          fixF = true;
        }
      }
      if (left < rcLeft) {
        const int32_t l = (int32_t)fm_backward_search(v, rev, (uint32_t)(len - left), sp, ep);
        if (left + l - 1 == rcRight && sp <= ep) {
          cfr_hit h; h.sp = sp; h.ep = ep; h.l = l; h.strand = -1; h.offset = left; h.pad = 0;
          R[j] = h;
          fixR = true;
        }
      }
    }
  }
  for (int32_t k = 0; k <= 1; ++k) {
    if (!(k ? fixF : fixR)) continue;
    cfr_hit *H = k ? F : R;
    const int32_t nh = k ? nF : nR;
    for (int32_t i = 0; i < nh - 1; ++i) {
      const int32_t starti = H[i].offset;
      const int32_t endi = starti + H[i].l - 1;
      for (int32_t q = i + 1; q < nh; ++q) {
        const int32_t startj = H[q].offset;
        if (startj > endi) break;
        const int32_t endj = startj + H[q].l - 1;
        if (H[q].l >= H[i].l) { H[i].l = startj - starti; break; }
        if (endj <= endi) H[q].l = 0;
        else { H[q].offset = endi + 1; H[q].l = endj - (endi + 1) + 1; break; }
      }
    }
  }
}

// rows BackwardToSampledSA is called on for one hit (Classifier.hpp:620-666)
__device__ __forceinline__ uint64_t hit_row_count(const DevView &v, const cfr_hit &h) {
  if (h.l < v.min_hit_len) return 0;
  const uint64_t range = h.ep - h.sp + 1;
  if (range <= v.max_entries || v.locate_all) return range;
  const uint64_t step = (range + v.max_entries - 1) / v.max_entries;
  const uint64_t fwd = (range + step - 1) / step;
  uint64_t bwd = v.max_entries > fwd ? v.max_entries - fwd : 1;   // break is tested AFTER each backward locate
  if (bwd > fwd) bwd = fwd;
  return fwd + bwd;
}

// append one strand list to the read's final hits, with its strand and the number of rows each hit will locate
__device__ __forceinline__ void emit_hits(const DevView &v, const cfr_hit *src, int32_t m, int32_t strand, cfr_hit *out,
                                          uint64_t *rows, uint64_t &cnt, uint64_t &row_total) {
  for (int32_t q = 0; q < m; ++q) {
    cfr_hit h = src[q];
    h.strand = strand;                                   // (pad stays: the row mask of a text-space hit)
    const uint64_t rc_ = hit_row_count(v, h);
    rows[cnt] = rc_;
    row_total += rc_;
    out[cnt++] = h;
  }
}

// Second half of SearchForwardAndReverse (Classifier.hpp:509-583): adjust both mates, merge mate lists
// (mate 2's '+' hits join the '-' list and vice versa, :551-552), score, pick strand(s) (:568-576).
// One lane per read.  Final hits -> fin[hit_off[i] ...), count -> fin_cnt[i], rows per hit -> fin_rows[...].
template <int CPR>
__global__ void k_adjust_select(DevView v, const uint8_t *bases1, const uint64_t *offs1, const uint8_t *bases2,
                                const uint64_t *offs2, size_t n, const uint64_t *hit_off, cfr_hit *raw,
                                const uint32_t *chain_cnt, cfr_hit *fin, uint64_t *fin_cnt, uint64_t *fin_rows,
                                uint64_t *read_rows) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t len1 = (int32_t)(offs1[i + 1] - offs1[i]);
  const uint32_t cap1 = chain_cap(v, (uint32_t)len1);
  cfr_hit *base = raw + hit_off[i];
  cfr_hit *F1 = base, *R1 = base + cap1, *F2 = nullptr, *R2 = nullptr;
  const int32_t nF1 = (int32_t)chain_cnt[CPR * i + 0], nR1 = (int32_t)chain_cnt[CPR * i + 1];
  int32_t nF2 = 0, nR2 = 0;
  adjust_boundaries(v, bases1 + offs1[i], len1, F1, nF1, R1, nR1);
  if (CPR == 4) {
    const int32_t len2 = (int32_t)(offs2[i + 1] - offs2[i]);
    const uint32_t cap2 = chain_cap(v, (uint32_t)len2);
    F2 = base + 2ull * cap1;
    R2 = F2 + cap2;
    nF2 = (int32_t)chain_cnt[CPR * i + 2];
    nR2 = (int32_t)chain_cnt[CPR * i + 3];
    adjust_boundaries(v, bases2 + offs2[i], len2, F2, nF2, R2, nR2);
  }
  // strandHits[1] = F1 ++ R2 ; strandHits[0] = R1 ++ F2
  uint64_t score_plus = 0, score_minus = 0;
  for (int32_t q = 0; q < nF1; ++q) score_plus += hit_score(v, F1[q].l);
  for (int32_t q = 0; q < nR2; ++q) score_plus += hit_score(v, R2[q].l);
  for (int32_t q = 0; q < nR1; ++q) score_minus += hit_score(v, R1[q].l);
  for (int32_t q = 0; q < nF2; ++q) score_minus += hit_score(v, F2[q].l);
  bool take_plus, take_minus;
  if (score_plus > score_minus + score_minus / 100) { take_plus = true; take_minus = false; }
  else if (score_minus > score_plus + score_plus / 100) { take_plus = false; take_minus = true; }
  else { take_plus = true; take_minus = true; }
  cfr_hit *out = fin + hit_off[i];
  uint64_t *rows = fin_rows + hit_off[i];
  uint64_t cnt = 0;
  uint64_t row_total = 0;
  if (take_plus) { emit_hits(v, F1, nF1, 1, out, rows, cnt, row_total); emit_hits(v, R2, nR2, 1, out, rows, cnt, row_total); }
  if (take_minus) { emit_hits(v, R1, nR1, -1, out, rows, cnt, row_total); emit_hits(v, F2, nF2, -1, out, rows, cnt, row_total); }
  fin_cnt[i] = cnt;
  if (read_rows) read_rows[i] = row_total;
}

// compaction of the per-read regions into dense arrays
__global__ void k_compact_hits(size_t n, const uint64_t *hit_off, const uint64_t *fin_off, const cfr_hit *fin,
                               const uint64_t *fin_rows, cfr_hit *hits, uint64_t *rows_per_hit) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t src = hit_off[i], dst = fin_off[i], m = fin_off[i + 1] - fin_off[i];
  for (uint64_t q = 0; q < m; ++q) {
    hits[dst + q] = fin[src + q];
    rows_per_hit[dst + q] = fin_rows[src + q];
  }
}

// the exact row sequence of Classifier.hpp:625-665 for each hit, one lane per hit
__global__ void k_enum_rows(DevView v, size_t nhits, const cfr_hit *hits, const uint64_t *row_off, uint64_t *rows) {
  const size_t hI = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (hI >= nhits) return;
  const cfr_hit h = hits[hI];
  uint64_t *out = rows + row_off[hI];
  const uint64_t total = row_off[hI + 1] - row_off[hI];
  if (total == 0) return;
  const uint64_t range = h.ep - h.sp + 1;
  // a row of a text-space hit leaves as kVirtRow | its text position (what k_locate / fm_locate answer from)
  auto row_of = [&](uint64_t j) -> uint64_t { return (h.sp & kVirtRow) ? (kVirtRow | virt_text_pos(v, h, j)) : j; };
  if (range <= v.max_entries || v.locate_all) {
    for (uint64_t q = 0; q < range; ++q) out[q] = row_of(h.sp + q);
    return;
  }
  const uint64_t step = (range + v.max_entries - 1) / v.max_entries;
  uint64_t k = 0;
  for (uint64_t j = h.sp; j <= h.ep; j += step) out[k++] = row_of(j);
  uint64_t resolved = k;
  for (uint64_t j = h.ep; j >= h.sp && j <= h.ep; j -= step) {
    out[k++] = row_of(j);
    ++resolved;
    if (resolved >= v.max_entries) break;
  }
}

// ---- protein path: the kernels of the translated search (helpers: dna_to_aa, AaView, prot_backward_search above)
__device__ __forceinline__ uint32_t prot_chain_cap(const DevView &v, uint32_t len) { return (len / 3u) / (uint32_t)(v.min_hit_len + 1) + 1u; }
// per read: 6 chains per mate (strand x frame), each with room for prot_chain_cap hits
__global__ void k_caps_prot(DevView v, const uint64_t *offs1, const uint64_t *offs2, size_t n, uint64_t *cap) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t c = 6ull * prot_chain_cap(v, (uint32_t)(offs1[i + 1] - offs1[i]));
  if (offs2) c += 6ull * prot_chain_cap(v, (uint32_t)(offs2[i + 1] - offs2[i]));
  cap[i] = c;
}
// The six translations of every read (Classifier::TranslatedSearch, :463-506: three frames of the read and of its reverse
// complement), written once as plain codes in the order the searches consume them (GetHitsFromRead walks a string from its end):
// read r of the batch at bases [o, o + len) owns the 8-byte aligned region from prot_code_base(o, r) on; chain c = 3 rc + frame
// takes prot_code_stride(len) bytes of it from c x that stride on (whole 8-byte words); byte j of a chain = code of amino acid
// k - 1 - j (k = (len - frame) / 3), 255 = not a symbol.
__device__ __forceinline__ uint64_t prot_code_stride(uint32_t len) { return ((uint64_t)(len / 3u) + 7ull) & ~7ull; }
__device__ __forceinline__ uint64_t prot_code_base(uint64_t o, uint64_t read) { return (2ull * o + 56ull * read + 7ull) & ~7ull; }   // (6 strides <= 2 len + 42)
// One WAVE per read (and mate): the read's characters are classified once into LDS (A C G T N other), every codon start gets
// its amino-acid code for both strands from a 125-entry table of DnaToAa's answers (F[y]: codon y, y+1, y+2 read forwards;
// R[y]: the same three characters complemented and read backwards), and the lanes then write the read's region word by word -
// consecutive lanes, consecutive 8-byte words.  (One LANE per chain walking DnaToAa's if/else ladder per amino acid took 8.3 ms per
// 4 M reads - 40 % of the protein step - and wrote 4.3 x the region's bytes in partial lines; this form: see DESIGN.md 4b.)
// Reads longer than kProtStage characters are translated from global memory, the same words.
constexpr uint32_t kProtStage = 1024;
#ifndef CFR_PROT_GROUP
#define CFR_PROT_GROUP 4
#endif
constexpr uint32_t kProtGroup = CFR_PROT_GROUP;
template <int MATES>
__global__ __launch_bounds__(256) void k_translate_prot(DevView v, const uint8_t *bases1, const uint64_t *offs1, const uint8_t *bases2, const uint64_t *offs2, size_t n,
                                                        uint8_t *codes1, uint8_t *codes2, uint64_t read0) {
  __shared__ uint8_t s_lut[128];
  __shared__ uint8_t s_cls[4][kProtStage + 8], s_f[4][kProtStage + 8], s_r[4][kProtStage + 8];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (tid < 125) {
    const char rep[5] = {'A', 'C', 'G', 'T', 'N'};
    s_lut[tid] = v.prot.code_of[(uint8_t)dna_to_aa((uint32_t)rep[tid / 25], (uint32_t)rep[(tid / 5) % 5], (uint32_t)rep[tid % 5])];
  }
  __syncthreads();
  auto wave_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // classes: A 0, C 1, G 2, T 3, N 4, anything else 5.  Forward strand: DnaToAa's ladder sends what it does not test down its last
  // (T) branch and only 'N' to '?' -> {0,1,2,3,4,3}; reverse strand (ReverseComplement: non-ACGT -> 'N') -> {3,2,1,0,4,4}
  auto cls_of = [](uint32_t ch) -> uint32_t { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : ch == 'N' ? 4u : 5u; };
  auto fw = [](uint32_t c) -> uint32_t { return (0x343210u >> (4u * c)) & 15u; };
  auto rv = [](uint32_t c) -> uint32_t { return (0x440123u >> (4u * c)) & 15u; };
  uint8_t *cls = s_cls[wv], *F = s_f[wv], *R = s_r[wv];
  // A wave takes kProtGroup reads at a time: their offsets, then the first 192 characters of each, are fetched together before the
  // first of them is worked on - one read at a time the wave stood through two memory round trips per read with nothing else to do
  // (3.2 ms per 4 M reads for 2.3 GB of traffic, round 3).
  const size_t nitems = n * MATES, nwaves = (size_t)gridDim.x * 4;
  for (size_t it0 = ((size_t)blockIdx.x * 4 + wv) * kProtGroup; it0 < nitems; it0 += nwaves * kProtGroup) {
   uint64_t og[kProtGroup];
   uint32_t leng[kProtGroup], bg[kProtGroup][3];
#pragma unroll
   for (uint32_t g = 0; g < kProtGroup; ++g) {
     const size_t it = it0 + g, i = it / MATES;
     const uint64_t *of = (it % MATES) ? offs2 : offs1;
     og[g] = it < nitems ? of[i] : 0ull;
     leng[g] = it < nitems ? (uint32_t)(of[i + 1] - og[g]) : 0u;
   }
#pragma unroll
   for (uint32_t g = 0; g < kProtGroup; ++g) {
     const uint8_t *sg = (((it0 + g) % MATES) ? bases2 : bases1) + og[g];
#pragma unroll
     for (uint32_t j = 0; j < 3; ++j) bg[g][j] = lane + 64u * j < leng[g] ? (uint32_t)sg[lane + 64u * j] : 0u;
   }
#pragma unroll
   for (uint32_t g = 0; g < kProtGroup; ++g) {
    const size_t it = it0 + g;
    if (it >= nitems) break;
    const size_t i = it / MATES;
    const uint32_t mate = (uint32_t)(it % MATES);
    const uint64_t o = og[g];
    const uint32_t len = leng[g];
    const uint8_t *s = (mate ? bases2 : bases1) + o;
    const uint32_t wpc = (uint32_t)(prot_code_stride(len) >> 3), nwords = 6u * wpc;       // words per chain, words of the read
    uint64_t *dst = reinterpret_cast<uint64_t *>((mate ? codes2 : codes1) + prot_code_base(o, read0 + i));
    const bool staged = len <= kProtStage;
    if (staged) {
#pragma unroll
      for (uint32_t j = 0; j < 3; ++j) if (lane + 64u * j < len) cls[lane + 64u * j] = (uint8_t)cls_of(bg[g][j]);
      for (uint32_t x = lane + 192u; x < len; x += 64) cls[x] = (uint8_t)cls_of(s[x]);
      wave_sync();
      for (uint32_t y = lane; y + 2 < len; y += 64) {
        const uint32_t c0 = cls[y], c1 = cls[y + 1], c2 = cls[y + 2];
        F[y] = s_lut[fw(c0) * 25u + fw(c1) * 5u + fw(c2)];
        R[y] = s_lut[rv(c2) * 25u + rv(c1) * 5u + rv(c0)];
      }
      wave_sync();
    }
    for (uint32_t q = lane; q < nwords; q += 64) {
      const uint32_t c = q / wpc, j0 = 8u * (q % wpc), rc = c >= 3u ? 1u : 0u, frame = c - 3u * rc;
      const uint32_t k = len >= frame + 3u ? (len - frame) / 3u : 0u;
      uint64_t w = 0;
      if (staged) {
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) {
          const uint32_t j = j0 + t;
          uint64_t code = 255ull;
          if (j < k) {
            const uint32_t x = frame + 3u * (k - 1u - j);                 // strand position of the codon
            code = rc ? R[len - 3u - x] : F[x];
          }
          w |= code << (8u * t);
        }
      } else {
        AaView a{s, (int32_t)len, (int32_t)rc, (int32_t)frame, (int32_t)k};
        for (uint32_t t = 0; t < 8; ++t) {
          const uint32_t j = j0 + t;
          const uint64_t code = j < k ? (uint64_t)(uint8_t)a.code(v.prot, (int32_t)(k - 1u - j)) : 255ull;
          w |= code << (8u * t);
        }
      }
      dst[q] = w;
    }
    wave_sync();                                                          // the LDS columns are the next read's
   }
  }
}
// GetHitsFromRead (Classifier.hpp:274-293) on one translated frame: chain = (6 * MATES) * read + 6 * mate + 3 * rc + frame
template <int MATES, int MINB>
__global__ __launch_bounds__(256, MINB) void k_search_prot(DevView v, const uint8_t *bases1, const uint64_t *offs1, const uint8_t *bases2, const uint64_t *offs2, size_t n,
                              const uint64_t *hit_off, cfr_hit *raw, uint32_t *chain_cnt, const uint8_t *codes1, const uint8_t *codes2, uint64_t read0) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t / (6 * MATES);
  if (i >= n) return;
  const uint32_t sub = (uint32_t)(t % (6 * MATES)), mate = sub / 6u, rc = (sub / 3u) & 1u, frame = sub % 3u;
  const uint32_t len1 = (uint32_t)(offs1[i + 1] - offs1[i]);
  const uint32_t len = mate ? (uint32_t)(offs2[i + 1] - offs2[i]) : len1;
  AaView s{mate ? bases2 + offs2[i] : bases1 + offs1[i], (int32_t)len, (int32_t)rc, (int32_t)frame, 0};
  s.k = (int32_t)len >= (int32_t)frame + 3 ? ((int32_t)len - (int32_t)frame) / 3 : 0;
  const uint32_t cap = prot_chain_cap(v, len);
  cfr_hit *out = raw + hit_off[i] + (mate ? 6ull * prot_chain_cap(v, len1) : 0ull) + (uint64_t)(3u * rc + frame) * cap;
  uint32_t cnt = 0;
  uint64_t sp = 0, ep = 0;
  int32_t remaining = s.k;
  // the chain's codes (k_translate_prot) are consumed front to back: a search at `remaining` starts at byte k - remaining
  const uint8_t *cb = mate ? codes2 : codes1;
  const uint64_t cbase = prot_code_base(mate ? offs2[i] : offs1[i], read0 + i) + (uint64_t)(3u * rc + frame) * prot_code_stride(len);
  auto run_chain = [&](const auto &codes8, uint64_t base) {
    while (remaining >= v.min_hit_len) {
      const int32_t m = remaining;
      const uint64_t at0 = base + (uint64_t)(s.k - remaining);
      ProtHit PH;
      const int32_t l = (int32_t)prot_search_full(v, codes8, at0, (uint32_t)m, PH);
      sp = PH.sp; ep = PH.ep;
      if (l >= v.min_hit_len && sp <= ep) {
        cfr_hit h;
        h.sp = sp; h.ep = ep; h.l = l; h.strand = 0; h.offset = s.k - remaining; h.pad = PH.pad;
        out[cnt++] = h;
      }
      remaining -= l + 1;
    }
  };
  // (Round 4 measured the chain's codes copied into LDS first - eight independent loads, every search then reads its codes from
  // there instead of starting with a dependent fetch: 16.4 against 15.0 ms per 4 M reads for translation + search.  The searches of
  // a frame do not wait for their codes - the stream is short and stays in the caches - so the copy only added its own work.)
  auto glob8 = [&](uint64_t at) -> uint64_t { return prot_codes8(cb, at); };
  run_chain(glob8, cbase);
  chain_cnt[t] = cnt;
}
// ---- k_search_prot_sm (round 4): the searches of k_search_prot with every lane a state machine.
// k_search_prot runs one chain per lane with prot_search_full inlined: the lanes of a wave are in different parts of it (table look-up,
// BWT steps, suffix-array fetch, text rounds) and every part that some lane is in costs the whole wave its memory round trip - a wave
// pays the sum of its lanes' paths, and five of a read's six frames are short paths next to one long one.  Here one iteration of the
// wave = one round trip for every lane whatever it is doing: (A) each lane runs the steps that need no memory until it stands at a
// fetch, (B) all fetches of the wave are issued together through ten slots (four of 16 bytes, four of 8, two of 4: what a slot
// holds depends on the lane's state), (C) each lane consumes its own.  A lane that finishes a chain goes on with chain + T (T = the
// lanes of the resident grid) without waiting for its neighbours; a frame's 46 chains per lane average the paths out.
// The chain's codes (k_translate_prot's stream) are kept as a 64-byte window in LDS (dword j of lane t at s_win[256 j + t]: no bank
// conflicts); a 150 bp read's chain fits in one window, a longer chain moves it.  Same results as k_search_prot, hit for hit.
struct __attribute__((packed)) U64a1 { uint64_t x; };
typedef uint32_t Q16 __attribute__((ext_vector_type(4)));     // one 16-byte slot: kept as ONE value so that a fetch lands in its registers
typedef Q16 Q16a4 __attribute__((aligned(4)));               //  (a 16-byte load from a 4-byte aligned address)
enum : uint32_t { PS_BEGIN, PS_FTKEY, PS_DECIDE, PS_TXTPRE, PS_END,                   // no memory
                  PS_NEW, PS_CODES, PS_FT, PS_EXT, PS_SA, PS_TXT, PS_DONE };          // from PS_NEW on: the lane waits for phase B
template <int MATES, int MINB>
__global__ __launch_bounds__(256, MINB) void k_search_prot_sm(DevView v, const uint64_t *offs1, const uint64_t *offs2, size_t n, const uint64_t *hit_off, cfr_hit *raw,
                                                        uint32_t *chain_cnt, const uint8_t *codes1, const uint8_t *codes2, uint64_t read0,
                                                        unsigned long long *tile_ctr, uint32_t tile) {
  // tile_ctr / tile (round 5): chains beyond every lane's first are handed out by WAVE TILES like the nucleotide search's (one atomic per
  // `tile` chains, the lanes that need a chain share the wave's tile by ballot) instead of chain + T: the six frames of a read are of very
  // different lengths - one matches, five end inside their first look-ups.  tile_ctr == nullptr: chain + T as before.
  __shared__ uint32_t s_win[16 * 256];
  __shared__ uint64_t s_C[33];
  const uint32_t t = threadIdx.x;
  if (t < 33) s_C[t] = v.prot.C[t];
  __syncthreads();
  constexpr uint32_t CH = 6 * MATES;
  const uint32_t nchains = (uint32_t)(n * CH), stride = gridDim.x * 256u;      // (the host sends at most 2^32 - 2^26 chains here)
  uint32_t chain = blockIdx.x * 256u + t;
  uint32_t st = chain < nchains ? (uint32_t)PS_NEW : (uint32_t)PS_DONE, ret = PS_BEGIN, wbase = 0, wreq = 0;
  uint32_t wt_next = 0, wt_end = 0;       // wave tiles: the chains [stride + wt_next, stride + wt_end) are this wave's and not taken yet
  bool want_chain = false;
  int32_t k = 0, remaining = 0, pad = 0;
  uint32_t m = 0, l = 0, s0 = 0, cnt = 0, ce = 0, ftdisk = 0, l0 = 0;
  uint64_t sp = 0, ep = 0, cbase = 0;
  bool no_text = false;
  uint32_t tp[4] = {0, 0, 0, 0}, idx[4] = {0, 1, 2, 3}, R = 0, mask = 0;
  const uint8_t *cb = codes1;
  cfr_hit *out = raw;
  const void *fptr = nullptr;
  const uint32_t K = v.ftabx_width, wd = v.ftab_width, sigma = v.prot.sigma;
  const bool text_ok = v.text8 != nullptr && v.sa32 != nullptr && v.steps.pos != nullptr;

  auto win = [&](uint32_t j) -> uint32_t { return s_win[((j < 15u ? j : 15u) << 8) + t]; };
  auto win_ok = [&](uint32_t p, uint32_t need) -> bool { return p >= wbase && p + need <= wbase + 64u; };
  auto code_at = [&](uint32_t p) -> uint32_t { const uint32_t o = p - wbase; return (win(o >> 2) >> (8u * (o & 3u))) & 0xffu; };
  // the twelve codes from p on (win_ok(p, 12)): eight in a, four in b
  auto codes12 = [&](uint32_t p, uint64_t &a, uint32_t &b) {
    const uint32_t o = p - wbase, j = o >> 2, sh = 8u * (o & 3u);
    const uint64_t d0 = win(j), d1 = win(j + 1), d2 = win(j + 2), d3 = win(j + 3);
    const uint64_t lo = (d0 | (d1 << 32)) >> sh, mid = (d1 | (d2 << 32)) >> sh, hi = (d2 | (d3 << 32)) >> sh;
    a = (lo & 0xffffffffull) | (mid << 32);
    b = (uint32_t)hi;
  };

  for (;;) {
    // ================================================================ (A) everything that needs no memory
    // One pass in the order a lane moves through these states (a loop "until every lane stands at a fetch" ran the whole ladder
    // three times per round: the kernel was bound by its instructions, 15 us per round of the wave at five waves per SIMD).  A lane
    // that ends a search without a fetch (a stop codon among the key's codes, a string that is used up) gets a second pass through
    // the front part; what is still not at a fetch after that sits this round out.
#pragma unroll 1
    for (int rep = 0; rep < 2; ++rep) {
      if (rep && __ballot(st == PS_END) == 0ull) break;
      if (st == PS_END) {                                      // the search is over with (sp, ep, l, pad)
        if ((int32_t)l >= v.min_hit_len && sp <= ep) {
          cfr_hit h;
          h.sp = sp; h.ep = ep; h.l = (int32_t)l; h.strand = 0; h.offset = k - remaining; h.pad = pad;
          out[cnt++] = h;
        }
        remaining -= (int32_t)l + 1;
        st = PS_BEGIN;
      }
      if (st == PS_BEGIN) {                                    // GetHitsFromRead's loop head (Classifier.hpp:274-293)
        if (remaining < v.min_hit_len) {
          chain_cnt[chain] = cnt;
          if (tile_ctr) { want_chain = true; st = PS_DONE; }                  // (its next chain: below, with the wave's other takers)
          else {
            st = nchains - chain > stride ? (uint32_t)PS_NEW : (uint32_t)PS_DONE;
            chain += stride;
          }
        } else { m = (uint32_t)remaining; s0 = (uint32_t)(k - remaining); l = 0; pad = 0; no_text = false; st = PS_FTKEY; }
      }
      if (st == PS_FTKEY) {                                    // the start of prot_search_full: which table entry
        if (!win_ok(s0, 12u)) { wreq = s0 & ~3u; ret = PS_FTKEY; st = PS_CODES; }
        else {
          uint64_t a; uint32_t b;
          codes12(s0, a, b);
          auto cd = [&](uint32_t i) -> uint32_t { return i < 8u ? (uint32_t)(a >> (8u * i)) & 0xffu : (b >> (8u * (i - 8u))) & 0xffu; };
          bool started = false;
          if (v.ftabx && m >= K) {
            uint64_t key = 0;
            bool ok = true;
            for (uint32_t i = 0; i < K; ++i) { const uint32_t c = cd(i); ok = ok && c < sigma; key = key * sigma + (c < sigma ? c : 0u); }
            if (ok) { fptr = v.ftabx + 2 * key; ftdisk = 0; st = PS_FT; started = true; }
          }
          if (!started) {                                      // on-disk ftab (FMIndex.hpp:388-422)
            if (m < wd) { sp = 0; ep = 0; l = 0; st = PS_END; }
            else if (wd > 0) {
              uint64_t key = 0;
              uint32_t bad = wd;
              for (uint32_t i = 0; i < wd; ++i) { const uint32_t c = cd(i); if (c > 31u && bad == wd) bad = i; key = (key << v.prot.bits) | (c & 31u); }
              if (bad < wd) { sp = 1; ep = 0; l = bad; st = PS_END; }
              else { fptr = v.ftab + 2 * key; ftdisk = 1; st = PS_FT; }
            } else { sp = 0; ep = v.n - 1; l = 0; st = PS_DECIDE; }
          }
        }
      }
    }
    if (st == PS_TXTPRE) {                                     // the head of a text round
      if (R == 1 && tp[0] == 0) { sp = ep = v.first_isa; no_text = true; st = PS_DECIDE; }   // single row at text position 0: back to the BWT
      else if (!win_ok(s0 + l, 12u)) { wreq = (s0 + l) & ~3u; ret = PS_TXTPRE; st = PS_CODES; }
      else st = PS_TXT;
    }
    if (st == PS_DECIDE) {                                     // the head of prot_search_full's loop
      if (l >= m) st = PS_END;
      else if (text_ok && !no_text && l >= v.text_min_l && m - l <= kVirtDeltaMax && ep - sp < 4 && !(sp == ep && sp == v.first_isa)) st = PS_SA;
      else if (!win_ok(s0 + l, 1u)) { wreq = (s0 + l) & ~3u; ret = PS_DECIDE; st = PS_CODES; }
      else {
        ce = code_at(s0 + l);
        st = ce > 31u ? (uint32_t)PS_END : (uint32_t)PS_EXT;
      }
    }
    if (tile_ctr) {                                                           // every lane of the wave is here: the tile's bookkeeping stays in step
      const uint64_t need = __ballot(want_chain);
      if (need) {
        const uint32_t lane = (uint32_t)__lane_id();
        const uint32_t kk = (uint32_t)__popcll(need), r = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
        const uint32_t avail = wt_end - wt_next;
        uint32_t mine;
        if (kk > avail) {
          const int leader = __ffsll((long long)need) - 1;
          unsigned long long base = 0;
          if ((int)lane == leader) base = atomicAdd(tile_ctr, (unsigned long long)tile);
          const uint32_t b32 = (uint32_t)__shfl((int)(uint32_t)base, leader);
          mine = r < avail ? wt_next + r : b32 + (r - avail);
          wt_next = b32 + (kk - avail);
          wt_end = b32 + tile;
        } else {
          mine = wt_next + r;
          wt_next += kk;
        }
        if (want_chain) {
          const uint64_t c64 = (uint64_t)stride + (uint64_t)mine;
          chain = c64 < (uint64_t)nchains ? (uint32_t)c64 : nchains;
          st = c64 < (uint64_t)nchains ? (uint32_t)PS_NEW : (uint32_t)PS_DONE;
          want_chain = false;
        }
      }
    }
    if (__ballot(st != PS_DONE) == 0ull) break;

    // ================================================================ (B) the fetches of this round
    uint32_t en = 0;
    const uint8_t *p0 = nullptr, *p1 = nullptr, *p2 = nullptr, *p3 = nullptr, *r0 = nullptr, *r1 = nullptr, *r2 = nullptr, *r3 = nullptr, *c0p = nullptr, *c1p = nullptr;
    if (st == PS_NEW) {
      const uint32_t ri = chain / CH, mate = (chain % CH) / 6u;
      p0 = reinterpret_cast<const uint8_t *>((mate ? offs2 : offs1) + ri);
      r0 = reinterpret_cast<const uint8_t *>(hit_off + ri);
      en = 0x11u;
      if (mate) { p1 = reinterpret_cast<const uint8_t *>(offs1 + ri); en |= 0x2u; }
    } else if (st == PS_CODES) {
      p0 = cb + cbase + wreq; p1 = p0 + 16; p2 = p0 + 32; p3 = p0 + 48;
      en = 0xfu;
    } else if (st == PS_FT) {
      p0 = reinterpret_cast<const uint8_t *>(fptr);
      en = 0x1u;
    } else if (st == PS_SA) {
      p0 = reinterpret_cast<const uint8_t *>(v.sa32 + sp);     // (256 zero bytes follow the array)
      en = 0x1u;
    } else if (st == PS_EXT) {
      const uint8_t *rs = reinterpret_cast<const uint8_t *>(v.prot.rec + (sp >> 6) * 16);
      p0 = rs + 88; p1 = rs + 104; r0 = rs + 120; c0p = rs + 4u * ce;
      en = 0x113u;
      if (sp != ep) {
        const uint8_t *re = reinterpret_cast<const uint8_t *>(v.prot.rec + ((ep + 1) >> 6) * 16);
        p2 = re + 88; p3 = re + 104; r1 = re + 120; c1p = re + 4u * ce;
        en |= 0x22cu;
      }
    } else if (st == PS_TXT) {
      // text bytes left of position tp[k]: T[tp - 8 .. tp - 1]  (16 zero bytes lie in front of the text)
      if (0 < R && tp[0]) { r0 = v.text8 + tp[0] - 8; en |= 0x10u; }
      if (1 < R && tp[1]) { r1 = v.text8 + tp[1] - 8; en |= 0x20u; }
      if (2 < R && tp[2]) { r2 = v.text8 + tp[2] - 8; en |= 0x40u; }
      if (3 < R && tp[3]) { r3 = v.text8 + tp[3] - 8; en |= 0x80u; }
    }
    Q16 q0 = {0, 0, 0, 0}, q1 = {0, 0, 0, 0}, q2 = {0, 0, 0, 0}, q3 = {0, 0, 0, 0};
    uint64_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    uint32_t c0 = 0, c1 = 0;
    if (en & 0x1u) q0 = *reinterpret_cast<const Q16a4 *>(p0);
    if (en & 0x2u) q1 = *reinterpret_cast<const Q16a4 *>(p1);
    if (en & 0x4u) q2 = *reinterpret_cast<const Q16a4 *>(p2);
    if (en & 0x8u) q3 = *reinterpret_cast<const Q16a4 *>(p3);
    if (en & 0x10u) d0 = reinterpret_cast<const U64a1 *>(r0)->x;
    if (en & 0x20u) d1 = reinterpret_cast<const U64a1 *>(r1)->x;
    if (en & 0x40u) d2 = reinterpret_cast<const U64a1 *>(r2)->x;
    if (en & 0x80u) d3 = reinterpret_cast<const U64a1 *>(r3)->x;
    if (en & 0x100u) c0 = *reinterpret_cast<const uint32_t *>(c0p);
    if (en & 0x200u) c1 = *reinterpret_cast<const uint32_t *>(c1p);
    // (every use of a fetched value stands behind these: without them the compiler moves a slot's first use - a byte swap, a
    //  decrement - up into the slot's block, and the wave waits there for that one fetch before it issues the next)
    asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3), "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3), "+v"(c0), "+v"(c1));
    auto u64of = [](uint32_t lo, uint32_t hi) -> uint64_t { return (uint64_t)lo | ((uint64_t)hi << 32); };

    // ================================================================ (C) what each lane does with its own
    if (st == PS_NEW) {
      const uint32_t ri = chain / CH, sub = chain % CH, mate = sub / 6u, rc = (sub / 3u) & 1u, frame = sub % 3u;
      const uint64_t o = u64of(q0.x, q0.y);
      const uint32_t len = (uint32_t)(u64of(q0.z, q0.w) - o);
      const uint32_t len1 = mate ? (uint32_t)(u64of(q1.z, q1.w) - u64of(q1.x, q1.y)) : len;
      k = (int32_t)len >= (int32_t)frame + 3 ? ((int32_t)len - (int32_t)frame) / 3 : 0;
      const uint32_t cap = prot_chain_cap(v, len);
      out = raw + d0 + (mate ? 6ull * prot_chain_cap(v, len1) : 0ull) + (uint64_t)(3u * rc + frame) * cap;
      cb = mate ? codes2 : codes1;
      cbase = prot_code_base(o, read0 + ri) + (uint64_t)(3u * rc + frame) * prot_code_stride(len);
      remaining = k;
      cnt = 0;
      if (k >= v.min_hit_len) { wreq = 0; ret = PS_BEGIN; st = PS_CODES; } else st = PS_BEGIN;
    } else if (st == PS_CODES) {
      s_win[(0u << 8) + t] = q0.x;  s_win[(1u << 8) + t] = q0.y;  s_win[(2u << 8) + t] = q0.z;  s_win[(3u << 8) + t] = q0.w;
      s_win[(4u << 8) + t] = q1.x;  s_win[(5u << 8) + t] = q1.y;  s_win[(6u << 8) + t] = q1.z;  s_win[(7u << 8) + t] = q1.w;
      s_win[(8u << 8) + t] = q2.x;  s_win[(9u << 8) + t] = q2.y;  s_win[(10u << 8) + t] = q2.z; s_win[(11u << 8) + t] = q2.w;
      s_win[(12u << 8) + t] = q3.x; s_win[(13u << 8) + t] = q3.y; s_win[(14u << 8) + t] = q3.z; s_win[(15u << 8) + t] = q3.w;
      wbase = wreq;
      st = ret;
    } else if (st == PS_FT) {
      const uint64_t ex = u64of(q0.x, q0.y), ey = u64of(q0.z, q0.w);
      if (!ftdisk) {
        l = (uint32_t)(ey & 0xffu);
        sp = ex;
        ep = ex + (ey >> 8) - 1;
        st = l < K ? (uint32_t)PS_END : (uint32_t)PS_DECIDE;
      } else if (ey == 0) { sp = 1; ep = 0; l = wd - 1; st = PS_END; }
      else { sp = ex; ep = ex + ey - 1; l = wd; st = PS_DECIDE; }
    } else if (st == PS_SA) {
      R = (uint32_t)(ep - sp) + 1u;
      mask = (1u << R) - 1u;
      tp[0] = q0.x; tp[1] = 1 < R ? q0.y : 0u; tp[2] = 2 < R ? q0.z : 0u; tp[3] = 3 < R ? q0.w : 0u;
      idx[0] = 0; idx[1] = 1; idx[2] = 2; idx[3] = 3;
      l0 = l;
      st = PS_TXTPRE;
    } else if (st == PS_EXT) {                                 // fm_extend on the 128-byte records (prot_rank, prot_access, fm_fix)
      const uint64_t ps[5] = {u64of(q0.x, q0.y), u64of(q0.z, q0.w), u64of(q1.x, q1.y), u64of(q1.z, q1.w), d0};
      const uint64_t ms = prot_match(ps, ce);
      const uint32_t rsb = (uint32_t)sp & 63u;
      const uint64_t Cc = s_C[ce];
      const uint64_t nsp = Cc + c0 + (rsb ? (uint64_t)__popcll(ms & ((1ull << rsb) - 1)) : 0ull) + fm_fix(v, ce, sp, 0);
      uint64_t nep;
      if (sp == ep) nep = nsp + (((ms >> rsb) & 1ull) ? 0ull : ~0ull);
      else {
        const uint64_t pe[5] = {u64of(q2.x, q2.y), u64of(q2.z, q2.w), u64of(q3.x, q3.y), u64of(q3.z, q3.w), d1};
        const uint32_t reb = (uint32_t)(ep + 1) & 63u;
        nep = Cc + c1 + (reb ? (uint64_t)__popcll(prot_match(pe, ce) & ((1ull << reb) - 1)) : 0ull) + fm_fix(v, ce, ep, 1) - 1;
      }
      if (nsp > nep || nep > v.n) st = PS_END;
      else { sp = nsp; ep = nep; ++l; st = PS_DECIDE; }
    } else if (st == PS_TXT) {                                 // one round of up to 8 characters on the text (prot_search_full)
      uint32_t Lc = m - l < 8u ? m - l : 8u;
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) if (q < R && tp[q] && tp[q] < Lc) Lc = tp[q];
      uint64_t rc8; uint32_t unused;
      codes12(s0 + l, rc8, unused);
      const uint64_t tx[4] = {d0, d1, d2, d3};
      uint32_t e[4] = {0, 0, 0, 0}, J = 0;
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) if (q < R && tp[q]) {
        const uint64_t x = __builtin_bswap64(tx[q]) ^ rc8;     // byte j = T[tp - 1 - j] against code l + j
        uint32_t eq = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
        if (eq > Lc) eq = Lc;
        e[q] = eq;
        if (eq > J) J = eq;
      }
      uint32_t cntR = 0, nmask = 0, ntp[4] = {0, 0, 0, 0}, nidx[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) if (q < R && e[q] >= J) {
#pragma unroll
        for (uint32_t z = 0; z < 4; ++z) if (z == cntR) { ntp[z] = tp[q] - J; nidx[z] = idx[q]; }
        nmask |= 1u << idx[q];
        ++cntR;
      }
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) { tp[q] = ntp[q]; idx[q] = nidx[q]; }
      R = cntR;
      mask = nmask;
      l += J;
      if (J < Lc || l >= m) {                                  // every row mismatched at character J, or the string is used up
        sp = kVirtRow | ((uint64_t)(l - l0) << kVirtDeltaShift) | sp;
        ep = sp + (R - 1u);
        pad = (int32_t)mask;
        st = PS_END;
      } else st = PS_TXTPRE;
    }
  }
}

// TranslatedSearch's choice of frame + the rest of SearchForwardAndReverse (:509-583) for a protein index.  The score that
// picks the frame is (number of hits) x (sum of the hits' scores): the loop at :489-493 adds the whole list once per hit.
template <int MATES>
__global__ void k_select_prot(DevView v, const uint64_t *offs1, const uint64_t *offs2, size_t n, const uint64_t *hit_off, const cfr_hit *raw,
                              const uint32_t *chain_cnt, cfr_hit *fin, uint64_t *fin_cnt, uint64_t *fin_rows, uint64_t *read_rows) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const cfr_hit *list[2][2];          // [mate][rc]
  int32_t cntl[2][2] = {{0, 0}, {0, 0}};
  uint64_t region = hit_off[i];
  for (int mate = 0; mate < MATES; ++mate) {
    const uint32_t len = mate ? (uint32_t)(offs2[i + 1] - offs2[i]) : (uint32_t)(offs1[i + 1] - offs1[i]);
    const uint32_t cap = prot_chain_cap(v, len);
    for (int rc = 0; rc < 2; ++rc) {
      uint64_t best = 0;
      int tag = 0;
      for (int f = 0; f < 3; ++f) {
        const cfr_hit *h = raw + region + (uint64_t)(3 * rc + f) * cap;
        const uint32_t c = chain_cnt[(6 * MATES) * i + 6 * (size_t)mate + 3 * (size_t)rc + (size_t)f];
        uint64_t sum = 0;
        for (uint32_t q = 0; q < c; ++q) sum += hit_score(v, h[q].l);
        const uint64_t score = sum * c;
        if (score > best) { best = score; tag = f; }
      }
      list[mate][rc] = raw + region + (uint64_t)(3 * rc + tag) * cap;
      cntl[mate][rc] = (int32_t)chain_cnt[(6 * MATES) * i + 6 * (size_t)mate + 3 * (size_t)rc + (size_t)tag];
    }
    region += 6ull * cap;
  }
  // strandHits[1] = r1 forward ++ r2 reverse ; strandHits[0] = r1 reverse ++ r2 forward (:551-552)
  const cfr_hit *F1 = list[0][0], *R1 = list[0][1], *F2 = MATES == 2 ? list[1][0] : nullptr, *R2 = MATES == 2 ? list[1][1] : nullptr;
  const int32_t nF1 = cntl[0][0], nR1 = cntl[0][1], nF2 = MATES == 2 ? cntl[1][0] : 0, nR2 = MATES == 2 ? cntl[1][1] : 0;
  uint64_t score_plus = 0, score_minus = 0;
  for (int32_t q = 0; q < nF1; ++q) score_plus += hit_score(v, F1[q].l);
  for (int32_t q = 0; q < nR2; ++q) score_plus += hit_score(v, R2[q].l);
  for (int32_t q = 0; q < nR1; ++q) score_minus += hit_score(v, R1[q].l);
  for (int32_t q = 0; q < nF2; ++q) score_minus += hit_score(v, F2[q].l);
  bool take_plus, take_minus;
  if (score_plus > score_minus + score_minus / 100) { take_plus = true; take_minus = false; }
  else if (score_minus > score_plus + score_plus / 100) { take_plus = false; take_minus = true; }
  else { take_plus = true; take_minus = true; }
  cfr_hit *out = fin + hit_off[i];
  uint64_t *rows = fin_rows + hit_off[i];
  uint64_t cnt = 0, row_total = 0;
  if (take_plus) { emit_hits(v, F1, nF1, 1, out, rows, cnt, row_total); emit_hits(v, R2, nR2, 1, out, rows, cnt, row_total); }
  if (take_minus) { emit_hits(v, R1, nR1, -1, out, rows, cnt, row_total); emit_hits(v, F2, nF2, -1, out, rows, cnt, row_total); }
  fin_cnt[i] = cnt;
  if (read_rows) read_rows[i] = row_total;
}

}  // namespace cfr

// =============================================================================== device tail
// Classifier::GetClassificationFromHits (Classifier.hpp:585-843) from the located sequence ids on,
// plus Taxonomy::SeqIdToTaxId / GetOrigTaxId / LCA / ReduceTaxIds (Taxonomy.hpp:718-724, 633-639, 733-836,
// 839-973).  One lane per read; the typical read has ~2 hits and ~3 located rows, so this is a short
// scalar program per lane.  Per-read scratch: `entries` (one slot per located row of the read) and the
// read's own slice of row_vals, which is free once the ids have been folded into `entries`.
namespace cfr {

__device__ __forceinline__ uint64_t d_seq_to_tax(const DevView &v, uint64_t seq_id) { return seq_id < v.seq_cnt ? v.seq_to_tax[seq_id] : v.node_cnt; }
__device__ __forceinline__ uint64_t d_orig_taxid(const DevView &v, uint64_t ctid) { return v.tax_orig[ctid >= v.node_cnt ? v.tax_root : ctid]; }

__device__ __forceinline__ void sort_u64(uint64_t *a, uint64_t m) {   // small arrays: insertion sort
  for (uint64_t i = 1; i < m; ++i) {
    const uint64_t x = a[i];
    uint64_t j = i;
    while (j > 0 && a[j - 1] > x) { a[j] = a[j - 1]; --j; }
    a[j] = x;
  }
}
__device__ __forceinline__ uint64_t unique_u64(uint64_t *a, uint64_t m) {
  if (m == 0) return 0;
  uint64_t w = 1;
  for (uint64_t i = 1; i < m; ++i) if (a[i] != a[w - 1]) a[w++] = a[i];
  return w;
}

// lowest common ancestor of the ids, in their order (root if all are root): same value as Taxonomy::LCA
__device__ __forceinline__ uint64_t d_tax_lca(const DevView &v, const uint64_t *ids, uint64_t cnt) {
  TaxFold F = tax_fold_begin(v.tax_root);              // (cfr_tax_fold.hpp: the rules on a forest; tax_depth is tabulated at load time)
  for (uint64_t i = 0; i < cnt; ++i) tax_fold_add(v.tax_parent, v.tax_depth, v.tax_root, F, ids[i]);
  return tax_fold_result(F, v.tax_root);
}

// the node the reference's walk files under rank level L for input id (or ~0 if none)
__device__ __forceinline__ uint64_t d_node_at_level(const DevView &v, uint64_t id, uint32_t L) {
  if (L == 0) return id;
  const uint32_t unk = v.rank_num[0];
  uint64_t x = id;
  uint32_t prev = 0;
  do {
    const uint32_t rn = v.rank_num[v.tax_rank[x]];
    if (rn != unk && rn > prev) {
      if (L <= rn) return x;                       // levels prev+1 .. rn all receive x
      prev = rn;
    }
    x = v.tax_parent[x];
  } while (x != v.tax_parent[x]);
  return ~0ull;
}

// Taxonomy::ReduceTaxIds: ids (cnt > k) -> out (<= max(k,1) entries, ascending); returns count. tmp: cnt slots.
// level_out: the rank level whose set was taken (0 when the ids were not reduced by levels, or came back as the root).
__device__ __forceinline__ uint32_t d_tax_reduce(const DevView &v, const uint64_t *ids, uint64_t cnt, int32_t k, uint64_t *tmp, uint64_t *out,
                                                 uint32_t *level_out = nullptr) {
  if (level_out) *level_out = 0;
  for (uint64_t i = 0; i < cnt; ++i) if (ids[i] >= v.node_cnt) { out[0] = v.node_cnt; return 1; }
  if (k == 1) { out[0] = d_tax_lca(v, ids, cnt); return 1; }
  const uint32_t unk = v.rank_num[0];
  for (uint32_t L = 0; L < unk; ++L) {
    uint64_t m = 0;
    for (uint64_t i = 0; i < cnt; ++i) {
      const uint64_t x = d_node_at_level(v, ids[i], L);
      if (x != ~0ull) tmp[m++] = x;
    }
    sort_u64(tmp, m);
    m = unique_u64(tmp, m);
    if ((int64_t)m <= (int64_t)k) {
      if (m == 0) { out[0] = v.tax_root; return 1; }
      for (uint64_t i = 0; i < m; ++i) out[i] = tmp[i];
      if (level_out) *level_out = L;
      return (uint32_t)m;
    }
  }
  out[0] = v.tax_root;
  return 1;
}

// ---- --expand-taxid (_classifierParam.outputExpandedResult, Classifier.hpp:22, 792-838): which ids ReduceTaxIds / LCA promoted into
// every reported id (promotedChildTaxIds, Taxonomy.hpp:839-973; lcaChildTaxIds, :733-836).  The lists leave through a pool of the image:
// a record is [global match slot, count, count ORIGINAL tax ids] (GetOrigTaxId, Classifier.hpp:833), appended with one atomicAdd; a
// match slot without a record has the empty string.  When the pool is too small the cursor still counts and the host repeats the call
// with a larger one.  `as_is`: the ids in input order (the out-of-tree branch); otherwise ascending and unique (std::map order).
__device__ __forceinline__ void exp_append(const DevView &v, uint64_t slot, uint64_t *ids, uint64_t cnt, bool as_is) {
  if (!as_is) { sort_u64(ids, cnt); cnt = unique_u64(ids, cnt); }
  if (cnt == 0) return;
  const uint64_t at = (uint64_t)atomicAdd(v.exp_cursor, (unsigned long long)(cnt + 2));
  if (at + cnt + 2 > v.exp_cap) return;
  v.exp_pool[at] = slot;
  v.exp_pool[at + 1] = cnt;
  for (uint64_t j = 0; j < cnt; ++j) v.exp_pool[at + 2 + j] = d_orig_taxid(v, ids[j]);
}

// ids[0..cnt): the compact tax ids that went into d_tax_reduce (cnt > k), promoted[0..nm) / level: what came out; tmp: cnt slots.
__device__ __forceinline__ void d_tax_expand(const DevView &v, uint64_t *ids, uint64_t cnt, int32_t k, const uint64_t *promoted, uint32_t nm,
                                             uint32_t level, uint64_t *tmp, uint64_t slot0) {
  for (uint64_t i = 0; i < cnt; ++i) if (ids[i] >= v.node_cnt) { exp_append(v, slot0, ids, cnt, true); return; }   // Taxonomy.hpp:866-872: every input id
  if (k == 1) {
    // lcaChildTaxIds: backboneChildTaxIds[j] of the LCA's place j on the backbone = the backbone's own node below it (:776) and, for
    // every other id, the node at which its path leaves the backbone when that happens right below the LCA (:812-813) - i.e. the child
    // of the LCA on the way to every non-root id that is not the LCA itself (ids that part further down share the backbone's child)
    const uint64_t lca = promoted[0];
    uint64_t m = 0;
    // a second top as the backbone (the first id that is not the root, cfr_tax_fold.hpp) is the backbone's own node below the root (:770)
    for (uint64_t i = 0; i < cnt; ++i) {
      if (ids[i] == v.tax_root) continue;
      if (ids[i] == v.tax_parent[ids[i]] && ids[i] != lca) tmp[m++] = ids[i];
      break;
    }
    for (uint64_t i = 0; i < cnt; ++i) {
      uint64_t x = ids[i];
      if (x == v.tax_parent[x] || x == lca) continue;            // a root id takes no part (:787-791); the LCA itself leaves nothing (iTmp < 0)
      for (;;) {
        const uint64_t p = v.tax_parent[x];
        if (p == lca || p == v.tax_parent[p]) break;
        x = p;
      }
      tmp[m++] = x;
    }
    exp_append(v, slot0, tmp, m, false);
    return;
  }
  if (level == 0) return;                                        // :939: only a set above the base level has children
  for (uint32_t q = 0; q < nm; ++q) {
    uint64_t m = 0;
    for (uint64_t i = 0; i < cnt; ++i) {
      const uint64_t t = d_node_at_level(v, ids[i], level - 1);  // the members of taxIdsInRankNum[ri - 1]
      if (t == ~0ull) continue;
      uint64_t x = t, owner = ~0ull;
      while (x != v.tax_parent[x]) {                             // :954-970: the first node above t filed at exactly this level
        x = v.tax_parent[x];
        const uint32_t rn = v.rank_num[v.tax_rank[x]];
        if (rn > level) break;
        if (rn == level) { owner = x; break; }
      }
      if (owner == promoted[q]) tmp[m++] = t;
    }
    exp_append(v, slot0 + q, tmp, m, false);
  }
}

// FUSED (locate memo at every row): the kernel reads the per-read regions k_adjust_select wrote (hit_begin = hit_off,
// fin_cnt = hits per read, row_off = per-READ row base), enumerates each hit's rows itself and takes their values from
// loc_memo - no compaction, no row arrays, no locate launch.  Otherwise: dense hits + per-hit row offsets + located values.
// The 19-comparator sorting network for 8 keys (checked exhaustively by the zero-one principle in tests/test_host_cpu.py).
#define CFR_NET8(CE) CE(0,1) CE(2,3) CE(4,5) CE(6,7) CE(0,2) CE(1,3) CE(4,6) CE(5,7) CE(1,2) CE(5,6) CE(0,4) CE(3,7) \
                     CE(1,5) CE(2,6) CE(1,4) CE(3,6) CE(2,4) CE(3,5) CE(3,4)

// Register form of the per-read fold below for the common small read: every hit locates <= 8 rows (all of its range)
// and the read ends with <= 8 (strand, seqId) entries.  Same arithmetic, same order; returns false (nothing written)
// when the read does not fit, and the caller runs the general form.  On success: best ids in bid[0..nb), R fields set.
struct TailFold { uint64_t best, second, best_len, second_len; };

template <class HitAt>
__device__ __forceinline__ bool tail_fold_small(const DevView &v, const HitAt &hit_at, uint64_t nh, bool mix,
                                                TailFold &F, uint64_t (&skey)[8], uint64_t (&ssc)[8], uint32_t &ne_out) {
  uint64_t key[8], sc[8];          // key = strand list << 32 | seqId ; ~0 = free slot
  int32_t ln[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { key[e] = ~0ull; sc[e] = 0; ln[e] = 0; }
  uint32_t ne = 0;
  uint64_t prev_id = 0, prev_score = 0;
  int32_t prev_len = 0;
  cfr_hit P;                        // the previous hit
  P.sp = 0; P.ep = 1; P.l = 0; P.strand = 0; P.offset = 0; P.pad = 0;
  for (uint64_t h = 0; h < nh; ++h) {
    const cfr_hit H = hit_at(h);
    if (H.l < v.min_hit_len) { P = H; continue; }
    const uint64_t range = H.ep - H.sp + 1;
    if (range > 8 || !(range <= v.max_entries || v.locate_all)) return false;
    uint64_t x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = (uint64_t)q < range ? locate_row(v, H, H.sp + q) : ~0ull;
#define CFR_CE(i, j) { const uint64_t lo_ = x[i] < x[j] ? x[i] : x[j], hi_ = x[i] < x[j] ? x[j] : x[i]; x[i] = lo_; x[j] = hi_; }
    CFR_NET8(CFR_CE)
#undef CFR_CE
    const uint64_t score = hit_score(v, H.l);
    const uint64_t kk = (uint64_t)((H.strand + 1) / 2);
    bool adjacent = false;
    if (!mix && h > 0 && H.ep == H.sp) adjacent = P.ep == P.sp && P.strand == H.strand && P.offset + P.l + 1 == H.offset;
    bool overflow = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint64_t id = x[q];
      const bool live = id != ~0ull && (q == 0 || id != x[q > 0 ? q - 1 : 0]);      // sorted: duplicates are neighbours
      if (live) {
        const uint64_t want = (kk << 32) | id;
        uint32_t idx = ne;
#pragma unroll
        for (int e = 0; e < 8; ++e) if (key[e] == want) idx = (uint32_t)e;
        const bool created = idx == ne;
        if (created && ne == 8) overflow = true;
        else {
          uint64_t s_old = 0;
          int32_t l_old = 0;
#pragma unroll
          for (int e = 0; e < 8; ++e) if ((uint32_t)e == idx) { s_old = sc[e]; l_old = ln[e]; }
          uint64_t s_new;
          int32_t l_new;
          if (adjacent && id == prev_id) {             // merge adjacent unique hits (Classifier.hpp:673-685)
            prev_len += H.l;
            const uint64_t merged = hit_score(v, prev_len);
            s_new = s_old - prev_score + merged;
            prev_score = merged;
            l_new = l_old + H.l;
          } else {
            s_new = created ? score : s_old + score;
            l_new = created ? H.l : l_old + H.l;
            if (H.ep == H.sp) { prev_id = id; prev_score = score; prev_len = H.l; }
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) if ((uint32_t)e == idx) { key[e] = want; sc[e] = s_new; ln[e] = l_new; }
          if (created) ++ne;
        }
      }
    }
    if (overflow) return false;
    P = H;
  }
  // std::map iteration order: strand list 0 then 1, ascending seqId = ascending key
#define CFR_CE(i, j) { const bool sw_ = key[i] > key[j]; \
    const uint64_t k_ = key[i], s_ = sc[i]; const int32_t l_ = ln[i]; \
    key[i] = sw_ ? key[j] : k_; sc[i] = sw_ ? sc[j] : s_; ln[i] = sw_ ? ln[j] : l_; \
    key[j] = sw_ ? k_ : key[j]; sc[j] = sw_ ? s_ : sc[j]; ln[j] = sw_ ? l_ : ln[j]; }
  CFR_NET8(CFR_CE)
#undef CFR_CE
  uint64_t best = 0, second = 0, best_len = 0, second_len = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) if ((uint32_t)e < ne) {
    if (sc[e] > best) { second = best; second_len = best_len; best = sc[e]; best_len = (uint64_t)(int64_t)ln[e]; }
    else if (sc[e] > second) { second = sc[e]; second_len = (uint64_t)(int64_t)ln[e]; }
  }
  F.best = best; F.second = second; F.best_len = best_len; F.second_len = second_len;
#pragma unroll
  for (int e = 0; e < 8; ++e) { skey[e] = key[e]; ssc[e] = sc[e]; }
  ne_out = ne;
  return true;
}

// The best ids of a small fold (registers) in map order, unique across the strand lists -> bid[0..nb); returns R.secondary_score
__device__ __forceinline__ uint64_t tail_small_ids(const DevView &v, const TailFold &F, const uint64_t (&skey)[8], const uint64_t (&ssc)[8],
                                                   uint32_t sne, uint64_t (&bid)[8], uint32_t &nb_out) {
  const bool take_second = F.second_len >= v.secondary_hit_len && F.second < F.best && F.second >= (uint64_t)(v.secondary_factor * (double)F.best);
  uint32_t nbr = 0, nb_best = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const uint64_t target = pass == 0 ? F.best : F.second;
    if (pass == 0 || take_second) {
#pragma unroll
      for (int e = 0; e < 8; ++e) if ((uint32_t)e < sne && ssc[e] == target) {
        const uint64_t id = skey[e] & 0xffffffffull;
        bool seen = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) if ((uint32_t)q < nbr && bid[q] == id) seen = true;
        if (!seen) {
#pragma unroll
          for (int q = 0; q < 8; ++q) if ((uint32_t)q == nbr) bid[q] = id;
          ++nbr;
        }
      }
    }
    if (pass == 0) nb_best = nbr;      // ids with the best score: what the general form's "nb > 1" test sees
  }
  nb_out = nbr;
  return take_second ? F.second : (nb_best > 1 ? F.best : F.second);
}

// General form of the per-read fold: entries in global scratch E (one slot per located row of the read), the ids of a
// hit in a scratch slice that is sorted in place.  MEMO: the kernel enumerates the rows of a hit itself (the sequence of
// Classifier.hpp:625-665, same as k_enum_rows) and answers each from the locate memo, slices taken from vals_base on;
// otherwise the located values are already in row_vals at row_off_h[h].  Leaves the best ids in best_ids[0..nb).
template <bool MEMO, class HitAt>
__device__ __forceinline__ void tail_fold_general(const DevView &v, const HitAt &hit_at, uint64_t nh, bool mix, uint64_t *vals_base,
                                                  uint64_t *row_vals, const uint64_t *row_off_h, TailEntry *E, uint64_t *best_ids,
                                                  TailFold &F, uint64_t &nb, uint64_t &sec_out) {
  uint64_t fused_off = 0;              // MEMO: where the next hit's row values go
  uint64_t ne = 0;
  uint64_t prev_id = 0, prev_score = 0;
  int32_t prev_len = 0;
  for (uint64_t h = 0; h < nh; ++h) {
    const cfr_hit H = hit_at(h);
    if (H.l < v.min_hit_len) continue;
    const uint64_t score = hit_score(v, H.l);
    const int32_t k = (H.strand + 1) / 2;
    uint64_t *vals;
    uint64_t m;
    if (MEMO) {
      vals = vals_base + fused_off;
      m = hit_row_count(v, H);
      fused_off += m;
      const uint64_t range = H.ep - H.sp + 1;
      if (range <= v.max_entries || v.locate_all) {
        for (uint64_t q = 0; q < range; ++q) vals[q] = locate_row(v, H, H.sp + q);
      } else {
        const uint64_t step = (range + v.max_entries - 1) / v.max_entries;
        uint64_t kq = 0;
        for (uint64_t j = H.sp; j <= H.ep; j += step) vals[kq++] = locate_row(v, H, j);
        uint64_t resolved = kq;
        for (uint64_t j = H.ep; j >= H.sp && j <= H.ep; j -= step) {
          vals[kq++] = locate_row(v, H, j);
          ++resolved;
          if (resolved >= v.max_entries) break;
        }
      }
    } else {
      vals = row_vals + row_off_h[h];
      m = row_off_h[h + 1] - row_off_h[h];
    }
    sort_u64(vals, m);
    m = unique_u64(vals, m);
    bool adjacent = false;
    if (!mix && h > 0 && H.ep == H.sp) {
      const cfr_hit P = hit_at(h - 1);
      adjacent = P.ep == P.sp && P.strand == H.strand && P.offset + P.l + 1 == H.offset;
    }
    for (uint64_t q = 0; q < m; ++q) {
      const uint64_t id = vals[q];
      uint64_t e = 0;
      while (e < ne && !(E[e].k == k && E[e].seq_id == id)) ++e;
      const bool created = e == ne;
      if (created) { E[ne].seq_id = id; E[ne].score = 0; E[ne].hit_length = 0; E[ne].k = k; ++ne; }
      if (adjacent && id == prev_id) {             // merge adjacent unique hits (Classifier.hpp:673-685)
        E[e].score -= prev_score;
        prev_len += H.l;
        prev_score = hit_score(v, prev_len);
        E[e].score += prev_score;
        E[e].hit_length += H.l;
      } else {
        if (created) { E[e].score = score; E[e].hit_length = H.l; }
        else { E[e].score += score; E[e].hit_length += H.l; }
        if (H.ep == H.sp) { prev_id = id; prev_score = score; prev_len = H.l; }
      }
    }
  }
  // std::map iteration order: strand list 0 then 1, ascending seqId
  for (uint64_t a = 1; a < ne; ++a) {
    const TailEntry x = E[a];
    uint64_t b = a;
    while (b > 0 && (E[b - 1].k > x.k || (E[b - 1].k == x.k && E[b - 1].seq_id > x.seq_id))) { E[b] = E[b - 1]; --b; }
    E[b] = x;
  }
  uint64_t best = 0, second = 0, best_len = 0, second_len = 0;
  for (uint64_t e = 0; e < ne; ++e) {
    if (E[e].score > best) { second = best; second_len = best_len; best = E[e].score; best_len = (uint64_t)(int64_t)E[e].hit_length; }
    else if (E[e].score > second) { second = E[e].score; second_len = (uint64_t)(int64_t)E[e].hit_length; }
  }
  F.best = best; F.second = second; F.best_len = best_len; F.second_len = second_len;
  // best sequence ids, in map order, unique across the two strand maps (the ids live in E; best_ids may alias the value slices)
  nb = 0;
  auto push_unique = [&](uint64_t id) {
    for (uint64_t q = 0; q < nb; ++q) if (best_ids[q] == id) return;
    best_ids[nb++] = id;
  };
  for (uint64_t e = 0; e < ne; ++e) if (E[e].score == best) push_unique(E[e].seq_id);
  sec_out = nb > 1 ? best : second;
  if (second_len >= v.secondary_hit_len && second < best && second >= (uint64_t)(v.secondary_factor * (double)best)) {
    for (uint64_t e = 0; e < ne; ++e) if (E[e].score == second) push_unique(E[e].seq_id);
    sec_out = second;
  }
}

// Hash form of the general fold (one-launch post stage, max_result > 0): the per-read score table is an open-addressing
// table of (strand list, seqId) in pool scratch, so a hit with m rows costs O(m) accesses instead of a sort plus an
// O(m x entries) scan.  What the reference's ordered maps decide is recovered without sorting:
//  * a row's id counts once per hit (the reference sorts + uniques the ids of a hit): tag = last hit that touched the entry;
//  * best / second / their hit lengths as the sequential scan over (strand list, seqId) order leaves them
//    (Classifier.hpp:710-736): best_len belongs to the smallest key with the best score; with two or more entries at the
//    best score second = best and its length is that of the second smallest such key; otherwise second is the largest
//    lower score and its length that of the smallest key holding it;
//  * an id is reported once, by its first entry in (class, strand list) order, class 1 = best score, class 2 = second
//    score when the secondary rule takes it (Classifier.hpp:738-781); the order of the ids only matters when they are
//    listed (nb <= max_result, at most 64 of them, sorted here) - ReduceTaxIds works on the set.
struct HashSlot { uint64_t key, score; int32_t hit_length, tag; };   // key = strand list << 63 | seqId ; ~0 = empty

template <class HitAt>
__device__ __forceinline__ void tail_fold_hash(const DevView &v, const HitAt &hit_at, uint64_t nh, bool mix, HashSlot *tab, uint32_t logc,
                                               uint64_t *ids_out, uint64_t *used, TailFold &F, uint64_t &nb, uint64_t &sec_out) {
  const uint64_t C = 1ull << logc, mask = C - 1;
  const uint64_t EMPTY = ~0ull;
  for (uint64_t s = 0; s < C; ++s) tab[s].key = EMPTY;
  auto slot_of = [&](uint64_t key) {                 // slot holding key, or the empty slot where it would go
    uint64_t s = (key * 0x9E3779B97F4A7C15ull) >> (64 - logc);
    for (;;) {
      const uint64_t kx = tab[s].key;
      if (kx == key || kx == EMPTY) return s;
      s = (s + 1) & mask;
    }
  };
  uint64_t ne = 0;                                    // occupied slots, in creation order: used[0..ne)
  uint64_t best = 0;                                  // scores only grow, so the running maximum is the final one
  uint64_t prev_id = 0, prev_score = 0;
  int32_t prev_len = 0;
  for (uint64_t h = 0; h < nh; ++h) {
    const cfr_hit H = hit_at(h);
    if (H.l < v.min_hit_len) continue;
    const uint64_t score = hit_score(v, H.l);
    const uint64_t kbit = (uint64_t)((H.strand + 1) / 2) << 63;
    bool adjacent = false;
    if (!mix && h > 0 && H.ep == H.sp) {
      const cfr_hit P = hit_at(h - 1);
      adjacent = P.ep == P.sp && P.strand == H.strand && P.offset + P.l + 1 == H.offset;
    }
    const int32_t tag = (int32_t)h + 1;
    auto add_row = [&](uint64_t row) {
      const uint64_t id = locate_row(v, H, row);
      const uint64_t s = slot_of(kbit | id);
      HashSlot e = tab[s];
      if (e.key == EMPTY) { e.key = kbit | id; e.score = 0; e.hit_length = 0; e.tag = 0; used[ne++] = s; }
      if (e.tag == tag) return;                      // this hit has counted the id already
      e.tag = tag;
      if (adjacent && id == prev_id) {               // merge adjacent unique hits (Classifier.hpp:673-685)
        e.score -= prev_score;
        prev_len += H.l;
        prev_score = hit_score(v, prev_len);
        e.score += prev_score;
        e.hit_length += H.l;
      } else {
        e.score += score;
        e.hit_length += H.l;
        if (H.ep == H.sp) { prev_id = id; prev_score = score; prev_len = H.l; }
      }
      if (e.score > best) best = e.score;
      tab[s] = e;
    };
    // the row sequence of Classifier.hpp:625-665 (same as k_enum_rows)
    const uint64_t range = H.ep - H.sp + 1;
    if (range <= v.max_entries || v.locate_all) {
      for (uint64_t q = 0; q < range; ++q) add_row(H.sp + q);
    } else {
      const uint64_t step = (range + v.max_entries - 1) / v.max_entries;
      uint64_t resolved = 0;
      for (uint64_t j = H.sp; j <= H.ep; j += step) { add_row(j); ++resolved; }
      for (uint64_t j = H.ep; j >= H.sp && j <= H.ep; j -= step) {
        add_row(j);
        ++resolved;
        if (resolved >= v.max_entries) break;
      }
    }
  }
  // ---- second and the lengths that go with best / second: one pass over the occupied slots
  uint64_t k1 = EMPTY, k2 = EMPTY, len1 = 0, len2 = 0;     // the two smallest keys at the best score
  uint64_t v2 = 0, kq = EMPTY, lenq = 0;                   // the largest lower score and its smallest key
  for (uint64_t q = 0; q < ne; ++q) {
    const HashSlot e = tab[used[q]];
    if (e.score == 0) continue;                            // (a zero score never enters best/second: both tests are strict)
    const uint64_t l = (uint64_t)(int64_t)e.hit_length;
    if (e.score == best) {
      if (e.key < k1) { k2 = k1; len2 = len1; k1 = e.key; len1 = l; }
      else if (e.key < k2) { k2 = e.key; len2 = l; }
    } else if (e.score > v2 || (e.score == v2 && e.key < kq)) { v2 = e.score; kq = e.key; lenq = l; }
  }
  uint64_t second, second_len;
  if (best == 0) { second = 0; second_len = 0; len1 = 0; }
  else if (k2 != EMPTY) { second = best; second_len = len2; }
  else { second = v2; second_len = v2 ? lenq : 0; }
  F.best = best; F.second = second; F.best_len = len1; F.second_len = second_len;
  const bool take_second = second_len >= v.secondary_hit_len && second < best && second >= (uint64_t)(v.secondary_factor * (double)best);
  // ---- the ids to report: every id once, by its first entry in (class, strand list) order
  auto cls = [&](uint64_t sc) -> uint32_t { return sc == best ? 1u : (take_second && sc == second ? 2u : 0u); };   // (a best score of 0 reports every entry, like the reference)
  nb = 0;
  uint64_t nb_best = 0;
  for (uint64_t q = 0; q < ne; ++q) {
    const HashSlot e = tab[used[q]];
    const uint32_t c = cls(e.score);
    if (!c) continue;
    const HashSlot o = tab[slot_of(e.key ^ (1ull << 63))];                // the same id in the other strand list, if any
    if (o.key != EMPTY) {
      const uint32_t cs = cls(o.score);
      if (cs && (cs < c || (cs == c && o.key < e.key))) continue;          // that list reports the id first
    }
    ids_out[nb++] = e.key;                 // (the class is recovered from the score when the list must be ordered)
    if (c == 1) ++nb_best;
  }
  sec_out = take_second ? second : (nb_best > 1 ? best : second);
  if ((int64_t)nb <= (int64_t)v.max_result || v.exp_pool) {
    // listed as they are: order by (class, strand list, id); nb <= 64.  (--expand-taxid: the order also shows when the ids are
    // reduced - an id outside the tree hands the input back as it came, Taxonomy.hpp:866-872.)
    for (uint64_t a = 1; a < nb; ++a) {
      const uint64_t x = ids_out[a];
      const uint32_t cx = cls(tab[slot_of(x)].score);
      uint64_t b = a;
      while (b > 0) {
        const uint64_t y = ids_out[b - 1];
        const uint32_t cy = cls(tab[slot_of(y)].score);
        if (cy < cx || (cy == cx && y < x)) break;
        ids_out[b] = y;
        --b;
      }
      ids_out[b] = x;
    }
  }
  for (uint64_t q = 0; q < nb; ++q) ids_out[q] &= ~(1ull << 63);           // plain sequence ids
}

// Names / tax ids of the result (Classifier.hpp:784-841): the best ids themselves, or their reduction when there are more
// than max_result.  best_ids[0..nb) is overwritten; tmp: 2*nb u64 of scratch (reduction only).
__device__ __forceinline__ void tail_emit(const DevView &v, uint64_t *best_ids, uint64_t nb, uint64_t *tmp, const TailFold &F, uint64_t sec_out,
                                          int32_t query_length, cfr_result &R, cfr_match *M, uint64_t slot0) {   // slot0: global index of M[0] (the key of the --expand-taxid lists)
  R.score = F.best;
  R.secondary_score = sec_out;
  R.hit_length = (int32_t)F.best_len;
  R.query_length = query_length;
  R.pad = 0;
  uint32_t nm = 0;
  if ((int64_t)nb <= (int64_t)v.max_result || v.max_result <= 0) {
    for (uint64_t q = 0; q < nb; ++q) {
      M[q].id = best_ids[q];
      M[q].taxid = d_orig_taxid(v, d_seq_to_tax(v, best_ids[q]));
      M[q].kind = 0;
      M[q].pad = 0;
    }
    nm = (uint32_t)nb;
  } else {
    for (uint64_t q = 0; q < nb; ++q) best_ids[q] = d_seq_to_tax(v, best_ids[q]);
    uint64_t *promoted = tmp + nb;     // fewer than nb of them, since this branch means nb > max_result
    uint32_t level = 0;
    nm = d_tax_reduce(v, best_ids, nb, v.max_result, tmp, promoted, &level);
    for (uint32_t q = 0; q < nm; ++q) {
      M[q].id = promoted[q];
      M[q].taxid = d_orig_taxid(v, promoted[q]);
      M[q].kind = 1;
      M[q].pad = 0;
    }
    if (v.exp_pool) d_tax_expand(v, best_ids, nb, v.max_result, promoted, nm, level, tmp, slot0);
  }
  R.n_match = (int32_t)nm;
}

// tail_emit for the register fold (<= 8 best ids, all in registers): listing, or the LCA of `-k 1`, without a local array (a
// dynamically indexed array would live in scratch memory).  Returns false when the ids need the general reduction (more than
// max_result > 1 of them): the caller then takes scratch from the pool.
__device__ __forceinline__ bool tail_emit_small(const DevView &v, const uint64_t (&bid)[8], uint32_t nb, const TailFold &F, uint64_t sec_out,
                                                int32_t query_length, cfr_result &R, cfr_match *M) {
  R.score = F.best;
  R.secondary_score = sec_out;
  R.hit_length = (int32_t)F.best_len;
  R.query_length = query_length;
  R.pad = 0;
  if ((int64_t)nb <= (int64_t)v.max_result || v.max_result <= 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) if ((uint32_t)q < nb) {
      cfr_match m;
      m.id = bid[q]; m.taxid = d_orig_taxid(v, d_seq_to_tax(v, bid[q])); m.kind = 0; m.pad = 0;
      M[q] = m;
    }
    R.n_match = (int32_t)nb;
    return true;
  }
  if (v.max_result != 1 || v.exp_pool) return false;          // (--expand-taxid: the general form keeps the promoted ids)
  // ReduceTaxIds with k = 1 (Taxonomy.hpp:839-973): an id outside the tree gives the node count, otherwise the LCA
  TaxFold L = tax_fold_begin(v.tax_root);                 // (cfr_tax_fold.hpp: bid is in the reference's order)
  bool outside = false;
#pragma unroll
  for (int q = 0; q < 8; ++q) if ((uint32_t)q < nb) {
    const uint64_t x = d_seq_to_tax(v, bid[q]);
    if (x >= v.node_cnt) outside = true;
    else tax_fold_add(v.tax_parent, v.tax_depth, v.tax_root, L, x);
  }
  const uint64_t out = outside ? v.node_cnt : tax_fold_result(L, v.tax_root);
  cfr_match m;
  m.id = out; m.taxid = d_orig_taxid(v, out); m.kind = 1; m.pad = 0;
  M[0] = m;
  R.n_match = 1;
  return true;
}

// FUSED (locate memo at every row): the kernel reads the per-read regions k_adjust_select wrote (hit_begin = hit_off,
// fin_cnt = hits per read, row_off = per-READ row base), enumerates each hit's rows itself and takes their values from
// loc_memo - no compaction, no row arrays, no locate launch.  Otherwise: dense hits + per-hit row offsets + located values.
template <bool FUSED>
__global__ void k_tail(DevView v, size_t n, const uint64_t *offs1, const uint64_t *offs2, const uint64_t *hit_begin,
                       const uint64_t *fin_cnt, const cfr_hit *hits, const uint64_t *row_off, uint64_t *row_vals,
                       TailEntry *entries, cfr_result *results, cfr_match *matches, uint64_t match_stride, uint64_t match_bias) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t hb = hit_begin[i], he = FUSED ? hb + fin_cnt[i] : hit_begin[i + 1];
  const uint64_t rbase = FUSED ? row_off[i] : row_off[hb];
  TailEntry *E = entries + rbase;      // per-read scratch: one entry per located row ...
  uint64_t *best_ids = row_vals + rbase;   // ... and the read's slice of the row values
  const uint64_t nh = he - hb;
  auto hit_at = [&](uint64_t h) { return hits[hb + h]; };
  bool mix = false;
  for (uint64_t h = 1; h < nh; ++h) if (hits[hb + h].strand != hits[hb + h - 1].strand) { mix = true; break; }

  TailFold F;
  uint64_t nb = 0, sec_out = 0;
  bool folded = false;
  if (FUSED) {
    uint64_t skey[8], ssc[8], bid[8];
    uint32_t sne = 0, nbr = 0;
    folded = tail_fold_small(v, hit_at, nh, mix, F, skey, ssc, sne);
    if (folded) {
      sec_out = tail_small_ids(v, F, skey, ssc, sne, bid, nbr);
#pragma unroll
      for (int q = 0; q < 8; ++q) if ((uint32_t)q < nbr) best_ids[q] = bid[q];
      nb = nbr;
    }
  }
  if (!folded) tail_fold_general<FUSED>(v, hit_at, nh, mix, row_vals + rbase, row_vals, row_off + hb, E, best_ids, F, nb, sec_out);

  const uint64_t mbase = v.max_result > 0 ? (uint64_t)i * match_stride : rbase;
  cfr_result R;
  tail_emit(v, best_ids, nb, reinterpret_cast<uint64_t *>(E), F, sec_out,
            (int32_t)(offs1[i + 1] - offs1[i]) + (offs2 ? (int32_t)(offs2[i + 1] - offs2[i]) : 0), R, matches + mbase, mbase + match_bias);
  R.match_begin = mbase + match_bias;       // matches[] is this sub-batch's buffer; match_begin is batch-global
  results[i] = R;
}

// Adjust/select and the whole tail in ONE launch (locate memo at every row, match slots per read): the final hit lists
// are never written out, the small fold needs no scratch at all, and a read that needs the general form takes its scratch
// from a pool with one atomicAdd - so a sub-batch runs without any host round trip.  A pool that runs dry raises
// *overflow and the host repeats that sub-batch through k_adjust_select + k_tail.
// One slot of a list for every lane that calls this, with ONE atomic per wave: the lanes that are here together (the branch they
// took) are counted by ballot, the first of them adds their number to the counter and hands the base round.  (Round 4: with hundreds
// of strains per species EVERY read goes to the list of team folds - 10 M returning atomics on one address were 113 of the 160 ms the
// post stage of such a batch took; bench.py --workload strains200.)
__device__ __forceinline__ unsigned long long wave_list_slot(unsigned long long *counter) {
  const uint64_t here = __ballot(1);
  const uint32_t lane = (uint32_t)__lane_id();
  const int leader = __ffsll((long long)here) - 1;
  unsigned long long base = 0;
  if ((int)lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(here));
  base = __shfl(base, leader);
  return base + (unsigned long long)__popcll(here & ((1ull << lane) - 1ull));
}

template <int CPR>
__device__ __forceinline__ void adjust_tail_one(const DevView &v, const uint8_t *bases1, const uint64_t *offs1, const uint8_t *bases2, const uint64_t *offs2,
                                                size_t i, const uint64_t *hit_off, cfr_hit *raw, const uint32_t *chain_cnt, TailEntry *pool_e,
                                                uint64_t *pool_v, unsigned long long *pool_cursor, uint64_t pool_cap, uint32_t *overflow,
                                                cfr_result *results, cfr_match *matches, uint64_t match_stride, uint64_t match_bias,
                                                uint64_t *heavy, unsigned long long *heavy_cnt, uint64_t *heavy2, unsigned long long *heavy2_cnt, uint32_t direct_rows) {
  const int32_t len1 = (int32_t)(offs1[i + 1] - offs1[i]);
  int32_t len2 = 0;
  const uint32_t cap1 = chain_cap(v, (uint32_t)len1);
  cfr_hit *base = raw + hit_off[i];
  cfr_hit *F1 = base, *R1 = base + cap1, *F2 = base, *R2 = base;
  const int32_t nF1 = (int32_t)chain_cnt[CPR * i + 0], nR1 = (int32_t)chain_cnt[CPR * i + 1];
  int32_t nF2 = 0, nR2 = 0;
  adjust_boundaries(v, bases1 + offs1[i], len1, F1, nF1, R1, nR1);
  if (CPR == 4) {
    len2 = (int32_t)(offs2[i + 1] - offs2[i]);
    const uint32_t cap2 = chain_cap(v, (uint32_t)len2);
    F2 = base + 2ull * cap1;
    R2 = F2 + cap2;
    nF2 = (int32_t)chain_cnt[CPR * i + 2];
    nR2 = (int32_t)chain_cnt[CPR * i + 3];
    adjust_boundaries(v, bases2 + offs2[i], len2, F2, nF2, R2, nR2);
  }
  // strandHits[1] = F1 ++ R2 ; strandHits[0] = R1 ++ F2 ; score, 1 % dominance rule (Classifier.hpp:568-576)
  uint64_t score_plus = 0, score_minus = 0;
  for (int32_t q = 0; q < nF1; ++q) score_plus += hit_score(v, F1[q].l);
  for (int32_t q = 0; q < nR2; ++q) score_plus += hit_score(v, R2[q].l);
  for (int32_t q = 0; q < nR1; ++q) score_minus += hit_score(v, R1[q].l);
  for (int32_t q = 0; q < nF2; ++q) score_minus += hit_score(v, F2[q].l);
  bool take_plus, take_minus;
  if (score_plus > score_minus + score_minus / 100) { take_plus = true; take_minus = false; }
  else if (score_minus > score_plus + score_plus / 100) { take_plus = false; take_minus = true; }
  else { take_plus = true; take_minus = true; }
  // the final hit list in k_adjust_select's order, read in place: plus part F1 ++ R2 (strand +1), minus part R1 ++ F2 (-1)
  const uint64_t c0 = take_plus ? (uint64_t)nF1 : 0, c1 = c0 + (take_plus ? (uint64_t)nR2 : 0);
  const uint64_t c2 = c1 + (take_minus ? (uint64_t)nR1 : 0), nh = c2 + (take_minus ? (uint64_t)nF2 : 0);
  auto hit_at = [&](uint64_t h) {
    cfr_hit H = h < c0 ? F1[h] : h < c1 ? R2[h - c0] : h < c2 ? R1[h - c1] : F2[h - c2];
    H.strand = h < c1 ? 1 : -1;
    return H;
  };
  const bool mix = c1 > 0 && nh > c1;   // both strands present = some neighbours differ in strand

  TailFold F;
  uint64_t nb = 0, sec_out = 0;
  uint64_t skey[8], ssc[8], bid[8];
  uint32_t sne = 0, nbr = 0;
  cfr_result R;
  cfr_match *M = matches + (uint64_t)i * match_stride;
  if (tail_fold_small(v, hit_at, nh, mix, F, skey, ssc, sne)) {
    sec_out = tail_small_ids(v, F, skey, ssc, sne, bid, nbr);
    if (!tail_emit_small(v, bid, nbr, F, sec_out, len1 + len2, R, M)) {
      // more than max_result > 1 best ids: the general reduction works on arrays - 24 u64 from the pool
      const uint64_t at = (uint64_t)atomicAdd(pool_cursor, 24ull);
      if (at + 24 > pool_cap) { atomicOr(overflow, 1u); return; }
      uint64_t *ids = pool_v + at;
#pragma unroll
      for (int q = 0; q < 8; ++q) ids[q] = bid[q];
      tail_emit(v, ids, nbr, ids + 8, F, sec_out, len1 + len2, R, M, (uint64_t)i * match_stride + match_bias);
    }
  } else if (heavy && nh < 65536) {
    // a read with many located rows (near-identical strains): k_tail_heavy folds it with a team of lanes and writes results[i].
    // (Every such read starts with the small teams; one whose ids do not fit their table is handed on to the large ones.  Sending
    // reads with many rows straight to the large teams was measured and is slower: 20 strains 3.2e8 -> 1.1e8 reads/s, 200 strains
    // 1.05e8 -> 5.5e7 - a large team keeps 32 lanes busy with what 8 do almost as fast, and a block holds 8 of them instead of 32.)
    uint64_t *L = heavy;
    unsigned long long *Lc = heavy_cnt;
    if (direct_rows && heavy2) {                // (test hook CFR_HEAVY_DIRECT_ROWS: reads with more located rows than this skip the small teams)
      uint64_t rows = 0;
      for (uint64_t h = 0; h < nh && rows <= direct_rows; ++h) rows += hit_row_count(v, hit_at(h));
      if (rows > direct_rows) { L = heavy2; Lc = heavy2_cnt; }
    }
    unsigned long long at;
    if (Lc == heavy_cnt) at = wave_list_slot(heavy_cnt); else at = wave_list_slot(heavy2_cnt);
    L[4 * at] = (uint64_t)i | (nh << 32);
    L[4 * at + 1] = c0 | (c1 << 16) | (c2 << 32);
    L[4 * at + 2] = hit_off[i];
    L[4 * at + 3] = (uint64_t)(uint32_t)len1 | ((uint64_t)(uint32_t)len2 << 32);
    return;
  } else {
    uint64_t rows = 0;
    for (uint64_t h = 0; h < nh; ++h) rows += hit_row_count(v, hit_at(h));
    // scratch from the pool: a table of >= 2 x rows slots (load <= 1/2) and 4 x rows u64 (ids: rows, reduction: 2 x rows,
    // occupied slots: rows)
    uint32_t logc = 2;
    while ((1ull << logc) < 2 * rows) ++logc;
    const uint64_t need = (1ull << logc) > 4 * rows ? (1ull << logc) : 4 * rows;
    const uint64_t at = (uint64_t)atomicAdd(pool_cursor, (unsigned long long)need);
    if (at + need > pool_cap) { atomicOr(overflow, 1u); return; }
    static_assert(sizeof(HashSlot) == sizeof(TailEntry), "the pool is shared with the two-kernel form");
    tail_fold_hash(v, hit_at, nh, mix, reinterpret_cast<HashSlot *>(pool_e + at), logc, pool_v + at, pool_v + at + 3 * rows, F, nb, sec_out);
    tail_emit(v, pool_v + at, nb, pool_v + at + rows, F, sec_out, len1 + len2, R, M, (uint64_t)i * match_stride + match_bias);
  }
  R.match_begin = (uint64_t)i * match_stride + match_bias;
  results[i] = R;
}

// one lane per read, or - with a grid smaller than the sub-batch - a grid-stride walk: beside the search of the next
// sub-batch the post stage is launched with a few blocks per CU so that it fills the search kernel's gaps instead of
// crowding it
// (Round 4 tried this kernel at 96 registers - `__launch_bounds__(256, 5)` - so that a wave of it fits on a SIMD beside the four waves of
// the search that runs at the same time: 1.2 KB of scratch per lane, and the step went from 12.9 to 78 ms.  It stays at 128 registers:
// beside a search it gets the CUs as that search's blocks drain, which is where the overlap's gain comes from.)
// list / list_cnt (round 5): the reads k_post_fast left for this kernel, instead of all n
template <int CPR>
__global__ void k_adjust_tail(DevView v, const uint8_t *bases1, const uint64_t *offs1, const uint8_t *bases2, const uint64_t *offs2,
                              size_t n, const uint64_t *hit_off, cfr_hit *raw, const uint32_t *chain_cnt, TailEntry *pool_e,
                              uint64_t *pool_v, unsigned long long *pool_cursor, uint64_t pool_cap, uint32_t *overflow,
                              cfr_result *results, cfr_match *matches, uint64_t match_stride, uint64_t match_bias,
                              uint64_t *heavy, unsigned long long *heavy_cnt, uint64_t *heavy2, unsigned long long *heavy2_cnt, uint32_t direct_rows,
                              const uint32_t *list, const unsigned long long *list_cnt) {
  const size_t total = list ? (size_t)*list_cnt : n;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (size_t)gridDim.x * blockDim.x)
    adjust_tail_one<CPR>(v, bases1, offs1, bases2, offs2, list ? (size_t)list[j] : j, hit_off, raw, chain_cnt, pool_e, pool_v, pool_cursor, pool_cap, overflow, results, matches,
                         match_stride, match_bias, heavy, heavy_cnt, heavy2, heavy2_cnt, direct_rows);
}

// The same kernel with the image description behind a POINTER (a copy of the DevView in device memory).  Passed by value, the
// description is a kernel argument, and the pairs instantiation indexes some of its arrays (C, the protein and run-block tables of the
// locate walk) with computed indexes: the compiler then copies the whole 1 KB structure into every lane's scratch memory at kernel entry
// (`k_adjust_tail<4>`: 1048 bytes of scratch, 56 sixteen-byte stores per lane before the first read is looked at; tools/dbg/scratch_sites.py).
// Behind a pointer the scalar fields are scalar loads as before and an indexed element is an ordinary (cached) load.
template <int CPR>
__global__ void k_adjust_tail_p(const DevView *vp, const uint8_t *bases1, const uint64_t *offs1, const uint8_t *bases2, const uint64_t *offs2,
                                size_t n, const uint64_t *hit_off, cfr_hit *raw, const uint32_t *chain_cnt, TailEntry *pool_e,
                                uint64_t *pool_v, unsigned long long *pool_cursor, uint64_t pool_cap, uint32_t *overflow,
                                cfr_result *results, cfr_match *matches, uint64_t match_stride, uint64_t match_bias,
                                uint64_t *heavy, unsigned long long *heavy_cnt, uint64_t *heavy2, unsigned long long *heavy2_cnt, uint32_t direct_rows,
                                const uint32_t *list, const unsigned long long *list_cnt) {
  const size_t total = list ? (size_t)*list_cnt : n;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (size_t)gridDim.x * blockDim.x)
    adjust_tail_one<CPR>(*vp, bases1, offs1, bases2, offs2, list ? (size_t)list[j] : j, hit_off, raw, chain_cnt, pool_e, pool_v, pool_cursor, pool_cap, overflow, results, matches,
                         match_stride, match_bias, heavy, heavy_cnt, heavy2, heavy2_cnt, direct_rows);
}

// ---- The post stage of the COMMON read, in registers only (round 5).  k_adjust_tail above carries every form of the post stage in one
// lane program - the boundary adjustment with its re-searches, the register fold, the hash fold through pool scratch, both reductions -
// and needs 128 registers for it, so a wave of it only starts where four waves of the search that runs beside it have left a SIMD.  What
// nearly every read of a sub-batch needs is much less: no hits on both strands of one mate (then AdjustHitBoundaryFromStrandHits,
// Classifier.hpp:303-401, has nothing to do), hits of at most 8 rows, at most 8 (strand list, sequence id) entries, values that fit 32 bits
// (sequence ids below 2^31 - 1, a read pair below 32768 bases: scores below 2^30), and either a listing or the LCA of -k 1.  This kernel is
// that read's post stage with 32-bit tables - same arithmetic, same order as tail_fold_small / tail_small_ids / tail_emit_small - and
// nothing else: a read that does not fit is put on a list and left alone.  Lists: `heavy` / `heavy2` (the team folds of k_tail_heavy: hits
// with many rows, more than 8 entries) and `slow` (everything else: k_adjust_tail over that list).  No scratch, no LDS, and few enough
// registers that its waves run UNDER a search (tests/test_kernel_resources.py holds it to 96).
template <int CPR>
__global__ __launch_bounds__(256, 5) void k_post_fast(DevView v, const uint64_t *offs1, const uint64_t *offs2, size_t n, const uint64_t *hit_off, const cfr_hit *raw,
                                                   const uint32_t *chain_cnt, cfr_result *results, cfr_match *matches, uint64_t match_stride, uint64_t match_bias,
                                                   uint64_t *heavy, unsigned long long *heavy_cnt, uint64_t *heavy2, unsigned long long *heavy2_cnt, uint32_t direct_rows,
                                                   uint32_t *slow, unsigned long long *slow_cnt) {
  constexpr uint32_t FREE = ~0u;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t len1 = (uint32_t)(offs1[i + 1] - offs1[i]);
    const uint32_t len2 = CPR == 4 ? (uint32_t)(offs2[i + 1] - offs2[i]) : 0u;
    const uint32_t cap1 = chain_cap(v, len1);
    const uint64_t hoff = hit_off[i];
    const cfr_hit *F1 = raw + hoff, *R1 = F1 + cap1, *F2 = F1, *R2 = F1;
    const uint32_t nF1 = chain_cnt[CPR * i + 0], nR1 = chain_cnt[CPR * i + 1];
    uint32_t nF2 = 0, nR2 = 0;
    if (CPR == 4) {
      F2 = F1 + 2ull * cap1;
      R2 = F2 + chain_cap(v, len2);
      nF2 = chain_cnt[CPR * i + 2];
      nR2 = chain_cnt[CPR * i + 3];
    }
    enum { DONE = 0, HEAVY = 1, SLOW = 2, HEAVY2 = 3 };
    int kind = DONE;
    uint32_t c0 = 0, c1 = 0, c2 = 0, nh = 0;
    if ((nF1 && nR1) || (nF2 && nR2) || len1 + len2 >= 32768u) kind = SLOW;      // hits on both strands of a mate: the boundary adjustment has work
    else {
      // strandHits[1] = F1 ++ R2 ; strandHits[0] = R1 ++ F2 ; score, 1 % dominance rule (Classifier.hpp:568-576)
      uint32_t score_plus = 0, score_minus = 0;
      for (uint32_t q = 0; q < nF1; ++q) score_plus += (uint32_t)hit_score(v, F1[q].l);
      for (uint32_t q = 0; q < nR2; ++q) score_plus += (uint32_t)hit_score(v, R2[q].l);
      for (uint32_t q = 0; q < nR1; ++q) score_minus += (uint32_t)hit_score(v, R1[q].l);
      for (uint32_t q = 0; q < nF2; ++q) score_minus += (uint32_t)hit_score(v, F2[q].l);
      bool take_plus = true, take_minus = true;
      if (score_plus > score_minus + score_minus / 100u) take_minus = false;
      else if (score_minus > score_plus + score_plus / 100u) take_plus = false;
      c0 = take_plus ? nF1 : 0u; c1 = c0 + (take_plus ? nR2 : 0u);
      c2 = c1 + (take_minus ? nR1 : 0u); nh = c2 + (take_minus ? nF2 : 0u);
    }
    const bool mix = c1 > 0 && nh > c1;
    uint32_t key[8], sc[8], ln[8];     // key = strand list << 31 | seqId ; FREE = free slot
#pragma unroll
    for (int e = 0; e < 8; ++e) { key[e] = FREE; sc[e] = 0; ln[e] = 0; }
    uint32_t ne = 0, prev_id = 0, prev_score = 0, prev_len = 0;
    bool p_unique = false;              // the previous hit: one row? its strand, and the offset a hit must have to follow it with one base between
    int32_t p_strand = 0, p_next = -1;
    for (uint32_t h = 0; h < nh && kind == DONE; ++h) {
      const cfr_hit *hp = h < c0 ? F1 + h : h < c1 ? R2 + (h - c0) : h < c2 ? R1 + (h - c1) : F2 + (h - c2);
      const ulonglong2 w0 = ld16(hp), w1 = ld16(reinterpret_cast<const uint64_t *>(hp) + 2);
      cfr_hit H;
      H.sp = w0.x; H.ep = w0.y; H.l = (int32_t)(uint32_t)w1.x; H.offset = (int32_t)(uint32_t)w1.y; H.pad = (int32_t)(uint32_t)(w1.y >> 32);
      H.strand = h < c1 ? 1 : -1;
      const bool uniq = H.ep == H.sp;
      if (H.l >= v.min_hit_len) {
        const uint64_t range = H.ep - H.sp + 1;
        if (range > 8 || !(range <= v.max_entries || v.locate_all)) { kind = HEAVY; break; }
        uint32_t x[8];
        bool wide_id = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          x[q] = FREE;
          if ((uint64_t)q < range) {
            const uint64_t id = locate_row(v, H, H.sp + q);
            wide_id |= id >= 0x7fffffffull;
            x[q] = (uint32_t)id;
          }
        }
        if (wide_id) { kind = HEAVY; break; }
#define CFR_CE(a, b) { const uint32_t lo_ = min(x[a], x[b]), hi_ = max(x[a], x[b]); x[a] = lo_; x[b] = hi_; }
        CFR_NET8(CFR_CE)
#undef CFR_CE
        const uint32_t score = (uint32_t)hit_score(v, H.l);
        const uint32_t kk = H.strand > 0 ? 0x80000000u : 0u;
        const bool adjacent = !mix && h > 0 && uniq && p_unique && p_strand == H.strand && p_next == H.offset;
        bool overflow = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const uint32_t id = x[q];
          const bool live = id != FREE && (q == 0 || id != x[q > 0 ? q - 1 : 0]);      // sorted: duplicates are neighbours
          if (live) {
            const uint32_t want = kk | id;
            uint32_t idx = ne;
#pragma unroll
            for (int e = 0; e < 8; ++e) if (key[e] == want) idx = (uint32_t)e;
            const bool created = idx == ne;
            if (created && ne == 8) overflow = true;
            else {
              uint32_t s_old = 0, l_old = 0;
#pragma unroll
              for (int e = 0; e < 8; ++e) if ((uint32_t)e == idx) { s_old = sc[e]; l_old = ln[e]; }
              uint32_t s_new, l_new;
              if (adjacent && id == prev_id) {             // merge adjacent unique hits (Classifier.hpp:673-685)
                prev_len += (uint32_t)H.l;
                const uint32_t merged = (uint32_t)hit_score(v, (int32_t)prev_len);
                s_new = s_old - prev_score + merged;
                prev_score = merged;
                l_new = l_old + (uint32_t)H.l;
              } else {
                s_new = created ? score : s_old + score;
                l_new = created ? (uint32_t)H.l : l_old + (uint32_t)H.l;
                if (uniq) { prev_id = id; prev_score = score; prev_len = (uint32_t)H.l; }
              }
#pragma unroll
              for (int e = 0; e < 8; ++e) if ((uint32_t)e == idx) { key[e] = want; sc[e] = s_new; ln[e] = l_new; }
              if (created) ++ne;
            }
          }
        }
        if (overflow) { kind = HEAVY; break; }
      }
      p_unique = uniq; p_strand = H.strand; p_next = H.offset + H.l + 1;
    }
    if (kind == DONE) {
      // std::map iteration order: strand list 0 then 1, ascending seqId = ascending key
#define CFR_CE(a, b) { const bool sw_ = key[a] > key[b]; \
      const uint32_t k_ = key[a], s_ = sc[a], l_ = ln[a]; \
      key[a] = sw_ ? key[b] : k_; sc[a] = sw_ ? sc[b] : s_; ln[a] = sw_ ? ln[b] : l_; \
      key[b] = sw_ ? k_ : key[b]; sc[b] = sw_ ? s_ : sc[b]; ln[b] = sw_ ? l_ : ln[b]; }
      CFR_NET8(CFR_CE)
#undef CFR_CE
      uint32_t best = 0, second = 0, best_len = 0, second_len = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) if ((uint32_t)e < ne) {
        if (sc[e] > best) { second = best; second_len = best_len; best = sc[e]; best_len = ln[e]; }
        else if (sc[e] > second) { second = sc[e]; second_len = ln[e]; }
      }
      const bool take_second = (uint64_t)second_len >= v.secondary_hit_len && second < best && (uint64_t)second >= (uint64_t)(v.secondary_factor * (double)(uint64_t)best);
      // the best ids in map order, unique across the strand lists (tail_small_ids)
      uint32_t bid[8];
      uint32_t nb = 0, nb_best = 0;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const uint32_t target = pass == 0 ? best : second;
        if (pass == 0 || take_second) {
#pragma unroll
          for (int e = 0; e < 8; ++e) if ((uint32_t)e < ne && sc[e] == target) {
            const uint32_t id = key[e] & 0x7fffffffu;
            bool seen = false;
#pragma unroll
            for (int q = 0; q < 8; ++q) if ((uint32_t)q < nb && bid[q] == id) seen = true;
            if (!seen) {
#pragma unroll
              for (int q = 0; q < 8; ++q) if ((uint32_t)q == nb) bid[q] = id;
              ++nb;
            }
          }
        }
        if (pass == 0) nb_best = nb;
      }
      cfr_result R;
      R.score = best;
      R.secondary_score = take_second ? second : (nb_best > 1 ? best : second);
      R.hit_length = (int32_t)best_len;
      R.query_length = (int32_t)(len1 + len2);
      R.pad = 0;
      R.match_begin = (uint64_t)i * match_stride + match_bias;
      cfr_match *M = matches + (uint64_t)i * match_stride;
      if ((int32_t)nb <= v.max_result) {
#pragma unroll
        for (int q = 0; q < 8; ++q) if ((uint32_t)q < nb) {
          cfr_match m;
          m.id = bid[q]; m.taxid = d_orig_taxid(v, d_seq_to_tax(v, bid[q])); m.kind = 0; m.pad = 0;
          M[q] = m;
        }
        R.n_match = (int32_t)nb;
        results[i] = R;
      } else if (v.max_result == 1 && !v.exp_pool) {
        // ReduceTaxIds with k = 1 (Taxonomy.hpp:839-973): an id outside the tree gives the node count, otherwise the LCA (tail_emit_small)
        TaxFold F = tax_fold_begin(v.tax_root);                 // (cfr_tax_fold.hpp: bid is in the reference's order)
        bool outside = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) if ((uint32_t)q < nb) {
          const uint64_t x = d_seq_to_tax(v, bid[q]);
          if (x >= v.node_cnt) outside = true;
          else tax_fold_add(v.tax_parent, v.tax_depth, v.tax_root, F, x);
        }
        const uint64_t out = outside ? v.node_cnt : tax_fold_result(F, v.tax_root);
        cfr_match m;
        m.id = out; m.taxid = d_orig_taxid(v, out); m.kind = 1; m.pad = 0;
        M[0] = m;
        R.n_match = 1;
        results[i] = R;
      } else kind = SLOW;                                       // the level-wise reduction of -k > 1 (and --expand-taxid) works on arrays
    }
    if (kind == HEAVY && !(heavy && nh < 65536u)) kind = SLOW;
    if (kind == HEAVY) {
      bool second_tier = false;
      if (direct_rows && heavy2) {                // reads with more located rows than this skip the small teams (k_adjust_tail's rule)
        uint64_t rows = 0;
        for (uint32_t h = 0; h < nh && rows <= direct_rows; ++h) {
          const cfr_hit *hp = h < c0 ? F1 + h : h < c1 ? R2 + (h - c0) : h < c2 ? R1 + (h - c1) : F2 + (h - c2);
          cfr_hit H;
          const ulonglong2 w0 = ld16(hp);
          H.sp = w0.x; H.ep = w0.y; H.l = hp->l;
          rows += hit_row_count(v, H);
        }
        if (rows > direct_rows) second_tier = true;
      }
      kind = second_tier ? HEAVY2 : HEAVY;
    }
    // one list per exit, each with its own ballot (three separate tests: the lanes of one list draw their slots together)
    if (kind == HEAVY) {
      const unsigned long long at = wave_list_slot(heavy_cnt);
      heavy[4 * at] = (uint64_t)i | ((uint64_t)nh << 32);
      heavy[4 * at + 1] = (uint64_t)c0 | ((uint64_t)c1 << 16) | ((uint64_t)c2 << 32);
      heavy[4 * at + 2] = hoff;
      heavy[4 * at + 3] = (uint64_t)len1 | ((uint64_t)len2 << 32);
    }
    if (kind == HEAVY2) {
      const unsigned long long at = wave_list_slot(heavy2_cnt);
      heavy2[4 * at] = (uint64_t)i | ((uint64_t)nh << 32);
      heavy2[4 * at + 1] = (uint64_t)c0 | ((uint64_t)c1 << 16) | ((uint64_t)c2 << 32);
      heavy2[4 * at + 2] = hoff;
      heavy2[4 * at + 3] = (uint64_t)len1 | ((uint64_t)len2 << 32);
    }
    if (kind == SLOW) {
      slow[wave_list_slot(slow_cnt)] = (uint32_t)i;
    }
  }
}

// ---- the fold of a read with many located rows, by a TEAM of kTeam lanes (64 / kTeam reads per wave).
// k_adjust_tail's register fold holds 8 (strand list, seqId) entries; a read over a family of near-identical strains
// locates tens of rows per hit, and one lane folding them through a hash table in global scratch (tail_fold_hash) is a long
// chain of dependent HBM accesses per row.  Here the lanes of a team take the rows of a hit side by side (their memo / suffix
// array entries are consecutive: one coalesced gather), the per-read score table lives in LDS (64 slots of 16 bytes per team,
// claimed with ds_cmpst, "this hit has counted the id already" decided by ds_max on the slot's tag), what the reference's
// ordered maps decide comes out of team-wide reductions exactly as tail_fold_hash derives it, and the LCA of `-k 1` is
// folded pairwise across the lanes.  Anything that does not fit - more than 48 entries, a sequence id >= 2^31, a listing
// reduction with k > 1 - is done by lane 0 of the team with the single-lane code and pool scratch.
#ifndef CFR_TEAM
#define CFR_TEAM 8
#endif
#ifndef CFR_TEAM_SLOTS
#define CFR_TEAM_SLOTS 64
#define CFR_TEAMS_PER_BLOCK 32
#define CFR_TEAM_MAXE 48
#endif
constexpr int kTeam = CFR_TEAM, kTeamSlots = CFR_TEAM_SLOTS, kTeamsPerBlock = CFR_TEAMS_PER_BLOCK, kTeamMaxEntries = CFR_TEAM_MAXE;
// second tier (round 4): a read whose ids do not fit 48 entries - hundreds of near-identical strains per species, 40 located rows per
// hit (Classifier.hpp:640-666) - is handed on to teams of 32 lanes with 256 slots (192 entries) instead of one lane with a table in
// global scratch: bench.py --workload strains200 spent 465 ms per 10 M reads in that single-lane fold
constexpr int kTeam2 = 32, kTeam2Slots = 256, kTeams2PerBlock = 8, kTeam2MaxEntries = 192;
struct TeamSlot { uint32_t key, tag_len; uint64_t score; };   // key = strand list << 31 | seqId, ~0 = empty ; tag_len = last hit that counted the id << 20 | sum of hit lengths
constexpr uint32_t kTeamLenBits = 20;

__device__ __forceinline__ void team_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// TEAM lanes per read, SLOTS table slots (a power of two <= 256), TPB teams per block, MAXE entries at most.
// next / next_cnt: the list a read goes to when its ids do not fit MAXE entries (nullptr: the single-lane form takes it here)
template <int CPR, int TEAM, int SLOTS, int TPB, int MAXE>
__global__ __launch_bounds__(TEAM * TPB) void k_tail_heavy(DevView v, const uint64_t *offs1, const uint64_t *offs2, const uint64_t *hit_off,
                                                                        const cfr_hit *raw, const uint64_t *heavy, const unsigned long long *heavy_cnt,
                                                                        TailEntry *pool_e, uint64_t *pool_v, unsigned long long *pool_cursor, uint64_t pool_cap,
                                                                        uint32_t *overflow, cfr_result *results, cfr_match *matches, uint64_t match_stride,
                                                                        uint64_t match_bias, uint64_t *next, unsigned long long *next_cnt) {
  constexpr int kTeam = TEAM, kTeamSlots = SLOTS, kTeamsPerBlock = TPB, kTeamMaxEntries = MAXE;      // (shadow the first tier's constants)
  constexpr uint32_t kHashShift = SLOTS == 256 ? 24u : SLOTS == 128 ? 25u : SLOTS == 64 ? 26u : 27u;
  static_assert(SLOTS == 256 || SLOTS == 128 || SLOTS == 64 || SLOTS == 32, "table size");
  auto team_shfl_xor = [](uint64_t x, int m) { return __shfl_xor(x, m, TEAM); };
  __shared__ TeamSlot s_tab[kTeamsPerBlock][kTeamSlots];
  __shared__ uint8_t s_list[kTeamsPerBlock][kTeamSlots];      // slots whose ids are reported
  __shared__ uint32_t s_ctl[kTeamsPerBlock][4];               // entries, reported ids, reported ids at the best score, bail-out flag
  const uint32_t team = threadIdx.x / kTeam, tl = threadIdx.x % kTeam;
  TeamSlot *tab = s_tab[team];
  uint8_t *list = s_list[team];
  uint32_t *ctl = s_ctl[team];
  const uint32_t EMPTY = ~0u;
  const unsigned long long nheavy = *heavy_cnt;
  for (unsigned long long qi = (unsigned long long)blockIdx.x * kTeamsPerBlock + team; qi < nheavy; qi += (unsigned long long)gridDim.x * kTeamsPerBlock) {
    const uint64_t w0 = heavy[4 * qi], w1 = heavy[4 * qi + 1], w3 = heavy[4 * qi + 3];
    const size_t i = (size_t)(w0 & 0xffffffffull);
    const uint64_t nh = w0 >> 32, c0 = w1 & 0xffffull, c1 = (w1 >> 16) & 0xffffull, c2 = (w1 >> 32) & 0xffffull;
    const int32_t len1 = (int32_t)(uint32_t)w3, len2 = (int32_t)(uint32_t)(w3 >> 32);
    const uint32_t cap1 = chain_cap(v, (uint32_t)len1);
    const cfr_hit *hbase = raw + heavy[4 * qi + 2];
    const cfr_hit *F1 = hbase, *R1 = hbase + cap1, *F2 = hbase, *R2 = hbase;
    if (CPR == 4) {
      F2 = hbase + 2ull * cap1;
      R2 = F2 + chain_cap(v, (uint32_t)len2);
    }
    auto hit_load = [&](uint64_t h) {
      cfr_hit H = h < c0 ? F1[h] : h < c1 ? R2[h - c0] : h < c2 ? R1[h - c1] : F2[h - c2];
      H.strand = h < c1 ? 1 : -1;
      return H;
    };
    // the first kTeam hits of the read, one per lane, fetched together; hit_at hands them round by shuffle
    cfr_hit Hmine;
    Hmine.sp = 0; Hmine.ep = 0; Hmine.l = 0; Hmine.offset = 0; Hmine.strand = 0; Hmine.pad = 0;
    if ((uint64_t)tl < nh) Hmine = hit_load(tl);
    auto hit_at = [&](uint64_t h) {
      if (h >= (uint64_t)kTeam) return hit_load(h);            // (team-uniform branch)
      cfr_hit H;
      const int src = (int)h;
      H.sp = __shfl(Hmine.sp, src, kTeam);
      H.ep = __shfl(Hmine.ep, src, kTeam);
      const uint64_t lo = __shfl((uint64_t)(uint32_t)Hmine.l | ((uint64_t)(uint32_t)Hmine.offset << 32), src, kTeam);
      H.l = (int32_t)(uint32_t)lo;
      H.offset = (int32_t)(uint32_t)(lo >> 32);
      H.strand = h < c1 ? 1 : -1;
      H.pad = __shfl(Hmine.pad, src, kTeam);
      return H;
    };
    const bool mix = c1 > 0 && nh > c1;
    cfr_match *M = matches + (uint64_t)i * match_stride;
    cfr_result R;

    // ---- the table
    for (uint32_t q = tl; q < (uint32_t)kTeamSlots; q += kTeam) { TeamSlot z; z.key = EMPTY; z.tag_len = 0; z.score = 0; tab[q] = z; }
    if (tl < 4) ctl[tl] = 0;
    team_sync();
    auto slot_for = [&](uint32_t key) -> uint32_t {           // the slot of key, claimed if new; kTeamSlots when the table is full
      uint32_t sl = (key * 0x9E3779B1u) >> kHashShift;
      for (int probe = 0; probe < kTeamSlots; ++probe) {
        const uint32_t k = atomicCAS(&tab[sl].key, EMPTY, key);
        if (k == EMPTY) { atomicAdd(&ctl[0], 1u); return sl; }
        if (k == key) return sl;
        sl = (sl + 1) & (kTeamSlots - 1);
      }
      return (uint32_t)kTeamSlots;
    };
    auto slot_of = [&](uint32_t key) -> uint32_t {            // read only: the slot of key, or kTeamSlots
      uint32_t sl = (key * 0x9E3779B1u) >> kHashShift;
      for (int probe = 0; probe < kTeamSlots; ++probe) {
        const uint32_t k = tab[sl].key;
        if (k == key) return sl;
        if (k == EMPTY) break;
        sl = (sl + 1) & (kTeamSlots - 1);
      }
      return (uint32_t)kTeamSlots;
    };
    uint32_t prev_id = 0;
    uint64_t prev_score = 0;
    int32_t prev_len = 0;
    bool bail = (uint64_t)(uint32_t)(len1 + len2) >= (1ull << kTeamLenBits) || nh >= (1ull << (32 - kTeamLenBits)) - 1;   // the packed tag / length word
    bool too_many = false;                                   // the read's ids do not fit this tier's table
    const uint32_t LEN_MASK = (1u << kTeamLenBits) - 1u;
    for (uint64_t h = 0; h < nh && !bail; ++h) {
      const cfr_hit H = hit_at(h);
      if (H.l < v.min_hit_len) continue;
      const uint64_t score = hit_score(v, H.l);
      const uint32_t kbit = H.strand > 0 ? 0x80000000u : 0u;
      const uint32_t tag = (uint32_t)h + 1;
      const uint64_t range = H.ep - H.sp + 1;
      if (range == 1) {
        // one row: every lane does the same (the merge of adjacent unique hits, Classifier.hpp:673-685, carries state from hit to hit)
        bool adjacent = false;
        if (!mix && h > 0) {
          const cfr_hit P = hit_at(h - 1);
          adjacent = P.ep == P.sp && P.strand == H.strand && P.offset + P.l + 1 == H.offset;
        }
        const uint32_t id = (uint32_t)locate_row(v, H, H.sp);
        uint32_t sl = (uint32_t)kTeamSlots;
        if (id < 0x80000000u) sl = slot_for(kbit | id);
        if (sl == (uint32_t)kTeamSlots) { bail = true; too_many = id < 0x80000000u; }
        else {
          team_sync();
          TeamSlot e = tab[sl];
          if ((e.tag_len >> kTeamLenBits) != tag) {
            if (adjacent && id == prev_id) {
              e.score -= prev_score;
              prev_len += H.l;
              prev_score = hit_score(v, prev_len);
              e.score += prev_score;
            } else {
              e.score += score;
              prev_id = id; prev_score = score; prev_len = H.l;
            }
            e.tag_len = (tag << kTeamLenBits) | ((e.tag_len & LEN_MASK) + (uint32_t)H.l);
            team_sync();                                       // everybody has read the slot
            if (tl == 0) tab[sl] = e;
          }
        }
      } else {
        // the row sequence of Classifier.hpp:625-665, one row per lane and pass
        uint64_t total = range, step = 1, fwd = range;
        if (!(range <= v.max_entries || v.locate_all)) {
          step = (range + v.max_entries - 1) / v.max_entries;
          fwd = (range + step - 1) / step;
          uint64_t bwd = v.max_entries > fwd ? v.max_entries - fwd : 1;
          if (bwd > fwd) bwd = fwd;
          total = fwd + bwd;
        }
        for (uint64_t idx = tl; idx < total; idx += kTeam) {
          const uint64_t row = idx < fwd ? H.sp + idx * step : H.ep - (idx - fwd) * step;
          const uint32_t id = (uint32_t)locate_row(v, H, row);
          uint32_t sl = (uint32_t)kTeamSlots;
          if (id < 0x80000000u) sl = slot_for(kbit | id);
          if (sl == (uint32_t)kTeamSlots) atomicOr(&ctl[3], id < 0x80000000u ? 2u : 1u);
          else {
            // ds_max with (tag << 20): whoever finds an older tag there is the first row of this hit with that id and
            // owns the slot's update (the maximum has wiped the length bits; the owner puts them back)
            const uint32_t old = atomicMax(&tab[sl].tag_len, tag << kTeamLenBits);
            if ((old >> kTeamLenBits) != tag) {
              tab[sl].tag_len = (tag << kTeamLenBits) | ((old & LEN_MASK) + (uint32_t)H.l);
              tab[sl].score += score;
            }
          }
        }
      }
      team_sync();
      if (ctl[3] || ctl[0] > (uint32_t)kTeamMaxEntries) { bail = true; too_many = !(ctl[3] & 1u); }
    }

    uint64_t best = 0, second = 0, len_best = 0, second_len = 0, sec_out = 0;
    bool take_second = false;
    uint32_t nb = 0;
    if (!bail) {
      // ---- best; the two smallest keys at the best score; the largest lower score and its smallest key (tail_fold_hash)
      const uint64_t NOKEY = ~0ull;
      for (uint32_t q = tl; q < (uint32_t)kTeamSlots; q += kTeam) if (tab[q].key != EMPTY && tab[q].score > best) best = tab[q].score;
      for (int m = kTeam / 2; m > 0; m >>= 1) { const uint64_t o = team_shfl_xor(best, m); if (o > best) best = o; }
      uint64_t k1 = NOKEY, k2 = NOKEY, l1 = 0, l2 = 0, v2 = 0, kq = NOKEY, lq = 0;
      // (selects, not branches: as `if (k < k1) { k2 = k1; ... }` the compiler kept the pairs as two-entry arrays in scratch memory,
      //  tools/dbg/scratch_sites.py)
#if defined(CFR_TEAM_BEST_BRANCHES) && CFR_TEAM_BEST_BRANCHES      // the form before (A/B: tools/dbg/ab_team_best.sh)
      auto take_best_key = [&](uint64_t k, uint64_t l) {
        if (k < k1) { k2 = k1; l2 = l1; k1 = k; l1 = l; }
        else if (k < k2) { k2 = k; l2 = l; }
      };
      auto take_lower = [&](uint64_t sc, uint64_t k, uint64_t l) {
        if (sc > v2 || (sc == v2 && k < kq)) { v2 = sc; kq = k; lq = l; }
      };
#else
      auto take_best_key = [&](uint64_t k, uint64_t l) {
        const bool a = k < k1, b = !a && k < k2;
        k2 = a ? k1 : (b ? k : k2); l2 = a ? l1 : (b ? l : l2);
        k1 = a ? k : k1; l1 = a ? l : l1;
      };
      auto take_lower = [&](uint64_t sc, uint64_t k, uint64_t l) {
        const bool t = sc > v2 || (sc == v2 && k < kq);
        v2 = t ? sc : v2; kq = t ? k : kq; lq = t ? l : lq;
      };
#endif
      for (uint32_t q = tl; q < (uint32_t)kTeamSlots; q += kTeam) {
        const TeamSlot e = tab[q];
        if (e.key == EMPTY || e.score == 0) continue;         // (a zero score never enters best/second: both tests are strict)
        if (e.score == best) take_best_key((uint64_t)e.key, (uint64_t)(e.tag_len & LEN_MASK));
        else take_lower(e.score, (uint64_t)e.key, (uint64_t)(e.tag_len & LEN_MASK));
      }
      for (int m = kTeam / 2; m > 0; m >>= 1) {
        const uint64_t ok1 = team_shfl_xor(k1, m), ol1 = team_shfl_xor(l1, m), ok2 = team_shfl_xor(k2, m), ol2 = team_shfl_xor(l2, m);
        const uint64_t ov2 = team_shfl_xor(v2, m), okq = team_shfl_xor(kq, m), olq = team_shfl_xor(lq, m);
        if (ok1 != NOKEY) take_best_key(ok1, ol1);
        if (ok2 != NOKEY) take_best_key(ok2, ol2);
        if (okq != NOKEY) take_lower(ov2, okq, olq);
      }
      if (best == 0) { second = 0; second_len = 0; len_best = 0; }
      else if (k2 != NOKEY) { second = best; second_len = l2; len_best = l1; }
      else { second = v2; second_len = v2 ? lq : 0; len_best = l1; }
      take_second = second_len >= v.secondary_hit_len && second < best && second >= (uint64_t)(v.secondary_factor * (double)best);
      auto cls = [&](uint64_t sc) -> uint32_t { return sc == best ? 1u : (take_second && sc == second ? 2u : 0u); };
      // ---- the ids to report: every id once, by its first entry in (class, strand list) order
      for (uint32_t q = tl; q < (uint32_t)kTeamSlots; q += kTeam) {
        const TeamSlot e = tab[q];
        if (e.key == EMPTY) continue;
        const uint32_t c = cls(e.score);
        if (!c) continue;
        const uint32_t os = slot_of(e.key ^ 0x80000000u);     // the same id in the other strand list, if any
        if (os != (uint32_t)kTeamSlots) {
          const uint32_t cs = cls(tab[os].score);
          if (cs && (cs < c || (cs == c && tab[os].key < e.key))) continue;      // that list reports the id first
        }
        list[atomicAdd(&ctl[1], 1u)] = (uint8_t)q;
        if (c == 1) atomicAdd(&ctl[2], 1u);
      }
      team_sync();
      nb = ctl[1];
      sec_out = take_second ? second : (ctl[2] > 1 ? best : second);
      R.score = best;
      R.secondary_score = sec_out;
      R.hit_length = (int32_t)len_best;
      R.query_length = len1 + len2;
      R.pad = 0;
      if ((int64_t)nb <= (int64_t)v.max_result) {
        // listed: order by (class, strand list, id) - a handful of ids, lane 0 sorts the slot list in place
        if (tl == 0) {
          for (uint32_t a = 1; a < nb; ++a) {
            const uint32_t x = list[a];
            const uint32_t cx = cls(tab[x].score), kx = tab[x].key;
            uint32_t b = a;
            while (b > 0) {
              const uint32_t y = list[b - 1];
              const uint32_t cy = cls(tab[y].score), ky = tab[y].key;
              if (cy < cx || (cy == cx && ky < kx)) break;
              list[b] = (uint8_t)y;
              --b;
            }
            list[b] = (uint8_t)x;
          }
          for (uint32_t q = 0; q < nb; ++q) {
            const uint64_t id = (uint64_t)(tab[list[q]].key & 0x7fffffffu);
            cfr_match m;
            m.id = id; m.taxid = d_orig_taxid(v, d_seq_to_tax(v, id)); m.kind = 0; m.pad = 0;
            M[q] = m;
          }
        }
        R.n_match = (int32_t)nb;
      } else if (v.max_result == 1 && !v.exp_pool) {            // (--expand-taxid: the single-lane form keeps the promoted ids)
        // ReduceTaxIds with k = 1 (Taxonomy.hpp:839-973): an id outside the tree gives the node count, otherwise Taxonomy::LCA.  On a
        // forest that is no set function of the ids (cfr_tax_fold.hpp): the first id that is not the root is the backbone even when
        // it is the top of a second tree.  The ids that are no top ARE folded as a set, per lane and then across the team; `first`
        // is the first non-root id in the reference's order (class, strand list, id), with bit 0 clear when that id is a top.
        TaxFold F = tax_fold_begin(v.tax_root);
        bool outside = false;
        uint64_t first = ~0ull, first_x = v.tax_root;
        for (uint32_t q = tl; q < nb; q += kTeam) {
          const TeamSlot e = tab[list[q]];
          const uint64_t x = d_seq_to_tax(v, (uint64_t)(e.key & 0x7fffffffu));
          if (x >= v.node_cnt) outside = true;
          else if (x != v.tax_root) {
            const bool top = x == v.tax_parent[x];
            const uint64_t ord = ((((uint64_t)cls(e.score) << 32) | (uint64_t)e.key) << 1) | (top ? 0ull : 1ull);
            if (ord < first) { first = ord; first_x = x; }
            if (!top) tax_fold_add(v.tax_parent, v.tax_depth, v.tax_root, F, x);
          }
        }
        // across the team: everybody up to the smallest depth, then level by level until all stand on one node (one
        // round of loads per level instead of a pairwise climb per butterfly step)
        uint64_t cur = F.cur;
        uint32_t dcur = F.dcur;
        bool have = F.have;
        uint32_t dmin = have ? dcur : ~0u;
        uint64_t any = ((uint64_t)have) | ((uint64_t)outside << 1);
        for (int m = kTeam / 2; m > 0; m >>= 1) {
          const uint64_t o = team_shfl_xor((uint64_t)dmin | (any << 32), m);
          if ((uint32_t)o < dmin) dmin = (uint32_t)o;
          any |= o >> 32;
          const uint64_t of = team_shfl_xor(first, m), ox = team_shfl_xor(first_x, m);
          if (of < first) { first = of; first_x = ox; }
        }
        outside = (any >> 1) & 1ull;
        const bool team_have = any & 1ull;
        if (team_have && !outside) {
          if (have) while (dcur > dmin) { cur = v.tax_parent[cur]; --dcur; }
          for (;;) {
            // depth 0: the lanes stand on the tops of their trees (or all on a second top): every path ends in the root.  dmin
            // is the same in every lane and counts down, so the climb ends on any forest
            if (dmin == 0) { cur = v.tax_root; break; }
            // the smallest node anybody stands on, and whether anybody stands elsewhere
            uint64_t ref = have ? cur : ~0ull;
            for (int m = kTeam / 2; m > 0; m >>= 1) { const uint64_t o = team_shfl_xor(ref, m); if (o < ref) ref = o; }
            uint64_t differ = have && cur != ref;
            for (int m = kTeam / 2; m > 0; m >>= 1) differ |= team_shfl_xor(differ, m);
            if (!differ) { cur = ref; break; }
            if (have) cur = v.tax_parent[cur];
            --dmin;
          }
          if (!(first & 1ull)) cur = v.tax_root;              // the backbone is a second top, and some id is none: the root
          have = true;
        } else if (!outside && first != ~0ull) { cur = first_x; have = true; }   // tops only: the first that is not the root
        const uint64_t out = outside ? v.node_cnt : (have ? cur : v.tax_root);
        if (tl == 0) {
          cfr_match m;
          m.id = out; m.taxid = d_orig_taxid(v, out); m.kind = 1; m.pad = 0;
          M[0] = m;
        }
        R.n_match = 1;
      } else bail = true;                                       // the level-wise reduction of k > 1: single-lane code
    }
    if (bail && too_many && next) {
      // ---- too many ids for this tier's table: the read goes on to the larger teams
      if (tl == 0) {
        const unsigned long long at = wave_list_slot(next_cnt);
        next[4 * at] = w0; next[4 * at + 1] = w1; next[4 * at + 2] = heavy[4 * qi + 2]; next[4 * at + 3] = w3;
      }
    } else if (bail) {
      // ---- the single-lane form with scratch from the pool (k_adjust_tail's general branch)
      if (tl == 0) {                                             // (hit_load: the shuffles of hit_at need the whole team)
        uint64_t rows = 0;
        for (uint64_t h = 0; h < nh; ++h) rows += hit_row_count(v, hit_load(h));
        uint32_t logc = 2;
        while ((1ull << logc) < 2 * rows) ++logc;
        const uint64_t need = (1ull << logc) > 4 * rows ? (1ull << logc) : 4 * rows;
        const uint64_t at = (uint64_t)atomicAdd(pool_cursor, (unsigned long long)need);
        if (at + need > pool_cap) atomicOr(overflow, 1u);
        else {
          TailFold F;
          uint64_t nbl = 0, so = 0;
          tail_fold_hash(v, hit_load, nh, mix, reinterpret_cast<HashSlot *>(pool_e + at), logc, pool_v + at, pool_v + at + 3 * rows, F, nbl, so);
          tail_emit(v, pool_v + at, nbl, pool_v + at + rows, F, so, len1 + len2, R, M, (uint64_t)i * match_stride + match_bias);
          R.match_begin = (uint64_t)i * match_stride + match_bias;
          results[i] = R;
        }
      }
    } else if (tl == 0) {
      R.match_begin = (uint64_t)i * match_stride + match_bias;
      results[i] = R;
    }
    team_sync();                                                // the table is the next read's
  }
}

// the few 8-byte values the host needs before it can enqueue the sub-batches of a resident batch - where every piece's reads and hit
// lists start - in ONE launch that stores them straight into pinned host memory (round 3 fetched them with 25-38 eight-byte copies,
// each a blit dispatch of its own in front of the first search)
struct PieceFirsts { uint64_t at[17]; uint32_t n; };            // first read of every piece, and the read count behind the last (n <= 17)
__global__ void k_fetch_piece_scalars(PieceFirsts f, const uint64_t *offs1, const uint64_t *offs2, const uint64_t *hit_all, uint64_t *out_b1, uint64_t *out_b2,
                                      uint64_t *out_hit) {
  const uint32_t k = threadIdx.x;
  if (k >= f.n) return;
  out_b1[k] = offs1[f.at[k]];
  out_b2[k] = offs2 ? offs2[f.at[k]] : 0ull;
  out_hit[k] = hit_all ? hit_all[f.at[k]] : 0ull;
}

// the results of a sub-batch in the narrow layout of cfr_classify_batch_resident_compact (include/cfr_hip.h): what leaves
// over PCIe is half as long.  One lane per read; a value that does not fit its field flags the read.
// side: the few reads whose values do not fit the narrow layout leave in the wide one as well - (read, cfr_result, its match
// slots) appended to a small list the host fetches with the call's last copy (cfr_compact_wide_reads)
struct WideSide { uint32_t *idx; cfr_result *res; cfr_match *match; unsigned long long *cnt; uint64_t cap; };
__global__ void k_compact_results(const cfr_result *res, const cfr_match *match, size_t n, uint64_t stride, cfr_result_compact *cres,
                                  cfr_match_compact *cmatch, uint64_t read_base, WideSide side) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const cfr_result R = res[i];
  cfr_result_compact C;
  bool wide = (R.score >> 32) != 0 || (R.secondary_score >> 32) != 0 || R.hit_length < 0 || R.query_length < 0 || R.n_match < 0 || R.n_match > 255 ||
              (uint64_t)R.n_match > stride;
  C.score = (uint32_t)R.score;
  C.secondary_score = (uint32_t)R.secondary_score;
  C.hit_length = (uint32_t)R.hit_length;
  C.query_length = (uint32_t)R.query_length;
  C.n_match = (uint8_t)R.n_match;
  C.pad = 0;
  const uint64_t used = wide ? 0 : (uint64_t)R.n_match;
  for (uint64_t q = 0; q < stride; ++q) {                  // every slot of the read is written: the ones it does not use are zero
    cfr_match_compact m;
    m.id_kind = 0; m.taxid_lo = 0; m.taxid_hi = 0;
    if (q < used) {
      const cfr_match M = match[i * stride + q];
      if ((M.id >> 31) != 0) wide = true;
      m.id_kind = (uint32_t)M.id | (M.kind ? 0x80000000u : 0u);
      m.taxid_lo = (uint32_t)M.taxid;
      m.taxid_hi = (uint32_t)(M.taxid >> 32);
    }
    cmatch[i * stride + q] = m;
  }
  C.flags = wide ? (uint8_t)CFR_COMPACT_WIDE : 0;
  cres[i] = C;
  if (wide && side.cnt) {
    const unsigned long long at = atomicAdd(side.cnt, 1ull);
    if (at < side.cap) {
      side.idx[at] = (uint32_t)(read_base + i);
      cfr_result W = R;
      W.match_begin = at * stride;
      side.res[at] = W;
      for (uint64_t q = 0; q < stride; ++q) side.match[at * stride + q] = match[i * stride + q];
    }
  }
}

}  // namespace cfr

// =============================================================================== SDUST on the device
// The pre-step the reference applies before Query (CentrifugerClass.cpp:276-316; Dustmasker.hpp:106-243, 357-421): same
// scan as csrc/cfr_dust.cpp (window 64, threshold 20, alphabet ACGT + one code for everything else), one lane per read.
// Per-lane state in LDS: the window's triplets (<= 62) and the two count tables over the 125 possible triplets, a byte each.
//
// The reference keeps its "perfect intervals" in a list sorted by descending start that grows to 1711 entries on a
// homopolymer and is rescanned from the front for every window suffix.  What the scan takes from that list is (1) the
// largest score/length ratio among the entries with start >= a threshold that only moves down during one FindPerfect call,
// and (2) from the entry at the back - smallest start, inserted last - its end.  Entries live only while their start is
// inside the window, so there are at most 62 distinct starts; per start it is enough to keep the best ratio (any
// representative: every later test compares ratios by cross-multiplication) and the end of the entry inserted last.
// That is a 64-slot table indexed by start mod 64 plus a 64-bit mask of the live starts, and one FindPerfect call folds
// every live start once.  Same masks, bounded state, linear work (tests/test_gpu_dust.py compares with the literal host twin).
//
// Shape of the kernel.  A lane's scan is a chain of cheap window steps (ShiftWindow, ~60 instructions) that now and then
// (1.5 % / 0.5 % of the steps of a random read, every step of a homopolymer) runs one of two loops: trimming the suffix
// after a fifth occurrence of a triplet, and FindPerfect.  Run inline, some lane of a wave is inside one of those loops in
// a third of all steps and the other 63 wait: 600 instructions per wave and base (round 1/2: 48 -> 26 ms per 10 M reads,
// 190 ms with 2 % low-complexity reads).  So the lanes are little state machines and the WAVE decides what runs: window
// steps while at least kDustQuorum lanes are ready for one; otherwise one round of each loop for all the lanes waiting for
// it, and one round of "next read" for the lanes that have finished (reads are handed out from a global counter, so a lane
// stuck in a poly-A read costs one lane, not a wave).  Every branch of the outer loop is wave-uniform.
// Counts are bytes inside the lane's own 32-bit LDS words (bank = lane: conflict-free, and a count changes with one
// ds_add/ds_sub on the word that also returns the old value).  Bases come through an 8-byte window that is refilled one
// word ahead.  Masked stretches are merged into one pending run per lane and written when the next one starts elsewhere.
namespace cfr {

#ifndef CFR_DUST_RING
#define CFR_DUST_RING 65
#endif
#ifndef CFR_DUST_RINGLESS
#define CFR_DUST_RINGLESS 0
#endif
#ifndef CFR_DUST_RING_WORDS
#define CFR_DUST_RING_WORDS 1
#endif
struct __attribute__((packed)) U32a1 { uint32_t x; };
#ifndef CFR_DUST_BLOCK
#define CFR_DUST_BLOCK 128
#endif
constexpr int kDustBlock = CFR_DUST_BLOCK, kDustWindow = 64, kDustThreshold = 20;      // (lanes per block: 128, or 64 - one wave - for a finer fit into the LDS)
#ifndef CFR_DUST_QUORUM
#define CFR_DUST_QUORUM 32
#endif
constexpr int kDustQuorum = CFR_DUST_QUORUM;       // window steps run while this many lanes of the wave can take one
constexpr uint32_t kDustPoolHead = 16;   // u32 words before the per-lane tables: the read counter

__device__ __forceinline__ uint32_t dust_code(uint32_t ch) {
  return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
}
__device__ __forceinline__ uint64_t rotr64(uint64_t x, uint32_t r) { r &= 63u; return r ? (x >> r) | (x << (64u - r)) : x; }
__device__ __forceinline__ uint64_t rotl64(uint64_t x, uint32_t r) { r &= 63u; return r ? (x << r) | (x >> (64u - r)) : x; }

#ifdef CFR_DUST_PROF
__device__ unsigned long long dust_prof[16];
#define DUSTP(k, v) prof[k] += (unsigned long long)(v)
#define DUSTT(k) { const unsigned long long now = clock64(); prof[k] += now - tk; tk = now; }
#else
#define DUSTP(k, v)
#define DUSTT(k)
#endif
enum : int { DS_NEXT = 0, DS_STEP = 1, DS_TRIM = 2, DS_FIND = 3, DS_DONE = 4, DS_SLOW = 5 };

// Which reads hold TWO OR MORE characters that are not A, C, G or T (one is handled by the 64-triplet instantiation, see k_dust).  A wave takes 64 consecutive reads - one contiguous stretch of the
// bases - and reads it in 16-byte pieces side by side, four bytes per test.  A piece with such a character is only queued
// (LDS); the queue is worked off by all lanes together, each looking its piece's characters up in the 65 offsets of the
// stretch: with one N per 1000 bases some lane of every wave would otherwise sit in that search on every pass.
// flags: one byte per read (every byte is written); list / list_cnt: the flagged reads.
__device__ __forceinline__ uint32_t dust_nonsymbol_bytes(uint32_t w) {     // bit 7 of every byte of w that is not 'A', 'C', 'G', 'T'
  auto nz = [](uint32_t v) { return (((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u; };   // bit 7 of every non-zero byte
  return nz(w ^ 0x41414141u) & nz(w ^ 0x43434343u) & nz(w ^ 0x47474747u) & nz(w ^ 0x54545454u);
}
__global__ __launch_bounds__(256) void k_dust_flags(const uint8_t *bases, const uint64_t *offs, size_t n, uint8_t *flags, uint32_t *list,
                                                    unsigned long long *list_cnt) {
  __shared__ uint64_t s_offs[4][65];
  __shared__ uint64_t s_queue[4][128];                                       // piece number << 16 | its 16 "not a symbol" bits
  __shared__ uint32_t s_hit[4][64], s_qn[4], s_out[4][256];                  // s_out: flagged reads waiting for their place in the list
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint64_t *so = s_offs[wv], *queue = s_queue[wv];
  uint32_t *hit = s_hit[wv], *qn = &s_qn[wv], *outq = s_out[wv];
  uint32_t nout = 0;                                                         // (wave-uniform)
  auto flush_out = [&]() {                                                   // one atomic on the list's counter per ~200 flagged reads:
    if (nout) {                                                              // a counter every stretch bumps serialises the kernel
      unsigned long long at = 0;
      if (lane == 0) at = atomicAdd(list_cnt, (unsigned long long)nout);
      at = __shfl(at, 0);
      for (uint32_t e = lane; e < nout; e += 64) list[at + e] = outq[e];
      nout = 0;
    }
  };
  auto wave_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const size_t nwaves = (size_t)gridDim.x * 4;
  for (size_t r0 = ((size_t)blockIdx.x * 4 + wv) * 64; r0 < n; r0 += nwaves * 64) {
    const uint32_t cnt = (uint32_t)(n - r0 < 64 ? n - r0 : 64);
    if (lane <= cnt) so[lane] = offs[r0 + lane];
    if (lane == 0) { so[cnt] = offs[r0 + cnt]; *qn = 0; }
    hit[lane] = 0;
    wave_sync();
    const uint64_t b0 = so[0], b1 = so[cnt];
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(bases + b0) & ~(uintptr_t)15;
    const uint8_t *p0 = reinterpret_cast<const uint8_t *>(a0);
    const int64_t first = (int64_t)(p0 - bases);                             // position of the first piece's first byte (may lie below b0)
    const uint64_t pieces = b1 > b0 ? (uint64_t)(((int64_t)b1 - first) + 15) >> 4 : 0;
    auto work_off = [&]() {                                                  // the queued pieces: whose reads are they?
      wave_sync();
      const uint32_t nq = *qn;
      for (uint32_t e = lane; e < nq; e += 64) {
        const uint64_t ent = queue[e];
        uint32_t bits = (uint32_t)ent & 0xffffu;
        while (bits) {
          const int j = __ffs((int)bits) - 1;
          bits &= bits - 1;
          const int64_t pos = first + (int64_t)(16 * (ent >> 16)) + j;
          if (pos >= (int64_t)b0 && pos < (int64_t)b1) {
            uint32_t a = 0, b = cnt;                                         // the read with so[a] <= pos < so[a + 1]
            while (b - a > 1) { const uint32_t mid = (a + b) >> 1; if (so[mid] <= (uint64_t)pos) a = mid; else b = mid; }
            atomicAdd(&hit[a], 1u);
          }
        }
      }
      wave_sync();
      if (lane == 0) *qn = 0;
      wave_sync();
    };
    for (uint64_t q0 = 0; q0 < pieces; q0 += 64) {                          // (uniform trip count: the queue is worked off by everybody)
      const uint64_t q = q0 + lane;
      if (q < pieces) {
        const uint4 w = *reinterpret_cast<const uint4 *>(p0 + 16 * q);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t m = dust_nonsymbol_bytes(ws[k]);                    // bit 7 of byte j -> bit 4k + j
          bits |= (((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u)) << (4 * k);
        }
        if (bits) queue[atomicAdd(qn, 1u)] = (q << 16) | bits;
      }
      wave_sync();
      if (*qn > 64u) work_off();                                             // room for the next pass's 64
    }
    work_off();
    // the stretch's flags and its part of the list: one global atomic per stretch
    const bool mine = lane < cnt && hit[lane] >= 2u;      // one such character: still the 64-triplet instantiation's (k_dust)
    const uint64_t m = __ballot(mine);
    if (lane < cnt) flags[r0 + lane] = mine ? 1 : 0;
    if (mine) outq[nout + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)(r0 + lane);
    nout += (uint32_t)__popcll(m);
    wave_sync();                                                             // the LDS is the next stretch's
    if (nout > 192u) flush_out();
  }
  wave_sync();
  flush_out();
}

// The screen in front of k_dust<true> (round 6).  SDUST only ever masks inside a "perfect interval": L >= 2 consecutive triplets, all inside one
// window of 62, with 10 x sum_t c_t (c_t - 1) / 2 > 20 (L - 1) (Dustmasker.hpp:172-243: FindPerfect inserts nothing else), i.e.
// sum_t e(c_t) >= -1 with e(c) = c (c - 5) / 2 = -2, -3, -3, -2, 0, 3, 7, .. for c = 1, 2, 3, ..: either some triplet occurs SIX times or more in
// the interval, or EVERY kind of triplet in it occurs exactly five times - then in particular the kinds of its last two triplets do.  So a read
// in which no step of a sliding 62-triplet window sees (a) the arriving triplet's count reach 6, or (b) reach 5 while the kind of the triplet
// before it also stands at 5 or more, holds no perfect interval and is left exactly as it is by the scan.  This kernel proves that for
// ~3 of 4 reads of a genome without much repeat structure (2 LDS updates per base, nothing else) and marks them flags[read] = 2, which
// k_dust<true> skips like the reads that are not its own.  Necessary, not sufficient: the reads it leaves at 0 go through the full scan as
// before.  Triplets that hold a character other than A, C, G, T are not counted (a PURE read has at most one such character: its three
// triplets are of kinds that occur once, k_dust's placeholder - they can end no interval of the second kind and add nothing to the first).
// One lane per read; counts are bytes in the lane's own LDS words (bank = lane).
__device__ __forceinline__ void conv4(uint32_t x, uint32_t &code8, uint32_t &valid4);      // (with the search kernels below)
__global__ __launch_bounds__(256) void k_dust_screen(const uint8_t *bases, const uint64_t *offs, size_t n, uint8_t *flags) {
  __shared__ uint32_t s_cnt[16 * 256];
  const uint32_t t = threadIdx.x;
  uint32_t *cnt = s_cnt + t;
  const uint64_t total = offs[n];
  for (size_t i = (size_t)blockIdx.x * 256 + t; i < n; i += (size_t)gridDim.x * 256) {
    if (flags[i] != 0) continue;
    const uint64_t o0 = offs[i], o1 = offs[i + 1];
    const uint32_t len = (uint32_t)(o1 - o0);
    if (len < 7u) { flags[i] = 2; continue; }                  // fewer than five triplets
#pragma unroll
    for (int e = 0; e < 16; ++e) cnt[e * 256] = 0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(bases + o0);
    const uint8_t *al = reinterpret_cast<const uint8_t *>(a & ~(uintptr_t)3);
    const uint32_t skip = (uint32_t)(a & 3u), nbytes = skip + len;
    const int64_t al_pos = (int64_t)o0 - (int64_t)skip;        // (up to 3 bytes below the buffer's start when the caller's pointer is not 4-byte aligned: signed)
    // 2-bit codes of the last 64 bases (newest in the low bits of lo) and which of them are not symbols (bit d: the base d back)
    uint64_t lo = 0, hi = 0, inv = ~0ull;
    bool hit = false;
    for (uint32_t off = 0; off < nbytes && !hit; off += 16) {
      uint32_t w[4];
      if (al_pos >= 0 && (uint64_t)al_pos + off + 16 <= total) {
        const ulonglong2 x = ld16(al + off);
        w[0] = (uint32_t)x.x; w[1] = (uint32_t)(x.x >> 32); w[2] = (uint32_t)x.y; w[3] = (uint32_t)(x.y >> 32);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = al_pos + (int64_t)(off + 4u * q) < (int64_t)total ? *reinterpret_cast<const uint32_t *>(al + off + 4 * q) : 0u;   // (the aligned word, like k_dust's refills)
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t code8, valid4;
        conv4(w[q], code8, valid4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t b = off + 4u * q + k;
          if (b >= skip && b < nbytes) {
            // the triplet that leaves the window of 62: the one that ends 62 bases before this one
            const uint32_t old_kind = (uint32_t)(hi >> 58) & 63u, old_bad = (uint32_t)(inv >> 61) & 7u;
            atomicSub(&cnt[(old_kind >> 2) * 256], old_bad ? 0u : 1u << (8u * (old_kind & 3u)));
            hi = (hi << 2) | (lo >> 62);
            lo = (lo << 2) | ((code8 >> (2 * k)) & 3u);
            inv = (inv << 1) | (((valid4 >> k) & 1u) ^ 1u);
            const uint32_t kind = (uint32_t)lo & 63u, bad = (uint32_t)inv & 7u, sh = 8u * (kind & 3u);
            const uint32_t before = (atomicAdd(&cnt[(kind >> 2) * 256], bad ? 0u : 1u << sh) >> sh) & 0xffu;
            if (!bad && before >= 4u) {                      // (a few per cent of the steps of a random read)
              const uint32_t pk = (uint32_t)(lo >> 2) & 63u;                                   // the triplet before this one
              const bool prev_five = !((inv >> 1) & 7u) && ((cnt[(pk >> 2) * 256] >> (8u * (pk & 3u))) & 0xffu) >= 5u;
              hit = hit || before >= 5u || prev_five;
            }
          }
        }
      }
    }
    if (!hit) flags[i] = 2;
  }
}

// PURE: the instantiation for reads of A, C, G, T with at most one other character (flags[read] == 0) - 64 possible triplets instead of 125, 193 bytes of
// LDS per lane instead of 319: three waves per SIMD instead of two.  The other instantiation takes the flagged reads.
template <bool PURE>
__global__ __launch_bounds__(kDustBlock) void k_dust(uint8_t *bases, const uint64_t *offs, size_t n, uint32_t *perfect_pool, uint32_t pool_block0,
                                                     const uint8_t *flags, const uint32_t *list, const unsigned long long *list_cnt) {
  // ring: 65 bytes per lane (one add per address; the odd stride spreads the lanes over the banks, and the kernel is bound
  // by its VALU instructions, not by LDS cycles).  counts: triplet e owns the 16-bit half (e & 1) of the lane's word
  // (e >> 1): low byte = count in the window (cw), high byte = count in the suffix (cv), so that ShiftWindow's two updates of
  // a triplet are ONE ds_add / ds_sub that also returns both old counts.
  constexpr int kCntWords = PURE ? 32 : 63;
  __shared__ uint32_t s_cnt[kCntWords * kDustBlock];
  // PURE keeps NO ring (round 4): the triplets of the window are the read's own bases, three per triplet, and the read is 150 bytes that sit
  // in the vector cache - a window entry is recomputed from an (unaligned) 4-byte load of the read where the other instantiation reads
  // its ring.  Without the ring a lane needs 128 instead of 193 bytes of LDS: 9 blocks per CU instead of 6.
  constexpr bool kRingless = PURE && CFR_DUST_RINGLESS;
  // (round 5) the ring is laid out by WORDS across the lanes - byte q of lane t at ((q >> 2) * 128 + t) * 4 + (q & 3) - so that a lane's
  // bytes all sit in the lane's own bank whatever entry it is at: the lanes of a wave stand at different ring positions, and with one
  // 65-byte stretch per lane (rounds 2-4) their accesses fell on each other's banks (SQ_LDS_BANK_CONFLICT / SQ_ACTIVE_INST_LDS = 0.42).
  __shared__ __attribute__((aligned(16))) uint8_t s_ring[kRingless ? 4 : (CFR_DUST_RING_WORDS ? 64 : CFR_DUST_RING) * kDustBlock];
  __shared__ uint8_t s_code[256];
  const uint32_t t = threadIdx.x;
  for (uint32_t ch = t; ch < 256; ch += kDustBlock) s_code[ch] = (uint8_t)dust_code(ch);
  __syncthreads();
  uint8_t *ring = s_ring + (kRingless ? 0 : CFR_DUST_RING_WORDS ? 4 * t : CFR_DUST_RING * t);
  uint32_t ns_pos = 0xffffffffu;        // kRingless: where the read's one non-symbol stands (a triplet that covers it is the placeholder)
  uint32_t *cnt = s_cnt + t;
  auto li = [](int e) { return CFR_DUST_RING_WORDS ? ((e >> 2) * (kDustBlock * 4)) | (e & 3) : e; };
  unsigned long long *next_read = reinterpret_cast<unsigned long long *>(perfect_pool) + (PURE ? 0 : 1);   // one counter per instantiation
  uint32_t *pf = perfect_pool + kDustPoolHead + ((size_t)(pool_block0 + blockIdx.x) * kDustBlock + t) * 64;   // slot (start & 63): score << 8 | (end - start)

  // the suffix count of triplet e goes up / down by one (on == false: by zero - no branch, so that several updates can be in
  // flight together); returns the old count
  // PURE also takes the reads with exactly ONE character that is not A, C, G or T (k_dust_flags counts them): the three triplets
  // that contain it are of three different kinds that occur nowhere else in the read, so each of them has count 1 while it is in
  // the window or the suffix - it adds nothing to any score, never reaches the trim level, is never the triplet a trim looks for,
  // and only counts as a position.  Such a triplet is kept in the ring as kDustPlaceholder and has no counter: every update of
  // it is an update by zero, and the count it reports is the one it would have (0 before an add, 1 before a removal).
  constexpr int kDustPlaceholder = 64;
  auto cv_add_if = [&](int e, bool on) -> int {
    const bool ph = PURE && e >= kDustPlaceholder;
    const uint32_t sh = ((uint32_t)e & 1u) * 16u + 8u;
    const int old = (int)((atomicAdd(&cnt[((PURE ? e & 63 : e) >> 1) * kDustBlock], on && !ph ? 1u << sh : 0u) >> sh) & 0xffu);
    return ph ? 0 : old;
  };
  auto cv_sub_if = [&](int e, bool on) -> int {
    const bool ph = PURE && e >= kDustPlaceholder;
    const uint32_t sh = ((uint32_t)e & 1u) * 16u + 8u;
    const int old = (int)((atomicSub(&cnt[((PURE ? e & 63 : e) >> 1) * kDustBlock], on && !ph ? 1u << sh : 0u) >> sh) & 0xffu);
    return ph ? 1 : old;
  };
  auto cv_dec_if = [&](int e, bool on) {
    const bool ph = PURE && e >= kDustPlaceholder;
    atomicSub(&cnt[((PURE ? e & 63 : e) >> 1) * kDustBlock], on && !ph ? 0x100u << (((uint32_t)e & 1u) * 16u) : 0u);
  };

  // ---- lane state (positions are offsets inside the read: a read is shorter than 4 G bases)
  int st = DS_NEXT;
  uint8_t *s = nullptr;                 // the read
  uint32_t len = 0, seg_i = 0, seg_end = 0, next_i = 0, pos = 0, ok_until = 0;
  // the next `have` bytes of the read (s[pos] lowest) and the aligned 32-bit word after them, fetched one refill ahead;
  // refills happen for the whole wave every fourth window step: 5 <= have <= 8 after one while the read has more
  uint64_t buf = 0;
  uint32_t pend = 0, have = 0, c_next = 4;
  const uint8_t *s_al = nullptr;        // s rounded down to 4 bytes
  uint32_t fetch_off = 0, end_off = 0;  // offsets from s_al: the word after pend, the end of the read
  int head = 0, tail = 0, rw = 0, rv = 0, lv = 0, tr = 0, old_nx = 0;
  uint32_t d1x25 = 0, d0x5 = 0;
  uint32_t since_ns = 3;                // PURE: characters since the read's non-symbol (3 = none among the last three)
  uint64_t wb0 = 0, wb1 = 0, wb2 = 0;   // kRingless: 2-bit codes of the last 96 bases, newest in the low bits of wb0
  uint64_t live = 0;                    // bit (start & 63): a perfect interval with that start is alive
  uint32_t base = 0;                    // every live start is in [base, base + 63] (relative to the segment): the window start
                                        // of the last step, ws_of(wf - 1) before the step at wf; set where it is used
  int32_t run_lo = 0, run_hi = -1;      // pending masked stretch (relative to the segment, inclusive); empty when hi < lo
  uint32_t it = 0;                      // window steps of this wave
  // the read after this one (0: none fetched, 1: fetched, 2: there is none) and the wave's chunk of reads
  int nx_state = 0;
  uint8_t *nx_s = nullptr;
  uint32_t nx_len = 0, nx_w0 = 0, nx_w1 = 0, nx_w2 = 0;
  size_t wq_base = 0;
  uint32_t wq_cnt = 0, wq_used = 0, wq_pick = 0;
  bool wq_end = false;
  uint64_t ocache = 0, oend = 0;        // where the chunk's read of this lane starts and ends
#ifdef CFR_DUST_PROF
  unsigned long long prof[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tk = clock64();
#endif

  auto size = [&]() { return (tail - head) & 63; };
  // the triplet that ends at base P of the read (P - 2 >= the segment's start), from the bases themselves
  // (round 5) ... kept where the lane has them at hand: the 2-bit codes of the last 96 bases in three registers (wb2:wb1:wb0, the base at
  // `pos` in the low two bits of wb0) - the triplet that ends at base P is the six bits at offset 2 (pos - P).  Round 4 recomputed a window
  // entry from a 4-byte load of the read (slower than the ring: 11.8 against 10.1 ms per 10 M reads even at 9 blocks per CU).
  auto trip_at = [&](uint32_t P) -> int {
    const uint32_t b = 2u * (pos - P);                                        // < 192 - 6: the window and the few entries the rounds look at beyond it
    const uint32_t wi = b >> 6, sh = b & 63u;
    const uint64_t m0 = wi == 0u ? ~0ull : 0ull, m1 = wi == 1u ? ~0ull : 0ull, m2 = wi == 2u ? ~0ull : 0ull;     // (masks, not selects of registers:
    const uint64_t lo = (wb0 & m0) | (wb1 & m1) | (wb2 & m2), hi = (wb1 & m0) | (wb2 & m1);                      //  the compiler made an array in scratch of those)
    const int t6 = (int)(((lo >> sh) | (sh ? hi << (64u - sh) : 0ull)) & 63ull);
    return ns_pos - (P - 2u) <= 2u ? 64 : t6;                                 // (64 = kDustPlaceholder, declared below)
  };
  auto at = [&](int q) -> int {
    if (kRingless) {                                 // entry q of the window: the last one ends at the base just taken
      const int32_t P = (int32_t)pos - (((tail - head) & 63) - 1 - q);              // (the rounds also ask for a few entries outside the window
      return trip_at(P < 2 ? 2u : (uint32_t)P);                                      //  whose values they do not use: never in front of the read)
    }
    return ring[li((head + q) & 63)];
  };
  auto write_run = [&]() {
    uint8_t *w = s + seg_i;
    for (int32_t p = run_lo; p <= run_hi; ++p) w[p] = 'N';
    run_hi = -1;
    run_lo = 0;
  };
  auto mask_add = [&](int32_t lo, int32_t hi) {
    if (run_hi >= run_lo && lo <= run_hi + 1 && lo >= run_lo) { if (hi > run_hi) run_hi = hi; }
    else { write_run(); run_lo = lo; run_hi = hi; }
  };
  auto ws_of = [](uint32_t wf) { return (wf > 63u ? wf : 63u) - 63u; };     // first position of the window that ends at wf
  auto flush_before = [&](uint32_t ws) {                   // Dustmasker::SaveMaskedRegions (:141-167)
    if (live) {
      uint64_t rot = rotr64(live, base);                    // bit p: start base + p
      const uint32_t smin = base + (uint32_t)__ffsll((long long)rot) - 1u;
      if (smin < ws) {
        // the entry at the back of the reference's list: smallest start, inserted last -> its end
        const uint32_t e = pf[smin & 63];
        mask_add((int32_t)smin, (int32_t)(smin + (e & 0xffu)));
        const uint32_t drop = ws - base;                    // every start below ws leaves the list
        rot = drop >= 64 ? 0ull : rot & ~((1ull << drop) - 1ull);
        live = rotl64(rot, base);
      }
    }
    base = ws;
  };
  auto word_at = [&](uint32_t off) -> uint32_t { return off < end_off ? *reinterpret_cast<const uint32_t *>(s_al + off) : 0u; };
  auto open_at = [&](uint32_t p) {                          // the byte window starts at s[p]
    const uintptr_t a = reinterpret_cast<uintptr_t>(s);
    s_al = reinterpret_cast<const uint8_t *>(a & ~(uintptr_t)3);
    const uint32_t lead = (uint32_t)(a & 3u);
    end_off = lead + len;
    const uint32_t o = (lead + p) & 3u, w = (lead + p) & ~3u;
    buf = ((uint64_t)word_at(w) | ((uint64_t)word_at(w + 4) << 32)) >> (8u * o);
    have = 8u - o;
    pend = word_at(w + 8);
    fetch_off = w + 12;
    c_next = s_code[(uint32_t)buf & 0xffu];
  };
  // after the step at pos: FindPerfect wanted?  otherwise on to the next position
  // FindPerfect (Dustmasker.hpp:172-243) changes something only when some suffix of the window - q .. end, size - q triplets - has a
  // score above threshold x (size - q - 1) / 10 = 2 (size - q - 1).  fp_ub is an upper bound of  max over q of  score(q) - 2 (size - q - 1):
  // a step that appends a triplet whose count in the window was a raises every suffix's score by at most a and its allowance by 2,
  // and the new one-triplet suffix stands at 0; a triplet that leaves the front only takes the longest suffix with it.  While the
  // bound is not positive the call would walk its suffixes, find none above the line and put the counts back: it is skipped
  // (on random reads the call condition rw > 2 lv holds in 0.5 % of the steps and the bound is positive in a tenth of those).
  int fp_ub = 0;
  auto after_trim = [&]() {
    static_assert(kDustThreshold == 20, "rw * 10 > lv * threshold is written as rw > 2 lv");
    if (rw > 2 * lv && fp_ub > 0) st = DS_FIND;
    else { ++pos; st = DS_STEP; }
  };

  auto top_up = [&]() {
    if (have <= 4u) {
      buf |= (uint64_t)pend << (8u * have);
      have += 4u;
      pend = word_at(fetch_off);
      fetch_off += 4u;
    }
  };
  // Dustmasker::ShiftWindow (:106-138) for the triplet tr at the end of the window, then what the position needs next
  auto shift_window = [&]() {
    // straight-line on purpose: both count updates are issued before either result is looked at (one LDS round trip per
    // step).  A window that is not full yet "removes" nothing: an add of zero to the word of whatever old_nx holds.
    const bool full = size() >= kDustWindow - 2;
    const int old = old_nx;                             // ring[head], read at the end of the previous shift
    const int nh = full ? (head + 1) & 63 : head;
    const bool both = full && lv > ((tail - nh) & 63);  // the suffix is the whole window: the triplet leaves it too
    const uint32_t sho = ((uint32_t)old & 1u) * 16u, sht = ((uint32_t)tr & 1u) * 16u;
    const bool old_ph = PURE && old >= kDustPlaceholder, tr_ph = PURE && tr >= kDustPlaceholder;
    uint32_t o = atomicSub(&cnt[((PURE ? old & 63 : old) >> 1) * kDustBlock], full && !old_ph ? (both ? 0x101u : 0x1u) << sho : 0u) >> sho;
    if (old_ph) o = 0x0101u;                            // (a placeholder leaves with count 1 in window and suffix)
    if (!kRingless) ring[li(tail)] = (uint8_t)tr;
    uint32_t a = atomicAdd(&cnt[((PURE ? tr & 63 : tr) >> 1) * kDustBlock], tr_ph ? 0u : 0x101u << sht) >> sht;
    if (tr_ph) a = 0u;
    if (!kRingless) old_nx = ring[li(nh)];              // after this shift's write: valid whenever the window is not empty
    head = nh;
    tail = (tail + 1) & 63;
    if (kRingless && ((tail - head) & 63) >= kDustWindow - 2) {                     // the front of a full window: what the next step removes -
      const uint32_t Pf = pos - (uint32_t)(kDustWindow - 3);                         // a fixed place in the registers (bits 122 .. 127)
      old_nx = ns_pos - (Pf - 2u) <= 2u ? 64 : (int)((wb1 >> 58) & 63ull);
    }
    rw += (int)(a & 0xffu) - (full ? (int)(o & 0xffu) - 1 : 0);
    fp_ub += (int)(a & 0xffu) - 2;
    fp_ub = fp_ub > 0 ? fp_ub : 0;
    const int cvt = (int)((a >> 8) & 0xffu);
    rv += cvt - (both ? (int)((o >> 8) & 0xffu) - 1 : 0);
    lv += both ? 0 : 1;
    if ((cvt + 1) * 10 > 2 * kDustThreshold) st = DS_TRIM;
    else after_trim();
  };
  auto take_base = [&](uint32_t c) {                         // the byte window moves on; tr = the triplet that ends at pos
    buf >>= 8;
    --have;
    c_next = s_code[(uint32_t)buf & 0xffu];                  // looked up one step ahead of its use
    if (PURE) {                                              // 6 bits: the last three of four symbols
      if (kRingless) { wb2 = (wb2 << 2) | (wb1 >> 62); wb1 = (wb1 << 2) | (wb0 >> 62); wb0 = (wb0 << 2) | (uint64_t)(c & 3u); }
      if (c == 4u) ns_pos = pos;
      since_ns = c == 4u ? 0u : (since_ns < 3u ? since_ns + 1u : 3u);
      const uint32_t t6 = ((d0x5 << 2) | (c & 3u)) & 63u;    // (d0x5 holds the last two symbols, 4 bits)
      tr = since_ns < 3u ? kDustPlaceholder : (int)t6;
      d0x5 = t6 & 15u;
    } else {
      tr = (int)(d1x25 + d0x5 + c);                          // dense form of the reference's 9-bit triplet
      d1x25 = d0x5 * 5u;
      d0x5 = c * 5u;
    }
  };
  // one position with everything that can happen at it (the window steps below take the common case themselves)
  auto full_step = [&]() {
    if (pos >= seg_end) { st = DS_NEXT; return; }           // the next-segment round closes this one
    const uint32_t c = c_next;
    if (c == 4u && pos >= ok_until) {
      // a run of non-symbols starts here: where does it end?  (cfr_dust.cpp dust_mask: leading runs are skipped, a
      // run of more than 64 or one that reaches the end of the read closes the segment before it)
      uint32_t r = pos + 1;
      {                                                         // first through the bytes already in the window (an isolated N ends there)
        uint64_t bb = buf >> 8;
        uint32_t hv = have - 1u;
        while (hv && r < len && s_code[(uint32_t)bb & 0xffu] == 4u) { ++r; bb >>= 8; --hv; }
        if (!hv) while (r < len && s_code[s[r]] == 4u) ++r;
      }
      if (r >= len) { seg_end = pos; next_i = len; return; }
      if (pos == seg_i) { seg_i = r; pos = r; ok_until = r; open_at(r); return; }
      if (r - pos > (uint32_t)kDustWindow) { seg_end = pos; next_i = r; return; }
      ok_until = r;
    }
    take_base(c);
    const uint32_t wf = pos - seg_i;
    if (wf < 2) { ++pos; return; }
    base = ws_of(wf - 1);
    flush_before(ws_of(wf));
    shift_window();
  };

  for (;;) {
    // ================================================================= window steps while the wave is mostly ready for one
    for (;;) {
      const int ready = __popcll(__ballot(st == DS_STEP));
      if (ready == 0) break;
      if ((it++ & 3u) == 0u) top_up();                       // every lane, whatever its state: the invariant is per lane
      DUSTP(0, 1); DUSTP(1, ready);
      if (st == DS_STEP) {
        const uint32_t c = c_next, wf = pos - seg_i;
        bool slow = (c == 4u && pos >= ok_until) || wf < 2u;
        if (live != 0ull && wf >= 2u) {                        // does an interval leave the window?
          const uint32_t b0 = ws_of(wf - 1);
          slow |= b0 + (uint32_t)__ffsll((long long)rotr64(live, b0)) - 1u < ws_of(wf);
        }
        if (pos >= seg_end) st = DS_NEXT;
        else if (slow) st = DS_SLOW;
        else {
          take_base(c);
          shift_window();
        }
      }
      if (ready < kDustQuorum) break;                        // one step for the few, then look after the others
    }
    DUSTT(10);
    if (__ballot(st == DS_SLOW)) {
      DUSTP(2, 1); DUSTP(3, __popcll(__ballot(st == DS_SLOW)));
      if ((it++ & 3u) == 0u) top_up();                       // a round that takes a base counts like a window step
      if (st == DS_SLOW) { st = DS_STEP; full_step(); }
    }
    DUSTT(11);
    if (__ballot(st == DS_TRIM)) {
      DUSTP(4, 1); DUSTP(5, __popcll(__ballot(st == DS_TRIM)));
      if (st == DS_TRIM) {
        // the suffix loses its front up to and including the first occurrence of tr (it has five): four ring entries and
        // four count updates in flight at a time - one LDS round trip per four entries instead of two per entry
        for (;;) {
          const int p0 = size() - lv;
          int q[4], o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) q[j] = at(p0 + j);      // tr is among the lv entries of the suffix: what lies behind is never taken
          const int hit = q[0] == tr ? 0 : q[1] == tr ? 1 : q[2] == tr ? 2 : q[3] == tr ? 3 : 4;
          const int take = hit < 4 ? hit + 1 : 4;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = cv_sub_if(q[j], j < take);
#pragma unroll
          for (int j = 0; j < 4; ++j) rv -= j < take ? o[j] - 1 : 0;
          lv -= take;
          if (hit < 4) break;
        }
        after_trim();
      }
    }
    DUSTT(12);
    if (__ballot(st == DS_FIND)) {
      DUSTP(6, 1); DUSTP(7, __popcll(__ballot(st == DS_FIND)));
      if (st == DS_FIND) {
        // Dustmasker::FindPerfect (:172-243); base == ws here, so start ws + q sits at bit q of the rotated mask
        base = ws_of(pos - seg_i);
        int rvl = rv, max_score = 0, max_cnt = 1;
        uint64_t unfolded = rotr64(live, base);                // live starts whose ratio has not entered (max_score, max_cnt) yet
        uint64_t fresh = 0;                                    // starts inserted by this call (already in the maximum)
        const int first = size() - lv - 1;
        // a suffix qualifies when its score rvl exceeds threshold x its triplet count; rvl never exceeds the whole window's
        // score rw, and the count only grows as q moves down: once threshold x count >= 10 rw no further start can qualify
        // (the reference's loop runs on to q = 0 without effect).  For a random window rw ~ 30: 15 iterations instead of 45.
        // threshold x (size - q - 1) >= 10 rw  <=>  q <= size - 1 - ceil(rw / 2): the loop covers q = first .. q_end + 1
        int q_end = size() - 1 - ((rw * 10 + kDustThreshold - 1) / kDustThreshold);
        if (q_end > first) q_end = first;
        if (q_end < -1) q_end = -1;
        for (int q0 = first; q0 > q_end; q0 -= 4) {
          int x[4], o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = at(q0 - j);
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = cv_add_if(x[j], q0 - j > q_end);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = q0 - j;
            if (q > q_end) {
              const int triplets = size() - q - 1;
              rvl += o[j];
              if (rvl * 10 > kDustThreshold * triplets) {
                // the entries with start >= ws + q, largest start first
                while (unfolded >> q) {
                  const int p = 63 - __clzll((long long)unfolded);
                  unfolded &= ~(1ull << p);
                  const uint32_t e = pf[(base + (uint32_t)p) & 63];
                  const int sc = (int)(e >> 8), cn = (int)(e & 0xffu) - 2;       // span of the interval = end - start - 2
                  if ((uint64_t)(int64_t)sc * (uint64_t)(int64_t)max_cnt > (uint64_t)(int64_t)max_score * (uint64_t)cn) { max_score = sc; max_cnt = cn; }
                }
                if (rvl * max_cnt >= max_score * triplets) {
                  max_score = rvl;
                  max_cnt = triplets;
                  pf[(base + (uint32_t)q) & 63] = ((uint32_t)rvl << 8) | (uint32_t)(size() + 1 - q);   // end - start = size + 1 - q
                  fresh |= 1ull << q;
                }
              }
            }
          }
        }
        live |= rotl64(fresh, base);
        for (int q0 = first; q0 > q_end; q0 -= 4) {
          int x[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = at(q0 - j);
#pragma unroll
          for (int j = 0; j < 4; ++j) cv_dec_if(x[j], q0 - j > q_end);
        }
        ++pos;
        st = DS_STEP;
      }
    }
    DUSTT(13);
    if (__ballot(st == DS_NEXT)) {
      DUSTP(8, 1); DUSTP(9, __popcll(__ballot(st == DS_NEXT)));
      if (st == DS_NEXT) {
        // ---- end of the segment the lane comes from: the intervals still alive, then the pending stretch
        if (live) {
          const uint32_t m = pos - seg_i;                      // >= 3: something was found
          base = ws_of(m - 1);
          uint32_t ws = ws_of(m);
          while (live) { flush_before(ws); ++ws; }
        }
        if (run_hi >= run_lo) write_run();
        bool start = false;
        if (next_i < len) {                                    // the read goes on behind a long run of non-symbols (rare)
          seg_i = next_i;
          open_at(seg_i);
          start = true;
        } else if (nx_state == 1) {                            // the read fetched while the previous one was scanned
          s = nx_s;
          len = nx_len;
          seg_i = 0;
          const uintptr_t a = reinterpret_cast<uintptr_t>(s);
          s_al = reinterpret_cast<const uint8_t *>(a & ~(uintptr_t)3);
          const uint32_t lead = (uint32_t)(a & 3u);
          end_off = lead + len;
          buf = ((uint64_t)nx_w0 | ((uint64_t)nx_w1 << 32)) >> (8u * lead);
          have = 8u - lead;
          pend = nx_w2;
          fetch_off = 12;
          c_next = s_code[(uint32_t)buf & 0xffu];
          nx_state = 0;
          start = true;
        } else if (nx_state == 2) st = DS_DONE;                // no read left; (state 0: wait for the fetch below)
        if (start) {
          pos = seg_i;
          ok_until = seg_i;
          seg_end = len;
          next_i = len;
#pragma unroll
          for (int e = 0; e < kCntWords; ++e) cnt[e * kDustBlock] = 0;
          head = tail = rw = rv = lv = 0;
          fp_ub = 0;
          if (seg_i == 0) ns_pos = 0xffffffffu;
          d1x25 = d0x5 = 0;
          since_ns = 3;
          live = 0;
          base = 0;
          run_lo = 0;
          run_hi = -1;
          // the first two bases only feed the running triplet (the reference starts its scan at the third); symbols
          // as a rule - anything else goes the long way
          const uint32_t c1 = s_code[(uint32_t)(buf >> 8) & 0xffu];
          if (len - seg_i >= 2u && c_next != 4u && c1 != 4u) {
            if (PURE) { d0x5 = (c_next << 2) | c1; wb0 = (uint64_t)d0x5; wb1 = 0; wb2 = 0; }
            else { d1x25 = c_next * 25u; d0x5 = c1 * 5u; }
            buf >>= 16;
            have -= 2u;
            c_next = s_code[(uint32_t)buf & 0xffu];
            pos = seg_i + 2u;
          }
          top_up();
          st = DS_STEP;
        }
      }
      // ---- every lane without a fetched read gets one: indices from the wave's chunk of 64 consecutive reads (one global
      // atomic per chunk), their offsets from the chunk's offsets held one per lane, the first three words of the bases
      // loaded now and used a read later.  All lanes take part in the shuffles.
      const bool want = nx_state == 0;
      const uint64_t m_want = __ballot(want);
      if (m_want) {
        const int lane = (int)(t & 63u);
        if (wq_used == wq_cnt) {
          unsigned long long first = 0;
          if (lane == 0) first = atomicAdd(next_read, 64ull);
          wq_base = (size_t)__shfl(first, 0);
          // PURE: the unflagged reads among 64 consecutive ones; otherwise 64 entries of the list of flagged reads (or, without
          // a list, 64 consecutive reads whatever they hold)
          const size_t total = PURE || !list ? n : (size_t)*list_cnt;
          wq_end = wq_base >= total;
          const bool in = wq_base + (size_t)lane < total;
          const size_t rd = !in ? 0 : (PURE || !list ? wq_base + (size_t)lane : (size_t)list[wq_base + (size_t)lane]);
          const bool mine = in && !(PURE && flags[rd] != 0);
          const uint64_t m_mine = __ballot(mine);              // the reads of the chunk that are this instantiation's
          wq_cnt = (uint32_t)__popcll(m_mine);
          wq_used = 0;
          // lane j learns which read of the chunk is the j-th of them: every lane pushes its own index - the lanes whose
          // read is ours to the front in order, the others to the back (a permutation: nobody collides)
          const uint64_t below = (1ull << lane) - 1ull;
          const uint32_t dst = mine ? (uint32_t)__popcll(m_mine & below) : 63u - (uint32_t)__popcll(~m_mine & below);
          wq_pick = (uint32_t)__builtin_amdgcn_ds_permute((int)(4u * dst), lane);
          ocache = mine ? offs[rd] : 0ull;
          oend = mine ? offs[rd + 1] : 0ull;
        }
        const uint32_t rank = (uint32_t)__popcll(m_want & ((1ull << lane) - 1ull)), avail = wq_cnt - wq_used;
        const uint32_t k = (uint32_t)__shfl((int)wq_pick, (int)((wq_used + rank) & 63u));   // the lane's read inside the chunk, if it gets one
        const uint64_t o0 = __shfl(ocache, (int)(k & 63u));
        const uint64_t o1 = __shfl(oend, (int)(k & 63u));
        if (want) {
          if (rank < avail) {
            nx_s = bases + o0;
            nx_len = (uint32_t)(o1 - o0);
            const uintptr_t a = reinterpret_cast<uintptr_t>(nx_s);
            const uint8_t *al = reinterpret_cast<const uint8_t *>(a & ~(uintptr_t)3);
            const uint32_t e_off = (uint32_t)(a & 3u) + nx_len;
            nx_w0 = 0u < e_off ? *reinterpret_cast<const uint32_t *>(al) : 0u;
            nx_w1 = 4u < e_off ? *reinterpret_cast<const uint32_t *>(al + 4) : 0u;
            nx_w2 = 8u < e_off ? *reinterpret_cast<const uint32_t *>(al + 8) : 0u;
            nx_state = 1;
          } else if (wq_end) nx_state = 2;                       // the chunk lies behind the last read
        }
        const uint32_t asked = (uint32_t)__popcll(m_want);
        wq_used += asked < avail ? asked : avail;
      }
    }
    DUSTT(14);
    if (!__ballot(st != DS_DONE)) break;
  }
#ifdef CFR_DUST_PROF
  if ((t & 63u) == 0) for (int k = 0; k < 16; ++k) atomicAdd(&dust_prof[k], prof[k]);
#endif
}

}  // namespace cfr

// =============================================================================== text-mode tables
namespace cfr {
// SA / ISA / text from the BWT alone: every row points to its LF image (the row of the suffix one position to the left);
// the row of text position 0 (firstISA) is the end of that list, and a row's text position is its distance to the end.
// List ranking by RULERS instead of pointer doubling over all rows: every kRulerStep-th row is a ruler; (1) each ruler
// walks LF to the next ruler and records (next ruler, steps) [k_ruler_walk]; (2) the ruler list (n / kRulerStep elements)
// is ranked by pointer jumping [k_ruler_jump]; (3) each ruler walks its stretch again and writes SA, ISA and the text
// symbol of every row it passes [k_ruler_fill].  2n dependent occ gathers in total, no n-sized temporaries, any n.
constexpr uint32_t kRulerShift = 8;                       // a ruler every 256 rows: walks of 256 steps on average (every 64: ranking the rulers was 0.9 of the
                                                          // 4.5 s at 40 Gbp and 15 GB of temporaries; every 1024: no better at 8 Gbp, worse at 1)

// LF(i) on the flat occ image and the symbol B[i] (FMIndex.hpp:382-386); i != firstISA
__device__ __forceinline__ uint64_t lf_step(const DevView &v, uint64_t i, uint32_t &sym) {
  if (v.prot.enabled) {
    const uint32_t c = prot_access(v.prot, i);
    sym = c;
    return v.prot.C[c] + prot_rank(v.prot, c, i, 1) + fm_fix(v, c, i, 1) - 1;
  }
  const uint64_t *rec = occ_rec(v, i);
  const uint32_t h = ((uint32_t)i >> 6) & 1u, j = (uint32_t)i & 63u;
  const ulonglong2 pl = ld16(rec + 4 + 2 * h);
  const uint32_t c = (uint32_t)((pl.x >> j) & 1u) | ((uint32_t)((pl.y >> j) & 1u) << 1);
  sym = c;
  return v.C[c] + occ_count(rec[c], pl.x, pl.y, c, i, 1) + fm_fix(v, c, i, 1) - 1;
}

// ruler k = row k << kRulerShift (k < nrulers); element nrulers is the terminal (the row of text position 0, the end of the
// list), element nrulers + 1 the HEAD of the list: the row of text position n-1, which no LF step leads to, so the rows
// between it and the first ruler would otherwise belong to nobody's stretch.  That row is C[last symbol]: the one-character
// suffix sorts first among the suffixes that start with it (what FMIndex::Rank's fix-up skips, FMIndex.hpp:352-362).
__device__ __forceinline__ uint64_t ruler_row(const DevView &v, uint64_t nrulers, uint64_t k) {
  return k < nrulers ? k << kRulerShift : (v.prot.enabled ? v.prot.C[v.last_code] : v.C[v.last_code]);
}
__global__ void k_ruler_walk(DevView v, uint64_t nrulers, uint32_t *next, uint64_t *dist) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nrulers + 1; k += (uint64_t)gridDim.x * blockDim.x) {
    if (k == nrulers) { next[k] = (uint32_t)nrulers; dist[k] = 0; continue; }
    uint64_t row = ruler_row(v, nrulers, k), d = 0;
    uint32_t nx = (uint32_t)nrulers;
    while (row != v.first_isa) {
      uint32_t sym;
      row = lf_step(v, row, sym);
      ++d;
      if (row == v.first_isa) break;
      if ((row & ((1ull << kRulerShift) - 1)) == 0) { nx = (uint32_t)(row >> kRulerShift); break; }
    }
    next[k] = nx;
    dist[k] = d;
  }
}
__global__ void k_ruler_jump(uint64_t cnt, const uint32_t *next_in, const uint64_t *dist_in, uint32_t *next_out, uint64_t *dist_out) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = next_in[k];
    next_out[k] = next_in[a];
    dist_out[k] = dist_in[k] + dist_in[a];
  }
}
// pos[k] = text position of ruler k.  WIDE: 36-bit packed SA entries (the table is zero-filled: neighbours share words),
// otherwise u32.  T[SA[i]-1] = B[i]; the row of position 0 holds T[n-1].
template <bool WIDE>
__global__ void k_ruler_fill(DevView v, uint64_t nrulers, const uint64_t *pos, uint32_t *sa, unsigned long long *text) {
  // A stretch walks the text leftwards, so its 2-bit symbols fill text words from the top down: a word the stretch entered at
  // its top slot and left at its bottom one is this lane's alone and leaves as one plain store; the words at the two ends of the
  // stretch are shared with the neighbouring stretches and are OR-ed in (the text is zero-filled).
  unsigned long long acc = 0;
  uint64_t acc_w = ~0ull;                                 // word being filled (none)
  bool acc_whole = false;                                 // entered at slot 31
  auto flush = [&](bool left_at_bottom) {
    if (acc_w == ~0ull) return;
    if (acc_whole && left_at_bottom) text[acc_w] = acc;
    else atomicOr(text + acc_w, acc);
    acc_w = ~0ull;
  };
  auto put = [&](uint64_t row, uint64_t p, uint32_t sym) {
    if (WIDE) st36_zeroed(sa, row, p);
    else sa[row] = (uint32_t)p;
    const uint64_t q = p == 0 ? v.n - 1 : p - 1;
    if (v.prot.enabled) { reinterpret_cast<uint8_t *>(text)[q] = (uint8_t)sym; return; }      // protein: one byte per symbol
    const uint64_t w = q >> 5;
    const uint32_t slot = (uint32_t)q & 31u;
    if (w != acc_w) { flush(true); acc_w = w; acc = 0; acc_whole = slot == 31u; }              // (a walk only leaves a word downwards)
    acc |= (unsigned long long)sym << (2u * slot);
    if (slot == 0) flush(true);
  };
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nrulers + 1; k += (uint64_t)gridDim.x * blockDim.x) {
    if (k == nrulers) {                                   // the row of text position 0
      put(v.first_isa, 0, bwt_access(v, v.first_isa));
      flush(false);
      continue;
    }
    uint64_t row = ruler_row(v, nrulers, k), p = pos[k];
    for (;;) {
      if (row == v.first_isa) break;                       // written by the terminal element
      uint32_t sym;
      const uint64_t nrow = lf_step(v, row, sym);
      put(row, p, sym);
      row = nrow;
      --p;
      if ((row & ((1ull << kRulerShift) - 1)) == 0) break; // the next ruler writes its own stretch
    }
    flush(false);
  }
}
// ---- the step function of the locate values (steps_value above) and the locate memo from the text order.
// BackwardToSampledSA(row) walks the text leftwards from SA[row] to the first row whose value is stored: the row of text
// position 0, a selectedSA row, or a sampled row.  If every sampled row's stored value equals the value of the nearest
// "breakpoint" (position 0 or a selectedSA position) at or left of its own position, then the walk from ANY position returns
// that breakpoint's value - the first stop it meets lies between the breakpoint and the position and carries the same value.
// k_memo_check verifies the premise on every sampled row (an index for which it fails runs without text mode and gets the
// plain walk, k_build_loc_memo).  The memo is then memo[row] = steps(SA[row]): one SA read and a short search per row
// instead of ~sample_rate dependent LF steps.
// Protein index: EVERY stop of the locate walk with its text position and the value GetSampledSA returns there (branch order of
// FMIndex.hpp:203-231: firstISA, then row % rate == 0, then the end-marker rows) - the sampled rows do not follow the end-marker
// positions alone (a '$' row that is also a sampled row answers with the sequence BEFORE the '$'), so the step function is built
// from all stops, sorted by position, runs of equal values merged.  Slots that are not stops of their own get position ~0.
__global__ void k_collect_stops_prot(DevView v, uint64_t nsamp, uint64_t *pos, uint64_t *val) {
  const uint64_t total = nsamp + v.prot.endmarker_n;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t row, value;
    bool stop = true;
    if (k < nsamp) {
      row = k * v.sample_rate;
      if (row >= v.n) stop = false;
      value = row == v.first_isa ? v.adjusted_sa0 : sampled_read(v, k);
    } else {
      row = k - nsamp;
      if (row == v.first_isa || row % v.sample_rate == 0) stop = false;       // answered by an earlier branch (listed above)
      const uint64_t bit = row * v.prot.endmarker_bits;
      const uint64_t w0 = v.prot.endmarker[bit >> 6], w1 = v.prot.endmarker[(bit >> 6) + 1];
      const uint32_t sh = (uint32_t)bit & 63u;
      uint64_t x = w0 >> sh;
      if (sh) x |= w1 << (64 - sh);
      value = v.prot.endmarker_bits >= 64 ? x : (x & ((1ull << v.prot.endmarker_bits) - 1));
    }
    pos[k] = stop ? sa_entry(v, row) : ~0ull;
    val[k] = value;
  }
}
__global__ void k_gather_sa(DevView v, const uint64_t *rows, uint64_t cnt, uint64_t *pos) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < cnt) pos[k] = sa_entry(v, rows[k]);
}
__global__ void k_memo_check(DevView v, uint64_t nsamp, unsigned long long *bad) {
  unsigned long long b = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nsamp; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t row = k * v.sample_rate;
    if (row == v.first_isa) continue;                 // (GetSampledSA answers that row from adjustedSA0, not from the sample)
    if (sampled_read(v, k) != steps_value(v.steps, sa_entry(v, row))) ++b;
  }
  if (b) atomicAdd(bad, b);
}
__global__ void k_memo_fill(DevView v, uint32_t shift, uint64_t entries, uint32_t *memo) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < entries; j += (uint64_t)gridDim.x * blockDim.x)
    memo[j] = (uint32_t)steps_value(v.steps, sa_entry(v, j << shift));
}

// Self-check of the derived tables (the probe behind cfr_selfcheck_tables): for every row i - SA[i] < n (0 exactly at the row
// of text position 0), the text symbol left of SA[i] is B[i], SA[LF(i)] == SA[i] - 1 (with the first two, SA is the inverse
// of the LF list: a permutation) - and for every 61st row the direct locate (memo / SA + step function) against the plain walk.
// bad[0] = SA, bad[1] = text, bad[2] = LF order, bad[3] = locate.
__global__ void k_selfcheck(DevView v, unsigned long long *bad) {
  auto text_at = [&](uint64_t q) -> uint32_t { return v.prot.enabled ? (uint32_t)v.text8[q] : (uint32_t)(v.text2[q >> 5] >> (2 * (q & 31))) & 3u; };
  const bool tables = v.sa32 != nullptr || v.sa36 != nullptr;
  const bool direct = (v.loc_memo && v.memo_shift == 0) || (tables && v.steps.pos);
  unsigned long long b0 = 0, b1 = 0, b2 = 0, b3 = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < v.n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (tables) {
      const uint64_t p = sa_entry(v, i);
      if (p >= v.n || (p == 0) != (i == v.first_isa)) ++b0;
      else if (i == v.first_isa) {
        if (text_at(v.n - 1) != bwt_access(v, i)) ++b1;
      } else {
        uint32_t sym;
        const uint64_t lf = lf_step(v, i, sym);
        if (text_at(p - 1) != sym) ++b1;
        if (sa_entry(v, lf) != p - 1) ++b2;
      }
    }
    if (i % 61 == 0) {
      uint32_t st;
      cfr_hit H;                                        // (a one-row hit in row space)
      H.sp = i; H.ep = i; H.l = 0; H.strand = 0; H.offset = 0; H.pad = 0;
      if (direct && locate_row(v, H, i) != fm_locate<false>(v, i, st)) ++b3;
      else if (!direct && v.loc_memo && fm_locate<true>(v, i, st) != fm_locate<false>(v, i, st)) ++b3;
    }
  }
  if (b0) atomicAdd(bad + 0, b0);
  if (b1) atomicAdd(bad + 1, b1);
  if (b2) atomicAdd(bad + 2, b2);
  if (b3) atomicAdd(bad + 3, b3);
}
}  // namespace cfr

// =============================================================================== search, v2
// GetHitsFromRead (Classifier.hpp:274-293) as a per-lane state machine with ONE memory round trip per
// loop iteration.  Structure of an iteration:
//   A. land   - consume what the previous iteration loaded, according to the lane's pending op;
//   B. decide - pick the lane's next op and compute the ADDRESSES it needs (no loads inside branches);
//   C. load   - every lane issues the same fixed set of loads (7-8 instructions) from its chosen addresses,
//               lanes that need nothing in a slot point it at one shared dummy line.
// Loads are kept out of divergent branches on purpose: a load whose destination is a loop-carried register
// inside a branch makes the compiler copy it right behind the load, i.e. wait for memory inside every branch
// (measured: 65 waits, ~15 us per iteration).  With unconditional loads there is a single wait per iteration,
// so lanes in different phases of their BackwardSearch never serialise each other.
//   * read characters: a 32-character register queue of 2-bit codes + validity bits, refilled one aligned
//     16-byte block at a time (SWAR conversion) - no cache access per step, a K-mer key is one shift;
//   * derived tables: ftabx (state after the first K characters) and, for ranges of <= 4 rows deep into a
//     match, text mode: SA -> compare the read with the 2-bit text 32 bases per step -> ISA;
//   * lanes walk chains grid-stride (persistent grid); the next chain's offsets ride in two load slots.
namespace cfr {

// 4 ASCII bytes -> 4 two-bit codes (byte j -> bits 2j..2j+1) and 4 validity bits (bit j): only A,C,G,T are symbols
__device__ __forceinline__ void conv4(uint32_t x, uint32_t &code8, uint32_t &valid4) {
  uint32_t k = (x >> 1) & 0x03030303u;
  k ^= (k >> 1) & 0x01010101u;                                    // A0 C1 G2 T3 per byte
  const uint32_t b0 = k & 0x01010101u, b1 = (k >> 1) & 0x01010101u;
  const uint32_t expect = 0x41414141u + b0 * 2u + b1 * 6u + (b0 & b1) * 11u;   // 'A','C','G','T'
  const uint32_t d = x ^ expect;
  const uint32_t nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;    // high bit set where the byte differs
  const uint32_t ok = ~nz & 0x80808080u;
  valid4 = ((ok >> 7) | (ok >> 14) | (ok >> 21) | (ok >> 28)) & 0xfu;
  code8 = (k | (k >> 6) | (k >> 12) | (k >> 18)) & 0xffu;
}

// one packed block -> 16 codes / 16 validity bits in CONSUMPTION order (first consumed character on top)
__device__ __forceinline__ void conv_block(uint64_t pk, uint32_t rc, uint32_t &cw, uint32_t &vw) {
  uint32_t c = (uint32_t)pk, vv = (uint32_t)(pk >> 32) & 0xffffu;
  if (rc) {   // the reverse complement walks ascending addresses: reverse the order, complement the codes
    uint32_t r = __brev(c);
    r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
    c = ~r;
    vv = __brev(vv) >> 16;
  }
  cw = c;
  vw = vv;
}

// pre-pass: every aligned 16-byte block of a read buffer -> one u64: 16 two-bit codes (byte j -> bits 2j..2j+1) in the
// low half, 16 validity bits at 32..47.  Coalesced 16 B in / 8 B out; bytes past the end of the buffer are "not a symbol".
__global__ void k_pack_reads(const uint8_t *buf, uint64_t total, uint64_t nblocks, uint64_t *packed) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const uint64_t a = b << 4;
  uint4 x = make_uint4(0, 0, 0, 0);
  if (a + 16 <= total) x = *reinterpret_cast<const uint4 *>(buf + a);
  else {
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    for (uint64_t k = a; k < total; ++k) {
      const uint32_t by = (uint32_t)buf[k] << (8u * ((uint32_t)(k - a) & 3u));
      const uint32_t q = (uint32_t)(k - a) >> 2;
      if (q == 0) w0 |= by; else if (q == 1) w1 |= by; else if (q == 2) w2 |= by; else w3 |= by;
    }
    x = make_uint4(w0, w1, w2, w3);
  }
  uint32_t c0, c1, c2, c3, v0, v1, v2, v3;
  conv4(x.x, c0, v0); conv4(x.y, c1, v1); conv4(x.z, c2, v2); conv4(x.w, c3, v3);
  const uint32_t c = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
  const uint32_t vv = v0 | (v1 << 4) | (v2 << 8) | (v3 << 12);
  packed[b] = (uint64_t)c | ((uint64_t)vv << 32);
}

// the inverse, for a caller that hands the batch over in packed form (cfr_classify_batch_packed: 0.5 byte per base over PCIe instead of
// 1): block -> its 16 characters, "ACGT" for the symbols and 'N' for everything that was not one (what was there is gone, and nothing
// on the path tells such characters apart: a non-symbol ends a match, counts as SDUST's fifth code, reverse-complements to 'N').
// 8 B in / 16 B out per lane.
// Only the characters [from, to) (offsets from buf, the first block's first character) are written: a block that two sub-batches share
// is unpacked by each for its own characters (the first one's may have been SDUST-masked by the time the second one arrives).
__global__ void k_unpack_reads(const uint64_t *packed, uint64_t nblocks, uint8_t *buf, uint64_t from, uint64_t to) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const uint64_t pk = packed[b];
  const uint32_t c = (uint32_t)pk, vv = (uint32_t)(pk >> 32) & 0xffffu;
  uint32_t w[4];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    uint32_t x = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t k = 4u * q + j, code = (c >> (2u * k)) & 3u;
      const uint32_t ch = ((vv >> k) & 1u) ? (0x54474341u >> (8u * code)) & 0xffu : (uint32_t)'N';       // "ACGT" little endian
      x |= ch << (8u * j);
    }
    w[q] = x;
  }
  const uint64_t a = b << 4;
  if (a >= from && a + 16 <= to) *reinterpret_cast<uint4 *>(buf + a) = make_uint4(w[0], w[1], w[2], w[3]);
  else for (uint64_t k = a > from ? a : from; k < a + 16 && k < to; ++k) buf[k] = (uint8_t)(w[(k - a) >> 2] >> (8u * ((uint32_t)(k - a) & 3u)));
}

struct SearchView {
  uint64_t n, first_isa;
  uint64_t C[4];
  const uint64_t *occ, *ftab, *ftabx, *text2;
  const uint32_t *sa;                // suffix array: u32 entries (n < 2^32) or 36-bit packed entries (the WIDE instantiation); nullptr = no text mode
  uint32_t last_code, ftab_width, ftabx_width, text_min_l;
  int32_t min_hit_len;
  uint32_t wide_rows;                // ranges of up to this many rows continue on the text (0 / <= 4: only the four-row form)
  uint32_t ftabx_e8;                 // derived K-mer table with 8-byte entries (ftabx8_encode)
};

// entry k (0..3) of four consecutive 36-bit entries from a 32-byte window {w0..w3} whose first entry starts at bit `o` (< 32)
__device__ __forceinline__ uint64_t u36_at(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t o, uint32_t k) {
  const uint32_t bit = o + 36u * k, wi = bit >> 6, sh = bit & 63u;           // bit <= 136
  const uint64_t a = wi == 0 ? w0 : wi == 1 ? w1 : w2, b = wi == 0 ? w1 : wi == 1 ? w2 : w3;
  const uint64_t x = sh ? (a >> sh) | (b << (64u - sh)) : a;
  return x & 0xfffffffffull;
}

enum : uint32_t { OP_NONE = 0, OP_TABLE, OP_TABLE10, OP_EXT, OP_SA, OP_TEXT, OP_VHIT, OP_SAW, OP_TEXTW };
#ifndef CFR_TEXT_STEP
#define CFR_TEXT_STEP 48
#endif
constexpr uint32_t kTextStep = CFR_TEXT_STEP;     // characters a text-mode step compares per row (what a 16-byte gather ending at the row's word always holds)

// wide text mode: ranges of 5 .. kWideRows rows (many near-identical strains) continue on the text like the <= 4-row ranges do,
// with the rows' text positions in LDS (one u32 column per row and lane, + one byte column of high bits for n >= 2^32, + one byte
// column of matched lengths) and four rows compared per loop iteration
constexpr uint32_t kWideRows = 24, kWideRowsWide = 24;
// blocks per CU the single-end 36-bit instantiation could be compiled for.  Measured (tools/dbg/ab_minblocks.sh and the 40 Gbp runs):
// forcing 5 (96 VGPRs, 48 bytes of scratch instead of 105 VGPRs) gains 2 % on 150 bp reads at 8 Gbp, nothing at 40 Gbp, and LOSES 7 %
// on long reads at 40 Gbp (74.0 -> 79.8 ms per 312 k reads); the paired instantiations lose as well (21.2 against 20.0 ms per 10 M
// pairs).  So nothing is forced: the 32-bit single-end instantiation reaches 5 blocks on its own, the others run 4.
#ifndef CFR_SEARCH_MIN_BLOCKS
#define CFR_SEARCH_MIN_BLOCKS 1
#endif

// PROF: per-op iteration counters (CFR_SEARCH_PROF=1; a diagnostic build of the same loop, never the timed one)
// WIDE: n >= 2^32 - text positions and rows are 36-bit (packed SA entries, two 16-byte slots for the SA fetch)
// DYN: a lane that has finished a chain draws the next one from a counter (*next_ctr, zero at launch) instead of taking every
//      stride-th chain: with few chains per lane (long reads) the static hand-out leaves lanes idle behind the longest pairs
// STAGE (round 6, the two-launch form of a search: the lanes of a wave are in different states, so a wave runs every branch of the loop in
// every iteration, and the code of wide text mode - a third of the loop's vector instructions, LDS columns, loops over up to 24 rows - runs
// in nearly every wave iteration although 8 % of the lane iterations need it):
// STAGE 1: the state machine WITHOUT wide text mode (no LDS, fewer registers).  A search that reaches a range of 5 .. wide_rows rows is not
//       continued here: the chain is handed over AT THE START OF THAT SEARCH through a list of 32-byte records {byte that search starts at,
//       len | t0 << 32, index of its hit list | hits so far << kListHitBits, chain}.  Slots are drawn a chunk of kListChunk at a time with one
//       atomic per wave and chunk (one returning atomic per wave ITERATION on one address costs 11 ns each: 3 M per step, profiles/
//       r6b_ab_lookup_stage.txt); what a wave leaves of a chunk is filled with hole records (chain = ~0).
// STAGE 2: the full state machine over that list: a record is the chain's parameters (the two P slots), the first search starts at the
//       record's t0 behind the hits the first stage wrote.  raw / chain_cnt are indexed by chain, so the order of the list does not matter.
constexpr uint32_t kListChunk = 64;
// A record's third word: the index of the chain's hit list in `raw` (36 bits: 2 TB of 32-byte hits) and the hits the first stage wrote
// (28 bits).  A chain is handed over with at most len / (min_hit_len + 1) hits; the host takes the two-launch form only where that stays
// below kListCntMax for every read of the batch (`split`, where cfr_device.hip launches the search), so the kernel does not look at the count.
constexpr uint32_t kListHitBits = 36, kListCntMax = (1u << (64 - kListHitBits)) - 1u;
template <int CPR, bool PROF = false, bool WIDE = false, bool DYN = false, int STAGE = 0>
#ifndef CFR_FIRST_MIN_BLOCKS
#define CFR_FIRST_MIN_BLOCKS 5
#endif
__global__ __launch_bounds__(256, STAGE == 1 && !WIDE && CPR == 2 ? CFR_FIRST_MIN_BLOCKS : (WIDE && CPR == 2) ? CFR_SEARCH_MIN_BLOCKS : 1) void k_search_chains_v2(SearchView v, const uint64_t *packed1, const uint64_t *offs1,
                                                          const uint64_t *packed2, const uint64_t *offs2, size_t n,
                                                          uint64_t nblk1, uint64_t nblk2, const uint64_t *hit_off,
                                                          cfr_hit *raw, uint32_t *chain_cnt, unsigned long long *prof = nullptr,
                                                          unsigned long long *next_ctr = nullptr, uint32_t dyn_chunk = 1,
                                                          uint64_t *list = nullptr, unsigned long long *list_ctr = nullptr) {
  constexpr bool FIRST = STAGE == 1, LIST = STAGE == 2;
  uint32_t pc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, p_iters = 0, p_ext2 = 0, p_text_rows = 0, p_blk = 0;
  // rows a wide range may have (the 36-bit form has an extra byte column: 36 KB per block, 4 blocks per CU)
  constexpr uint32_t kRowsHere = FIRST ? 0u : WIDE ? kWideRowsWide : kWideRows;
  __shared__ uint32_t s_wpos[FIRST ? 1 : kRowsHere * 256];
  __shared__ uint8_t s_whi[WIDE && !FIRST ? kRowsHere * 256 : 1], s_we[FIRST ? 1 : kRowsHere * 256];
  const uint32_t tid = threadIdx.x;
  const uint64_t nchains = LIST ? (uint64_t)*list_ctr : (uint64_t)n * CPR;
  uint32_t lc_base = ~0u, lc_used = kListChunk;      // FIRST: this wave's chunk of the list (wave-uniform: only ballots and the leader's draw change them)
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t cap_div = (uint32_t)(v.min_hit_len + 1);
  const char *const dummy = reinterpret_cast<const char *>(v.ftab);   // one shared, always valid, 16-byte aligned line
  // ---- the next chain of this lane (grid-stride); its parameters arrive through the P slots
  // (DYN: chains are drawn dyn_chunk at a time - 1 for long reads, a handful for short ones, where one atomic per chain on one
  // counter would be 20 M of them per step; the lane's first chunk is its own: chunk number = its global lane number)
  uint64_t chain_next = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * (DYN && dyn_chunk < 64u ? (uint64_t)dyn_chunk : 1ull);
  uint32_t dyn_left = DYN ? dyn_chunk : 0u;
  uint32_t wt_next = 0, wt_end = 0;       // wave tiles: the chains [stride + wt_next, stride + wt_end) are this wave's and not taken yet
  bool params_valid = false, params_pending = false;
  uint64_t nx_o1a = 0, nx_o1b = 0, nx_o2a = 0, nx_o2b = 0, nx_hoff = 0;
  // ---- chain state
  bool have_chain = false, in_bs = false;
  uint64_t chain = 0;
  const uint64_t *buf = packed1;         // packed blocks of the buffer this chain's read lives in
  uint64_t buf_blocks = 0;
  uint32_t len = 0, rc = 0, t0 = 0, m = 0, l = 0, cnt = 0;
  uint64_t sp = 0, ep = 0;
  cfr_hit *out = raw;
  // ---- character queue: q_hi:q_lo hold q_n <= 64 characters, next one to consume in the top 2 bits of q_hi
  uint64_t q_hi = 0, q_lo = 0;
  uint64_t q_valid = 0;                   // validity of character j at bit 63-j
  uint32_t q_n = 0;
  int64_t blk_next = 0;                   // next block (in consumption order) to append; refills take two blocks = 32 characters
  uint32_t first_skip = 0;                // characters to drop from the first block of a chain
  bool blk_pending = false;
  // ---- text mode: the <= 4 rows of the range as text positions (row order)
  bool tmode = false, need_end = false;
  // ---- wide text mode (5 .. kWideRows rows): wload = the SA entries are being fetched, wmode = text rounds
  bool wload = false, wmode = false;
  uint32_t wR = 0, wg = 0, wJ = 0;       // rows, group in flight / next group, running maximum of the round
  constexpr uint32_t kPlainNext = 0xffffffffu;   // l = this value between a landing and B3: the 8-byte K-mer entry of the search about to
                                                 // start was the escape - on-disk ftab + extends (no extra per-lane state)
  uint32_t sa_o = 0, sa_o2 = 0;
  // text-space hits (virt_text_pos): l0 = characters matched when the search moved to the text; tsel = which rows of the range it
  // had then are still alive - a bit mask in wide text mode, the rows' numbers (5 bits each, slot order) in the four-row form
  uint32_t l0 = 0, tsel = 0;
  using tpos_t = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
  uint32_t R = 0, tL = 0;
  tpos_t tp0 = 0, tp1 = 0, tp2 = 0, tp3 = 0;
  auto wpos_get = [&](uint32_t k) -> tpos_t {
    if (WIDE) return (tpos_t)((uint64_t)s_wpos[k * 256 + tid] | ((uint64_t)s_whi[k * 256 + tid] << 32));
    return (tpos_t)s_wpos[k * 256 + tid];
  };
  auto wpos_set = [&](uint32_t k, uint64_t val) {
    s_wpos[k * 256 + tid] = (uint32_t)val;
    if (WIDE) s_whi[k * 256 + tid] = (uint8_t)(val >> 32);
  };
  // ---- the memory op in flight and the load slots
  uint32_t op = OP_NONE, ext_c = 0;
  ulonglong2 A = make_ulonglong2(0, 0), B = make_ulonglong2(0, 0), Cq = make_ulonglong2(0, 0), Dq = make_ulonglong2(0, 0);
  ulonglong2 P1 = make_ulonglong2(0, 0), P3 = make_ulonglong2(0, 0);
  uint64_t P2 = 0;
  ulonglong2 L = make_ulonglong2(0, 0);

  auto consume = [&](uint32_t k) {        // drop k characters from the head of the queue
    if (k >= q_n) { q_hi = 0; q_lo = 0; q_valid = 0; q_n = 0; }   // (only at the very end of a chain)
    else if (k) {
      const uint32_t sh = 2 * k;
      if (sh >= 64) { q_hi = q_lo << (sh - 64); q_lo = 0; }
      else { q_hi = (q_hi << sh) | (q_lo >> (64 - sh)); q_lo <<= sh; }
      q_valid <<= k;
      q_n -= k;
    }
  };

  // a search that ended on the text: the hit keeps the range it entered the text with, and which of its rows survived - or, where
  // the record has room for them, the survivors' text positions themselves (kVirtInline: one row, or two rows of 32 bits; the
  // four-row form is the only caller with rows <= 4, and tp0 / tp1 are its survivors in row order).  The post stage then needs
  // no suffix-array entry for the hit.  The lookup stage of the two-launch search keeps the mask (12 bytes of scratch otherwise).
  auto emit_text_hit = [&](uint32_t rows, uint32_t mask) {
    if ((int32_t)l >= v.min_hit_len) {                    // (GetHitsFromRead keeps the hit, Classifier.hpp:283-290; rows >= 1 so sp <= ep)
      cfr_hit h;
      const bool inl = !FIRST && (rows == 1u || (!WIDE && rows == 2u));
      h.sp = kVirtRow | ((uint64_t)(l - l0) << kVirtDeltaShift) | (inl ? kVirtInline | (uint64_t)tp0 : sp);
      h.ep = h.sp + (rows - 1u); h.l = (int32_t)l; h.strand = 0; h.offset = (int32_t)t0;
      h.pad = (int32_t)(!FIRST && !WIDE && rows == 2u ? (uint32_t)tp1 : mask);
      if (PROF && inl) ++pc[9];
      out[cnt++] = h;
    }
    in_bs = false;
    t0 += l + 1;
    consume(1);                                         // text mode consumed the matched characters; skip the next one
  };
  auto emit_wide = [&]() { emit_text_hit(wR, tsel); wmode = false; };
  for (;;) {
    // ===================== A. land the loads issued in the previous iteration
    bool bs_end = false;
    uint32_t pending_consume = 0;         // characters of an ended search that are still in the queue
    bool push = false;                    // FIRST: this lane hands its chain over in this iteration
    if (params_pending) {
      if (LIST) { nx_o1a = P1.x; nx_o1b = P1.y; nx_hoff = P3.x; nx_o2a = P3.y; }      // a record: first byte, len | t0 << 32, hit list | hits << kListHitBits, chain
      else {
        nx_o1a = P1.x; nx_o1b = P1.y; nx_hoff = P2;
        if (CPR == 4) { nx_o2a = P3.x; nx_o2b = P3.y; }
      }
      params_pending = false;
      params_valid = true;
    }
    // matched length of a row against the queue: window = text symbols tp-1, tp-2, ... from the top bits down.
    // slot layout: the 16 bytes that END with the 4-byte word holding position tp-1 (text_slot below): 64 symbols, of
    // which the 49 .. 64 below tp count - a step compares up to kTextStep = 48 characters per gathered row.
    auto matched = [&](const ulonglong2 &w, tpos_t tp) -> uint32_t {
      if (tp == 0) return 0u;                                      // the row of text position 0 has no left neighbour
      const uint32_t sh = 30u - 2u * ((uint32_t)(tp - 1u) & 15u); // bits above position tp-1 in the slot's last word
      const uint64_t win_hi = sh ? (w.y << sh) | (w.x >> (64u - sh)) : w.y, win_lo = w.x << sh;
      const uint64_t xh = win_hi ^ q_hi, xl = win_lo ^ q_lo;
      const uint32_t e = xh ? (uint32_t)__clzll((long long)xh) >> 1 : 32u + (xl ? (uint32_t)__clzll((long long)xl) >> 1 : 32u);
      return e < tL ? e : tL;
    };
    // where that slot is: text2 carries 16 bytes of padding in front, so the slot of a position near 0 is addressable
    auto text_slot = [&](tpos_t tp) -> const char * {
      return reinterpret_cast<const char *>(v.text2) + 4ull * ((uint64_t)(tp - 1u) >> 4) - 12;
    };
    if (op == OP_TABLE) {                 // derived K-mer entry: state after the first K characters (or where it stopped)
      bool usable = true;
      if (v.ftabx_e8) usable = ftabx8_decode(A.x, v.ftabx_width, l, sp, ep);
      else {
        l = (uint32_t)(A.y & 0xffu);
        sp = A.x;
        ep = A.x + ftabx16_count(A.y) - 1;
      }
      if (!usable) l = kPlainNext;        // escape entry: nothing consumed, B3 starts the same search through the on-disk ftab
      else if (l < v.ftabx_width || l >= m) { bs_end = true; pending_consume = l + 1; }
      else {
        in_bs = true;
        consume(l);
        if (!v.ftabx_e8 && (A.y & kFtabxTextPos) && v.sa != nullptr && m - l <= kVirtDeltaMax) {
          // the one row's text position came with the entry: what OP_SA would have fetched in the next iteration (k_ftabx_textpos)
          tp0 = (tpos_t)ftabx16_textpos(A.y); tp1 = 0; tp2 = 0; tp3 = 0;
          R = 1u;
          l0 = l; tsel = 0u | (1u << 5) | (2u << 10) | (3u << 15);
          tmode = true; need_end = false;
        }
      }
    } else if (op == OP_TABLE10) {        // on-disk ftab entry (FMIndex.hpp:405-414)
      if (A.y == 0) { sp = 1; ep = 0; l = v.ftab_width - 1; bs_end = true; pending_consume = l + 1; }
      else {
        sp = A.x; ep = A.x + A.y - 1; l = v.ftab_width;
        if (l >= m) { bs_end = true; pending_consume = l + 1; } else { in_bs = true; consume(l); }
      }
    } else if (op == OP_EXT) {            // BackwardExtend + stop rule (FMIndex.hpp:364-379, :503)
      const uint64_t fix_s = (ext_c == v.last_code && sp <= v.first_isa) ? 1ull : 0ull;               // exclusive rank at sp
      const uint64_t nsp = v.C[ext_c] + occ_count(Cq.x, A.x, A.y, ext_c, sp, 0) + fix_s;
      uint64_t nep;
      if (sp != ep) {
        const uint64_t fix_e = (ext_c == v.last_code && ep < v.first_isa) ? 1ull : 0ull;              // inclusive rank at ep
        nep = v.C[ext_c] + occ_count(Dq.x, B.x, B.y, ext_c, ep, 1) + fix_e - 1;
      } else {
        const uint32_t j = (uint32_t)sp & 63u;
        const uint32_t sym = (uint32_t)((A.x >> j) & 1u) | ((uint32_t)((A.y >> j) & 1u) << 1);
        nep = nsp + (sym == ext_c ? 0ull : ~0ull);
      }
      consume(1);                                                    // the character just tried (matched or skipped)
      if (nsp > nep || nep > v.n) { bs_end = true; in_bs = false; }
      else { sp = nsp; ep = nep; ++l; if (l >= m) { bs_end = true; in_bs = false; pending_consume = 1; } }
    } else if (op == OP_SA) {             // SA[sp .. sp+3] have landed
      if (WIDE) {
        tp0 = (tpos_t)u36_at(Cq.x, Cq.y, Dq.x, Dq.y, sa_o, 0); tp1 = (tpos_t)u36_at(Cq.x, Cq.y, Dq.x, Dq.y, sa_o, 1);
        tp2 = (tpos_t)u36_at(Cq.x, Cq.y, Dq.x, Dq.y, sa_o, 2); tp3 = (tpos_t)u36_at(Cq.x, Cq.y, Dq.x, Dq.y, sa_o, 3);
      } else { tp0 = (uint32_t)Cq.x; tp1 = (uint32_t)(Cq.x >> 32); tp2 = (uint32_t)Cq.y; tp3 = (uint32_t)(Cq.y >> 32); }
      tmode = true; need_end = false;
    } else if (!FIRST && op == OP_SAW) {            // SA entries of the next rows of a wide range: 16 per iteration (u32), 8 (36-bit entries)
      if (WIDE) {
        const uint32_t r0 = 8u * wg;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          if (r0 + q < wR) wpos_set(r0 + q, u36_at(A.x, A.y, B.x, B.y, sa_o, q));
          if (r0 + 4 + q < wR) wpos_set(r0 + 4 + q, u36_at(Cq.x, Cq.y, Dq.x, Dq.y, sa_o2, q));
        }
        ++wg;
        if (8u * wg >= wR) { wload = false; wmode = true; wg = 0; }
      } else {
        const uint32_t r0 = 16u * wg;
        const uint64_t e8[8] = {A.x, A.y, B.x, B.y, Cq.x, Cq.y, Dq.x, Dq.y};
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
          if (r0 + 2 * q < wR) wpos_set(r0 + 2 * q, (uint32_t)e8[q]);
          if (r0 + 2 * q + 1 < wR) wpos_set(r0 + 2 * q + 1, (uint32_t)(e8[q] >> 32));
        }
        ++wg;
        if (16u * wg >= wR) { wload = false; wmode = true; wg = 0; }
      }
    } else if (!FIRST && op == OP_TEXTW) {          // four rows of the round's comparison have landed
      const uint32_t r0 = 4u * wg;
      const uint32_t f0 = matched(A, wpos_get(r0));
      const uint32_t f1 = r0 + 1 < wR ? matched(B, wpos_get(r0 + 1)) : 0u;
      const uint32_t f2 = r0 + 2 < wR ? matched(Cq, wpos_get(r0 + 2)) : 0u;
      const uint32_t f3 = r0 + 3 < wR ? matched(Dq, wpos_get(r0 + 3)) : 0u;
      s_we[r0 * 256 + tid] = (uint8_t)f0;
      if (r0 + 1 < wR) s_we[(r0 + 1) * 256 + tid] = (uint8_t)f1;
      if (r0 + 2 < wR) s_we[(r0 + 2) * 256 + tid] = (uint8_t)f2;
      if (r0 + 3 < wR) s_we[(r0 + 3) * 256 + tid] = (uint8_t)f3;
      uint32_t mx = f0 > f1 ? f0 : f1;
      if (f2 > mx) mx = f2;
      if (f3 > mx) mx = f3;
      if (mx > wJ) wJ = mx;
      ++wg;
      if (4u * wg >= wR) {                // the round is complete: the rows that matched all J characters survive, in row order
        const uint32_t J = wJ;
        uint32_t cntR = 0, m_in = tsel, m_out = 0;
        for (uint32_t k = 0; k < wR; ++k) {
          const uint32_t bit = m_in & (0u - m_in);        // LDS slot k holds the k-th surviving row of the entry range
          m_in ^= bit;
          if ((uint32_t)s_we[k * 256 + tid] >= J) { wpos_set(cntR, (uint64_t)wpos_get(k) - J); ++cntR; m_out |= bit; }
        }
        tsel = m_out;
        wR = cntR;
        wg = 0;
        l += J;
        consume(J);
        const bool ended = J < tL || l >= m;      // every row mismatched at character J, or the read is exhausted
        if (wR <= 4) {                            // hand over to the four-row form: it owns the end of a search and the corner cases
          tp0 = wpos_get(0);
          tp1 = wR > 1 ? wpos_get(1) : (tpos_t)0; tp2 = wR > 2 ? wpos_get(2) : (tpos_t)0; tp3 = wR > 3 ? wpos_get(3) : (tpos_t)0;
          R = wR;
          {                                               // the survivors' row numbers, slot order (the four-row form's bookkeeping)
            uint32_t mm = tsel, packed = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) if (mm) { packed |= ((uint32_t)__ffs((int)mm) - 1u) << (5u * q); mm &= mm - 1u; }
            tsel = packed;
          }
          wmode = false;
          tmode = true;
          need_end = ended;
        } else if (ended) emit_wide();            // the search ends with 5 or more rows: they go to the pool
      }
    } else if (op == OP_TEXT) {
      const uint32_t e0 = matched(A, tp0);
      const uint32_t e1 = R > 1 ? matched(B, tp1) : 0u;
      const uint32_t e2 = R > 2 ? matched(Cq, tp2) : 0u;
      const uint32_t e3 = R > 3 ? matched(Dq, tp3) : 0u;
      uint32_t J = e0;
      if (e1 > J) J = e1;
      if (e2 > J) J = e2;
      if (e3 > J) J = e3;
      // rows that matched all J characters survive, in row order (LF keeps the order of rows with equal BWT symbol)
      tpos_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
      uint32_t cntR = 0, osel = 0;
      // (written with selects only: as an if-chain on cntR the compiler turned o0..o3 into a four-entry array in SCRATCH memory, indexed by
      //  cntR - twelve scratch stores / loads in every text step of every lane, tools/dbg/scratch_sites.py; row `slot` can only land in
      //  o0 .. o<slot>)
#if defined(CFR_TEXT_KEEP_CHAIN) && CFR_TEXT_KEEP_CHAIN      // the form before (A/B: tools/dbg/ab_keep.sh)
      auto keep = [&](bool live, uint32_t e, tpos_t tp, uint32_t slot) {
        if (live && e >= J) {
          const tpos_t val = tp - J;
          if (cntR == 0) o0 = val; else if (cntR == 1) o1 = val; else if (cntR == 2) o2 = val; else o3 = val;
          osel |= ((tsel >> (5u * slot)) & 31u) << (5u * cntR);
          ++cntR;
        }
      };
#else
      auto keep = [&](bool live, uint32_t e, tpos_t tp, uint32_t slot) {
        const bool k = live && e >= J;
        const tpos_t val = tp - J;
        o0 = (k && cntR == 0u) ? val : o0;
        if (slot >= 1) o1 = (k && cntR == 1u) ? val : o1;
        if (slot >= 2) o2 = (k && cntR == 2u) ? val : o2;
        if (slot >= 3) o3 = (k && cntR == 3u) ? val : o3;
        osel |= k ? ((tsel >> (5u * slot)) & 31u) << (5u * cntR) : 0u;
        cntR += k ? 1u : 0u;
      };
#endif
      keep(true, e0, tp0, 0); keep(R > 1, e1, tp1, 1); keep(R > 2, e2, tp2, 2); keep(R > 3, e3, tp3, 3);
      tp0 = o0; tp1 = o1; tp2 = o2; tp3 = o3; R = cntR; tsel = osel;
      l += J;
      consume(J);
      if (J < tL || l >= m) need_end = true;                        // every row mismatched at character J, or the read is exhausted
    }
    op = OP_NONE;
    if (blk_pending) {                    // append 32 characters (fewer for the first pair of a chain); there is room: q_n <= 32 when requested
      uint32_t c0, v0, c1, v1;            // L.x = lower-address block, L.y = the next one
      conv_block(rc ? L.x : L.y, rc, c0, v0);    // first consumed: ascending walks take the lower block first
      conv_block(rc ? L.y : L.x, rc, c1, v1);
      uint64_t cw = ((uint64_t)c0 << 32) | c1;
      uint32_t vw = (v0 << 16) | v1;
      const uint32_t take = 32u - first_skip;
      cw <<= 2 * first_skip;
      vw <<= first_skip;
      const uint32_t sh = 2 * q_n;
      if (sh == 0) q_hi |= cw;
      else if (sh < 64) { q_hi |= cw >> sh; q_lo |= cw << (64 - sh); }
      else q_lo |= cw;
      q_valid |= (uint64_t)vw << (32 - q_n);
      q_n += take;
      first_skip = 0;
      blk_pending = false;
    }

    // ===================== B. decide the next op; only addresses are produced here
    const char *aA = dummy, *aB = dummy, *aC = dummy, *aD = dummy, *aL = dummy, *aP1 = dummy, *aP2 = dummy, *aP3 = dummy;

    // ---- B1w. wide text mode: fetch the rows' SA entries, then rounds of <= 32 characters, four rows per iteration
    if (!FIRST && have_chain && in_bs && wload) {
      op = OP_SAW;
      if (WIDE) {      // rows 8 wg .. : two 32-byte windows (4 entries each) from the 4-byte words their first entries start in
        const uint64_t b0 = 36ull * (sp + 8ull * wg), b1 = b0 + 144ull;
        sa_o = (uint32_t)b0 & 31u; sa_o2 = (uint32_t)b1 & 31u;
        aA = reinterpret_cast<const char *>(v.sa + (b0 >> 5)); aB = aA + 16;
        aC = reinterpret_cast<const char *>(v.sa + (b1 >> 5)); aD = aC + 16;
      } else {
        aA = reinterpret_cast<const char *>(v.sa + sp + 16ull * wg); aB = aA + 16; aC = aA + 32; aD = aA + 48;
      }
    }
    if (!FIRST && have_chain && in_bs && wmode) {
      bool go = true;
      if (wg == 0) {                                    // a round starts: how many characters it may compare
        if (q_n == 0) go = false;                       // (the block carrying the next characters is in flight)
        else {
          uint32_t Lc = q_n < kTextStep ? q_n : kTextStep;
          if (m - l < Lc) Lc = m - l;
          const uint32_t lead_valid = (uint32_t)__clzll((long long)(~q_valid | ((1ull << (64u - kTextStep)) - 1ull)));   // leading symbols, at most kTextStep
          if (lead_valid < Lc) Lc = lead_valid;
          for (uint32_t k = 0; k < wR; ++k) { const tpos_t t = wpos_get(k); if (t && t < Lc) Lc = (uint32_t)t; }   // no row may cross text position 0 inside a step
          if (Lc == 0) {                                // the next character is not a symbol: the match ends here
            emit_wide();
            go = false;
          } else { tL = Lc; wJ = 0; }
        }
      }
      if (go) {
        op = OP_TEXTW;
        const uint32_t r0 = 4u * wg;
        const tpos_t t0 = wpos_get(r0);
        if (t0) aA = text_slot(t0);
        if (r0 + 1 < wR) { const tpos_t t = wpos_get(r0 + 1); if (t) aB = text_slot(t); }
        if (r0 + 2 < wR) { const tpos_t t = wpos_get(r0 + 2); if (t) aC = text_slot(t); }
        if (r0 + 3 < wR) { const tpos_t t = wpos_get(r0 + 3); if (t) aD = text_slot(t); }
        if (PROF) p_text_rows += (wR - r0 < 4u ? wR - r0 : 4u);
      }
    }
    // ---- B1. a search in progress needs its next character(s)
    if (have_chain && in_bs && tmode) {
      bool to_end = need_end;
      if (!to_end && q_n > 0) {
        uint32_t Lc = q_n < kTextStep ? q_n : kTextStep;
        if (m - l < Lc) Lc = m - l;
        const uint32_t lead_valid = (uint32_t)__clzll((long long)(~q_valid | ((1ull << (64u - kTextStep)) - 1ull)));   // leading symbols, at most kTextStep
        if (lead_valid < Lc) Lc = lead_valid;
        if (Lc == 0) to_end = true;                     // next character is not a symbol: the match ends here (FMIndex.hpp:500-501)
        else if (R == 1 && tp0 == 0) {                  // single row at text position 0: the reference's Access path decides
          sp = ep = v.first_isa;                        //   (SURVEY.md Appendix B item 4) - take that one step on the BWT
          tmode = false;
        } else {
          // no row may cross text position 0 inside a step (the row AT 0 simply fails its first comparison)
          if (tp0 && tp0 < Lc) Lc = (uint32_t)tp0;
          if (R > 1 && tp1 && tp1 < Lc) Lc = (uint32_t)tp1;
          if (R > 2 && tp2 && tp2 < Lc) Lc = (uint32_t)tp2;
          if (R > 3 && tp3 && tp3 < Lc) Lc = (uint32_t)tp3;
          tL = Lc;
          op = OP_TEXT;
          if (tp0) aA = text_slot(tp0);
          if (R > 1 && tp1) aB = text_slot(tp1);
          if (R > 2 && tp2) aC = text_slot(tp2);
          if (R > 3 && tp3) aD = text_slot(tp3);
        }
      }
      if (to_end) {                                     // the search ends here with l final; the hit stays in text space
        uint32_t mask = 1u << (tsel & 31u);
        if (R > 1) mask |= 1u << ((tsel >> 5) & 31u);
        if (R > 2) mask |= 1u << ((tsel >> 10) & 31u);
        if (R > 3) mask |= 1u << ((tsel >> 15) & 31u);
        if (PROF && (int32_t)l >= v.min_hit_len) ++pc[OP_VHIT];
        emit_text_hit(R, mask);
        tmode = false; need_end = false;
      }
    }
    if (have_chain && in_bs && !tmode && !wmode && !wload && op == OP_NONE && q_n > 0) {
      if (!((q_valid >> 63) & 1ull)) { bs_end = true; in_bs = false; pending_consume = 1; }   // non-symbol ends the match (FMIndex.hpp:500-501)
      else if (v.sa != nullptr && l >= v.text_min_l && m - l <= kVirtDeltaMax && ep - sp < 4 && !(sp == ep && sp == v.first_isa)) {
        op = OP_SA;                                     // small range deep into a match: continue on the text
        R = (uint32_t)(ep - sp) + 1u;
        l0 = l; tsel = 0u | (1u << 5) | (2u << 10) | (3u << 15);
        if (WIDE) {                                     // 144 bits from bit 36 sp on: two 16-byte slots from the 4-byte word they start in
          const uint64_t b0 = 36ull * sp;
          sa_o = (uint32_t)b0 & 31u;
          aC = reinterpret_cast<const char *>(v.sa + (b0 >> 5));
          aD = aC + 16;
        } else aC = reinterpret_cast<const char *>(v.sa + sp);
      } else if (v.sa != nullptr && l >= v.text_min_l && m - l <= kVirtDeltaMax && ep - sp >= 4 && ep - sp < v.wide_rows) {
        if (FIRST) push = true;                         // 5 .. kWideRows rows: the second stage's (this search starts over there)
        else {
          wR = (uint32_t)(ep - sp) + 1u;                // 5 .. kWideRows rows: wide text mode (the loads start with the next iteration)
          wg = 0;
          wload = true;
          l0 = l; tsel = (1u << wR) - 1u;
        }
      } else {
        const uint32_t c = (uint32_t)(q_hi >> 62);
        ext_c = c;
        op = OP_EXT;
        const uint64_t *rs = v.occ + (sp >> 7) * 8;
        aC = reinterpret_cast<const char *>(rs + c);
        aA = reinterpret_cast<const char *>(rs + 4 + 2 * (((uint32_t)sp >> 6) & 1u));
        if (sp != ep) {
          const uint64_t *re = v.occ + (ep >> 7) * 8;
          aD = reinterpret_cast<const char *>(re + c);
          aB = reinterpret_cast<const char *>(re + 4 + 2 * (((uint32_t)ep >> 6) & 1u));
        }
      }
    }
    if (FIRST) {                          // hand-over: slots from the wave's chunk; one atomic when the chunk is used up
      const uint64_t pm = __ballot(push);
      if (pm) {
        const uint32_t lane = (uint32_t)__lane_id();
        const uint32_t k = (uint32_t)__popcll(pm);
        if (lc_used + k > kListChunk) {
          const uint64_t act = __ballot(1);              // what is left of the old chunk: holes, written by the lanes still in the loop
          const uint32_t nact = (uint32_t)__popcll(act);
          for (uint32_t i = lc_used + (uint32_t)__popcll(act & ((1ull << lane) - 1ull)); i < kListChunk; i += nact) {
            uint64_t *rec = list + 4ull * ((uint64_t)lc_base + i);
            *reinterpret_cast<ulonglong2 *>(rec) = make_ulonglong2(0, 0);
            *reinterpret_cast<ulonglong2 *>(rec + 2) = make_ulonglong2(0, ~0ull);
          }
          const int leader = __ffsll((long long)pm) - 1;
          uint32_t base = 0;
          if ((int)lane == leader) base = (uint32_t)atomicAdd(list_ctr, (unsigned long long)kListChunk);
          lc_base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
          lc_used = 0;
        }
        if (push) {
          // the byte this search started at, from the queue: its head is l characters further (no block is in flight here: A landed it, B6 asks later)
          const uint64_t a_start = rc ? (uint64_t)(16 * blk_next - (int64_t)q_n - (int64_t)l) : (uint64_t)(16 * (blk_next + 1) + (int64_t)q_n - 1 + (int64_t)l);
          uint64_t *rec = list + 4ull * (lc_base + lc_used + (uint32_t)__popcll(pm & ((1ull << lane) - 1ull)));
          *reinterpret_cast<ulonglong2 *>(rec) = make_ulonglong2(a_start, (uint64_t)len | ((uint64_t)t0 << 32));
          *reinterpret_cast<ulonglong2 *>(rec + 2) = make_ulonglong2((uint64_t)(out - raw) | ((uint64_t)cnt << kListHitBits), chain);
          have_chain = false; in_bs = false;
        }
        lc_used += k;
      }
    }
    // ---- B2. a search ended: GetHitsFromRead bookkeeping (Classifier.hpp:283-290)
    if (bs_end) {
      if ((int32_t)l >= v.min_hit_len && sp <= ep) {
        cfr_hit h;
        h.sp = sp; h.ep = ep; h.l = (int32_t)l; h.strand = 0; h.offset = (int32_t)t0; h.pad = 0;
        out[cnt++] = h;
      }
      t0 += l + 1;
      consume(pending_consume);
      in_bs = false;
    }
    // ---- B3. start the next search of the chain
    if (have_chain && !in_bs && op == OP_NONE) {
      const int32_t remaining = (int32_t)len - (int32_t)t0;
      if (remaining < v.min_hit_len) {
        chain_cnt[chain] = cnt;
        have_chain = false;
      } else {
        m = (uint32_t)remaining;
        const uint32_t w = v.ftab_width, K = v.ftabx_width;
        if (m < w) { if (q_n >= 1) { l = 0; t0 += 1; consume(1); } }   // BackwardSearch returns 0 (FMIndex.hpp:489-490): no hit, skip one character
        else if (w == 0) { sp = 0; ep = v.n - 1; l = 0; in_bs = true; }
        else {
          const uint32_t span = (v.ftabx && m >= K && l != kPlainNext) ? K : w;
          if (q_n >= span) {                           // else: the block carrying the missing characters is in flight
            const uint64_t key = q_hi >> (64 - 2 * span);
            const uint32_t inval = (~(uint32_t)(q_valid >> 32)) >> (32 - span);   // bit (span-1-i) set: character i is not a symbol
            const uint32_t bad = inval ? (uint32_t)__clz((int)inval) - (32 - span) : span;
            if (bad < w) { l = bad; t0 += l + 1; consume(l + 1); }            // l = i, range (1,0): no hit (FMIndex.hpp:396-401)
            else if (span == w || bad < span) {        // plain ftab (a non-symbol between w and K lets the walk decide)
              op = OP_TABLE10;
              aA = reinterpret_cast<const char *>(v.ftab + 2 * (key >> (2 * (span - w))));
            } else {
              op = OP_TABLE;
              aA = reinterpret_cast<const char *>(v.ftabx + (v.ftabx_e8 ? key : 2 * key));   // (8-byte entries: the slot's 16-byte load starts at the entry)
            }
          }
        }
      }
    }
    // ---- B4. next chain of this lane (parameters come through the P slots, requested a chain ahead)
    // DYN with dyn_chunk >= 64 (round 5): chains are handed out from WAVE TILES - a wave owns dyn_chunk consecutive chains at a time, the
    // lanes that take a chain in this iteration (ballot) share the next ones of the tile among themselves, and only when the tile is used
    // up one lane draws the next tile with ONE atomic (a few thousand per launch instead of one per chain or per handful of chains).  The
    // tile state is computed by every lane of the wave from wave-uniform values (ballot, the leader's draw by shuffle), outside the
    // divergent part, so the lanes' copies cannot drift apart whatever registers the compiler keeps them in.
    const bool take = !have_chain && params_valid;
    uint64_t tile_chain = 0;
    if (DYN && dyn_chunk >= 64u) {
      const uint64_t need = __ballot(take);
      if (need) {
        const uint32_t lane = (uint32_t)__lane_id();
        const uint32_t kk = (uint32_t)__popcll(need), r = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
        const uint32_t avail = wt_end - wt_next;
        if (kk > avail) {
          const int leader = __ffsll((long long)need) - 1;
          unsigned long long base = 0;
          if ((int)lane == leader) base = atomicAdd(next_ctr, (unsigned long long)dyn_chunk);
          const uint32_t b32 = (uint32_t)__shfl((int)(uint32_t)base, leader);
          tile_chain = stride + (uint64_t)(r < avail ? wt_next + r : b32 + (r - avail));
          wt_next = b32 + (kk - avail);
          wt_end = b32 + dyn_chunk;
        } else {
          tile_chain = stride + (uint64_t)(wt_next + r);
          wt_next += kk;
        }
      }
    }
    if (take) {
      chain = LIST ? nx_o2a : chain_next;
      const uint32_t mate = CPR == 4 ? (uint32_t)(chain >> 1) & 1u : 0u;
      rc = (uint32_t)chain & 1u;
      const uint32_t len1 = (uint32_t)(nx_o1b - nx_o1a);
      uint64_t rabs;
      if (mate) { buf = packed2; buf_blocks = nblk2; rabs = nx_o2a; len = (uint32_t)(nx_o2b - nx_o2a); }
      else { buf = packed1; buf_blocks = nblk1; rabs = nx_o1a; len = len1; }
      out = raw + nx_hoff + (mate ? 2ull * (len1 / cap_div + 1u) : 0ull) + (rc ? (uint64_t)(len / cap_div + 1u) : 0ull);
      cnt = 0; t0 = 0; l = 0; m = 0; in_bs = false; tmode = false; need_end = false; wmode = false; wload = false;
      if (LIST) {                         // the record says it all (the buffer follows the mate)
        len = (uint32_t)nx_o1b; t0 = (uint32_t)(nx_o1b >> 32);
        out = raw + (nx_hoff & ((1ull << kListHitBits) - 1ull)); cnt = (uint32_t)(nx_hoff >> kListHitBits);
      }
      if (DYN) {
        if (dyn_chunk >= 64u) chain_next = tile_chain;
        else if (--dyn_left) ++chain_next;
        else { chain_next = (stride + (uint64_t)atomicAdd(next_ctr, 1ull)) * (uint64_t)dyn_chunk; dyn_left = dyn_chunk; }
      } else chain_next += stride;
      params_valid = false;
      if (LIST && chain == ~0ull) { }                             // a hole of the list: the next record follows
      else if ((int32_t)len < v.min_hit_len) chain_cnt[chain] = 0;     // nothing to search; the next chain follows
      else {
        have_chain = true;
        // first character consumed: rc -> first byte of the read (ascending), forward -> last byte (descending); a LIST record carries the byte its search starts at
        const uint64_t a0 = LIST ? nx_o1a : rabs + (rc ? 0u : len - 1u);
        blk_next = (int64_t)(a0 >> 4);
        first_skip = rc ? (uint32_t)(a0 & 15u) : 15u - (uint32_t)(a0 & 15u);
        q_hi = 0; q_lo = 0; q_valid = 0; q_n = 0;
        blk_pending = false;
      }
    }
    if (!have_chain && !params_valid && !params_pending && chain_next >= nchains) break;
    if (PROF) {
      ++p_iters;
#pragma unroll
      for (uint32_t q = 0; q < 9; ++q) pc[q] += op == q ? 1u : 0u;
      if (op == OP_EXT && sp != ep) ++p_ext2;
      if (op == OP_TEXT) p_text_rows += R;
    }
    // request the parameters of the lane's next chain as soon as the slot is free
    if (!params_valid && !params_pending && chain_next < nchains) {
      if (LIST) { aP1 = reinterpret_cast<const char *>(list + 4ull * chain_next); aP3 = aP1 + 16; }
      else {
        const uint64_t i = chain_next / CPR;
        aP1 = reinterpret_cast<const char *>(offs1 + i);
        aP2 = reinterpret_cast<const char *>(hit_off + i);
        if (CPR == 4) aP3 = reinterpret_cast<const char *>(offs2 + i);
      }
      params_pending = true;
    }
    // keep the queue fed: one pair of blocks (32 characters) in flight at most, requested when there is room for it.
    // The packed buffers carry 4 zero blocks ("not a symbol") on either side, so a pair next to the buffer's ends is readable.
    if (have_chain && !blk_pending && q_n <= 32) {
      const int64_t first = rc ? blk_next : blk_next - 1;                        // lower-address block of the pair
      if (first >= -4 && first + 1 < (int64_t)buf_blocks + 4) aL = reinterpret_cast<const char *>(buf + first);
      blk_next += rc ? 2 : -2;
      blk_pending = true;
      if (PROF) ++p_blk;
    }

    // ===================== C. the loads of this iteration: same instructions for every lane
    if (CFR_GATHER_NT == 2) { if (op == OP_TABLE) A = ld16_nt(aA); else A = ld16(aA); }      // (the K-mer table only)
    else A = ld16_gather(aA);
    B = ld16_gather(aB);
    Cq = ld16_gather(aC);     // (EXT uses .x only; the extra 8 bytes stay inside the record / padded arrays)
    Dq = ld16_gather(aD);
    P1 = ld16(aP1);
    if (!LIST) P2 = *reinterpret_cast<const uint64_t *>(aP2);
    if (CPR == 4 || LIST) P3 = ld16(aP3);
    L = ld16(aL);
    if (aL == dummy) L = make_ulonglong2(0, 0);                      // far outside the buffer: no symbols
  }
  if (FIRST) {                            // what this wave leaves of its last chunk: holes.  Lanes left the loop at different times, so the
    uint64_t key = (lc_base == ~0u ? 0ull : ((uint64_t)lc_base + 1ull) << 8) | lc_used;               // newest copy of (chunk, used) is the largest (bases only grow for a wave; none yet = 0)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint64_t other = __shfl_xor(key, o); key = other > key ? other : key; }
    const uint64_t b = (key >> 8) - 1ull; const uint32_t u = (uint32_t)key & 0xffu;
    const uint32_t lane = (uint32_t)__lane_id();
    if ((key >> 8) != 0 && u + lane < kListChunk) {
      uint64_t *rec = list + 4ull * (b + u + lane);
      *reinterpret_cast<ulonglong2 *>(rec) = make_ulonglong2(0, 0);
      *reinterpret_cast<ulonglong2 *>(rec + 2) = make_ulonglong2(0, ~0ull);
    }
  }
  if (PROF) {
#pragma unroll
    for (uint32_t q = 0; q < 7; ++q) atomicAdd(prof + q, (unsigned long long)pc[q]);
    atomicAdd(prof + 11, (unsigned long long)pc[OP_SAW]);
    atomicAdd(prof + 12, (unsigned long long)pc[OP_TEXTW]);
    atomicAdd(prof + 7, (unsigned long long)p_iters);
    atomicAdd(prof + 8, (unsigned long long)p_ext2);
    atomicAdd(prof + 9, (unsigned long long)p_text_rows);
    atomicAdd(prof + 10, (unsigned long long)p_blk);
    atomicAdd(prof + 13, (unsigned long long)pc[9]);      // text hits that carry their positions (kVirtInline)
  }
}

// ------------------------------------------------------------------------------------ --merge-readpair
// ReadPairMerger::Merge (ReadPairMerger.hpp:132-233; host twin: cfr_merge.cpp) for pairs that are already in HBM: k_merge_decide
// finds kind / overlap / offset and the new lengths of every pair, a scan turns the lengths into offsets, k_merge_write writes the
// new reads (merged pair: read 1 = the merged read, read 2 = empty; the others as they are).
//
// One wave per pair, lanes = candidate offsets j of IsMateOverlap (ReadPairMerger.hpp:20-50).  Without the reference's early exit:
// with K = min(flen - j, slen) compared positions and mism mismatches among them, its running test
// matchCnt + (flen - (j + k) - 1) < T is (flen - j) - mism_k < T with mism_k non-decreasing in k, so offset j passes iff
// (flen - j) - mism >= T(flen - j) (always when K == 0), and overlapSize = K.  One side of every compare is the complemented mate
// (A C G T N only), so a byte of the raw side matches only if it is one of those five: both sides as three bit planes of the codes
// A 0, C 1, G 2, T 3, N 4, anything else 5 (raw side only), mism = popcount of (x0^y0)|(x1^y1)|(x2^y2) over the first sequence's
// planes funnel-shifted by j.  Mates of up to kMergeFastLen bases keep their planes in LDS; longer ones are compared byte by byte
// from memory (correct for any length below 2^31, not fast).
constexpr int kMergeFastLen = 512, kMergeWords = kMergeFastLen / 64;
__constant__ int32_t c_merge_thr[100];      // int(L * similarityThreshold) for L < 100, filled by the host twin's own expression (merge_threshold_table)

__device__ __forceinline__ uint32_t merge_code_raw(uint8_t c) {
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : c == 'N' ? 4u : 5u;
}
__device__ __forceinline__ uint32_t merge_code_comp(uint8_t c) {      // code of _compChar[c]
  return c == 'A' ? 3u : c == 'C' ? 2u : c == 'G' ? 1u : c == 'T' ? 0u : 4u;
}
__device__ __forceinline__ uint8_t merge_comp_char(uint8_t c) {       // _compChar (ReadPairMerger.hpp:105-111)
  return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
}
__device__ __forceinline__ int merge_threshold(int L) {               // from 100 on: one IEEE double multiply (nothing to contract it with)
  return L < 100 ? c_merge_thr[L] : (int)((double)L * 0.85);
}

// IsMateOverlap's offset loop on the planes: F = first sequence (flen), S = second (slen).  cnt = offsets that pass, last = the largest of them
__device__ __forceinline__ void merge_pass_planes(const uint64_t (*F)[kMergeWords + 1], const uint64_t (*S)[kMergeWords + 1], int flen, int slen,
                                                  int min_overlap, uint32_t lane, int &cnt, int &last) {
  cnt = 0; last = -1;
  const int nj = flen - min_overlap;
  for (int j0 = 0; j0 < nj; j0 += 64) {
    const int j = j0 + (int)lane;
    bool ok = false;
    if (j < nj) {
      const int L = flen - j, K = L < slen ? L : slen;
      const int q = j >> 6, sh = j & 63;
      int mism = 0;
      for (int w = 0; w * 64 < K; ++w) {
        uint64_t d = 0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const uint64_t lo = F[b][q + w], hi = F[b][q + w + 1];
          const uint64_t x = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
          d |= x ^ S[b][w];
        }
        const int rem = K - w * 64;
        if (rem < 64) d &= (1ull << rem) - 1ull;
        mism += __popcll(d);
      }
      ok = K == 0 || L - mism >= merge_threshold(L);
    }
    const unsigned long long m = __ballot(ok);
    if (m) { cnt += __popcll(m); last = j0 + 63 - __clzll((long long)m); }
  }
}

// the same loop on the bytes themselves (long mates).  RC_FIRST: the first sequence is the reverse complement of r2 (the
// read-through pass), else r1 (the plain pass); the other one is the second sequence
template <bool RC_FIRST>
__device__ __forceinline__ void merge_pass_bytes(const uint8_t *r1, int len1, const uint8_t *r2, int len2, int min_overlap, uint32_t lane,
                                                 int &cnt, int &last) {
  cnt = 0; last = -1;
  const int flen = RC_FIRST ? len2 : len1, slen = RC_FIRST ? len1 : len2;
  const int nj = flen - min_overlap;
  for (int j0 = 0; j0 < nj; j0 += 64) {
    bool ok = false;
    if ((int)lane < nj - j0) {            // (j0 + lane may not fit an int for the lanes past the end)
      const int j = j0 + (int)lane;
      const int L = flen - j, K = L < slen ? L : slen;
      const int T = merge_threshold(L);
      int mism = 0;
      for (int k = 0; k < K && L - mism >= T; ++k) {
        const uint8_t a = RC_FIRST ? merge_comp_char(r2[len2 - 1 - (j + k)]) : r1[j + k];
        const uint8_t c = RC_FIRST ? r1[k] : merge_comp_char(r2[len2 - 1 - k]);
        mism += a != c;
      }
      ok = K == 0 || L - mism >= T;
    }
    const unsigned long long m = __ballot(ok);
    if (m) { cnt += __popcll(m); last = j0 + 63 - __clzll((long long)m); }
    if (nj - j0 <= 64) break;
  }
}

// kind: 0 no merge, 1 overlap, 2 read-through; overlap / offset: what ReadPairMerger::Merge leaves in overlapSize / offset (for kind 0:
// -1 and the last offset that passed, or -1); len1 / len2: lengths of the pair's reads after the merge (entry n of both is left alone:
// the caller zeroes it for the scan)
__global__ __launch_bounds__(256) void k_merge_decide(const uint8_t *bases1, const uint64_t *offs1, const uint8_t *bases2, const uint64_t *offs2, size_t n,
                                                      int32_t *kind, int32_t *overlap, int32_t *offset, uint64_t *len1_out, uint64_t *len2_out) {
  __shared__ uint64_t s_planes[4][2][3][kMergeWords + 1];      // per wave: [0] r1 as it is, [1] the reverse complement of r2
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint64_t (*P1)[kMergeWords + 1] = s_planes[wv][0];
  uint64_t (*P2)[kMergeWords + 1] = s_planes[wv][1];
  auto wave_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  for (size_t pair = (size_t)blockIdx.x * 4 + wv; pair < n; pair += (size_t)gridDim.x * 4) {
    const uint64_t a1 = offs1[pair], a2 = offs2[pair];
    const uint8_t *r1 = bases1 + a1, *r2 = bases2 + a2;
    const int len1 = (int)(offs1[pair + 1] - a1), len2 = (int)(offs2[pair + 1] - a2);
    const int64_t tenth = ((int64_t)len1 + (int64_t)len2) / 10;
    const int min_overlap = tenth > 31 ? 31 : (int)tenth;
    const bool fast = len1 <= kMergeFastLen && len2 <= kMergeFastLen;
    if (fast) {
      const int nw = ((len1 > len2 ? len1 : len2) + 63) >> 6;          // words in use; one more (zero) word for the funnel shift
      for (int w = 0; w <= nw; ++w) {
        const int p = w * 64 + (int)lane;
        const uint32_t c1 = p < len1 ? merge_code_raw(r1[p]) : 0u;
        const uint32_t c2 = p < len2 ? merge_code_comp(r2[len2 - 1 - p]) : 0u;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const unsigned long long m1 = __ballot((c1 >> b) & 1u), m2 = __ballot((c2 >> b) & 1u);
          if (lane == (uint32_t)b) { P1[b][w] = m1; P2[b][w] = m2; }
        }
      }
      wave_sync();
    }
    int cnt = 0, last = -1, k = 0, ov = -1, off = -1;
    // read through: first = rc(r2), second = r1, no tandem check
    if (fast) merge_pass_planes(P2, P1, len2, len1, min_overlap, lane, cnt, last);
    else merge_pass_bytes<true>(r1, len1, r2, len2, min_overlap, lane, cnt, last);
    if (last >= 0) off = last;
    if (cnt == 1) {
      k = 2;
      ov = len2 - last < len1 ? len2 - last : len1;
    } else {
      // plain overlap: first = r1, second = rc(r2)
      if (fast) merge_pass_planes(P1, P2, len1, len2, min_overlap, lane, cnt, last);
      else merge_pass_bytes<false>(r1, len1, r2, len2, min_overlap, lane, cnt, last);
      if (last >= 0) off = last;
      if (cnt == 1) {
        const int K = len1 - last < len2 ? len1 - last : len2;
        bool tandem = false;
        if (K <= 2 * min_overlap) {       // K <= 62: lane i tests the repeat size i (ReadPairMerger.hpp:57-79): every full block equals the first
          bool t = false;
          const int i = (int)lane;
          if (i >= 1 && i <= K / 2) {
            t = true;
            const int m = (K / i) * i;
            for (int x = i; x < m; ++x)
              if (merge_comp_char(r2[len2 - 1 - x]) != merge_comp_char(r2[len2 - 1 - (x - i)])) { t = false; break; }
          }
          tandem = __ballot(t) != 0ull;
        }
        if (!tandem) { k = 1; ov = K; }
      }
    }
    if (lane == 0) {
      kind[pair] = k; overlap[pair] = ov; offset[pair] = off;
      len1_out[pair] = k == 2 ? (uint64_t)ov : k == 1 ? (uint64_t)off + (uint64_t)len2 : (uint64_t)len1;
      len2_out[pair] = k ? 0ull : (uint64_t)len2;
    }
    if (fast) wave_sync();                // the planes are overwritten by the next pair
  }
}

// The reads after the merge, one wave per pair, lanes along the bytes.  q1 / q2: the qualities (both or neither: without them the
// quality terms of ReadPairMerger.hpp:171-185, 211 drop out as its q1 != NULL tests do), compared as signed char; oq1 / oq2: the
// qualities of the new reads when the caller wants them (the parity probe), else nullptr
__global__ __launch_bounds__(256) void k_merge_write(const uint8_t *bases1, const uint64_t *offs1, const int8_t *q1, const uint8_t *bases2, const uint64_t *offs2,
                                                     const int8_t *q2, size_t n, const int32_t *kind, const int32_t *offset, const uint64_t *noffs1,
                                                     const uint64_t *noffs2, uint8_t *ob1, int8_t *oq1, uint8_t *ob2, int8_t *oq2) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  for (size_t pair = (size_t)blockIdx.x * 4 + wv; pair < n; pair += (size_t)gridDim.x * 4) {
    const uint64_t a1 = offs1[pair], a2 = offs2[pair];
    const uint64_t len1 = offs1[pair + 1] - a1, len2 = offs2[pair + 1] - a2;
    const uint8_t *r1 = bases1 + a1, *r2 = bases2 + a2;
    const int8_t *qa = q1 ? q1 + a1 : nullptr, *qb = q2 ? q2 + a2 : nullptr;
    const uint64_t d1 = noffs1[pair], m = noffs1[pair + 1] - d1, d2 = noffs2[pair];
    const int k = kind[pair];
    const uint64_t off = k ? (uint64_t)offset[pair] : 0;
    if (k == 0) {
      for (uint64_t i = lane; i < len1; i += 64) { ob1[d1 + i] = r1[i]; if (oq1 && qa) oq1[d1 + i] = qa[i]; }
      for (uint64_t i = lane; i < len2; i += 64) { ob2[d2 + i] = r2[i]; if (oq2 && qb) oq2[d2 + i] = qb[i]; }
    } else if (k == 2) {                  // read through: r1[0 .. overlapSize), the mate's base where its quality is higher or r1 has 'N'
      for (uint64_t i = lane; i < m; i += 64) {
        uint8_t c = r1[i];
        int8_t q = 0;
        if (qa) {
          q = qa[i];
          const uint64_t p = len2 - 1 - (i + off);
          const int8_t mq = qb[p];
          if (mq > q || c == 'N') { c = merge_comp_char(r2[p]); q = mq; }
        }
        ob1[d1 + i] = c;
        if (oq1 && qa) oq1[d1 + i] = q;
      }
    } else {                              // overlap: offset + len2 bases; r1's base in front of the overlap, and inside it unless the mate's quality wins by more than 14
      for (uint64_t i = lane; i < m; i += 64) {
        uint8_t c = 0;
        int8_t q = 0;
        bool take_r1 = i < off;
        if (!take_r1) {
          const uint64_t p = len2 - 1 - (i - off);
          c = merge_comp_char(r2[p]);
          if (qb) q = qb[p];
          take_r1 = i < len1 && ((qa && (int)qa[i] >= (int)q - 14) || c == 'N');
        }
        if (take_r1) { c = r1[i]; if (qa) q = qa[i]; }
        ob1[d1 + i] = c;
        if (oq1 && qa) oq1[d1 + i] = q;
      }
    }
  }
}

}  // namespace cfr
