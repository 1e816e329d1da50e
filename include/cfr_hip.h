/*
 * cfr_hip.h — C-ABI of libcfr_hip.so: the MI355X (gfx950) replacement for Centrifuger's
 * per-read classification hot path.
 *
 * The reference has no FFI layer; the seam this library replaces is the per-batch thread
 * fan-out around Classifier<Sequence_RunBlock>::Query:
 *
 *   reference                                                   this library
 *   ---------------------------------------------------------   ---------------------------
 *   Classifier::Init(idxPrefix, param)   Classifier.hpp:902-947  cfr_index_open + cfr_device_index_create
 *   FMIndex::Load / Taxonomy::Load       FMIndex.hpp:588-606,    (inside cfr_index_open)
 *                                        Taxonomy.hpp:1259-1287
 *   pthread_create(ClassifyReads_Thread) CentrifugerClass.cpp:   cfr_classify_batch
 *     ... Query(r1, r2, result) ...        681-688, 240-340,
 *                                          Classifier.hpp:950-961
 *   SearchForwardAndReverse              Classifier.hpp:509-583  cfr_search_batch  (device)
 *   FMIndex::BackwardToSampledSA         FMIndex.hpp:514-524     cfr_locate_rows   (device)
 *   FMIndex::Rank / Sequence::Access     FMIndex.hpp:352-362,    cfr_rank_batch    (device; parity probe of
 *                                        Sequence.hpp:44-55                          the "operator API" of the path)
 *   FMIndex::BackwardSearch              FMIndex.hpp:487-510     cfr_backward_search_batch (device probe)
 *   ResultWriter::Output                 ResultWriter.hpp:199-242 cfr_format_tsv
 *
 * Conventions: plain pointers and sizes only; the caller owns every host buffer; the library
 * owns device memory.  Every call returns a cfr_status; cfr_last_error() gives the message of
 * the last failing call on this thread.  The library never calls exit().  There is NO CPU
 * fallback: without a usable HIP device cfr_device_index_create fails with CFR_ERR_NO_DEVICE.
 *
 * Reads are passed as one flat ASCII buffer plus n+1 byte offsets (no terminators), already
 * dust-masked if the caller wants dust (the reference masks before Query,
 * CentrifugerClass.cpp:276-316; cfr_dust_mask_batch does the same on the host).
 */
#ifndef CFR_HIP_H
#define CFR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int cfr_status;
enum {
  CFR_OK = 0,
  CFR_ERR_IO = 1,          /* cannot open / short read */
  CFR_ERR_FORMAT = 2,      /* malformed or unsupported .cfr content */
  CFR_ERR_NO_DEVICE = 3,   /* no HIP device / HIP runtime error at setup */
  CFR_ERR_HIP = 4,         /* HIP runtime error during a batch */
  CFR_ERR_ARG = 5,         /* bad argument */
  CFR_ERR_CAPACITY = 6,    /* caller-provided output buffer too small */
  CFR_ERR_BUSY = 7         /* another thread is inside a call on this device index, or too many batches are queued */
};

typedef struct cfr_index cfr_index;           /* host copy of <prefix>.{1,2,4}.cfr */
typedef struct cfr_dev_index cfr_dev_index;   /* flat image of the index in one GPU's HBM */

/* _classifierParam (Classifier.hpp:17-38) */
typedef struct {
  int32_t max_result;               /* -k, default 1 */
  int32_t min_hit_len;              /* --min-hitlen, <=0: infer (Classifier.hpp:113-129) */
  int32_t max_result_per_hit_factor;/* --hitk-factor, default 40 */
  int32_t output_expanded;          /* --expand-taxid (outputExpandedResult, Classifier.hpp:22): keep, for every reported tax id, the ids that
                                       ReduceTaxIds / LCA promoted into it; they are handed out by cfr_classify_batch_expanded */
  uint64_t consider_secondary_hit_len;     /* 2000 */
  double consider_secondary_score_factor;  /* 0.995 */
} cfr_params;

/* _BWTHit (Classifier.hpp:70-85) */
typedef struct {
  uint64_t sp, ep;
  int32_t l, strand, offset, pad;
} cfr_hit;

/* _classifierResult (Classifier.hpp:41-59) as POD.  Matches live in a separate array:
 * read i owns matches [match_begin, match_begin + n_match). */
typedef struct {
  uint64_t score, secondary_score;
  int32_t hit_length, query_length;
  int32_t n_match;            /* 0 = unclassified */
  int32_t pad;
  uint64_t match_begin;
} cfr_result;

typedef struct {
  uint64_t id;       /* kind 0: seqId (name = sequence name); kind 1: compact tax id (name = rank string) */
  uint64_t taxid;    /* ORIGINAL tax id (column 3 of the TSV) */
  int32_t kind, pad;
} cfr_match;

/* index geometry, for tests and sizing */
typedef struct {
  uint64_t n;                  /* BWT length */
  uint64_t first_isa;
  uint64_t block_size;         /* run-block b (== n when built with --rbbwt-b 1) */
  uint64_t precompute_width;   /* ftab chars */
  uint64_t sample_rate;
  uint64_t selected_cnt;
  uint64_t seq_cnt, node_cnt;
  int32_t min_hit_len;         /* after inference */
  char last_chr;
  uint8_t is_protein;          /* 1: amino-acid index (.4.cfr sequence_type amino_acid): reads are searched translated, never dust-masked */
  char pad[2];
  uint64_t device_bytes;       /* 0 for a host index */
} cfr_index_info;

/* kernel timing of the last batch call on a device index (HIP events on the library's stream) */
typedef struct {
  float pack_ms, search_ms, adjust_ms, rows_ms, locate_ms, tail_ms, total_ms;
  uint64_t n_chains, n_hits, n_rows;   /* n_hits / n_rows stay 0 on the paths that never need those totals on the host (fused tail; one-launch post stage) */
} cfr_batch_stats;

void cfr_params_default(cfr_params *p);
const char *cfr_last_error(void);
const char *cfr_version(void);

/* ---- index lifetime ---- */
cfr_status cfr_index_open(const char *idx_prefix, const cfr_params *params, cfr_index **out);
void cfr_index_destroy(cfr_index *idx);
cfr_status cfr_index_get_info(const cfr_index *idx, cfr_index_info *info);
/* A 64-bit digest (FNV-1a) of everything cfr_index_open parsed - scalars, bit strings, tables, taxonomy, inferred parameters.
 * Two opens of the same files with the same parameters give the same value (what the open/destroy stress test asserts); no
 * reference counterpart. */
cfr_status cfr_index_digest(const cfr_index *idx, uint64_t *digest);
/* How many bytes of the index's bit strings this handle reads straight from the read-only mapping of the .1.cfr file (the ranks of a node
 * share those pages through the page cache) and how many it holds as private copies.  A nucleotide index opened normally maps all of
 * them; a protein index is decoded into the process and maps none.  No reference counterpart (FMIndex::Load reads everything,
 * FMIndex.hpp:588-606). */
cfr_status cfr_index_mapped_bytes(const cfr_index *idx, uint64_t *mapped, uint64_t *copied);

cfr_status cfr_device_count(int *count);
cfr_status cfr_device_index_create(const cfr_index *idx, int device, cfr_dev_index **out);

/* What the device image is built with.  Nothing here changes a result; it trades load time and HBM for throughput.
 * cfr_device_index_create == cfr_device_index_create_ex with the defaults.  (The CFR_* environment variables listed in
 * profiles/HISTORY.md section 5 override these fields when set: they exist for A/B runs and for the variant tests.) */
typedef enum { CFR_PROFILE_THROUGHPUT = 0, CFR_PROFILE_FAST_LOAD = 1, CFR_PROFILE_BALANCED = 2 } cfr_profile;
typedef struct {
  int32_t profile;        /* cfr_profile.  FAST_LOAD: K-mer table of at most 4^13 entries, no text-mode tables, no locate memo
                             (shortest load).  BALANCED: the 4^13 table WITH the text-mode tables and the locate memo (no 68 GB
                             allocation: what the command line uses).  THROUGHPUT: everything, K up to 17 */
  int32_t ftabx_width;    /* K of the derived K-mer table; -1 = automatic (17 with 8-byte entries - 137 GB - for indexes of 2.7e8 symbols and more when it fits, else log4(n)+2, at most 16), 0 = none */
  int32_t text_mode;      /* derived SA / ISA / 2-bit text (n < 2^32): -1 = by profile, 0 = off, 1 = on */
  int32_t run_block_layout; /* 1 = keep the run-block components compressed in HBM instead of the flat occurrence image */
  double loc_memo_gb;     /* byte budget of the locate memo in GB; negative = by profile (16 / none), 0 = none */
  uint64_t sub_batch;     /* reads per sub-batch of one batch call; 0 = default */
} cfr_device_options;
void cfr_device_options_default(cfr_device_options *o);
cfr_status cfr_device_index_create_ex(const cfr_index *idx, int device, const cfr_device_options *options, cfr_dev_index **out);
void cfr_device_index_destroy(cfr_dev_index *d);
cfr_status cfr_device_index_get_info(const cfr_dev_index *d, cfr_index_info *info);

/* ---- primitive probes (device): used by the parity tests of L0-L2 ---- */
/* FMIndex::Rank(c, pos, inclusive) and Sequence::Access(pos) for n queries.
 * chars[i] in "ACGT"; out_rank may be NULL, out_access may be NULL. */
cfr_status cfr_rank_batch(cfr_dev_index *d, const char *chars, const uint64_t *pos, const uint8_t *inclusive,
                          size_t n, uint64_t *out_rank, char *out_access);
/* FMIndex::BackwardSearch(s = read[0..m), m): out_l / out_sp / out_ep (sp,ep untouched -> value 0 when l==0 path) */
cfr_status cfr_backward_search_batch(cfr_dev_index *d, const uint8_t *bases, const uint64_t *offsets,
                                     const uint32_t *m, size_t n, uint64_t *out_l, uint64_t *out_sp, uint64_t *out_ep);
/* FMIndex::BackwardToSampledSA(row): value (a sequence id) and LF-step count */
cfr_status cfr_locate_rows(cfr_dev_index *d, const uint64_t *rows, size_t n, uint64_t *out_val, uint32_t *out_steps);

/* Self-check of the tables the device image derives at load time, against the BWT itself (no reference counterpart: the
 * reference has no derived tables).  out[0..3] = number of rows where the suffix array (SA[i] < n, 0 exactly at the row of text
 * position 0), the text (symbol left of SA[i] = B[i]), the LF order (SA[LF(i)] = SA[i] - 1) and the direct locate (memo, or
 * suffix array + step function; every 61st row, against the plain FMIndex::BackwardToSampledSA walk) disagree - all 0 on a sound
 * image; out[4] = 1 if the text-mode tables exist, out[5] = 0 without a locate memo, else 1 + log2 of its row rate. */
cfr_status cfr_selfcheck_tables(cfr_dev_index *d, uint64_t out[6]);

/* ---- the path ---- */
/* SearchForwardAndReverse for n reads (mates optional: bases2/offsets2 == NULL for single-end).
 * hits of read i are out_hits[hit_begin[i] .. hit_begin[i+1]) ; hit_begin has n+1 entries.
 * out_hits capacity in elements = hit_cap ; CFR_ERR_CAPACITY if too small (needed size in hit_begin[n]). */
cfr_status cfr_search_batch(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1,
                            const uint8_t *bases2, const uint64_t *offsets2, size_t n,
                            cfr_hit *out_hits, size_t hit_cap, uint64_t *hit_begin);

/* Query for n reads, entirely on the device (search, locate, scoring, LCA / tax-id reduction).
 * results: n entries.  Matches of read i are matches[results[i].match_begin .. +n_match):
 *   max_result  > 0: match_begin = i * max_result (slots a read does not use are left untouched);
 *   max_result <= 0: match_begin = the read's offset in the located-row space.
 * *n_matches receives the number of match SLOTS the call needs (the extent of the matches array);
 * CFR_ERR_CAPACITY if match_cap is smaller.  Host buffers in, host buffers out (any host memory works;
 * memory from cfr_host_alloc is pinned and transfers at PCIe rate). */
cfr_status cfr_classify_batch(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1,
                              const uint8_t *bases2, const uint64_t *offsets2, size_t n,
                              cfr_result *results, cfr_match *matches, size_t match_cap, size_t *n_matches);

/* The same call with the bases in PACKED form: block b (one uint64_t) holds the 16 characters [16 b, 16 b + 16) of the flat buffer
 * the offsets refer to - character j of the block as a 2-bit code (A 0, C 1, G 2, T 3) at bits 2j..2j+1, and bit 32 + j set when
 * the character is one of the upper-case letters A, C, G, T (anything else - N, lower case, IUPAC codes, bytes past the end of the
 * buffer - has the bit clear and code bits that do not matter).  (total + 15) / 16 blocks per buffer.  Half the bytes of the ASCII
 * form cross PCIe (the ASCII entry is bound by its 1 byte per base: 3.2e8 reads/s of 150 bp from pinned memory); results are those of
 * cfr_classify_batch on the same reads, SDUST on the device included when it is switched on - nothing on the path tells two
 * non-symbols apart (a non-symbol ends a match, FMIndex.hpp:396-401; is SDUST's fifth code; reverse-complements to 'N',
 * Classifier.hpp:846-856).  Nucleotide indexes only: the translated search of a protein index does tell them apart (DnaToAa,
 * Classifier.hpp:131-241), so the call returns CFR_ERR_ARG there.  cfr_pack_reads makes the blocks from an ASCII buffer on `threads` host threads (a parser can also
 * emit them directly).  The reference reads ASCII through kseq (ReadFiles.hpp:337); there is no packed form there. */
cfr_status cfr_pack_reads(const uint8_t *bases, uint64_t total, int threads, uint64_t *packed);
cfr_status cfr_classify_batch_packed(cfr_dev_index *d, const uint64_t *packed1, const uint64_t *offsets1,
                                     const uint64_t *packed2, const uint64_t *offsets2, size_t n,
                                     cfr_result *results, cfr_match *matches, size_t match_cap, size_t *n_matches);

/* cfr_classify_batch with the lists of `--expand-taxid` (Classifier.hpp:792-838; Taxonomy::ReduceTaxIds / LCA with
 * promotedChildTaxIds, Taxonomy.hpp:733-973): for every match slot m of `matches` the ORIGINAL tax ids (GetOrigTaxId) of the
 * children that were promoted into matches[m] are ids[spans[m].begin .. spans[m].begin + spans[m].count), in the order the
 * reference prints them; count 0 = the empty string (every sequence-level match, Classifier.hpp:792-795).  The index must have
 * been opened with cfr_params.output_expanded = 1 (CFR_ERR_ARG otherwise).  spans: match_cap entries, every one is written.
 * *n_ids = ids used; CFR_ERR_CAPACITY (and *n_ids = the number needed) when ids_cap is too small.  SDUST on the device and the
 * streamed upload work as in cfr_classify_batch. */
typedef struct { uint64_t begin, count; } cfr_span;
cfr_status cfr_classify_batch_expanded(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1,
                                       const uint8_t *bases2, const uint64_t *offsets2, size_t n,
                                       cfr_result *results, cfr_match *matches, cfr_span *spans, size_t match_cap, size_t *n_matches,
                                       uint64_t *ids, size_t ids_cap, size_t *n_ids);

/* Asynchronous form of cfr_classify_batch.  The reference overlaps reading, classification and output of consecutive batches
 * (CentrifugerClass.cpp:776-800: the next batch is read while the threads classify this one); a caller of this library gets the
 * same by submitting batch k+1 before it waits for batch k:
 *   cfr_classify_batch_submit  queues the call and returns at once with a ticket.  Every buffer handed over (reads, offsets,
 *                              results, matches) must stay valid and untouched until the ticket has been waited for.
 *   cfr_classify_batch_wait    blocks until that batch is done, returns ITS status (cfr_last_error() then holds its message)
 *                              and, through n_matches, what cfr_classify_batch would have stored there.  A ticket is waited
 *                              for exactly once.
 * Batches of one cfr_dev_index run in submission order on the index's own worker thread; at most CFR_MAX_PENDING may be
 * outstanding (CFR_ERR_BUSY beyond that).  cfr_device_index_destroy waits for queued batches first.
 * One cfr_dev_index serves one call at a time: a synchronous entry (classify / search / probes / dust) called while another
 * thread - or a queued batch - is inside the same cfr_dev_index returns CFR_ERR_BUSY instead of racing on its buffers. */
#define CFR_MAX_PENDING 8
typedef uint64_t cfr_ticket;
cfr_status cfr_classify_batch_submit(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1,
                                     const uint8_t *bases2, const uint64_t *offsets2, size_t n,
                                     cfr_result *results, cfr_match *matches, size_t match_cap, cfr_ticket *ticket);
cfr_status cfr_classify_batch_wait(cfr_dev_index *d, cfr_ticket ticket, size_t *n_matches);

/* Same, with the read buffers ALREADY RESIDENT in this device's HBM (device pointers; the caller has
 * synchronised whatever produced them).  This is the entry bench.py times. */
cfr_status cfr_classify_batch_resident(cfr_dev_index *d, const void *d_bases1, const void *d_offsets1,
                                       const void *d_bases2, const void *d_offsets2, size_t n,
                                       uint64_t total_bases1, uint64_t total_bases2,
                                       cfr_result *results, cfr_match *matches, size_t match_cap, size_t *n_matches);

/* The same call with the results in a narrow layout: 20 + 12 bytes per read and match slot instead of 40 + 24.  At several
 * hundred million reads per second the step is co-limited by the device-to-host copy of its results (64 bytes per single-end
 * read, 160 per pair with -k 5); the fields are the same, in the widths they need for reads below 64 k bases.
 *   max_result > 0 only; the match slots of read i are [i * max_result, i * max_result + n_match) (no match_begin field).
 *   The match slots a read does not use are zero.
 *   A read one of whose values does not fit (score >= 2^32, sequence id >= 2^31 ...) has CFR_COMPACT_WIDE set in `flags`: its
 *   other fields are not meaningful; cfr_compact_wide_reads hands out such reads in the wide layout (no second pass over the batch). */
#define CFR_COMPACT_WIDE 1u
typedef struct {
  uint32_t score, secondary_score;
  uint32_t hit_length, query_length;
  uint8_t n_match, flags;
  uint16_t pad;
} cfr_result_compact;                 /* 20 bytes */
typedef struct {
  uint32_t id_kind;                   /* bit 31: kind (cfr_match.kind), bits 0..30: id */
  uint32_t taxid_lo, taxid_hi;        /* ORIGINAL tax id */
} cfr_match_compact;                  /* 12 bytes */
cfr_status cfr_classify_batch_resident_compact(cfr_dev_index *d, const void *d_bases1, const void *d_offsets1,
                                               const void *d_bases2, const void *d_offsets2, size_t n,
                                               uint64_t total_bases1, uint64_t total_bases2,
                                               cfr_result_compact *results, cfr_match_compact *matches, size_t match_cap, size_t *n_matches);
/* The reads of the LAST cfr_classify_batch_resident_compact call on d that carry CFR_COMPACT_WIDE, in the wide layout: *n of them,
 * read_index[j] = which read of the batch, results[j] = its cfr_result with match_begin pointing into matches[] (max_result slots
 * per entry).  The arrays belong to d and stay valid until its next classify call.  CFR_ERR_CAPACITY (and *n = their number)
 * if the batch held more than 65536 such reads: take cfr_classify_batch_resident for it. */
cfr_status cfr_compact_wide_reads(cfr_dev_index *d, size_t *n, const uint32_t **read_index, const cfr_result **results, const cfr_match **matches);

/* pinned host memory for result buffers (hipHostMalloc); NULL on failure */
void *cfr_host_alloc(size_t bytes);
void cfr_host_free(void *p);

cfr_status cfr_last_batch_stats(const cfr_dev_index *d, cfr_batch_stats *st);

/* Host-only tail of Query: GetClassificationFromHits (Classifier.hpp:585-843) once the device has
 * produced the hits and the located sequence ids.  hits of read i: [hit_begin[i], hit_begin[i+1]);
 * located ids of hit h: row_vals[row_begin[h] .. row_begin[h+1]).  query_len[i] = strlen(r1)+strlen(r2). */
cfr_status cfr_classify_from_hits(const cfr_index *idx, const cfr_hit *hits, const uint64_t *hit_begin,
                                  const uint64_t *row_begin, const uint64_t *row_vals, const int32_t *query_len,
                                  size_t n, int threads, cfr_result *results, cfr_match *matches, size_t match_cap,
                                  size_t *n_matches);

/* cfr_classify_from_hits with the lists of --expand-taxid (see cfr_classify_batch_expanded; idx opened with output_expanded = 1) */
cfr_status cfr_classify_from_hits_expanded(const cfr_index *idx, const cfr_hit *hits, const uint64_t *hit_begin,
                                           const uint64_t *row_begin, const uint64_t *row_vals, const int32_t *query_len,
                                           size_t n, int threads, cfr_result *results, cfr_match *matches, cfr_span *spans, size_t match_cap,
                                           size_t *n_matches, uint64_t *ids, size_t ids_cap, size_t *n_ids);

/* ---- host helpers around the path ---- */
/* SDUST pre-step (Dustmasker.hpp:357-421 + CentrifugerClass.cpp:283-289): masked bases -> 'N', in place */
cfr_status cfr_dust_mask_batch(uint8_t *bases, const uint64_t *offsets, size_t n, int threads);
/* the same masks computed with the reference's data structure as it is (a list of perfect intervals that reaches 1711 entries on a
 * homopolymer and is rescanned per window suffix: milliseconds per poly-A read); the anchor the two fast forms are tested against */
cfr_status cfr_dust_mask_batch_literal(uint8_t *bases, const uint64_t *offsets, size_t n, int threads);

/* The same masking on the device.  cfr_device_index_set_dust(d, 1): every following cfr_classify_batch /
 * cfr_classify_batch_resident call on d masks its reads in HBM before searching them (the caller's buffers are not modified),
 * so unmasked reads can be handed over and the host pre-step disappears; results equal cfr_dust_mask_batch + classify.
 * cfr_dust_mask_device: the device scan alone, host buffer in and out (parity probe). */
cfr_status cfr_device_index_set_dust(cfr_dev_index *d, int on);
cfr_status cfr_dust_mask_device(cfr_dev_index *d, uint8_t *bases, const uint64_t *offsets, size_t n);

/* ---- --merge-readpair: overlapping mates merged into one read before SDUST and Query (ReadPairMerger::Merge,
 * ReadPairMerger.hpp:132-233, called at CentrifugerClass.cpp:271-273) ----
 * A pair whose mates overlap (kind 1) or whose fragment is shorter than the reads (read-through, kind 2) becomes
 * read 1 = the merged read, read 2 = empty; the result of classifying that pair is the reference's Query(rm, NULL).  Every other
 * pair (kind 0) stays as it is.  qual1 / qual2: the quality characters of the mates, laid out by the same offsets as the bases;
 * both NULL for FASTA input, and CFR_ERR_ARG when only one is given (the reference dereferences a null pointer there).
 *
 * cfr_merge_pairs: the merge on `threads` host threads (the literal restatement of the reference; what the kernels are tested
 *   against).  out_bases1 / out_qual1: room for total1 + total2 bytes; out_bases2 / out_qual2: total2 bytes; out_offsets*: n + 1
 *   entries.  kind / overlap / offset (n entries each, any may be NULL): the return value of Merge and what it leaves in
 *   overlapSize / offset (for kind 0: -1 and the last offset that passed either test, or -1).  out_qual* may be NULL (always without
 *   qualities): the merged qualities are then not handed out.
 * cfr_merge_pairs_device: the same through the device kernels, host buffers in and out (parity probe). */
cfr_status cfr_merge_pairs(const uint8_t *bases1, const uint64_t *offsets1, const char *qual1,
                           const uint8_t *bases2, const uint64_t *offsets2, const char *qual2, size_t n, int threads,
                           uint8_t *out_bases1, uint64_t *out_offsets1, char *out_qual1,
                           uint8_t *out_bases2, uint64_t *out_offsets2, char *out_qual2,
                           int32_t *kind, int32_t *overlap, int32_t *offset);
cfr_status cfr_merge_pairs_device(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1, const char *qual1,
                                  const uint8_t *bases2, const uint64_t *offsets2, const char *qual2, size_t n,
                                  uint8_t *out_bases1, uint64_t *out_offsets1, char *out_qual1,
                                  uint8_t *out_bases2, uint64_t *out_offsets2, char *out_qual2,
                                  int32_t *kind, int32_t *overlap, int32_t *offset);
/* cfr_device_index_set_merge(d, 1): every following cfr_classify_batch_merged / cfr_classify_batch_resident_merged call on d merges
 * its pairs in HBM first (then SDUST when cfr_device_index_set_dust is on, then the search); the caller's buffers are not modified.
 * Switched off (the default) those two calls are cfr_classify_batch / cfr_classify_batch_resident.  A single-end batch is classified
 * as it is either way.  The other entries never merge; cfr_classify_batch_packed returns CFR_ERR_ARG while the switch is on (the
 * packed form cannot tell 'N' from other bytes, the merge compares them).  CFR_ERR_ARG on a protein index.
 * merge_kind: n entries (may be NULL), the kind of every pair (all 0 when nothing was merged).
 * cfr_last_merge_ms: device time of the merge pre-step of the last such call (0 when it did not run). */
cfr_status cfr_device_index_set_merge(cfr_dev_index *d, int on);
cfr_status cfr_classify_batch_merged(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1, const char *qual1,
                                     const uint8_t *bases2, const uint64_t *offsets2, const char *qual2, size_t n,
                                     cfr_result *results, cfr_match *matches, size_t match_cap, size_t *n_matches, int32_t *merge_kind);
cfr_status cfr_classify_batch_resident_merged(cfr_dev_index *d, const void *d_bases1, const void *d_offsets1, const void *d_qual1,
                                              const void *d_bases2, const void *d_offsets2, const void *d_qual2, size_t n,
                                              uint64_t total_bases1, uint64_t total_bases2,
                                              cfr_result *results, cfr_match *matches, size_t match_cap, size_t *n_matches, int32_t *merge_kind);
cfr_status cfr_last_merge_ms(const cfr_dev_index *d, float *ms);

/* ResultWriter::Output rows for one read (ResultWriter.hpp:209-240).  Returns bytes needed (without the NUL); writes at most cap and always
 * NUL-terminates a non-empty buffer: a return value >= cap means the text was cut at cap - 1 and the caller retries with value + 1. */
size_t cfr_format_tsv(const cfr_index *idx, const char *read_id, const cfr_result *r, const cfr_match *matches,
                      char *buf, size_t cap);
const char *cfr_tsv_header(void);
/* the same rows with the expandedTaxIDs column of --expand-taxid (ResultWriter.hpp:194-195, 226-227, 239-240): spans / ids as
 * cfr_classify_batch_expanded filled them */
size_t cfr_format_tsv_expanded(const cfr_index *idx, const char *read_id, const cfr_result *r, const cfr_match *matches,
                               const cfr_span *spans, const uint64_t *ids, char *buf, size_t cap);
const char *cfr_tsv_header_expanded(void);

/* ---- centrifuger-quant: abundance estimation from read assignments (Quantifier, Quantifier.hpp; CentrifugerQuant.cpp) ----
 * cfr_quant_open reads <prefix>.2.cfr (taxonomy) and <prefix>.3.cfr (sequence lengths) only - never the FM index - and computes the
 * genome length of every tax id (Taxonomy::ConvertSeqLengthToTaxLength, Taxonomy.hpp:1111-1213).
 *   reference                                                      this library
 *   Quantifier::Init(idxPrefix)             Quantifier.hpp:432-458   cfr_quant_open
 *   Quantifier::LoadReadAssignments         :515-622                 cfr_quant_add_tsv      (plain, gz, "-" = stdin; several calls add up)
 *   Quantifier::AddReadAssignment           :624-637                 cfr_quant_add_results  (+ the filter of LoadReadAssignments)
 *   CoalesceAssignments                     :490-513                 cfr_quant_assignments  (device: k_quant_coalesce)
 *   Quantification / EstimateAbundanceWithEM :640-743, 186-281       cfr_quant_run          (device: the E-step of every round)
 *   Quantifier::Output                      :746-818                 cfr_quant_write
 * options.device >= 0: records are coalesced in that GPU's HBM and the E-step of every EM round runs there (CFR_ERR_NO_DEVICE
 * without it: no fall-back); device = -1: the host twin alone, no GPU is touched.  Both give the same bits: the coalesce sums
 * integers (a weight is 4^-d, d <= 11, summed in units of 2^-22), the E-step keeps the reference's order of additions.
 * A handle is used by one thread at a time. */
typedef struct cfr_quant cfr_quant;
typedef struct {
  uint64_t min_score;     /* --min-score: rows below it are dropped */
  int32_t min_length;     /* --min-length: rows whose hitLength is below it are dropped */
  int32_t device;         /* HIP device ordinal; -1: host twin only */
  uint64_t table_slots;   /* slots of the device coalesce table at the start (rounded up to a power of two, at least 64); 0 = default.
                             The table grows when it is half full: a small value only makes a test meet that path */
  int32_t threads;        /* threads of the TSV reader; 0 = automatic (at most 16) */
  int32_t pad;
} cfr_quant_options;
typedef struct {
  double reader_ms, coalesce_ms, em_ms;   /* wall time spent reading rows, coalescing (device: upload, kernels, growth, download; sort), in cfr_quant_run */
  uint64_t grow_count, table_slots;       /* device coalesce table: times it was grown, slots at the end (0 on the host twin) */
  int32_t em_rounds, pad;
} cfr_quant_stats;
void cfr_quant_options_default(cfr_quant_options *o);
cfr_status cfr_quant_open(const char *idx_prefix, const cfr_quant_options *o, cfr_quant **out);
/* rows of a classification TSV: the first line is the header; consecutive kept rows with one read id are one assignment */
cfr_status cfr_quant_add_tsv(cfr_quant *q, const char *path);
/* results as cfr_classify_batch left them: every read is its own assignment; n_match == 0 is unclassified; the filter and the weight
 * of the TSV path (score, hit_length, query_length, secondary_score) apply */
cfr_status cfr_quant_add_results(cfr_quant *q, const cfr_result *r, const cfr_match *m, size_t n);
/* The coalesced assignments in the reference's order (by size, then by the targets in order): list i is
 * targets[begin[i] .. begin[i + 1]) - compact tax ids, node_cnt for a tax id the tree does not hold.  The arrays belong to q.
 * Nothing can be added after this call or cfr_quant_run. */
cfr_status cfr_quant_assignments(cfr_quant *q, size_t *n, const uint64_t **begin, const uint32_t **targets, const double **weight,
                                 const uint64_t **count, const uint64_t **uniq);
cfr_status cfr_quant_run(cfr_quant *q, int32_t *em_rounds);
/* after cfr_quant_run: abund / read_count / uniq_count have node_cnt + 1 entries (compact tax ids), taxid_length node_cnt + 1; any may be NULL */
cfr_status cfr_quant_values(const cfr_quant *q, const double **abund, const double **read_count, const double **uniq_count,
                            const uint64_t **taxid_length, uint64_t *node_cnt);
/* format 0..3 as --output-format (0 centrifuge, 1 metaphlan, 2 CAMI, 3 kraken-report); path "-" = stdout */
cfr_status cfr_quant_write(const cfr_quant *q, int format, const char *path);
cfr_status cfr_quant_get_stats(const cfr_quant *q, cfr_quant_stats *st);
void cfr_quant_destroy(cfr_quant *q);
/* The E-step of EMupdate alone (Quantifier.hpp:196-208; parity probe of k_quant_estep_terms / k_quant_estep_sum and of their host
 * twin): assignment i has the targets a_target[a_begin[i] .. a_begin[i + 1]) (each below n_nodes; a_begin[0] = 0) and the weight
 * a_weight[i].  One E-step object is made through the seam cfr_quant_run uses (device >= 0: that GPU; -1: the host twin) and runs,
 * in this order, the init round (weight / targetCnt) if init_round != 0 and then n_rounds rounds, round k on the n_nodes doubles at
 * abund + k * n_nodes.  out_read_count receives every round's readCount, n_nodes doubles each: (init_round ? 1 : 0) + n_rounds vectors. */
cfr_status cfr_quant_estep_probe(int32_t device, const uint64_t *a_begin, const uint32_t *a_target, const double *a_weight, size_t n_assign,
                                 uint64_t n_nodes, int32_t init_round, const double *abund, size_t n_rounds, double *out_read_count);

/* ---- centrifuger-inspect: what an index prefix holds besides the FM index (CentrifugerInspect.cpp) ----
 * cfr_taxonomy_open reads <prefix>.2.cfr (Taxonomy::Load) and, with_lengths != 0, <prefix>.3.cfr (sequence id -> length) - never
 * .1.cfr - and hands out the tables bin/centrifuger-inspect prints.  The pointers belong to the handle.
 *   parent / orig_taxid / rank: node_cnt entries (compact tax ids; GetOrigTaxId, the rank codes of Taxonomy.hpp:25-59)
 *   seq_to_tax: seq_cnt entries; sequence names: n_seq_names of them (MapID: a name stored twice keeps its first id)
 *   taxid_length: node_cnt + 1 genome lengths (Taxonomy::ConvertSeqLengthToTaxLength, as cfr_quant_values hands them out)
 *   length_seq_id / length_value: the n_seq_lengths pairs of .3.cfr in ascending sequence-id order (a later pair replaced an earlier one)
 * taxid_length, length_seq_id and length_value are NULL when the handle was opened without lengths. */
typedef struct cfr_taxonomy cfr_taxonomy;
typedef struct {
  uint64_t node_cnt, seq_cnt, extra_seq_cnt, root;
  uint64_t n_seq_names, n_seq_lengths;
  const uint64_t *parent, *orig_taxid, *seq_to_tax;
  const uint8_t *rank;
  const uint64_t *taxid_length, *length_seq_id, *length_value;
} cfr_taxonomy_tables;
cfr_status cfr_taxonomy_open(const char *idx_prefix, int with_lengths, cfr_taxonomy **out);
cfr_status cfr_taxonomy_get_tables(const cfr_taxonomy *t, cfr_taxonomy_tables *tables);
const char *cfr_taxonomy_tax_name(const cfr_taxonomy *t, uint64_t compact_taxid);   /* Taxonomy::GetTaxIdName: "Unknown" beyond the tree */
const char *cfr_taxonomy_seq_name(const cfr_taxonomy *t, uint64_t seq_id);          /* NULL beyond n_seq_names */
const char *cfr_tax_rank_string(uint8_t rank);                                      /* Taxonomy::GetTaxRankString (Taxonomy.hpp:497-532) */
void cfr_taxonomy_close(cfr_taxonomy *t);
/* Taxonomy::LCA of n_lists lists of compact tax ids (list i = ids[begin[i] .. begin[i + 1]), every id below node_cnt), for tests.
 * form 0: the host tail's literal restatement (cfr_tail.cpp tax_lca); form 1: the fold the kernels use (csrc/cfr_tax_fold.hpp) with the
 * depth table of the device image.  out: n_lists results; steps (may be NULL; form 1): the fold's loop iterations per list. */
cfr_status cfr_taxonomy_lca_probe(const cfr_taxonomy *t, const uint64_t *ids, const uint64_t *begin, size_t n_lists, int32_t form,
                                  uint64_t *out, uint32_t *steps);

/* ---- centrifuger-promote: assignments rewritten to a chosen rank, or folded into their LCA (the reference's Perl script
 * centrifuger-promote:44-149; the semantics are stated in csrc/cfr_promote_core.hpp) ----
 * level: "lca" or a rank string ("genus", "species", "no rank" ...); a string that names no rank is legal and promotes nothing.
 * cfr_promote_open reads <prefix>.2.cfr only.  device = -1: the host twin alone, no GPU is touched; device >= 0: the kernels of
 *   cfr_promote.hip on that GPU (CFR_ERR_NO_DEVICE without it: no fall-back).
 * cfr_promote_apply: in place on results / matches as the classify entries leave them (host buffers in and out): read i owns
 *   matches[match_begin .. + n_match); the kept matches move to the front of the read's slots and n_match becomes their number.
 *   src_slot (may be NULL; as many entries as matches): for every kept match slot, the slot of `matches` the match came from.
 * cfr_promote_lca_warnings: the tax ids of the "Couldn't find parent of taxID ... - directly assigned to root." lines the script
 *   prints for these reads (as they are BEFORE cfr_promote_apply) in lca mode; none in rank mode.  Host only.  *count = their
 *   number; CFR_ERR_CAPACITY when cap is smaller (taxids may then be NULL).
 * A handle is used by one thread at a time; a handle that is not open (never was, or was closed) is CFR_ERR_ARG. */
typedef struct cfr_promote cfr_promote;
typedef struct {
  float table_ms;     /* device time of k_promote_table, which ran once when the handle was opened (0: host twin, lca) */
  float reads_ms;     /* device time of the per-read kernel of the last cfr_promote_apply (host twin: its wall time) */
} cfr_promote_stats;
cfr_status cfr_promote_open(const char *idx_prefix, const char *level, int device, cfr_promote **out);
cfr_status cfr_promote_apply(cfr_promote *h, cfr_result *results, cfr_match *matches, size_t n, uint64_t *src_slot);
cfr_status cfr_promote_lca_warnings(cfr_promote *h, const cfr_result *results, const cfr_match *matches, size_t n,
                                    uint64_t *taxids, size_t cap, size_t *count);
cfr_status cfr_promote_get_stats(cfr_promote *h, cfr_promote_stats *st);
cfr_status cfr_promote_close(cfr_promote *h);
/* cfr_device_index_set_promote(d, level): every following call of the wide classify entries (cfr_classify_batch, _resident,
 * _submit / _wait, _packed, _merged, _resident_merged) promotes its results in HBM - after the tail has written a sub-batch and
 * before the sub-batch is copied out, on the same stream, with the same kernels and the taxonomy tables of the image.  level NULL
 * switches it off (the default; nothing new is launched then).  While it is on, cfr_classify_batch_resident_compact and
 * cfr_classify_batch_expanded return CFR_ERR_ARG (the script cannot process the expanded column either).
 * cfr_last_promote_ms: device time of the promotion kernels of the last classify call, all sub-batches (0 when switched off). */
cfr_status cfr_device_index_set_promote(cfr_dev_index *d, const char *level);
cfr_status cfr_last_promote_ms(const cfr_dev_index *d, float *ms);

/* ---- centrifuger-kreport: the Kraken-style report, reads counted per taxon (the reference's Perl script centrifuger-kreport;
 * the semantics are stated in csrc/cfr_kreport_core.hpp) ----
 * Bins: node_cnt + 1 of them, the compact nodes and then "unclassified" (tax id 0).
 * cfr_kreport_open reads <prefix>.2.cfr only; a taxonomy without a node of tax id 1 is CFR_ERR_FORMAT.  device = -1: the host twin
 *   alone, no GPU is touched; device >= 0: the kernels of cfr_kreport.hip on that GPU (CFR_ERR_NO_DEVICE without it: no fall-back).
 * cfr_kreport_add_results: reads as the wide classify entries leave them (host buffers), unpromoted; read i owns
 *   matches[match_begin, match_begin + n_match).  Not with no_lca (CFR_ERR_ARG): that mode adds fractions in file order.
 * cfr_kreport_add_tsv: a classification file, plain or gz, "-" = stdin; columns are found by the names in its header line; rows are
 *   grouped by numMatches as the script does.  no_lca runs on the host, one thread, whatever `device` is.
 * cfr_kreport_add_count_table: rows of `taxID count` (the script's --is-count-table).  Host only.
 * cfr_kreport_add_counts: bins downloaded from device images (cfr_device_index_kreport_counts, below) added in; n = node_cnt + 1.
 * cfr_kreport_counts: own and clade counts, own and clade maximum scores (each node_cnt + 1 entries, any may be NULL) and the
 *   script's $seq_count; cap = entries every array given can take (CFR_ERR_CAPACITY below node_cnt + 1).
 * cfr_kreport_warnings: the tax ids of the "Couldn't find parent of taxID ... - directly assigned to root." lines the script
 *   prints for everything added so far, in its order.  *count = their number; CFR_ERR_CAPACITY when cap is smaller.
 * cfr_kreport_write: the report; path NULL or "-" = stdout.  Nothing counted: CFR_ERR_ARG with the script's message ("No sequence
 *   matches with given settings") in cfr_last_error(), and nothing is written. */
typedef struct cfr_kreport cfr_kreport;
typedef struct {
  int32_t has_min_score, has_min_length;   /* whether --min-score / --min-length were given */
  uint64_t min_score;
  int64_t min_length;
  int32_t no_lca, show_zeros, score_data;  /* --no-lca, --show-zeros, --report-score-data */
  uint32_t max_blocks;                     /* device: at most that many blocks per kernel (the lanes stride); 0 = as many as the reads need */
  uint32_t lds_slots;                      /* device: slots of the accumulate kernel's LDS table, a power of two in [64, 2048]; 0 = 1024 */
  int32_t threads;                         /* host twin: threads over the reads; 0 = up to 16 */
  int32_t pad;
} cfr_kreport_options;
typedef struct {
  float fold_ms;        /* device time of k_kreport_fold of the last cfr_kreport_add_results (host twin: its wall time) */
  float accumulate_ms;  /* ... of k_kreport_accumulate (host twin: 0) */
  float parse_ms;       /* wall time of reading and parsing files so far, without the add_results calls inside */
} cfr_kreport_stats;
void cfr_kreport_options_default(cfr_kreport_options *o);
cfr_status cfr_kreport_open(const char *idx_prefix, const cfr_kreport_options *opts, int device, cfr_kreport **out);
cfr_status cfr_kreport_add_results(cfr_kreport *h, const cfr_result *results, const cfr_match *matches, size_t n);
cfr_status cfr_kreport_scan_warnings(cfr_kreport *h, const cfr_result *results, const cfr_match *matches, size_t n);   /* the warning lines of these (unpromoted) reads alone, nothing counted: for reads a device image counts */
cfr_status cfr_kreport_add_tsv(cfr_kreport *h, const char *path);
cfr_status cfr_kreport_add_count_table(cfr_kreport *h, const char *path);
cfr_status cfr_kreport_add_counts(cfr_kreport *h, const uint64_t *own, const uint64_t *own_score, size_t n);
cfr_status cfr_kreport_bins(cfr_kreport *h, size_t *n);
cfr_status cfr_kreport_counts(cfr_kreport *h, uint64_t *own, uint64_t *clade, uint64_t *own_score, uint64_t *clade_score, size_t cap,
                              double *seq_count);
cfr_status cfr_kreport_warnings(cfr_kreport *h, uint64_t *taxids, size_t cap, size_t *count);
cfr_status cfr_kreport_write(cfr_kreport *h, const char *path);
cfr_status cfr_kreport_get_stats(cfr_kreport *h, cfr_kreport_stats *st);
cfr_status cfr_kreport_close(cfr_kreport *h);
/* cfr_device_index_set_kreport(d, opts): every following call of the wide classify entries (cfr_classify_batch, _resident, _submit /
 * _wait, _packed, _merged, _resident_merged) counts its reads into node_cnt + 1 bins that stay in the image's HBM: k_kreport_fold runs
 * per sub-batch behind the tail, in front of a promotion (the report sees unpromoted assignments), into arrays of the call;
 * k_kreport_accumulate runs once when the call has settled - a sub-batch or a batch that the pipeline computes a second time is
 * counted once, a call that fails is not counted.  opts NULL switches it off (the default; nothing is allocated or launched then);
 * switching it on zeroes the bins; no_lca is CFR_ERR_ARG, a taxonomy without tax id 1 CFR_ERR_FORMAT.  Only the filters of opts
 * matter here.  While it is on, cfr_classify_batch_resident_compact and cfr_classify_batch_expanded return CFR_ERR_ARG.
 * cfr_device_index_kreport_counts: waits for the image's stream and copies the bins out (own counts, own maximum scores; either may
 * be NULL; cap = entries each can take, CFR_ERR_CAPACITY below node_cnt + 1) and their sum; feed them to cfr_kreport_add_counts.
 * cfr_last_kreport_ms: device time of the report's kernels of the last classify call, all sub-batches (0 when switched off). */
cfr_status cfr_device_index_set_kreport(cfr_dev_index *d, const cfr_kreport_options *opts);
cfr_status cfr_device_index_kreport_counts(cfr_dev_index *d, uint64_t *own, uint64_t *own_score, size_t cap, double *seq_count);
cfr_status cfr_last_kreport_ms(const cfr_dev_index *d, float *ms);

/* ---- raw FASTA/FASTQ text -> flat bases + offsets (what ReadFiles.hpp:212-330 and kseq do line by line) ----
 * The tokeniser accepts "regular" text - 4-line FASTQ, FASTA whose sequence lines start with neither '@' nor '+' - and refuses the
 * rest rather than guessing; the grammar is stated in csrc/cfr_tokenize_core.hpp.  What it delivers is a prefix of what the
 * sequential grammar (kseq) reads from the same text; at the first record that breaks a rule it stops, says so (irregular,
 * irregular_at) and the caller continues there with a sequential reader.
 * The handle is its own, independent of any cfr_dev_index; one call at a time per handle.
 * cfr_tokenizer_open: device = -1: the host twin, no GPU is touched; device >= 0: the kernels of cfr_tokenize.hip on that GPU
 *   (CFR_ERR_NO_DEVICE without it: no fall-back).
 * cfr_tokenize: text[0] must be '>' or '@' and len below 2^32 (CFR_ERR_ARG otherwise; len = 0 is CFR_OK with nothing delivered).
 *   final != 0: the text ends here, so a last line without '\n' counts and the last FASTA record is complete.  max_records 0: no cap;
 *   otherwise n_records = min(cap, complete records, records before the irregular one).  consumed: the offset of the header line of
 *   the first record that was not delivered, or len.  n_records == 0 with consumed == 0 is CFR_OK: hand over more text.
 *   The call returns with its stream synchronised.
 * cfr_tokenizer_fetch: the result of the last cfr_tokenize to host memory; any pointer may be NULL; n_records records,
 *   n_records + 1 offsets, total_bases bases (ASCII, bytes as they are in the text).  The id of record r is the id_len bytes at
 *   text + header + 1.
 * cfr_tokenizer_device_reads: device handle only (CFR_ERR_ARG on the host twin): the flat bases and the 64-bit offsets in HBM, in
 *   the form cfr_classify_batch_resident takes; valid until the next cfr_tokenize or close on the handle.
 * cfr_tokenizer_get_stats: the parts of the last call's device_ms. */
typedef struct cfr_tokenizer cfr_tokenizer;
typedef struct { uint64_t header, qual; uint32_t header_len, id_len; } cfr_read_record;   /* 24 bytes; offsets into the text; qual = 0 for FASTA */
typedef struct {
  uint64_t n_records, consumed, total_bases;
  uint64_t irregular_at;      /* offset of the irregular record's header line; meaningful when irregular != 0 */
  int32_t fastq, irregular;
  double device_ms;           /* stream time of the last call: copy in, kernels, copies out (host twin: wall time) */
} cfr_token_info;
cfr_status cfr_tokenizer_open(int device, cfr_tokenizer **out);
cfr_status cfr_tokenize(cfr_tokenizer *t, const uint8_t *text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info);
cfr_status cfr_tokenizer_fetch(cfr_tokenizer *t, cfr_read_record *records, uint64_t *offsets, uint8_t *bases);
cfr_status cfr_tokenizer_device_reads(cfr_tokenizer *t, const void **d_bases, const void **d_offsets);
/* the parts of device_ms of the last cfr_tokenize, from events on the handle's stream (both 0 on the host twin) */
typedef struct {
  double copy_in_ms;          /* the text to the device, its padding */
  double kernel_ms;           /* the five kernels and the scans, the wait for the line count between them included */
} cfr_token_stats;
cfr_status cfr_tokenizer_get_stats(cfr_tokenizer *t, cfr_token_stats *st);
void cfr_tokenizer_close(cfr_tokenizer *t);

/* ---- the rows of a batch as one text (ResultWriter::Output, ResultWriter.hpp:199-242, for n reads at once; the semantics are stated
 * in csrc/cfr_tsv_core.hpp) ----
 * The bytes are those of cfr_format_tsv, read after read: the 8 columns, no header line, no NUL.  The barcode, UMI and expandedTaxIDs
 * columns are not made here.
 * cfr_tsv_open: the sequence names and rank codes of idx are copied (device >= 0: uploaded once, the kernels of cfr_tsv.hip run on that
 *   GPU; CFR_ERR_NO_DEVICE without it: no fall-back).  device = -1: the host twin on `threads` host threads, no GPU is touched.
 *   options (NULL = defaults; a field of 0 = its default): tile_bytes - a block of 256 reads whose rows take at most that many bytes
 *   builds them in LDS and streams them out with 16-byte stores, a longer span is written straight to HBM (16 .. 163776);
 *   max_blocks - at most that many blocks per kernel (the blocks stride).  Both exist for the tests.
 * cfr_tsv_format: results / matches as the wide classify entries leave them (host arrays): read i owns
 *   matches[match_begin, match_begin + n_match) when n_match > 0; n_slots = entries of matches.  id i = id_bytes[id_offsets[i],
 *   id_offsets[i + 1]).  *len = the bytes the text needs; more than cap: CFR_ERR_CAPACITY, *len set, nothing promised about text.
 *   row_offsets (may be NULL): n + 1 entries, the rows of read i are text[row_offsets[i], row_offsets[i + 1]).
 *   Checked on the host before anything is launched (CFR_ERR_ARG, cfr_last_error() names the read): null pointers, id_offsets that
 *   decrease, match_begin + n_match > n_slots.
 * cfr_tsv_get_stats: device times of the last cfr_tsv_format from events (the host twin: wall times of its two passes in len_ms and
 *   write_ms); blocks = blocks of 256 reads, direct_blocks = those that took the path straight to HBM.
 * A handle is used by one thread at a time. */
typedef struct cfr_tsv cfr_tsv;
typedef struct { int32_t tile_bytes, max_blocks, threads, pad; } cfr_tsv_options;
typedef struct { float upload_ms, len_ms, scan_ms, write_ms, download_ms; uint64_t blocks, direct_blocks; } cfr_tsv_stats;
void cfr_tsv_options_default(cfr_tsv_options *o);
cfr_status cfr_tsv_open(const cfr_index *idx, int device, const cfr_tsv_options *o, cfr_tsv **out);
cfr_status cfr_tsv_format(cfr_tsv *t, const cfr_result *results, const cfr_match *matches, size_t n_slots, size_t n,
                          const char *id_bytes, const uint64_t *id_offsets, char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets);
cfr_status cfr_tsv_get_stats(cfr_tsv *t, cfr_tsv_stats *st);
void cfr_tsv_close(cfr_tsv *t);
/* cfr_device_index_set_tsv(d, 1): every following call of the wide classify entries (cfr_classify_batch, _resident, _submit / _wait,
 * _packed, _merged, _resident_merged) keeps its final wide results in HBM, in arrays of the image: every sub-batch is copied device to
 * device behind its promotion (the rows are the promoted ones under cfr_device_index_set_promote), a sub-batch that is computed again
 * overwrites its slice; the host copies are delivered as before.  Needs max_result > 0 (CFR_ERR_ARG otherwise).  While it is on,
 * cfr_classify_batch_resident_compact and cfr_classify_batch_expanded return CFR_ERR_ARG.  Off (the default) nothing is allocated or
 * launched.
 * cfr_device_index_tsv_last: the rows of the LAST classify call from the kept arrays, as cfr_tsv_format gives them; ids are host
 *   bytes, uploaded by the call.  CFR_ERR_ARG if the switch was off for that call or a batch is queued, CFR_ERR_BUSY under the usual guard.
 * cfr_device_index_tsv_last_resident: the same with the ids where the tokeniser left them: d_text / d_records of
 *   cfr_tokenizer_device_records (mate 1's tokeniser for pairs) - id of read i = the id_len bytes at d_text + header + 1; no id
 *   crosses PCIe.  The records must be those of the reads of that call, in order.
 * cfr_last_tsv_ms: device time of the kernels of the last cfr_device_index_tsv_last* since the last classify call (0 when there was none). */
cfr_status cfr_device_index_set_tsv(cfr_dev_index *d, int on);
cfr_status cfr_device_index_tsv_last(cfr_dev_index *d, const char *id_bytes, const uint64_t *id_offsets,
                                     char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets);
cfr_status cfr_device_index_tsv_last_resident(cfr_dev_index *d, const void *d_text, const void *d_records,
                                              char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets);
cfr_status cfr_tokenizer_device_records(cfr_tokenizer *t, const void **d_text, const void **d_records);   /* device handle only; valid until the next cfr_tokenize / close */
cfr_status cfr_last_tsv_ms(const cfr_dev_index *d, float *ms);

/* ---- a text as BGZF members, and the --un / --cl read dumps made and compressed in one call (ResultWriter::OutputRead,
 * ResultWriter.hpp:254-275, for a batch at once; the framing, the encoder and the records are stated in csrc/cfr_gz_core.hpp) ----
 * BGZF is gzip cut into members of at most 64 KiB, each with its size in an extra field: every gunzip reads the concatenation, and
 * readers that know the field inflate the members in parallel.  The bytes are NOT those of zlib; what they inflate to is the contract.
 * cfr_gz_open: device >= 0: the kernels of cfr_gz.hip on that GPU (CFR_ERR_NO_DEVICE without it: no fall-back); device = -1: the host
 *   twin on `threads` host threads, the same bytes.  options (NULL = defaults; a field of 0 = its default): block_bytes - the input
 *   bytes per member, 1 .. 65280 (the default, htslib's); max_blocks - at most that many workgroups per kernel.  Both exist for the tests.
 *   codes - 0: every stream is fixed-Huffman or stored (the default); 1: dynamic mode - a member whose block is smaller with Huffman
 *   codes of its own (BTYPE 10) gets them, every other member has the bytes of codes = 0, so no member grows; anything else: CFR_ERR_ARG.
 * cfr_gz_compress: host text in; *out points at the members, back to back, in a buffer the handle owns until its next call.  No
 *   end-of-file member.  n = 0 gives *out_n = 0.
 * cfr_gz_dump: one call makes the text of up to 4 files and compresses each; on the device the text never exists on the host.  Read i
 *   has id id_bytes[id_off[i], id_off[i + 1]) in every file; select[i] = 0 leaves it out.  Its record in file f is
 *   ">id\nseq\n", or "@id\nseq\n+\nqual\n" where files[f].qual is not NULL and files[f].has_qual[i] is not 0.  A record of 8192 bytes
 *   or more is left out of that file alone (what gzprintf does with it).  out / out_n: n_files entries, as for cfr_gz_compress.
 * cfr_gz_eof: the 28-byte end-of-file member, to be written once behind the last member of a file (a file of it alone is an empty text).
 * cfr_gz_get_stats: the last call: device times from events (host twin: wall times of making the text and of compressing it in
 *   format_ms and deflate_ms), summed over the files of a dump; blocks = members, stored_blocks = those that hold a stored block,
 *   dynamic_blocks = those that hold a dynamic block (0 with codes = 0).
 * A handle is used by one thread at a time. */
typedef struct cfr_gz cfr_gz;
typedef struct { int32_t block_bytes, max_blocks, threads, codes; } cfr_gz_options;
typedef struct { float upload_ms, format_ms, deflate_ms, pack_ms, download_ms; uint32_t dynamic_blocks; uint64_t blocks, stored_blocks, bytes_in, bytes_out; } cfr_gz_stats;
typedef struct {
  const uint8_t *seq; const uint64_t *seq_off;      /* n + 1 offsets */
  const char *qual; const uint64_t *qual_off;       /* NULL, or n + 1 offsets */
  const uint8_t *has_qual;                          /* n bytes; may be NULL when qual is */
} cfr_gz_file;
void cfr_gz_options_default(cfr_gz_options *o);
cfr_status cfr_gz_open(int device, const cfr_gz_options *o, cfr_gz **out);
cfr_status cfr_gz_compress(cfr_gz *h, const void *text, uint64_t n, const uint8_t **out, uint64_t *out_n);
cfr_status cfr_gz_dump(cfr_gz *h, const char *id_bytes, const uint64_t *id_off, const uint8_t *select, size_t n,
                       const cfr_gz_file *files, int n_files, const uint8_t **out, uint64_t *out_n);
void cfr_gz_eof(const uint8_t **bytes, size_t *n);
cfr_status cfr_gz_get_stats(cfr_gz *h, cfr_gz_stats *st);
void cfr_gz_close(cfr_gz *h);

/* ---- BGZF members back into text (the inverse of cfr_gz_compress: any BGZF, not only this library's; the framing, the decoder
 * and the statuses are stated in csrc/cfr_inflate_core.hpp) ----
 * cfr_inflate_open: device >= 0: the kernel of cfr_inflate.hip on that GPU (CFR_ERR_NO_DEVICE without it: no fall-back);
 *   device = -1: the host twin (no zlib call), the same text and statuses.
 * cfr_inflate_bgzf: `members` is n bytes of whole BGZF members back to back.  Bytes that are no BGZF header where one is due:
 *   CFR_ERR_ARG, nothing is launched.  A member that frames but does not inflate to what its trailer says is CFR_OK: it is counted
 *   in info->bad_members (first_bad: its index, first_bad_status: why), its ISIZE bytes of the text are zero, the other members are
 *   not touched - the caller decides.  n = 0: CFR_OK and no text.  4 GiB of text or more in one call: CFR_ERR_ARG.
 *   fetch_text != 0: *text points at the text in a buffer the handle owns until its next call; fetch_text = 0 on a device handle:
 *   the text stays in HBM (cfr_inflate_device_text) and *text is NULL.  *text_n is the text's size either way.
 * cfr_inflate_member_status: the last call's members: status[i] (a cfr_inflate_member_code) for i < members and
 *   text_off[i] for i <= members, the exclusive sum of the members' text sizes; either pointer may be NULL; cap = the entries
 *   status holds (text_off: cap + 1), CFR_ERR_CAPACITY when the call had more members.
 * cfr_inflate_device_text: device handle only (CFR_ERR_ARG on the host twin): the last call's text in HBM; valid until the next
 *   call or close on the handle.
 * cfr_inflate_get_stats: device times of the last call from events (the host twin: wall time in inflate_ms).
 * A handle is used by one thread at a time. */
typedef struct cfr_inflate cfr_inflate;
typedef enum {
  CFR_INF_OK = 0,
  CFR_INF_BAD_HEADER = 1,      /* ISIZE above 65536, or whole bytes between the deflate stream and the trailer */
  CFR_INF_BAD_BLOCK_TYPE = 2,  /* BTYPE 11 */
  CFR_INF_BAD_STORED_LEN = 3,  /* LEN is not the complement of NLEN */
  CFR_INF_BAD_CODE_SET = 4,    /* over-subscribed or incomplete lengths, too many symbols, a bad repeat, no end-of-block code */
  CFR_INF_BAD_SYMBOL = 5,      /* a code no symbol has, length symbol 286 / 287, distance symbol 30 / 31, a distance in front of the member */
  CFR_INF_INPUT = 6,           /* the stream ends inside a block */
  CFR_INF_OUTPUT_LONG = 7,     /* more text than ISIZE */
  CFR_INF_OUTPUT_SHORT = 8,    /* less text than ISIZE */
  CFR_INF_BAD_CRC = 9
} cfr_inflate_member_code;
typedef struct { uint64_t members, bad_members, first_bad, bytes_in, bytes_out; int32_t first_bad_status; } cfr_inflate_info;
typedef struct { float upload_ms, inflate_ms, download_ms; } cfr_inflate_stats;
cfr_status cfr_inflate_open(int device, cfr_inflate **out);
cfr_status cfr_inflate_bgzf(cfr_inflate *h, const uint8_t *members, uint64_t n, int fetch_text,
                            const uint8_t **text, uint64_t *text_n, cfr_inflate_info *info);
cfr_status cfr_inflate_member_status(cfr_inflate *h, uint8_t *status, uint64_t *text_off, uint64_t cap);
cfr_status cfr_inflate_device_text(cfr_inflate *h, const void **d_text, uint64_t *n);
cfr_status cfr_inflate_get_stats(cfr_inflate *h, cfr_inflate_stats *st);
void cfr_inflate_close(cfr_inflate *h);
/* cfr_tokenize_resident: cfr_tokenize with its source in the memory of the tokeniser's own device (cfr_inflate_device_text, or a
 *   range inside it): one device-to-device copy into the tokeniser's padded buffer, then everything as in cfr_tokenize - the same
 *   rules, limits and results.  CFR_ERR_ARG on the host twin.
 * cfr_tokenizer_fetch_ids: the ids of the last call's records back to back without terminators, and n_records + 1 offsets
 *   (either pointer may be NULL).  ids_cap below the ids' bytes: CFR_ERR_CAPACITY (no id is longer than its header line, so the
 *   text's length is always enough).  On the device a gather kernel and one copy; the host twin has kept them. */
cfr_status cfr_tokenize_resident(cfr_tokenizer *t, const void *d_text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info);
cfr_status cfr_tokenizer_fetch_ids(cfr_tokenizer *t, char *ids, uint64_t ids_cap, uint64_t *id_off);

/* ---- single-cell input: read formats, barcode whitelist, barcode translation (ReadFormatter.hpp, BarcodeCorrector.hpp,
 * BarcodeTranslator.hpp; the flow of CentrifugerClass.cpp:163-224, :565-574) ----
 * Handles of their own, independent of any cfr_dev_index; one call at a time per handle.  Barcodes, reads and comments are flat
 * byte arrays with n + 1 offsets, as everywhere in this header.
 *
 * cfr_read_format_parse: ReadFormatter::Init on `r1|r2|bc|um:START:END[:STRAND]` and `bc:hd:FIELD|PREFIX:START:END`, separated by
 *   ',' or ';'.  CFR_ERR_FORMAT with the reference's "Format description error in <spec>" for what it refuses.
 * cfr_read_format_info: segment count, NeedExtract, IsInComment of one category (any pointer may be NULL).
 * cfr_read_format_extract: one category over n records.  inplace = 1: InplaceExtractSeqAndQual (what the classifier does to reads,
 *   barcodes and UMIs); inplace = 0: Extract into a buffer of its own (what the background pass of the whitelist does).  A category
 *   whose first segment is an `hd:` one is cut from `comments` (Extract on the comment; no qualities come out).  Bases are
 *   complemented after a strand '-', qualities only reversed.  out_offsets (n + 1, from 0) is always written; with out_bases NULL
 *   nothing else is: call once for the sizes, once for the bytes.  qual / out_qual / comments may be NULL. */
typedef struct cfr_read_format cfr_read_format;
enum { CFR_FORMAT_READ1 = 0, CFR_FORMAT_READ2 = 1, CFR_FORMAT_BARCODE = 2, CFR_FORMAT_UMI = 3 };
cfr_status cfr_read_format_parse(const char *spec, cfr_read_format **out);
cfr_status cfr_read_format_info(const cfr_read_format *f, int category, int32_t *n_segments, int32_t *need_extract, int32_t *in_comment);
cfr_status cfr_read_format_extract(const cfr_read_format *f, int category, int inplace, const uint8_t *bases, const uint64_t *offsets,
                                   const char *qual, const uint8_t *comments, const uint64_t *comment_offsets, size_t n,
                                   uint8_t *out_bases, uint64_t *out_offsets, char *out_qual);
void cfr_read_format_destroy(cfr_read_format *f);

/* cfr_barcode_open: BarcodeCorrector::SetWhitelist (plain or gz).  device >= 0: when every valid entry has one length L <= 32 the
 *   whitelist is also built as a hash table in the HBM of that device (cfr_barcode.hip) and cfr_barcode_count / cfr_barcode_correct
 *   run there; a barcode whose length is not L, and every barcode of a whitelist of mixed lengths or L > 32, goes through the host
 *   twin (a trie as in the reference) - the stats count them.  device = -1: host only, no GPU is touched.
 * cfr_barcode_count: CollectBackgroundDistribution over the first min(n, max_records) barcodes (already extracted): + 1 for every
 *   barcode that is on the list; calls add up.  max_records caps THIS call: a caller that feeds the pass in several calls keeps
 *   the remainder of the reference's 2 000 000 itself.
 * cfr_barcode_correct: BarcodeCorrector::Correct per barcode.  status[i]: 0 on the list (this includes a proper prefix of an entry
 *   and, with it, the empty barcode), 1 corrected by one substitution, -1 not correctable (the classifier then prints "N").
 *   out_bases: the barcodes after the call, same offsets.  qual may be NULL.  threads: host threads of the twin and of the copy.
 * cfr_barcode_correct_host: the same through the twin whatever the handle holds.
 * A barcode of 256 bytes or more is CFR_ERR_ARG (the reference's buffer ends there).
 * cfr_barcode_counts: every entry and its count (whitelist lines + background hits), sorted (A < C < G < T, a prefix first); the
 *   pointers stay valid until the next call on the handle. */
typedef struct cfr_barcode cfr_barcode;
typedef struct {
  uint64_t whitelist_size;        /* distinct valid entries */
  uint64_t table_slots;           /* slots of the device table, 0: host only */
  uint64_t host_barcodes;         /* barcodes of the last count / correct call that went through the host twin */
  uint64_t host_barcodes_total;   /* ... of all calls */
  double device_ms;               /* stream time of the last call on the device: copies in, kernels, copies out */
  int32_t barcode_length;         /* L, 0: mixed lengths (or no entry) */
  int32_t on_device;
} cfr_barcode_stats;
cfr_status cfr_barcode_open(const char *whitelist_path, int device, cfr_barcode **out);
cfr_status cfr_barcode_count(cfr_barcode *bc, const uint8_t *bases, const uint64_t *offsets, size_t n, size_t max_records);
cfr_status cfr_barcode_correct(cfr_barcode *bc, const uint8_t *bases, const uint64_t *offsets, const char *qual, size_t n, int threads,
                               int8_t *status, uint8_t *out_bases);
cfr_status cfr_barcode_correct_host(cfr_barcode *bc, const uint8_t *bases, const uint64_t *offsets, const char *qual, size_t n, int threads,
                                    int8_t *status, uint8_t *out_bases);
cfr_status cfr_barcode_counts(cfr_barcode *bc, size_t *n_entries, const uint8_t **bases, const uint64_t **offsets, const uint32_t **counts);
cfr_status cfr_barcode_get_stats(const cfr_barcode *bc, cfr_barcode_stats *st);
void cfr_barcode_destroy(cfr_barcode *bc);

/* cfr_barcode_translate_open: BarcodeTranslator::SetTranslateTable, lines `TO<sep>FROM` (sep: the first ',', tab or space).
 * cfr_barcode_translate_apply: Translate per barcode - cut into len / from_len pieces, each looked up, joined with '-'.  status
 *   (may be NULL): a barcode with status -1 becomes "N" and is not translated (CentrifugerClass.cpp:189-205).  Sizes first, bytes
 *   second, as cfr_read_format_extract.  A piece that is not in the table: CFR_ERR_FORMAT, and cfr_last_error() is the reference's
 *   "Barcode <piece> does not exist in the translation table." (it exits with status 255 there). */
typedef struct cfr_barcode_translate cfr_barcode_translate;
cfr_status cfr_barcode_translate_open(const char *path, cfr_barcode_translate **out);
cfr_status cfr_barcode_translate_apply(const cfr_barcode_translate *t, const uint8_t *bases, const uint64_t *offsets, const int8_t *status,
                                       size_t n, uint8_t *out_bases, uint64_t *out_offsets);
void cfr_barcode_translate_destroy(cfr_barcode_translate *t);

/* ResultWriter::OutputHeader / Output with the barcode and UMI columns (ResultWriter.hpp:186-242): they stand before
 * expandedTaxIDs.  has_barcode / has_umi: the column is there; a NULL string prints a bare tab (PrintExtraCol).  With neither column
 * the bytes are those of cfr_tsv_header / cfr_format_tsv (expanded = 0) or cfr_tsv_header_expanded / cfr_format_tsv_expanded. */
const char *cfr_tsv_header_ex(int has_barcode, int has_umi, int expanded);
size_t cfr_format_tsv_ex(const cfr_index *idx, const char *read_id, const cfr_result *r, const cfr_match *matches, int has_barcode,
                         const char *barcode, int has_umi, const char *umi, int expanded, const cfr_span *spans, const uint64_t *ids,
                         char *buf, size_t cap);

/* ---- index writer (outside the classification path) ----
 * What `centrifuger-build` produces (Builder::Build + FMBuilder, Builder.hpp:86-313, compactds/FMBuilder.hpp:209-313):
 * <out_prefix>.{1,2,3,4}.cfr for nucleotide sequences, default layout options (--rbbwt-b / --offrate / --ftabchars
 * honoured).  The suffix array is built in the HBM of one MI355X (texts below 2^34 symbols); there is no CPU path.
 * bin/centrifuger-build is the command line on top of it. */
typedef struct {
  uint64_t n_seqs;
  const char *const *seq_names;     /* conversion-table order = sequence ids */
  const uint64_t *seq_taxids;       /* original tax id of every sequence */
  const uint64_t *seq_lens;         /* length of every sequence */
  const uint8_t *text;              /* the sequences back to back: upper-case A,C,G,T only (SequenceCompactor.hpp:59-84 drops the rest) */
  uint64_t n_nodes;                 /* nodes.dmp */
  const uint64_t *node_taxid, *node_parent;
  const char *const *node_rank;
  uint64_t n_names;                 /* names.dmp, scientific names */
  const uint64_t *name_taxid;
  const char *const *name_text;
  /* Genomes of the text when they are not simply "every sequence, in conversion-table order" (Builder.hpp:108-165: the text
   * follows the FASTA order, a conversion table may name sequences the FASTA does not hold, and a FASTA sequence the table
   * does not name is added as an extra name without a tax id).  n_genomes = 0: genome g = sequence g with seq_lens[g]. */
  uint64_t n_genomes;
  const uint64_t *genome_seq;       /* sequence id (index into seq_names) of every genome of the text, in text order; no id twice */
  const uint64_t *genome_lens;      /* their lengths; seq_lens is not read when n_genomes > 0 */
  uint64_t n_extra;                 /* the LAST n_extra entries of seq_names are extra names (Taxonomy::AddExtraSeqName): seq_taxids not read for them */
  /* further tax ids whose lineages stay in the tree: Taxonomy::Init keeps every id the conversion table MENTIONS
   * (Taxonomy.hpp:275-300), also one that no sequence ends up with (a name listed twice gets the LCA of its ids) */
  uint64_t n_present_taxids;
  const uint64_t *present_taxids;
  const void *selection;            /* cfr_build_index_assembled only: the cfr_build_selection made from this input, or NULL */
} cfr_build_input;
typedef struct {
  int32_t ftab_chars;   /* --ftabchars, default 10 */
  int32_t offrate;      /* --offrate, default 4: SA sampled every 2^offrate rows */
  int32_t device;       /* HIP device ordinal */
  int32_t threads;      /* host threads of the compression / writing half, 0 = automatic */
  uint64_t rbbwt_b;     /* --rbbwt-b, 0 = automatic block size */
  int32_t verbose;
  int32_t protein;      /* --protein (CentrifugerBuild.cpp:221-227, Builder.hpp:95-101): `text` holds the proteins back to back, letters of
                         * "ARNDCEQGHILKMFPSTWYV" only, lengths in residues; the writer closes every protein with '$' and writes an
                         * FMIndex<Sequence_RunBlockOneTree> with endMarkerSA.  ftab_chars <= 6 (the reference's default is 4), n < 2^32 */
} cfr_build_options;
typedef struct {
  uint64_t n, block_size, first_isa;
  double seconds_sa, seconds_total;
  int32_t rounds, pad;
} cfr_build_report;
void cfr_build_options_default(cfr_build_options *o);
cfr_status cfr_build_index(const cfr_build_input *in, const cfr_build_options *opt, const char *out_prefix, cfr_build_report *report);

/* ---- the reference text of the index writer: filter and assemble (csrc/cfr_refseq_core.hpp states the grammar) ----
 * The front end of bin/centrifuger-build: the bytes of the reference files go in chunk by chunk, the symbols the index keeps come
 * out as one stream U, and cfr_refseq_assemble copies segments of U - records dropped, records regrouped - into the text T of the
 * index, in the HBM of the GPU that sorts its suffixes.
 * cfr_refseq_open: device >= 0: the kernels of cfr_refseq.hip on that GPU (nucleotide only: protein is CFR_ERR_ARG there;
 *   CFR_ERR_NO_DEVICE without the GPU: no fall-back); device = -1: the host twin, no GPU is touched, U and T are ASCII.
 * cfr_refseq_feed: one chunk of one file, len below 2^32.  A chunk never begins inside a header line; at_line_start: its first byte
 *   begins a line (a file's first chunk: 1; later chunks: what the previous call returned in info).  final: the file ends with this
 *   chunk.  A chunk that ends inside a header line without final is looked at up to that '>' (info->consumed): continue there.  A
 *   header line that fills a whole chunk that is not final is CFR_ERR_CAPACITY.
 * cfr_refseq_fetch: the info->n_records records of the last feed.
 * cfr_refseq_assemble: segments (src symbol in U, length, dst symbol in T) sorted by dst, none empty, covering [0, n) exactly; U is
 *   freed, no further feed.  cfr_refseq_text: T as n ASCII bytes.
 * cfr_build_index_assembled: cfr_build_index with the text taken from the handle (in->text is not read; a device handle must sit
 *   on opt->device and gives its T away).  in->selection: what cfr_build_select returned, or NULL (then in->genome_* describe T).
 * A handle is used by one thread at a time; a handle that is not open is CFR_ERR_ARG. */
typedef struct cfr_refseq cfr_refseq;
typedef struct { uint32_t header, header_len, id_len, kept; } cfr_refseq_record;   /* offset of the '>' in the chunk; bytes of the header line without its '\n'; bytes of the id behind the '>'; symbols kept up to the next header */
typedef struct {
  uint64_t n_records, consumed;
  uint64_t lead_kept;      /* kept symbols before the chunk's first header: they continue the previous chunk's last record */
  uint64_t kept;           /* kept symbols of the chunk, lead_kept included */
  uint64_t u_start;        /* where the chunk's symbols begin in U (a multiple of 32) */
  int32_t at_line_start, pad;
  double device_ms;
} cfr_refseq_info;
typedef struct { uint64_t src, len, dst; } cfr_refseq_segment;
typedef struct { double feed_ms, copy_in_ms, assemble_ms; } cfr_refseq_stats;      /* sums over the feeds (copy_in_ms is part of feed_ms); the last assemble */
cfr_status cfr_refseq_open(int device, int protein, cfr_refseq **out);
cfr_status cfr_refseq_feed(cfr_refseq *h, const uint8_t *text, uint64_t len, int at_line_start, int final, cfr_refseq_info *info);
cfr_status cfr_refseq_fetch(cfr_refseq *h, cfr_refseq_record *records);
cfr_status cfr_refseq_assemble(cfr_refseq *h, const cfr_refseq_segment *segments, uint64_t n_segments, uint64_t n);
cfr_status cfr_refseq_text(cfr_refseq *h, uint8_t *ascii_out);
cfr_status cfr_refseq_get_stats(cfr_refseq *h, cfr_refseq_stats *st);
void cfr_refseq_close(cfr_refseq *h);

/* ---- selection: which records of the reference files become which genomes of the text (Builder::Build, Builder.hpp:104-211) ----
 * records: every FASTA record in reading order - its id, its file, and where its kept symbols lie in U (pieces first_piece ..
 * first_piece + n_pieces of `pieces`: a record cut by a chunk end has more than one).  in: the conversion table (seq_names, seq_taxids,
 * present_taxids; with file_level the file list with Utils::GetFileBaseName names - cfr_file_base_name), nodes and names; its genome
 * fields are not read.  The result holds the segments for cfr_refseq_assemble and, behind in->selection, everything
 * cfr_build_index_assembled needs: extra names, genomes, the compact tax ids (computed once, shared with the writer of .2.cfr).
 * Nothing left to index: CFR_ERR_ARG with the reference's "found 0 genomes" message. */
typedef struct cfr_build_selection cfr_build_selection;
typedef struct { const char *id; const char *file; uint64_t first_piece, n_pieces; } cfr_select_record;
typedef struct { uint64_t src, len; } cfr_select_piece;
typedef struct {
  int32_t file_level;              /* a two-column -l list is the conversion table: names are file base names, a file's records add into one genome */
  int32_t concat_tax_genome;       /* --concat-tax-genome */
  int32_t ignore_uncategorized;    /* --ignore-uncategorized-genome */
  int32_t protein;
  uint64_t subset_tax;             /* --subset-tax, 0: off */
  int32_t ftab_chars, pad;
} cfr_select_options;
cfr_status cfr_build_select(const cfr_build_input *in, const cfr_select_options *so, const cfr_select_record *records, uint64_t n_records,
                            const cfr_select_piece *pieces, uint64_t n_pieces, cfr_build_selection **out);
/* the segments (valid until cfr_build_selection_free), the length of the text, its genomes and the extra names */
cfr_status cfr_build_selection_get(const cfr_build_selection *s, const cfr_refseq_segment **segments, uint64_t *n_segments, uint64_t *n,
                                   uint64_t *n_genomes, uint64_t *n_extra);
void cfr_build_selection_free(cfr_build_selection *s);
size_t cfr_file_base_name(const char *path, char *out, size_t cap);      /* returns the length of the name; out (may be NULL) gets at most cap - 1 bytes and a 0 */
cfr_status cfr_build_index_assembled(cfr_refseq *h, const cfr_build_input *in, const cfr_build_options *opt, const char *out_prefix, cfr_build_report *report);

#ifdef __cplusplus
}
#endif
#endif /* CFR_HIP_H */
