// cfr_capi.cpp — the extern "C" surface declared in include/cfr_hip.h.
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "cfr_barcode.hpp"
#include "cfr_build.hpp"
#include "cfr_device.hpp"
#include "cfr_kreport.hpp"
#include "cfr_promote.hpp"
#include "cfr_quant.hpp"
#include "cfr_tail.hpp"
#include "cfr_threads.hpp"
#include "cfr_refseq_core.hpp"
#include "cfr_tokenize_core.hpp"
#include "cfr_tsv.hpp"
#include "cfr_gz.hpp"
#include "cfr_inflate.hpp"

struct cfr_index { cfr::HostIndex *h; };
struct cfr_read_format { cfr::ReadFormat f; };
struct cfr_barcode { cfr::Barcode *b; };
struct cfr_barcode_translate { cfr::BarcodeTranslate *t; };
struct cfr_taxonomy {
  cfr::Taxonomy tax;
  std::vector<std::string> seq_names;                     // MapID order: a name stored twice keeps its first id
  bool with_lengths = false;
  std::vector<uint64_t> taxid_length, length_seq_id, length_value;
};
struct cfr_promote { cfr::Promote *p; };
struct cfr_kreport { cfr::Kreport *k; };
struct cfr_tokenizer { cfr::Tokenizer *t; };
struct cfr_refseq { cfr::Refseq *r; bool protein; };
struct cfr_build_selection { cfr::BuildInput in; std::vector<cfr_refseq_segment> segments; uint64_t n = 0; };
struct cfr_tsv { cfr::Tsv *t; };
struct cfr_gz { cfr::Gz *g; };
struct cfr_inflate { cfr::Inflate *i; };
struct cfr_quant { cfr::Quant *q; std::vector<double> weight; int32_t rounds = 0; bool ran = false; };
// One call at a time per device image: `busy` is held for the length of every entry that touches the image (try_lock:
// CFR_ERR_BUSY for the second caller) and by the worker thread while it runs a submitted batch.
struct cfr_async_job { std::function<cfr_status(std::string &, size_t &)> run; uint64_t ticket; };
struct cfr_async_done { cfr_status status; std::string err; size_t n_matches; };
struct cfr_dev_index {
  cfr::DeviceIndex *d; const cfr_index *host; int tail_threads;
  std::mutex busy;
  // submitted batches (cfr_classify_batch_submit / _wait)
  std::mutex qmu;
  std::condition_variable qcv, dcv;
  std::deque<cfr_async_job> queue;
  std::map<uint64_t, cfr_async_done> done;
  std::set<uint64_t> live;                               // tickets handed out and not yet waited for
  uint64_t next_ticket = 1;
  bool stop = false, worker_started = false;
  std::thread worker;
  cfr_dev_index(cfr::DeviceIndex *dd, const cfr_index *h, int t) : d(dd), host(h), tail_threads(t) {}
};

namespace {
thread_local std::string g_err;

template <class F> cfr_status guarded(F &&f) {
  try {
    return f();
  } catch (const cfr::IoError &e) {
    g_err = e.msg; return CFR_ERR_IO;
  } catch (const cfr::FormatError &e) {
    g_err = e.msg; return CFR_ERR_FORMAT;
  } catch (const cfr::CapacityError &e) {
    g_err = e.msg; return CFR_ERR_CAPACITY;
  } catch (const cfr::HipError &e) {
    g_err = e.msg; return e.code == -1 ? CFR_ERR_NO_DEVICE : CFR_ERR_HIP;
  } catch (const std::exception &e) {
    g_err = e.what(); return CFR_ERR_ARG;
  }
}
cfr_status bad_arg(const char *m) { g_err = m; return CFR_ERR_ARG; }

// the cfr_promote handles that are open: a call on anything else is CFR_ERR_ARG, not a wild pointer
std::mutex g_promote_mu;
std::set<const cfr_promote *> g_promote_live;
bool promote_live(const cfr_promote *h) {
  std::lock_guard<std::mutex> lk(g_promote_mu);
  return h && g_promote_live.count(h) != 0;
}

// ... the cfr_kreport handles
std::mutex g_kreport_mu;
std::set<const cfr_kreport *> g_kreport_live;
bool kreport_live(const cfr_kreport *h) {
  std::lock_guard<std::mutex> lk(g_kreport_mu);
  return h && g_kreport_live.count(h) != 0;
}

// ... and the cfr_tokenizer handles
std::mutex g_tokenizer_mu;
std::set<const cfr_tokenizer *> g_tokenizer_live;
bool tokenizer_live(const cfr_tokenizer *h) {
  std::lock_guard<std::mutex> lk(g_tokenizer_mu);
  return h && g_tokenizer_live.count(h) != 0;
}

// ... and the cfr_refseq handles
std::mutex g_refseq_mu;
std::set<const cfr_refseq *> g_refseq_live;
bool refseq_live(const cfr_refseq *h) {
  std::lock_guard<std::mutex> lk(g_refseq_mu);
  return h && g_refseq_live.count(h) != 0;
}

// ... and the cfr_tsv handles
std::mutex g_tsv_mu;
std::set<const cfr_tsv *> g_tsv_live;
bool tsv_live(const cfr_tsv *h) {
  std::lock_guard<std::mutex> lk(g_tsv_mu);
  return h && g_tsv_live.count(h) != 0;
}

// ... and the cfr_gz handles
std::mutex g_gz_mu;
std::set<const cfr_gz *> g_gz_live;
bool gz_live(const cfr_gz *h) {
  std::lock_guard<std::mutex> lk(g_gz_mu);
  return h && g_gz_live.count(h) != 0;
}

// ... and the cfr_inflate handles
std::mutex g_inflate_mu;
std::set<const cfr_inflate *> g_inflate_live;
bool inflate_live(const cfr_inflate *h) {
  std::lock_guard<std::mutex> lk(g_inflate_mu);
  return h && g_inflate_live.count(h) != 0;
}

// entry guard: the image's buffers, streams and statistics belong to one call at a time
struct BusyGuard {
  std::unique_lock<std::mutex> lk;
  explicit BusyGuard(cfr_dev_index *d) : lk(d->busy, std::try_to_lock) {}
  bool ok() const { return lk.owns_lock(); }
};
#define CFR_ENTER(d, what)                                                                                                   \
  BusyGuard busy_guard_(d);                                                                                                  \
  if (!busy_guard_.ok()) { g_err = what ": this cfr_dev_index is in use by another call (one call at a time per device image)"; return CFR_ERR_BUSY; }

void worker_loop(cfr_dev_index *d) {
  for (;;) {
    cfr_async_job job;
    {
      std::unique_lock<std::mutex> lk(d->qmu);
      d->qcv.wait(lk, [&] { return d->stop || !d->queue.empty(); });
      if (d->queue.empty()) return;                      // stop, nothing left to run
      job = std::move(d->queue.front());
      d->queue.pop_front();
    }
    cfr_async_done r{CFR_OK, "", 0};
    {
      std::lock_guard<std::mutex> run(d->busy);          // (waits for a synchronous call that is inside the image)
      r.status = job.run(r.err, r.n_matches);
    }
    {
      std::lock_guard<std::mutex> lk(d->qmu);
      d->done.emplace(job.ticket, std::move(r));
    }
    d->dcv.notify_all();
  }
}

void fill_info(const cfr::HostIndex &h, cfr_index_info *info, uint64_t dev_bytes) {
  memset(info, 0, sizeof(*info));
  info->n = h.n; info->first_isa = h.first_isa; info->block_size = h.b; info->precompute_width = h.precompute_width;
  info->sample_rate = (uint64_t)h.sample_rate; info->selected_cnt = h.selected_rows.size();
  info->seq_cnt = h.tax.seq_cnt; info->node_cnt = h.tax.node_cnt; info->min_hit_len = h.params.min_hit_len;
  info->last_chr = h.last_chr; info->is_protein = h.prot.enabled ? 1 : 0; info->device_bytes = dev_bytes;
}

int default_tail_threads() {
  unsigned hc = std::thread::hardware_concurrency();
  if (hc == 0) hc = 1;
  return (int)std::min(hc, 64u);
}
}  // namespace

extern "C" {

void cfr_params_default(cfr_params *p) {   // _classifierParam() (Classifier.hpp:28-37)
  p->max_result = 1; p->min_hit_len = 0; p->max_result_per_hit_factor = 40; p->output_expanded = 0;
  p->consider_secondary_hit_len = 2000; p->consider_secondary_score_factor = 0.995;
}
const char *cfr_last_error(void) { return g_err.c_str(); }
const char *cfr_version(void) { return "centrifuger_amd 0.1 (gfx950); path parity with Centrifuger v1.1.3-r347"; }

cfr_status cfr_index_open(const char *idx_prefix, const cfr_params *params, cfr_index **out) {
  if (!idx_prefix || !out) return bad_arg("cfr_index_open: null argument");
  return guarded([&]() -> cfr_status {
    cfr::HostIndex *h = cfr::load_index(idx_prefix, params);
    *out = new cfr_index{h};
    return CFR_OK;
  });
}
void cfr_index_destroy(cfr_index *idx) { if (idx) { delete idx->h; delete idx; } }
cfr_status cfr_index_get_info(const cfr_index *idx, cfr_index_info *info) {
  if (!idx || !info) return bad_arg("cfr_index_get_info: null argument");
  fill_info(*idx->h, info, 0);
  return CFR_OK;
}

cfr_status cfr_index_digest(const cfr_index *idx, uint64_t *digest) {
  if (!idx || !digest) return bad_arg("cfr_index_digest: null argument");
  *digest = cfr::index_digest(*idx->h);
  return CFR_OK;
}

cfr_status cfr_index_mapped_bytes(const cfr_index *idx, uint64_t *mapped, uint64_t *copied) {
  if (!idx || !mapped || !copied) return bad_arg("cfr_index_mapped_bytes: null argument");
  const cfr::HostIndex &h = *idx->h;
  uint64_t m = 0, c = 0;
  auto add = [&](const cfr::RawWords &w) { (w.mapped() ? m : c) += (uint64_t)w.size() * 8; };
  add(h.use_run_block.bits);
  for (int k = 0; k < 3; ++k) { add(h.wavelet_seq.node[k].bits); add(h.run_block_seq.node[k].bits); }
  add(h.sampled_words);
  *mapped = m;
  *copied = c;
  return CFR_OK;
}

cfr_status cfr_device_count(int *count) {
  if (!count) return bad_arg("cfr_device_count: null argument");
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) { *count = 0; g_err = "hipGetDeviceCount failed"; return CFR_ERR_NO_DEVICE; }
  *count = c;
  return CFR_OK;
}
void cfr_device_options_default(cfr_device_options *o) {
  if (!o) return;
  o->profile = CFR_PROFILE_THROUGHPUT;
  o->ftabx_width = -1;
  o->text_mode = -1;
  o->run_block_layout = 0;
  o->loc_memo_gb = -1.0;
  o->sub_batch = 0;
}
cfr_status cfr_device_index_create_ex(const cfr_index *idx, int device, const cfr_device_options *options, cfr_dev_index **out) {
  if (!idx || !out) return bad_arg("cfr_device_index_create: null argument");
  cfr_device_options o;
  cfr_device_options_default(&o);
  if (options) o = *options;
  if (o.profile != CFR_PROFILE_THROUGHPUT && o.profile != CFR_PROFILE_FAST_LOAD && o.profile != CFR_PROFILE_BALANCED) return bad_arg("cfr_device_index_create_ex: unknown profile");
  if (o.ftabx_width < -1 || o.ftabx_width > 16) return bad_arg("cfr_device_index_create_ex: ftabx_width out of range");
  return guarded([&]() -> cfr_status {
    cfr::DeviceIndex *d = new cfr::DeviceIndex(*idx->h, device, o);
    *out = new cfr_dev_index(d, idx, default_tail_threads());
    return CFR_OK;
  });
}
cfr_status cfr_device_index_create(const cfr_index *idx, int device, cfr_dev_index **out) {
  return cfr_device_index_create_ex(idx, device, nullptr, out);
}
void cfr_device_index_destroy(cfr_dev_index *d) {
  if (!d) return;
  if (d->worker_started) {                               // queued batches run to completion first (their buffers are the caller's)
    { std::lock_guard<std::mutex> lk(d->qmu); d->stop = true; }
    d->qcv.notify_all();
    d->worker.join();
  }
  { std::lock_guard<std::mutex> wait_for_a_running_call(d->busy); }
  delete d->d;
  delete d;
}
cfr_status cfr_device_index_get_info(const cfr_dev_index *d, cfr_index_info *info) {
  if (!d || !info) return bad_arg("cfr_device_index_get_info: null argument");
  fill_info(d->d->host(), info, d->d->device_bytes());
  return CFR_OK;
}

cfr_status cfr_rank_batch(cfr_dev_index *d, const char *chars, const uint64_t *pos, const uint8_t *inclusive, size_t n,
                          uint64_t *out_rank, char *out_access) {
  if (!d || (n && (!chars || !pos || !inclusive))) return bad_arg("cfr_rank_batch: null argument");
  for (size_t i = 0; i < n; ++i) if (pos[i] >= d->d->host().n) return bad_arg("cfr_rank_batch: position out of range");
  CFR_ENTER(d, "cfr_rank_batch");
  return guarded([&]() -> cfr_status { d->d->rank_batch(chars, pos, inclusive, n, out_rank, out_access); return CFR_OK; });
}
cfr_status cfr_backward_search_batch(cfr_dev_index *d, const uint8_t *bases, const uint64_t *offsets, const uint32_t *m, size_t n,
                                     uint64_t *out_l, uint64_t *out_sp, uint64_t *out_ep) {
  if (!d || (n && (!bases || !offsets || !m || !out_l || !out_sp || !out_ep))) return bad_arg("cfr_backward_search_batch: null argument");
  for (size_t i = 0; i < n; ++i) if (m[i] > offsets[i + 1] - offsets[i]) return bad_arg("cfr_backward_search_batch: m exceeds read length");
  CFR_ENTER(d, "cfr_backward_search_batch");
  return guarded([&]() -> cfr_status { d->d->backward_search_batch(bases, offsets, m, n, out_l, out_sp, out_ep); return CFR_OK; });
}
cfr_status cfr_locate_rows(cfr_dev_index *d, const uint64_t *rows, size_t n, uint64_t *out_val, uint32_t *out_steps) {
  if (!d || (n && (!rows || !out_val))) return bad_arg("cfr_locate_rows: null argument");
  for (size_t i = 0; i < n; ++i) if (rows[i] >= d->d->host().n) return bad_arg("cfr_locate_rows: row out of range");
  CFR_ENTER(d, "cfr_locate_rows");
  return guarded([&]() -> cfr_status { d->d->locate_rows(rows, n, out_val, out_steps); return CFR_OK; });
}

void cfr_build_options_default(cfr_build_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->ftab_chars = 10; o->offrate = 4;
}
// the conversion table and the taxonomy files of a cfr_build_input (not its genomes, not its text)
static void build_input_tables(const cfr_build_input *in, cfr::BuildInput &bi) {
  for (uint64_t i = 0; i < in->n_seqs; ++i) {
    bi.names.emplace_back(in->seq_names[i]);
    if (i < in->n_seqs - in->n_extra) bi.taxids.push_back(in->seq_taxids[i]);
  }
  bi.n_extra = in->n_extra;
  if (in->n_present_taxids && in->present_taxids) bi.present_taxids.assign(in->present_taxids, in->present_taxids + in->n_present_taxids);
  for (uint64_t i = 0; i < in->n_nodes; ++i) bi.nodes.push_back(cfr::TaxNode{in->node_taxid[i], in->node_parent[i], in->node_rank[i] ? in->node_rank[i] : ""});
  for (uint64_t i = 0; i < in->n_names; ++i) bi.tax_names.emplace_back(in->name_taxid[i], in->name_text[i] ? in->name_text[i] : "");
}
static cfr::BuildOptions build_options(const cfr_build_options *opt) {
  cfr::BuildOptions bo;
  if (opt) { bo.ftab_chars = opt->ftab_chars; bo.offrate = opt->offrate; bo.device = opt->device; bo.threads = opt->threads; bo.rbbwt_b = opt->rbbwt_b; bo.verbose = opt->verbose != 0; bo.protein = opt->protein != 0; }
  return bo;
}
static void build_report(const cfr::BuildReport &rep, cfr_build_report *report) {
  if (!report) return;
  report->n = rep.n; report->block_size = rep.block_size; report->first_isa = rep.first_isa;
  report->seconds_sa = rep.seconds_sa; report->seconds_total = rep.seconds_total; report->rounds = rep.rounds; report->pad = 0;
}

cfr_status cfr_build_index(const cfr_build_input *in, const cfr_build_options *opt, const char *out_prefix, cfr_build_report *report) {
  if (!in || !out_prefix) return bad_arg("cfr_build_index: null argument");
  if (!in->n_seqs || !in->seq_names || !in->seq_taxids || !in->text) return bad_arg("cfr_build_index: empty input");
  if (in->n_genomes ? (!in->genome_seq || !in->genome_lens) : !in->seq_lens) return bad_arg("cfr_build_index: genome lengths missing");
  if (in->n_extra > in->n_seqs || (!in->n_genomes && in->n_extra)) return bad_arg("cfr_build_index: n_extra needs the genome list and cannot exceed n_seqs");
  if ((in->n_nodes && (!in->node_taxid || !in->node_parent || !in->node_rank)) || (in->n_names && (!in->name_taxid || !in->name_text)))
    return bad_arg("cfr_build_index: taxonomy arrays missing");
  return guarded([&]() -> cfr_status {
    cfr::BuildInput bi;
    build_input_tables(in, bi);
    if (in->n_genomes) {
      bi.genome_seq.assign(in->genome_seq, in->genome_seq + in->n_genomes);
      bi.lens.assign(in->genome_lens, in->genome_lens + in->n_genomes);
    } else {
      for (uint64_t i = 0; i < in->n_seqs; ++i) { bi.genome_seq.push_back(i); bi.lens.push_back(in->seq_lens[i]); }
    }
    bi.text = in->text;
    cfr::BuildReport rep;
    cfr::build_index_files(bi, build_options(opt), out_prefix, &rep);
    build_report(rep, report);
    return CFR_OK;
  });
}

// ---- the reference text of the index writer (cfr_refseq_core.hpp), the selection, and the build from the assembled text ----
cfr_status cfr_refseq_open(int device, int protein, cfr_refseq **out) {
  if (!out) return bad_arg("cfr_refseq_open: null argument");
  *out = nullptr;
  if (device < -1) return bad_arg("cfr_refseq_open: device is a HIP ordinal, or -1 for the host twin");
  if (device >= 0 && protein) return bad_arg("cfr_refseq_open: protein text goes through the host twin (device -1)");
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_refseq> h(new cfr_refseq{nullptr, protein != 0});
    h->r = device < 0 ? cfr::make_refseq_host(protein != 0) : cfr::make_refseq_device(device);
    { std::lock_guard<std::mutex> lk(g_refseq_mu); g_refseq_live.insert(h.get()); }
    *out = h.release();
    return CFR_OK;
  });
}
cfr_status cfr_refseq_feed(cfr_refseq *h, const uint8_t *text, uint64_t len, int at_line_start, int final, cfr_refseq_info *info) {
  if (!refseq_live(h)) return bad_arg("cfr_refseq_feed: not an open cfr_refseq handle");
  if (!info || (len && !text)) return bad_arg("cfr_refseq_feed: null argument");
  if (len >> 32) return bad_arg("cfr_refseq_feed: len must be below 2^32 (offsets inside a chunk are 32 bits wide): hand the file over in pieces");
  return guarded([&]() -> cfr_status {
    // (RefseqCapacity is a std::runtime_error of its own so that the host twin builds without the device headers)
    try { h->r->feed(text, len, at_line_start, final, info); } catch (const cfr::RefseqCapacity &e) { throw cfr::CapacityError{e.what()}; }
    return CFR_OK;
  });
}
cfr_status cfr_refseq_fetch(cfr_refseq *h, cfr_refseq_record *records) {
  if (!refseq_live(h)) return bad_arg("cfr_refseq_fetch: not an open cfr_refseq handle");
  return guarded([&]() -> cfr_status { h->r->fetch(records); return CFR_OK; });
}
cfr_status cfr_refseq_assemble(cfr_refseq *h, const cfr_refseq_segment *segments, uint64_t n_segments, uint64_t n) {
  if (!refseq_live(h)) return bad_arg("cfr_refseq_assemble: not an open cfr_refseq handle");
  if (n_segments && !segments) return bad_arg("cfr_refseq_assemble: null argument");
  return guarded([&]() -> cfr_status { h->r->assemble(segments, n_segments, n); return CFR_OK; });
}
cfr_status cfr_refseq_text(cfr_refseq *h, uint8_t *ascii_out) {
  if (!refseq_live(h)) return bad_arg("cfr_refseq_text: not an open cfr_refseq handle");
  if (!ascii_out) return bad_arg("cfr_refseq_text: null argument");
  return guarded([&]() -> cfr_status { h->r->text(ascii_out); return CFR_OK; });
}
cfr_status cfr_refseq_get_stats(cfr_refseq *h, cfr_refseq_stats *st) {
  if (!refseq_live(h)) return bad_arg("cfr_refseq_get_stats: not an open cfr_refseq handle");
  if (!st) return bad_arg("cfr_refseq_get_stats: null argument");
  h->r->stats(st);
  return CFR_OK;
}
void cfr_refseq_close(cfr_refseq *h) {
  {
    std::lock_guard<std::mutex> lk(g_refseq_mu);
    if (!h || !g_refseq_live.erase(h)) return;
  }
  delete h->r;
  delete h;
}

size_t cfr_file_base_name(const char *path, char *out, size_t cap) {
  const std::string b = cfr::file_base_name(path ? path : "");
  if (out && cap) { const size_t k = std::min(b.size(), cap - 1); memcpy(out, b.data(), k); out[k] = 0; }
  return b.size();
}

cfr_status cfr_build_select(const cfr_build_input *in, const cfr_select_options *so, const cfr_select_record *records, uint64_t n_records,
                            const cfr_select_piece *pieces, uint64_t n_pieces, cfr_build_selection **out) {
  if (!in || !so || !out || (n_records && !records) || (n_pieces && !pieces)) return bad_arg("cfr_build_select: null argument");
  *out = nullptr;
  if (in->n_extra) return bad_arg("cfr_build_select: the input is the conversion table alone, without extra names");
  if ((in->n_seqs && (!in->seq_names || !in->seq_taxids)) || (in->n_nodes && (!in->node_taxid || !in->node_parent || !in->node_rank)) ||
      (in->n_names && (!in->name_taxid || !in->name_text)))
    return bad_arg("cfr_build_select: table or taxonomy arrays missing");
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_build_selection> sel(new cfr_build_selection);
    build_input_tables(in, sel->in);
    std::vector<cfr::SelectRecord> recs((size_t)n_records);
    for (uint64_t k = 0; k < n_records; ++k) {
      recs[k].id = records[k].id ? records[k].id : "";
      recs[k].file = records[k].file ? records[k].file : "";
      if (records[k].first_piece > n_pieces || records[k].n_pieces > n_pieces - records[k].first_piece) throw std::invalid_argument("cfr_build_select: a record's pieces lie outside the piece list");
      for (uint64_t q = 0; q < records[k].n_pieces; ++q) recs[k].pieces.push_back(cfr::SelectPiece{pieces[records[k].first_piece + q].src, pieces[records[k].first_piece + q].len});
    }
    cfr::SelectOptions o;
    o.file_level = so->file_level != 0; o.concat = so->concat_tax_genome != 0; o.ignore_uncategorized = so->ignore_uncategorized != 0; o.protein = so->protein != 0;
    o.subset_tax = so->subset_tax; o.ftab_chars = so->ftab_chars;
    std::vector<cfr::SelectSegment> segs;
    cfr::select_genomes(sel->in, o, recs, segs, sel->n);
    for (const auto &g : segs) sel->segments.push_back(cfr_refseq_segment{g.src, g.len, g.dst});
    *out = sel.release();
    return CFR_OK;
  });
}
cfr_status cfr_build_selection_get(const cfr_build_selection *s, const cfr_refseq_segment **segments, uint64_t *n_segments, uint64_t *n, uint64_t *n_genomes, uint64_t *n_extra) {
  if (!s) return bad_arg("cfr_build_selection_get: null argument");
  if (segments) *segments = s->segments.data();
  if (n_segments) *n_segments = s->segments.size();
  if (n) *n = s->n;
  if (n_genomes) *n_genomes = s->in.genome_seq.size();
  if (n_extra) *n_extra = s->in.n_extra;
  return CFR_OK;
}
void cfr_build_selection_free(cfr_build_selection *s) { delete s; }

cfr_status cfr_build_index_assembled(cfr_refseq *h, const cfr_build_input *in, const cfr_build_options *opt, const char *out_prefix, cfr_build_report *report) {
  if (!refseq_live(h)) return bad_arg("cfr_build_index_assembled: not an open cfr_refseq handle");
  if (!in || !out_prefix) return bad_arg("cfr_build_index_assembled: null argument");
  if (!in->selection && (!in->n_seqs || !in->seq_names || !in->seq_taxids || !in->n_genomes || !in->genome_seq || !in->genome_lens))
    return bad_arg("cfr_build_index_assembled: without a selection the input names the genomes of the text itself");
  return guarded([&]() -> cfr_status {
    cfr::BuildInput bi;
    if (in->selection) bi = static_cast<const cfr_build_selection *>(in->selection)->in;
    else {
      build_input_tables(in, bi);
      bi.genome_seq.assign(in->genome_seq, in->genome_seq + in->n_genomes);
      bi.lens.assign(in->genome_lens, in->genome_lens + in->n_genomes);
    }
    const cfr::BuildOptions bo = build_options(opt);
    if (bo.protein != h->protein) throw std::invalid_argument("cfr_build_index_assembled: the handle and the options disagree about protein");
    uint64_t total = 0;
    for (uint64_t l : bi.lens) total += l;
    if (total != h->r->text_len()) throw std::invalid_argument("cfr_build_index_assembled: the genomes' lengths do not add up to the assembled text");
    if (h->r->device() >= 0) {
      if (h->r->device() != bo.device) throw std::invalid_argument("cfr_build_index_assembled: the text was assembled on another device than the one that is to sort it");
      cfr::Refseq *r = h->r;
      bi.take_packed_text = [r]() { return r->release_device_text(); };
    } else bi.text = h->r->host_text();
    cfr::BuildReport rep;
    cfr::build_index_files(bi, bo, out_prefix, &rep);
    build_report(rep, report);
    return CFR_OK;
  });
}

cfr_status cfr_selfcheck_tables(cfr_dev_index *d, uint64_t out[6]) {
  if (!d || !out) return bad_arg("cfr_selfcheck_tables: null argument");
  CFR_ENTER(d, "cfr_selfcheck_tables");
  return guarded([&]() -> cfr_status { d->d->selfcheck(out); return CFR_OK; });
}

cfr_status cfr_search_batch(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1, const uint8_t *bases2,
                            const uint64_t *offsets2, size_t n, cfr_hit *out_hits, size_t hit_cap, uint64_t *hit_begin) {
  if (!d || !hit_begin || (n && (!bases1 || !offsets1))) return bad_arg("cfr_search_batch: null argument");
  if ((bases2 == nullptr) != (offsets2 == nullptr)) return bad_arg("cfr_search_batch: bases2/offsets2 must both be given");
  CFR_ENTER(d, "cfr_search_batch");
  return guarded([&]() -> cfr_status {
    cfr::DeviceIndex::BatchOut out;
    d->d->run_batch_host(bases1, offsets1, bases2, offsets2, n, false, out);
    memcpy(hit_begin, out.hit_begin.data(), (n + 1) * 8);
    if (out.hits.size() > hit_cap) { g_err = "cfr_search_batch: hit buffer too small"; return CFR_ERR_CAPACITY; }
    if (!out.hits.empty()) memcpy(out_hits, out.hits.data(), out.hits.size() * sizeof(cfr_hit));
    return CFR_OK;
  });
}

cfr_status cfr_classify_batch(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1, const uint8_t *bases2,
                              const uint64_t *offsets2, size_t n, cfr_result *results, cfr_match *matches, size_t match_cap,
                              size_t *n_matches) {
  if (!d || (n && (!bases1 || !offsets1 || !results))) return bad_arg("cfr_classify_batch: null argument");
  if ((bases2 == nullptr) != (offsets2 == nullptr)) return bad_arg("cfr_classify_batch: bases2/offsets2 must both be given");
  CFR_ENTER(d, "cfr_classify_batch");
  return guarded([&]() -> cfr_status {
    d->d->classify_host(bases1, offsets1, bases2, offsets2, n, results, matches, match_cap, n_matches);
    return CFR_OK;
  });
}

// --expand-taxid: the records the tail appended (slot, count, ids ...) in whatever order its atomics fell, made into spans over an id
// array in match-slot order.  A sub-batch that ran twice (scratch pool too small the first time) left two records for a slot, with
// the same ids: the last one counts.
static cfr_status expanded_out(const std::vector<uint64_t> &raw, cfr_span *spans, size_t match_cap, uint64_t *ids, size_t ids_cap, size_t *n_ids) {
  for (size_t m = 0; m < match_cap; ++m) spans[m] = cfr_span{0, 0};
  std::vector<std::pair<uint64_t, size_t>> recs;             // (slot, position of the record)
  for (size_t at = 0; at + 2 <= raw.size(); at += 2 + (size_t)raw[at + 1]) recs.emplace_back(raw[at], at);
  std::stable_sort(recs.begin(), recs.end(), [](const std::pair<uint64_t, size_t> &a, const std::pair<uint64_t, size_t> &b) { return a.first < b.first; });
  size_t need = 0;
  for (size_t j = 0; j < recs.size(); ++j) if (j + 1 == recs.size() || recs[j + 1].first != recs[j].first) need += (size_t)raw[recs[j].second + 1];
  if (n_ids) *n_ids = need;
  if (need > ids_cap) { g_err = "cfr_classify_batch_expanded: id buffer too small"; return CFR_ERR_CAPACITY; }
  size_t out = 0;
  for (size_t j = 0; j < recs.size(); ++j) {
    if (j + 1 < recs.size() && recs[j + 1].first == recs[j].first) continue;
    const size_t at = recs[j].second, cnt = (size_t)raw[at + 1];
    if (recs[j].first >= match_cap) { g_err = "cfr_classify_batch_expanded: a list for a match slot outside the match buffer"; return CFR_ERR_HIP; }
    spans[recs[j].first] = cfr_span{out, cnt};
    memcpy(ids + out, raw.data() + at + 2, cnt * 8);
    out += cnt;
  }
  return CFR_OK;
}

cfr_status cfr_classify_batch_expanded(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1, const uint8_t *bases2,
                                       const uint64_t *offsets2, size_t n, cfr_result *results, cfr_match *matches, cfr_span *spans,
                                       size_t match_cap, size_t *n_matches, uint64_t *ids, size_t ids_cap, size_t *n_ids) {
  if (!d || (n && (!bases1 || !offsets1 || !results)) || (match_cap && !spans) || (ids_cap && !ids)) return bad_arg("cfr_classify_batch_expanded: null argument");
  if ((bases2 == nullptr) != (offsets2 == nullptr)) return bad_arg("cfr_classify_batch_expanded: bases2/offsets2 must both be given");
  if (!d->d->host().params.output_expanded) return bad_arg("cfr_classify_batch_expanded: the index was opened without cfr_params.output_expanded");
  if (d->d->promote()) return bad_arg("cfr_classify_batch_expanded: promotion is switched on (cfr_device_index_set_promote) and does not cover the expanded lists");
  if (d->d->kreport()) return bad_arg("cfr_classify_batch_expanded: the report is switched on (cfr_device_index_set_kreport) and is made by the wide entries only");
  if (d->d->tsv()) return bad_arg("cfr_classify_batch_expanded: the rows are made on the device (cfr_device_index_set_tsv), which does not make the expandedTaxIDs column");
  CFR_ENTER(d, "cfr_classify_batch_expanded");
  return guarded([&]() -> cfr_status {
    d->d->classify_host(bases1, offsets1, bases2, offsets2, n, results, matches, match_cap, n_matches);
    return expanded_out(d->d->expanded_raw_, spans, match_cap, ids, ids_cap, n_ids);
  });
}

// cfr_pack_reads: the packed form of a read buffer (what k_pack_reads makes on the device), on host threads
cfr_status cfr_pack_reads(const uint8_t *bases, uint64_t total, int threads, uint64_t *packed) {
  if ((total && !bases) || !packed) return bad_arg("cfr_pack_reads: null argument");
  const uint64_t nblk = (total + 15) / 16;
  auto conv4 = [](uint32_t x, uint32_t &code8, uint32_t &valid4) {        // 4 ASCII bytes -> 4 two-bit codes + 4 validity bits (the device's conv4)
    uint32_t k = (x >> 1) & 0x03030303u;
    k ^= (k >> 1) & 0x01010101u;
    const uint32_t b0 = k & 0x01010101u, b1 = (k >> 1) & 0x01010101u;
    const uint32_t expect = 0x41414141u + b0 * 2u + b1 * 6u + (b0 & b1) * 11u;
    const uint32_t d = x ^ expect;
    const uint32_t nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;
    const uint32_t ok = ~nz & 0x80808080u;
    valid4 = ((ok >> 7) | (ok >> 14) | (ok >> 21) | (ok >> 28)) & 0xfu;
    code8 = (k | (k >> 6) | (k >> 12) | (k >> 18)) & 0xffu;
  };
  cfr::parallel_slices(nblk, nblk < 4096 ? 1 : threads, [&](size_t lo, size_t hi, int) {
    for (uint64_t b = lo; b < hi; ++b) {
      uint32_t w[4] = {0, 0, 0, 0};
      const uint64_t a = b << 4;
      if (a + 16 <= total) memcpy(w, bases + a, 16);
      else memcpy(w, bases + a, (size_t)(total - a));               // bytes past the end: zero = not a symbol
      uint32_t c = 0, vv = 0;
      for (int q = 0; q < 4; ++q) { uint32_t c8, v4; conv4(w[q], c8, v4); c |= c8 << (8 * q); vv |= v4 << (4 * q); }
      packed[b] = (uint64_t)c | ((uint64_t)vv << 32);
    }
  });
  return CFR_OK;
}

cfr_status cfr_classify_batch_packed(cfr_dev_index *d, const uint64_t *packed1, const uint64_t *offsets1, const uint64_t *packed2,
                                     const uint64_t *offsets2, size_t n, cfr_result *results, cfr_match *matches, size_t match_cap,
                                     size_t *n_matches) {
  if (!d || (n && (!packed1 || !offsets1 || !results))) return bad_arg("cfr_classify_batch_packed: null argument");
  if ((packed2 == nullptr) != (offsets2 == nullptr)) return bad_arg("cfr_classify_batch_packed: packed2/offsets2 must both be given");
  if (d->d->host().prot.enabled) return bad_arg("cfr_classify_batch_packed: a protein index needs the characters themselves (DnaToAa tells non-symbols apart): use cfr_classify_batch");
  if (d->d->merge()) return bad_arg("cfr_classify_batch_packed: --merge-readpair is switched on and the packed form cannot tell 'N' from other bytes (ReadPairMerger compares them): use cfr_classify_batch_merged");
  CFR_ENTER(d, "cfr_classify_batch_packed");
  return guarded([&]() -> cfr_status {
    d->d->classify_host_packed(packed1, offsets1, packed2, offsets2, n, results, matches, match_cap, n_matches);
    return CFR_OK;
  });
}

cfr_status cfr_classify_batch_submit(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1, const uint8_t *bases2,
                                     const uint64_t *offsets2, size_t n, cfr_result *results, cfr_match *matches, size_t match_cap,
                                     cfr_ticket *ticket) {
  if (!d || !ticket || (n && (!bases1 || !offsets1 || !results))) return bad_arg("cfr_classify_batch_submit: null argument");
  if ((bases2 == nullptr) != (offsets2 == nullptr)) return bad_arg("cfr_classify_batch_submit: bases2/offsets2 must both be given");
  std::lock_guard<std::mutex> lk(d->qmu);
  if (d->live.size() >= CFR_MAX_PENDING) { g_err = "cfr_classify_batch_submit: CFR_MAX_PENDING batches are outstanding on this cfr_dev_index"; return CFR_ERR_BUSY; }
  if (!d->worker_started) { d->worker = std::thread(worker_loop, d); d->worker_started = true; }
  cfr_async_job job;
  job.ticket = d->next_ticket++;
  job.run = [=](std::string &err, size_t &nm) -> cfr_status {
    const cfr_status st = guarded([&]() -> cfr_status {
      d->d->classify_host(bases1, offsets1, bases2, offsets2, n, results, matches, match_cap, &nm);
      return CFR_OK;
    });
    if (st != CFR_OK) err = g_err;                       // (the worker's thread-local message travels with the ticket)
    return st;
  };
  *ticket = job.ticket;
  d->live.insert(job.ticket);
  d->queue.push_back(std::move(job));
  d->qcv.notify_one();
  return CFR_OK;
}
cfr_status cfr_classify_batch_wait(cfr_dev_index *d, cfr_ticket ticket, size_t *n_matches) {
  if (!d) return bad_arg("cfr_classify_batch_wait: null argument");
  std::unique_lock<std::mutex> lk(d->qmu);
  if (!d->live.count(ticket)) { g_err = "cfr_classify_batch_wait: unknown ticket, or one that has been waited for already"; return CFR_ERR_ARG; }
  d->live.erase(ticket);                                 // (a second waiter for the same ticket gets the error above)
  d->dcv.wait(lk, [&] { return d->done.count(ticket) != 0; });
  cfr_async_done r = std::move(d->done[ticket]);
  d->done.erase(ticket);
  lk.unlock();
  if (n_matches) *n_matches = r.n_matches;
  if (r.status != CFR_OK) g_err = r.err;
  return r.status;
}

cfr_status cfr_classify_batch_resident(cfr_dev_index *d, const void *d_bases1, const void *d_offsets1, const void *d_bases2,
                                       const void *d_offsets2, size_t n, uint64_t total_bases1, uint64_t total_bases2,
                                       cfr_result *results, cfr_match *matches, size_t match_cap, size_t *n_matches) {
  if (!d || (n && (!d_bases1 || !d_offsets1 || !results))) return bad_arg("cfr_classify_batch_resident: null argument");
  if ((d_bases2 == nullptr) != (d_offsets2 == nullptr)) return bad_arg("cfr_classify_batch_resident: mate buffers must both be given");
  CFR_ENTER(d, "cfr_classify_batch_resident");
  return guarded([&]() -> cfr_status {
    d->d->classify_device((const uint8_t *)d_bases1, (const uint64_t *)d_offsets1, (const uint8_t *)d_bases2,
                          (const uint64_t *)d_offsets2, n, total_bases1, total_bases2, results, matches, match_cap, n_matches);
    return CFR_OK;
  });
}

cfr_status cfr_classify_batch_resident_compact(cfr_dev_index *d, const void *d_bases1, const void *d_offsets1, const void *d_bases2,
                                               const void *d_offsets2, size_t n, uint64_t total_bases1, uint64_t total_bases2,
                                               cfr_result_compact *results, cfr_match_compact *matches, size_t match_cap, size_t *n_matches) {
  if (!d || (n && (!d_bases1 || !d_offsets1 || !results || !matches))) return bad_arg("cfr_classify_batch_resident_compact: null argument");
  if ((d_bases2 == nullptr) != (d_offsets2 == nullptr)) return bad_arg("cfr_classify_batch_resident_compact: mate buffers must both be given");
  if (d->d->promote()) return bad_arg("cfr_classify_batch_resident_compact: promotion is switched on (cfr_device_index_set_promote) and works on the wide layout: use cfr_classify_batch_resident");
  if (d->d->kreport()) return bad_arg("cfr_classify_batch_resident_compact: the report is switched on (cfr_device_index_set_kreport) and works on the wide layout: use cfr_classify_batch_resident");
  if (d->d->tsv()) return bad_arg("cfr_classify_batch_resident_compact: the rows are made on the device (cfr_device_index_set_tsv) from the wide layout: use cfr_classify_batch_resident");
  CFR_ENTER(d, "cfr_classify_batch_resident_compact");
  return guarded([&]() -> cfr_status {
    d->d->classify_device((const uint8_t *)d_bases1, (const uint64_t *)d_offsets1, (const uint8_t *)d_bases2,
                          (const uint64_t *)d_offsets2, n, total_bases1, total_bases2, reinterpret_cast<cfr_result *>(results),
                          reinterpret_cast<cfr_match *>(matches), match_cap, n_matches, nullptr, /*compact=*/true);
    return CFR_OK;
  });
}

cfr_status cfr_compact_wide_reads(cfr_dev_index *d, size_t *n, const uint32_t **read_index, const cfr_result **results, const cfr_match **matches) {
  if (!d || !n) return bad_arg("cfr_compact_wide_reads: null argument");
  CFR_ENTER(d, "cfr_compact_wide_reads");
  const cfr::DeviceIndex &D = *d->d;
  *n = (size_t)D.wide_total_;
  if (read_index) *read_index = D.wide_idx_.data();
  if (results) *results = D.wide_res_.data();
  if (matches) *matches = D.wide_match_.data();
  if (D.wide_total_ > D.wide_idx_.size()) { g_err = "cfr_compact_wide_reads: more flagged reads than the side list holds"; return CFR_ERR_CAPACITY; }
  return CFR_OK;
}

void *cfr_host_alloc(size_t bytes) { return cfr::host_alloc_pinned(bytes); }
void cfr_host_free(void *p) { cfr::host_free_pinned(p); }

cfr_status cfr_classify_from_hits(const cfr_index *idx, const cfr_hit *hits, const uint64_t *hit_begin, const uint64_t *row_begin,
                                  const uint64_t *row_vals, const int32_t *query_len, size_t n, int threads, cfr_result *results,
                                  cfr_match *matches, size_t match_cap, size_t *n_matches) {
  if (!idx || !hit_begin || (n && (!results || !query_len))) return bad_arg("cfr_classify_from_hits: null argument");
  return guarded([&]() -> cfr_status {
    cfr::DeviceIndex::BatchOut out;
    out.hit_begin.assign(hit_begin, hit_begin + n + 1);
    const uint64_t nh = hit_begin[n];
    out.hits.assign(hits, hits + nh);
    out.row_begin.assign(row_begin, row_begin + nh + 1);
    out.row_vals.assign(row_vals, row_vals + row_begin[nh]);
    out.read_len.assign(query_len, query_len + n);
    std::vector<cfr_match> mv;
    cfr::classify_batch_tail(*idx->h, out, n, threads, results, mv);
    if (n_matches) *n_matches = mv.size();
    if (mv.size() > match_cap) { g_err = "cfr_classify_from_hits: match buffer too small"; return CFR_ERR_CAPACITY; }
    if (!mv.empty()) memcpy(matches, mv.data(), mv.size() * sizeof(cfr_match));
    return CFR_OK;
  });
}

cfr_status cfr_classify_from_hits_expanded(const cfr_index *idx, const cfr_hit *hits, const uint64_t *hit_begin, const uint64_t *row_begin,
                                           const uint64_t *row_vals, const int32_t *query_len, size_t n, int threads, cfr_result *results,
                                           cfr_match *matches, cfr_span *spans, size_t match_cap, size_t *n_matches, uint64_t *ids, size_t ids_cap,
                                           size_t *n_ids) {
  if (!idx || !hit_begin || (n && (!results || !query_len)) || (match_cap && !spans) || (ids_cap && !ids)) return bad_arg("cfr_classify_from_hits_expanded: null argument");
  if (!idx->h->params.output_expanded) return bad_arg("cfr_classify_from_hits_expanded: the index was opened without cfr_params.output_expanded");
  return guarded([&]() -> cfr_status {
    cfr::DeviceIndex::BatchOut out;
    out.hit_begin.assign(hit_begin, hit_begin + n + 1);
    const uint64_t nh = hit_begin[n];
    out.hits.assign(hits, hits + nh);
    out.row_begin.assign(row_begin, row_begin + nh + 1);
    out.row_vals.assign(row_vals, row_vals + row_begin[nh]);
    out.read_len.assign(query_len, query_len + n);
    std::vector<cfr_match> mv;
    cfr::ExpandedLists x;
    cfr::classify_batch_tail(*idx->h, out, n, threads, results, mv, &x);
    if (n_matches) *n_matches = mv.size();
    if (n_ids) *n_ids = x.ids.size();
    if (mv.size() > match_cap) { g_err = "cfr_classify_from_hits_expanded: match buffer too small"; return CFR_ERR_CAPACITY; }
    if (x.ids.size() > ids_cap) { g_err = "cfr_classify_from_hits_expanded: id buffer too small"; return CFR_ERR_CAPACITY; }
    if (!mv.empty()) memcpy(matches, mv.data(), mv.size() * sizeof(cfr_match));
    for (size_t m = 0; m < match_cap; ++m) spans[m] = m < x.spans.size() ? x.spans[m] : cfr_span{0, 0};
    if (!x.ids.empty()) memcpy(ids, x.ids.data(), x.ids.size() * 8);
    return CFR_OK;
  });
}

cfr_status cfr_last_batch_stats(const cfr_dev_index *d, cfr_batch_stats *st) {
  if (!d || !st) return bad_arg("cfr_last_batch_stats: null argument");
  *st = d->d->last_stats;
  return CFR_OK;
}

static cfr_status dust_batch(uint8_t *bases, const uint64_t *offsets, size_t n, int threads, void (*mask)(uint8_t *, size_t)) {
  if (n && (!bases || !offsets)) return bad_arg("cfr_dust_mask_batch: null argument");
  // a contiguous slice per thread (reads are independent; the reference strides them, the result is the same)
  cfr::parallel_slices(n, threads, [&](size_t lo, size_t hi, int) {
    for (size_t i = lo; i < hi; ++i) mask(bases + offsets[i], offsets[i + 1] - offsets[i]);
  });
  return CFR_OK;
}
cfr_status cfr_dust_mask_batch(uint8_t *bases, const uint64_t *offsets, size_t n, int threads) {
  return dust_batch(bases, offsets, n, threads, cfr::dust_mask);
}
cfr_status cfr_dust_mask_batch_literal(uint8_t *bases, const uint64_t *offsets, size_t n, int threads) {
  return dust_batch(bases, offsets, n, threads, cfr::dust_mask_literal);
}

cfr_status cfr_device_index_set_dust(cfr_dev_index *d, int on) {
  if (!d) return bad_arg("cfr_device_index_set_dust: null argument");
  CFR_ENTER(d, "cfr_device_index_set_dust");
  d->d->set_dust(on != 0);
  return CFR_OK;
}
cfr_status cfr_dust_mask_device(cfr_dev_index *d, uint8_t *bases, const uint64_t *offsets, size_t n) {
  if (!d || (n && (!bases || !offsets))) return bad_arg("cfr_dust_mask_device: null argument");
  CFR_ENTER(d, "cfr_dust_mask_device");
  return guarded([&]() -> cfr_status {
    d->d->dust_mask_host(bases, offsets, n);
    return CFR_OK;
  });
}

// ---- centrifuger-quant ----
void cfr_quant_options_default(cfr_quant_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->device = 0;
}

cfr_status cfr_quant_open(const char *idx_prefix, const cfr_quant_options *o, cfr_quant **out) {
  if (!idx_prefix || !out) return bad_arg("cfr_quant_open: null argument");
  *out = nullptr;
  return guarded([&]() -> cfr_status {
    cfr::QuantOptions qo;
    if (o) { qo.min_score = o->min_score; qo.min_length = o->min_length; qo.device = o->device; qo.table_slots = o->table_slots; qo.threads = o->threads; }
    else qo.device = 0;
    cfr_quant *q = new cfr_quant();
    try { q->q = new cfr::Quant(idx_prefix, qo); } catch (...) { delete q; throw; }
    *out = q;
    return CFR_OK;
  });
}

cfr_status cfr_quant_add_tsv(cfr_quant *q, const char *path) {
  if (!q || !path) return bad_arg("cfr_quant_add_tsv: null argument");
  return guarded([&]() -> cfr_status { q->q->add_tsv(path); return CFR_OK; });
}

cfr_status cfr_quant_add_results(cfr_quant *q, const cfr_result *r, const cfr_match *m, size_t n) {
  if (!q || (n && (!r || !m))) return bad_arg("cfr_quant_add_results: null argument");
  return guarded([&]() -> cfr_status { q->q->add_results(r, m, n); return CFR_OK; });
}

cfr_status cfr_quant_assignments(cfr_quant *q, size_t *n, const uint64_t **begin, const uint32_t **targets, const double **weight,
                                 const uint64_t **count, const uint64_t **uniq) {
  if (!q || !n) return bad_arg("cfr_quant_assignments: null argument");
  return guarded([&]() -> cfr_status {
    const cfr::QuantAssignments &a = q->q->assignments();
    q->weight.resize(a.n());
    for (size_t i = 0; i < a.n(); ++i) q->weight[i] = (double)a.weight_units[i] / (double)(1ull << cfr::kQuantWeightShift);
    *n = a.n();
    if (begin) *begin = a.begin.data();
    if (targets) *targets = a.targets.data();
    if (weight) *weight = q->weight.data();
    if (count) *count = a.count.data();
    if (uniq) *uniq = a.uniq.data();
    return CFR_OK;
  });
}

cfr_status cfr_quant_run(cfr_quant *q, int32_t *em_rounds) {
  if (!q) return bad_arg("cfr_quant_run: null argument");
  return guarded([&]() -> cfr_status {
    q->rounds = q->q->run();
    q->ran = true;
    if (em_rounds) *em_rounds = q->rounds;
    return CFR_OK;
  });
}

cfr_status cfr_quant_values(const cfr_quant *q, const double **abund, const double **read_count, const double **uniq_count,
                            const uint64_t **taxid_length, uint64_t *node_cnt) {
  if (!q) return bad_arg("cfr_quant_values: null argument");
  if (abund) *abund = q->q->abund().data();
  if (read_count) *read_count = q->q->read_count().data();
  if (uniq_count) *uniq_count = q->q->uniq_count().data();
  if (taxid_length) *taxid_length = q->q->taxid_length().data();
  if (node_cnt) *node_cnt = q->q->node_cnt();
  return CFR_OK;
}

cfr_status cfr_quant_write(const cfr_quant *q, int format, const char *path) {
  if (!q || !path) return bad_arg("cfr_quant_write: null argument");
  if (!q->ran) return bad_arg("cfr_quant_write: cfr_quant_run has not been called");
  const bool to_stdout = !strcmp(path, "-");
  FILE *fp = to_stdout ? stdout : fopen(path, "w");
  if (!fp) { g_err = std::string("cannot write ") + path; return CFR_ERR_IO; }
  q->q->write(fp, format);
  if (to_stdout) fflush(fp); else fclose(fp);
  return CFR_OK;
}

cfr_status cfr_quant_get_stats(const cfr_quant *q, cfr_quant_stats *st) {
  if (!q || !st) return bad_arg("cfr_quant_get_stats: null argument");
  memset(st, 0, sizeof(*st));
  st->reader_ms = q->q->reader_ms; st->coalesce_ms = q->q->coalesce_ms; st->em_ms = q->q->em_ms;
  const cfr::QuantDeviceStats d = q->q->device_stats();
  st->grow_count = d.grow_count; st->table_slots = d.table_slots; st->em_rounds = q->rounds;
  return CFR_OK;
}

void cfr_quant_destroy(cfr_quant *q) {
  if (!q) return;
  delete q->q;
  delete q;
}

cfr_status cfr_quant_estep_probe(int32_t device, const uint64_t *a_begin, const uint32_t *a_target, const double *a_weight, size_t n_assign,
                                 uint64_t n_nodes, int32_t init_round, const double *abund, size_t n_rounds, double *out_read_count) {
  if (!a_begin || (n_assign && !a_weight) || (n_rounds && !abund) || ((init_round || n_rounds) && !out_read_count))
    return bad_arg("cfr_quant_estep_probe: null argument");
  if (n_nodes == 0 || n_nodes >= 0xffffffffull) return bad_arg("cfr_quant_estep_probe: n_nodes must be 1 .. 2^32 - 2");
  if (a_begin[0] != 0) return bad_arg("cfr_quant_estep_probe: a_begin[0] must be 0");
  for (size_t i = 0; i < n_assign; ++i)
    if (a_begin[i + 1] < a_begin[i]) return bad_arg("cfr_quant_estep_probe: a_begin must not decrease");
  const uint64_t n_slots = a_begin[n_assign];
  if (n_slots && !a_target) return bad_arg("cfr_quant_estep_probe: null argument");
  for (uint64_t s = 0; s < n_slots; ++s)
    if (a_target[s] >= n_nodes) return bad_arg("cfr_quant_estep_probe: a target is not below n_nodes");
  return guarded([&]() -> cfr_status {
    cfr::QuantCsr csr;
    csr.n_nodes = n_nodes;
    csr.a_begin.assign(a_begin, a_begin + n_assign + 1);
    csr.a_target.assign(a_target, a_target + n_slots);
    csr.a_weight.assign(a_weight, a_weight + n_assign);
    cfr::quant_csr_finish(csr);
    std::unique_ptr<cfr::QuantEStep> estep(device >= 0 ? cfr::make_device_estep(device, csr) : cfr::make_host_estep(csr));
    double *out = out_read_count;
    if (init_round) { estep->run(nullptr, true, out); out += n_nodes; }
    for (size_t k = 0; k < n_rounds; ++k, out += n_nodes) estep->run(abund + k * n_nodes, false, out);
    return CFR_OK;
  });
}

// ---- centrifuger-inspect ----
cfr_status cfr_taxonomy_open(const char *idx_prefix, int with_lengths, cfr_taxonomy **out) {
  if (!idx_prefix || !out) return bad_arg("cfr_taxonomy_open: null argument");
  *out = nullptr;
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_taxonomy> t(new cfr_taxonomy());
    cfr::load_taxonomy(std::string(idx_prefix) + ".2.cfr", t->tax);
    const uint64_t nc = t->tax.node_cnt;
    if (t->tax.rank.size() < nc || t->tax.orig_taxid.size() < nc) throw cfr::FormatError{std::string(idx_prefix) + ".2.cfr: taxonomy tables shorter than the node count"};
    for (uint64_t i = 0; i < nc; ++i)
      if (t->tax.parent[i] >= nc) throw cfr::FormatError{std::string(idx_prefix) + ".2.cfr: the parent of node " + std::to_string(i) + " is outside the tree"};
    std::set<std::string> seen;
    for (const std::string &s : t->tax.seq_name) if (seen.insert(s).second) t->seq_names.push_back(s);
    if (with_lengths) {
      t->with_lengths = true;
      const std::map<uint64_t, uint64_t> len = cfr::read_seq_lengths(idx_prefix);
      for (const auto &kv : len) { t->length_seq_id.push_back(kv.first); t->length_value.push_back(kv.second); }
      cfr::tax_genome_lengths(t->tax, len, t->taxid_length);
    }
    *out = t.release();
    return CFR_OK;
  });
}

cfr_status cfr_taxonomy_get_tables(const cfr_taxonomy *t, cfr_taxonomy_tables *o) {
  if (!t || !o) return bad_arg("cfr_taxonomy_get_tables: null argument");
  memset(o, 0, sizeof(*o));
  o->node_cnt = t->tax.node_cnt; o->seq_cnt = t->tax.seq_cnt; o->extra_seq_cnt = t->tax.extra_seq_cnt; o->root = t->tax.root;
  o->n_seq_names = t->seq_names.size(); o->n_seq_lengths = t->length_seq_id.size();
  o->parent = t->tax.parent.data(); o->orig_taxid = t->tax.orig_taxid.data(); o->seq_to_tax = t->tax.seq_to_tax.data(); o->rank = t->tax.rank.data();
  if (t->with_lengths) { o->taxid_length = t->taxid_length.data(); o->length_seq_id = t->length_seq_id.data(); o->length_value = t->length_value.data(); }
  return CFR_OK;
}

const char *cfr_taxonomy_tax_name(const cfr_taxonomy *t, uint64_t ctid) {
  if (!t || ctid >= t->tax.node_cnt) return "Unknown";
  return t->tax.tax_name[ctid].c_str();
}
const char *cfr_taxonomy_seq_name(const cfr_taxonomy *t, uint64_t seq_id) {
  if (!t || seq_id >= t->seq_names.size()) return nullptr;
  return t->seq_names[seq_id].c_str();
}
const char *cfr_tax_rank_string(uint8_t rank) { return cfr::quant_rank_string(rank); }
void cfr_taxonomy_close(cfr_taxonomy *t) { delete t; }

cfr_status cfr_taxonomy_lca_probe(const cfr_taxonomy *t, const uint64_t *ids, const uint64_t *begin, size_t n_lists, int32_t form,
                                  uint64_t *out, uint32_t *steps) {
  if (!t || !begin || !out || (n_lists && begin[n_lists] && !ids)) return bad_arg("cfr_taxonomy_lca_probe: null argument");
  if (form != 0 && form != 1) return bad_arg("cfr_taxonomy_lca_probe: form is 0 or 1");
  return guarded([&]() -> cfr_status {
    for (size_t i = 0; i < n_lists; ++i) if (begin[i] > begin[i + 1]) throw std::invalid_argument("cfr_taxonomy_lca_probe: begin must ascend");
    for (uint64_t j = 0; j < begin[n_lists]; ++j) if (ids[j] >= t->tax.node_cnt) throw std::invalid_argument("cfr_taxonomy_lca_probe: id outside the tree");
    const std::vector<uint32_t> depth = cfr::promote_depths(t->tax.parent);
    std::vector<uint64_t> one;
    for (size_t i = 0; i < n_lists; ++i) {
      uint32_t st = 0;
      if (form == 0) { one.assign(ids + begin[i], ids + begin[i + 1]); out[i] = cfr::tax_lca(t->tax, one); }
      else out[i] = cfr::tax_lca_fold(t->tax, depth, ids + begin[i], (size_t)(begin[i + 1] - begin[i]), &st);
      if (steps) steps[i] = st;
    }
    return CFR_OK;
  });
}

// ---- centrifuger-promote ----
cfr_status cfr_promote_open(const char *idx_prefix, const char *level, int device, cfr_promote **out) {
  if (!idx_prefix || !level || !out) return bad_arg("cfr_promote_open: null argument");
  *out = nullptr;
  if (device < -1) return bad_arg("cfr_promote_open: device is a HIP ordinal, or -1 for the host twin");
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_promote> h(new cfr_promote{nullptr});
    h->p = new cfr::Promote(idx_prefix, level, device);
    { std::lock_guard<std::mutex> lk(g_promote_mu); g_promote_live.insert(h.get()); }
    *out = h.release();
    return CFR_OK;
  });
}

cfr_status cfr_promote_apply(cfr_promote *h, cfr_result *results, cfr_match *matches, size_t n, uint64_t *src_slot) {
  if (!promote_live(h)) return bad_arg("cfr_promote_apply: not an open cfr_promote handle");
  if (n && !results) return bad_arg("cfr_promote_apply: null argument");
  for (size_t i = 0; i < n; ++i) {
    if (results[i].n_match > 0 && !matches) return bad_arg("cfr_promote_apply: null argument");
    if (results[i].n_match > 0 && results[i].match_begin + (uint64_t)results[i].n_match < results[i].match_begin) return bad_arg("cfr_promote_apply: match_begin + n_match wraps");
  }
  return guarded([&]() -> cfr_status { h->p->apply(results, matches, n, src_slot); return CFR_OK; });
}

cfr_status cfr_promote_lca_warnings(cfr_promote *h, const cfr_result *results, const cfr_match *matches, size_t n, uint64_t *taxids, size_t cap,
                                    size_t *count) {
  if (!promote_live(h)) return bad_arg("cfr_promote_lca_warnings: not an open cfr_promote handle");
  if (!count || (n && !results) || (cap && !taxids)) return bad_arg("cfr_promote_lca_warnings: null argument");
  for (size_t i = 0; i < n; ++i) if (results[i].n_match > 0 && !matches) return bad_arg("cfr_promote_lca_warnings: null argument");
  return guarded([&]() -> cfr_status {
    std::vector<uint64_t> w;
    h->p->lca_warnings(results, matches, n, w);
    *count = w.size();
    if (w.size() > cap) { g_err = "cfr_promote_lca_warnings: tax id buffer too small"; return CFR_ERR_CAPACITY; }
    if (!w.empty()) memcpy(taxids, w.data(), w.size() * 8);
    return CFR_OK;
  });
}

cfr_status cfr_promote_get_stats(cfr_promote *h, cfr_promote_stats *st) {
  if (!promote_live(h)) return bad_arg("cfr_promote_get_stats: not an open cfr_promote handle");
  if (!st) return bad_arg("cfr_promote_get_stats: null argument");
  st->table_ms = h->p->table_ms(); st->reads_ms = h->p->reads_ms();
  return CFR_OK;
}

cfr_status cfr_promote_close(cfr_promote *h) {
  {
    std::lock_guard<std::mutex> lk(g_promote_mu);
    if (!h || !g_promote_live.erase(h)) return bad_arg("cfr_promote_close: not an open cfr_promote handle");
  }
  delete h->p;
  delete h;
  return CFR_OK;
}

cfr_status cfr_device_index_set_promote(cfr_dev_index *d, const char *level) {
  if (!d) return bad_arg("cfr_device_index_set_promote: null argument");
  CFR_ENTER(d, "cfr_device_index_set_promote");
  return guarded([&]() -> cfr_status { d->d->set_promote(level); return CFR_OK; });
}
cfr_status cfr_last_promote_ms(const cfr_dev_index *d, float *ms) {
  if (!d || !ms) return bad_arg("cfr_last_promote_ms: null argument");
  *ms = d->d->last_promote_ms;
  return CFR_OK;
}

// ---- centrifuger-kreport ----
void cfr_kreport_options_default(cfr_kreport_options *o) {
  if (o) memset(o, 0, sizeof(*o));
}

cfr_status cfr_kreport_open(const char *idx_prefix, const cfr_kreport_options *opts, int device, cfr_kreport **out) {
  if (!idx_prefix || !opts || !out) return bad_arg("cfr_kreport_open: null argument");
  *out = nullptr;
  if (device < -1) return bad_arg("cfr_kreport_open: device is a HIP ordinal, or -1 for the host twin");
  if (opts->lds_slots && (opts->lds_slots < 64 || opts->lds_slots > 2048 || (opts->lds_slots & (opts->lds_slots - 1))))
    return bad_arg("cfr_kreport_open: lds_slots is 0 or a power of two in [64, 2048]");
  return guarded([&]() -> cfr_status {
    cfr::KreportOptions o;
    o.has_min_score = opts->has_min_score != 0; o.has_min_length = opts->has_min_length != 0;
    o.min_score = opts->min_score; o.min_length = opts->min_length;
    o.no_lca = opts->no_lca != 0; o.show_zeros = opts->show_zeros != 0; o.score_data = opts->score_data != 0;
    std::unique_ptr<cfr_kreport> h(new cfr_kreport{nullptr});
    h->k = new cfr::Kreport(idx_prefix, o, device, opts->max_blocks, opts->lds_slots, opts->threads);
    { std::lock_guard<std::mutex> lk(g_kreport_mu); g_kreport_live.insert(h.get()); }
    *out = h.release();
    return CFR_OK;
  });
}

cfr_status cfr_kreport_add_results(cfr_kreport *h, const cfr_result *results, const cfr_match *matches, size_t n) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_add_results: not an open cfr_kreport handle");
  if (n && !results) return bad_arg("cfr_kreport_add_results: null argument");
  for (size_t i = 0; i < n; ++i) {
    if (results[i].n_match > 0 && !matches) return bad_arg("cfr_kreport_add_results: null argument");
    if (results[i].n_match > 0 && results[i].match_begin + (uint64_t)results[i].n_match < results[i].match_begin) return bad_arg("cfr_kreport_add_results: match_begin + n_match wraps");
  }
  return guarded([&]() -> cfr_status { h->k->add_results(results, matches, n); return CFR_OK; });
}

cfr_status cfr_kreport_scan_warnings(cfr_kreport *h, const cfr_result *results, const cfr_match *matches, size_t n) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_scan_warnings: not an open cfr_kreport handle");
  if (n && !results) return bad_arg("cfr_kreport_scan_warnings: null argument");
  for (size_t i = 0; i < n; ++i) if (results[i].n_match > 0 && !matches) return bad_arg("cfr_kreport_scan_warnings: null argument");
  return guarded([&]() -> cfr_status { h->k->scan_warnings(results, matches, n); return CFR_OK; });
}

cfr_status cfr_kreport_add_tsv(cfr_kreport *h, const char *path) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_add_tsv: not an open cfr_kreport handle");
  if (!path) return bad_arg("cfr_kreport_add_tsv: null argument");
  return guarded([&]() -> cfr_status { h->k->add_tsv(path); return CFR_OK; });
}

cfr_status cfr_kreport_add_count_table(cfr_kreport *h, const char *path) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_add_count_table: not an open cfr_kreport handle");
  if (!path) return bad_arg("cfr_kreport_add_count_table: null argument");
  return guarded([&]() -> cfr_status { h->k->add_count_table(path); return CFR_OK; });
}

cfr_status cfr_kreport_add_counts(cfr_kreport *h, const uint64_t *own, const uint64_t *own_score, size_t n) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_add_counts: not an open cfr_kreport handle");
  if (!own) return bad_arg("cfr_kreport_add_counts: null argument");
  return guarded([&]() -> cfr_status { h->k->add_counts(own, own_score, n); return CFR_OK; });
}

cfr_status cfr_kreport_bins(cfr_kreport *h, size_t *n) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_bins: not an open cfr_kreport handle");
  if (!n) return bad_arg("cfr_kreport_bins: null argument");
  *n = (size_t)h->k->bins();
  return CFR_OK;
}

cfr_status cfr_kreport_counts(cfr_kreport *h, uint64_t *own, uint64_t *clade, uint64_t *own_score, uint64_t *clade_score, size_t cap, double *seq_count) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_counts: not an open cfr_kreport handle");
  if (!seq_count) return bad_arg("cfr_kreport_counts: null argument");
  if ((own || clade || own_score || clade_score) && cap < h->k->bins()) { g_err = "cfr_kreport_counts: the arrays take node_cnt + 1 entries"; return CFR_ERR_CAPACITY; }
  return guarded([&]() -> cfr_status {
    std::vector<uint64_t> a, b, c, d;
    h->k->counts(a, b, c, d, *seq_count);
    if (own) memcpy(own, a.data(), a.size() * 8);
    if (clade) memcpy(clade, b.data(), b.size() * 8);
    if (own_score) memcpy(own_score, c.data(), c.size() * 8);
    if (clade_score) memcpy(clade_score, d.data(), d.size() * 8);
    return CFR_OK;
  });
}

cfr_status cfr_kreport_warnings(cfr_kreport *h, uint64_t *taxids, size_t cap, size_t *count) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_warnings: not an open cfr_kreport handle");
  if (!count || (cap && !taxids)) return bad_arg("cfr_kreport_warnings: null argument");
  const std::vector<uint64_t> &w = h->k->warnings();
  *count = w.size();
  if (w.size() > cap) { g_err = "cfr_kreport_warnings: tax id buffer too small"; return CFR_ERR_CAPACITY; }
  if (!w.empty()) memcpy(taxids, w.data(), w.size() * 8);
  return CFR_OK;
}

cfr_status cfr_kreport_write(cfr_kreport *h, const char *path) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_write: not an open cfr_kreport handle");
  return guarded([&]() -> cfr_status { h->k->write(path); return CFR_OK; });     // (nothing counted: std::runtime_error -> CFR_ERR_ARG with the script's message)
}

cfr_status cfr_device_index_set_kreport(cfr_dev_index *d, const cfr_kreport_options *opts) {
  if (!d) return bad_arg("cfr_device_index_set_kreport: null argument");
  CFR_ENTER(d, "cfr_device_index_set_kreport");
  return guarded([&]() -> cfr_status {
    if (!opts) { d->d->set_kreport(nullptr); return CFR_OK; }
    cfr::KreportOptions o;
    o.has_min_score = opts->has_min_score != 0; o.has_min_length = opts->has_min_length != 0;
    o.min_score = opts->min_score; o.min_length = opts->min_length;
    o.no_lca = opts->no_lca != 0; o.show_zeros = opts->show_zeros != 0; o.score_data = opts->score_data != 0;
    d->d->set_kreport(&o);
    return CFR_OK;
  });
}
cfr_status cfr_device_index_kreport_counts(cfr_dev_index *d, uint64_t *own, uint64_t *own_score, size_t cap, double *seq_count) {
  if (!d) return bad_arg("cfr_device_index_kreport_counts: null argument");
  CFR_ENTER(d, "cfr_device_index_kreport_counts");
  if ((own || own_score) && cap < d->d->kreport_bins()) { g_err = "cfr_device_index_kreport_counts: the arrays take node_cnt + 1 entries"; return CFR_ERR_CAPACITY; }
  return guarded([&]() -> cfr_status { d->d->kreport_counts(own, own_score, seq_count); return CFR_OK; });
}
cfr_status cfr_last_kreport_ms(const cfr_dev_index *d, float *ms) {
  if (!d || !ms) return bad_arg("cfr_last_kreport_ms: null argument");
  *ms = d->d->last_kreport_ms;
  return CFR_OK;
}

cfr_status cfr_kreport_get_stats(cfr_kreport *h, cfr_kreport_stats *st) {
  if (!kreport_live(h)) return bad_arg("cfr_kreport_get_stats: not an open cfr_kreport handle");
  if (!st) return bad_arg("cfr_kreport_get_stats: null argument");
  st->fold_ms = h->k->fold_ms(); st->accumulate_ms = h->k->accumulate_ms(); st->parse_ms = h->k->parse_ms();
  return CFR_OK;
}

cfr_status cfr_kreport_close(cfr_kreport *h) {
  {
    std::lock_guard<std::mutex> lk(g_kreport_mu);
    if (!h || !g_kreport_live.erase(h)) return bad_arg("cfr_kreport_close: not an open cfr_kreport handle");
  }
  delete h->k;
  delete h;
  return CFR_OK;
}

// ---- the tokeniser of raw FASTA/FASTQ text (cfr_tokenize_core.hpp) ----
cfr_status cfr_tokenizer_open(int device, cfr_tokenizer **out) {
  if (!out) return bad_arg("cfr_tokenizer_open: null argument");
  *out = nullptr;
  if (device < -1) return bad_arg("cfr_tokenizer_open: device is a HIP ordinal, or -1 for the host twin");
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_tokenizer> h(new cfr_tokenizer{nullptr});
    h->t = device < 0 ? cfr::make_tokenizer_host() : cfr::make_tokenizer_device(device);
    { std::lock_guard<std::mutex> lk(g_tokenizer_mu); g_tokenizer_live.insert(h.get()); }
    *out = h.release();
    return CFR_OK;
  });
}

cfr_status cfr_tokenize(cfr_tokenizer *t, const uint8_t *text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info) {
  if (!tokenizer_live(t)) return bad_arg("cfr_tokenize: not an open cfr_tokenizer handle");
  if (!info || (len && !text)) return bad_arg("cfr_tokenize: null argument");
  if (len >> 32) return bad_arg("cfr_tokenize: len must be below 2^32 (offsets inside a call are 32 bits wide on the device): hand the text over in pieces");
  if (len && text[0] != '>' && text[0] != '@') return bad_arg("cfr_tokenize: the text starts with neither '>' (FASTA) nor '@' (FASTQ)");
  return guarded([&]() -> cfr_status { t->t->tokenize(text, len, final, max_records, info); return CFR_OK; });
}

cfr_status cfr_tokenizer_fetch(cfr_tokenizer *t, cfr_read_record *records, uint64_t *offsets, uint8_t *bases) {
  if (!tokenizer_live(t)) return bad_arg("cfr_tokenizer_fetch: not an open cfr_tokenizer handle");
  return guarded([&]() -> cfr_status { t->t->fetch(records, offsets, bases); return CFR_OK; });
}

cfr_status cfr_tokenizer_device_reads(cfr_tokenizer *t, const void **d_bases, const void **d_offsets) {
  if (!tokenizer_live(t)) return bad_arg("cfr_tokenizer_device_reads: not an open cfr_tokenizer handle");
  if (!t->t->device_reads(d_bases, d_offsets)) return bad_arg("cfr_tokenizer_device_reads: the handle is the host twin (opened with device -1)");
  return CFR_OK;
}

cfr_status cfr_tokenizer_get_stats(cfr_tokenizer *t, cfr_token_stats *st) {
  if (!tokenizer_live(t)) return bad_arg("cfr_tokenizer_get_stats: not an open cfr_tokenizer handle");
  if (!st) return bad_arg("cfr_tokenizer_get_stats: null argument");
  t->t->stats(st);
  return CFR_OK;
}

void cfr_tokenizer_close(cfr_tokenizer *t) {
  {
    std::lock_guard<std::mutex> lk(g_tokenizer_mu);
    if (!t || !g_tokenizer_live.erase(t)) return;
  }
  delete t->t;
  delete t;
}

cfr_status cfr_tokenizer_device_records(cfr_tokenizer *t, const void **d_text, const void **d_records) {
  if (!tokenizer_live(t)) return bad_arg("cfr_tokenizer_device_records: not an open cfr_tokenizer handle");
  if (!t->t->device_records(d_text, d_records)) return bad_arg("cfr_tokenizer_device_records: the handle is the host twin (opened with device -1)");
  return CFR_OK;
}

// ---- the rows of a batch as one text (cfr_tsv_core.hpp) ----
void cfr_tsv_options_default(cfr_tsv_options *o) { if (o) memset(o, 0, sizeof(*o)); }

cfr_status cfr_tsv_open(const cfr_index *idx, int device, const cfr_tsv_options *o, cfr_tsv **out) {
  if (!idx || !out) return bad_arg("cfr_tsv_open: null argument");
  *out = nullptr;
  if (device < -1) return bad_arg("cfr_tsv_open: device is a HIP ordinal, or -1 for the host twin");
  cfr_tsv_options opt{};
  if (o) opt = *o;
  if (opt.tile_bytes < 0 || opt.max_blocks < 0 || opt.threads < 0) return bad_arg("cfr_tsv_open: an option below 0");
  return guarded([&]() -> cfr_status {
    cfr::TsvTables t;
    t.set_names(idx->h->tax.seq_name);
    t.rank = idx->h->tax.rank;
    t.rank.resize((size_t)idx->h->tax.node_cnt);
    t.set_rank_strings(cfr::tax_rank_string);
    std::unique_ptr<cfr_tsv> h(new cfr_tsv{nullptr});
    h->t = device < 0 ? cfr::make_tsv_host(t, opt.threads) : cfr::make_tsv_device(device, t, opt);
    { std::lock_guard<std::mutex> lk(g_tsv_mu); g_tsv_live.insert(h.get()); }
    *out = h.release();
    return CFR_OK;
  });
}

cfr_status cfr_tsv_format(cfr_tsv *t, const cfr_result *results, const cfr_match *matches, size_t n_slots, size_t n, const char *id_bytes,
                          const uint64_t *id_offsets, char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets) {
  if (!tsv_live(t)) return bad_arg("cfr_tsv_format: not an open cfr_tsv handle");
  return guarded([&]() -> cfr_status {
    if (t->t->format(results, matches, n_slots, n, id_bytes, id_offsets, text, cap, len, row_offsets)) return CFR_OK;
    g_err = "cfr_tsv_format: the text takes " + std::to_string(*len) + " bytes, the buffer holds " + std::to_string(cap);
    return CFR_ERR_CAPACITY;
  });
}

cfr_status cfr_tsv_get_stats(cfr_tsv *t, cfr_tsv_stats *st) {
  if (!tsv_live(t)) return bad_arg("cfr_tsv_get_stats: not an open cfr_tsv handle");
  if (!st) return bad_arg("cfr_tsv_get_stats: null argument");
  t->t->stats(st);
  return CFR_OK;
}

void cfr_tsv_close(cfr_tsv *t) {
  {
    std::lock_guard<std::mutex> lk(g_tsv_mu);
    if (!t || !g_tsv_live.erase(t)) return;
  }
  delete t->t;
  delete t;
}

// ---- a text as BGZF members, the read dumps (cfr_gz_core.hpp) ----
void cfr_gz_options_default(cfr_gz_options *o) { if (o) memset(o, 0, sizeof(*o)); }

cfr_status cfr_gz_open(int device, const cfr_gz_options *o, cfr_gz **out) {
  if (!out) return bad_arg("cfr_gz_open: null argument");
  *out = nullptr;
  if (device < -1) return bad_arg("cfr_gz_open: device is a HIP ordinal, or -1 for the host twin");
  cfr_gz_options opt{};
  if (o) opt = *o;
  return guarded([&]() -> cfr_status {
    (void)cfr::gz_block_bytes(opt);
    (void)cfr::gz_dynamic(opt);
    std::unique_ptr<cfr_gz> h(new cfr_gz{nullptr});
    h->g = device < 0 ? cfr::make_gz_host(opt) : cfr::make_gz_device(device, opt);
    { std::lock_guard<std::mutex> lk(g_gz_mu); g_gz_live.insert(h.get()); }
    *out = h.release();
    return CFR_OK;
  });
}

cfr_status cfr_gz_compress(cfr_gz *h, const void *text, uint64_t n, const uint8_t **out, uint64_t *out_n) {
  if (!gz_live(h)) return bad_arg("cfr_gz_compress: not an open cfr_gz handle");
  return guarded([&]() -> cfr_status { h->g->compress((const uint8_t *)text, n, out, out_n); return CFR_OK; });
}

cfr_status cfr_gz_dump(cfr_gz *h, const char *id_bytes, const uint64_t *id_off, const uint8_t *select, size_t n, const cfr_gz_file *files, int n_files,
                       const uint8_t **out, uint64_t *out_n) {
  if (!gz_live(h)) return bad_arg("cfr_gz_dump: not an open cfr_gz handle");
  return guarded([&]() -> cfr_status { h->g->dump(id_bytes, id_off, select, n, files, n_files, out, out_n); return CFR_OK; });
}

void cfr_gz_eof(const uint8_t **bytes, size_t *n) {
  static const uint8_t eof[cfr::kGzEofBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (bytes) *bytes = eof;
  if (n) *n = sizeof(eof);
}

cfr_status cfr_gz_get_stats(cfr_gz *h, cfr_gz_stats *st) {
  if (!gz_live(h)) return bad_arg("cfr_gz_get_stats: not an open cfr_gz handle");
  if (!st) return bad_arg("cfr_gz_get_stats: null argument");
  h->g->stats(st);
  return CFR_OK;
}

void cfr_gz_close(cfr_gz *h) {
  {
    std::lock_guard<std::mutex> lk(g_gz_mu);
    if (!h || !g_gz_live.erase(h)) return;
  }
  delete h->g;
  delete h;
}

// ---- BGZF members back into text (cfr_inflate_core.hpp) ----
cfr_status cfr_inflate_open(int device, cfr_inflate **out) {
  if (!out) return bad_arg("cfr_inflate_open: null argument");
  *out = nullptr;
  if (device < -1) return bad_arg("cfr_inflate_open: device is a HIP ordinal, or -1 for the host twin");
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_inflate> h(new cfr_inflate{nullptr});
    h->i = device < 0 ? cfr::make_inflate_host() : cfr::make_inflate_device(device);
    { std::lock_guard<std::mutex> lk(g_inflate_mu); g_inflate_live.insert(h.get()); }
    *out = h.release();
    return CFR_OK;
  });
}

cfr_status cfr_inflate_bgzf(cfr_inflate *h, const uint8_t *members, uint64_t n, int fetch_text, const uint8_t **text, uint64_t *text_n, cfr_inflate_info *info) {
  if (!inflate_live(h)) return bad_arg("cfr_inflate_bgzf: not an open cfr_inflate handle");
  return guarded([&]() -> cfr_status { h->i->inflate(members, n, fetch_text, text, text_n, info); return CFR_OK; });
}

cfr_status cfr_inflate_member_status(cfr_inflate *h, uint8_t *status, uint64_t *text_off, uint64_t cap) {
  if (!inflate_live(h)) return bad_arg("cfr_inflate_member_status: not an open cfr_inflate handle");
  if (h->i->member_status(status, text_off, cap)) return CFR_OK;
  g_err = "cfr_inflate_member_status: the last call had more than " + std::to_string(cap) + " members";
  return CFR_ERR_CAPACITY;
}

cfr_status cfr_inflate_device_text(cfr_inflate *h, const void **d_text, uint64_t *n) {
  if (!inflate_live(h)) return bad_arg("cfr_inflate_device_text: not an open cfr_inflate handle");
  if (!h->i->device_text(d_text, n)) return bad_arg("cfr_inflate_device_text: the handle is the host twin (opened with device -1)");
  return CFR_OK;
}

cfr_status cfr_inflate_get_stats(cfr_inflate *h, cfr_inflate_stats *st) {
  if (!inflate_live(h)) return bad_arg("cfr_inflate_get_stats: not an open cfr_inflate handle");
  if (!st) return bad_arg("cfr_inflate_get_stats: null argument");
  h->i->stats(st);
  return CFR_OK;
}

void cfr_inflate_close(cfr_inflate *h) {
  {
    std::lock_guard<std::mutex> lk(g_inflate_mu);
    if (!h || !g_inflate_live.erase(h)) return;
  }
  delete h->i;
  delete h;
}

cfr_status cfr_tokenize_resident(cfr_tokenizer *t, const void *d_text, uint64_t len, int final, uint64_t max_records, cfr_token_info *info) {
  if (!tokenizer_live(t)) return bad_arg("cfr_tokenize_resident: not an open cfr_tokenizer handle");
  if (!info || (len && !d_text)) return bad_arg("cfr_tokenize_resident: null argument");
  if (len >> 32) return bad_arg("cfr_tokenize_resident: len must be below 2^32 (offsets inside a call are 32 bits wide on the device): hand the text over in pieces");
  return guarded([&]() -> cfr_status {
    if (t->t->tokenize_resident(d_text, len, final, max_records, info)) return CFR_OK;
    g_err = "cfr_tokenize_resident: the handle is the host twin (opened with device -1)";
    return CFR_ERR_ARG;
  });
}

cfr_status cfr_tokenizer_fetch_ids(cfr_tokenizer *t, char *ids, uint64_t ids_cap, uint64_t *id_off) {
  if (!tokenizer_live(t)) return bad_arg("cfr_tokenizer_fetch_ids: not an open cfr_tokenizer handle");
  return guarded([&]() -> cfr_status {
    uint64_t need = 0;
    if (t->t->fetch_ids(ids, ids_cap, id_off, &need)) return CFR_OK;
    g_err = "cfr_tokenizer_fetch_ids: the ids take " + std::to_string(need) + " bytes, the buffer holds " + std::to_string(ids_cap);
    return CFR_ERR_CAPACITY;
  });
}

cfr_status cfr_device_index_set_tsv(cfr_dev_index *d, int on) {
  if (!d) return bad_arg("cfr_device_index_set_tsv: null argument");
  CFR_ENTER(d, "cfr_device_index_set_tsv");
  return guarded([&]() -> cfr_status { d->d->set_tsv(on != 0); return CFR_OK; });
}

static cfr_status tsv_last(cfr_dev_index *d, const char *what, const cfr::TsvIds &ids, bool host_ids, char *text, uint64_t cap, uint64_t *len, uint64_t *row_offsets) {
  if (!d || !len || (!text && cap)) return bad_arg("cfr_device_index_tsv_last: null argument");
  {
    std::lock_guard<std::mutex> lk(d->qmu);
    if (!d->live.empty()) return bad_arg("cfr_device_index_tsv_last: a batch is queued (cfr_classify_batch_submit): wait for it first, the rows are those of the last call");
  }
  BusyGuard busy_guard_(d);
  if (!busy_guard_.ok()) { g_err = std::string(what) + ": this cfr_dev_index is in use by another call (one call at a time per device image)"; return CFR_ERR_BUSY; }
  return guarded([&]() -> cfr_status {
    if (d->d->tsv_last(ids, host_ids, text, cap, len, row_offsets)) return CFR_OK;
    g_err = std::string(what) + ": the text takes " + std::to_string(*len) + " bytes, the buffer holds " + std::to_string(cap);
    return CFR_ERR_CAPACITY;
  });
}
cfr_status cfr_device_index_tsv_last(cfr_dev_index *d, const char *id_bytes, const uint64_t *id_offsets, char *text, uint64_t cap, uint64_t *len,
                                     uint64_t *row_offsets) {
  return tsv_last(d, "cfr_device_index_tsv_last", cfr::TsvIds{id_bytes, id_offsets, nullptr}, true, text, cap, len, row_offsets);
}
cfr_status cfr_device_index_tsv_last_resident(cfr_dev_index *d, const void *d_text, const void *d_records, char *text, uint64_t cap, uint64_t *len,
                                              uint64_t *row_offsets) {
  return tsv_last(d, "cfr_device_index_tsv_last_resident", cfr::TsvIds{(const char *)d_text, nullptr, (const cfr_read_record *)d_records}, false, text, cap, len,
                  row_offsets);
}
cfr_status cfr_last_tsv_ms(const cfr_dev_index *d, float *ms) {
  if (!d || !ms) return bad_arg("cfr_last_tsv_ms: null argument");
  *ms = d->d->last_tsv_ms;
  return CFR_OK;
}

// ---- single-cell input: read formats, barcode whitelist, barcode translation ----
cfr_status cfr_read_format_parse(const char *spec, cfr_read_format **out) {
  if (!spec || !out) return bad_arg("cfr_read_format_parse: null argument");
  *out = nullptr;
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_read_format> f(new cfr_read_format());
    if (!f->f.init(spec)) throw cfr::FormatError{std::string("Format description error in ") + spec};   // ReadFormatter.hpp:212
    *out = f.release();
    return CFR_OK;
  });
}

cfr_status cfr_read_format_info(const cfr_read_format *f, int category, int32_t *n_segments, int32_t *need_extract, int32_t *in_comment) {
  if (!f || category < 0 || category >= cfr::kFormatCategories) return bad_arg("cfr_read_format_info: bad argument");
  if (n_segments) *n_segments = f->f.segment_count(category);
  if (need_extract) *need_extract = f->f.need_extract(category) ? 1 : 0;
  if (in_comment) *in_comment = f->f.in_comment(category) ? 1 : 0;
  return CFR_OK;
}

cfr_status cfr_read_format_extract(const cfr_read_format *f, int category, int inplace, const uint8_t *bases, const uint64_t *offsets, const char *qual,
                                   const uint8_t *comments, const uint64_t *comment_offsets, size_t n, uint8_t *out_bases, uint64_t *out_offsets,
                                   char *out_qual) {
  if (!f || !out_offsets || category < 0 || category >= cfr::kFormatCategories) return bad_arg("cfr_read_format_extract: bad argument");
  const bool hd = f->f.in_comment(category);
  if (n && (hd ? (!comments || !comment_offsets) : (!bases || !offsets))) return bad_arg("cfr_read_format_extract: null argument");
  const uint8_t *src = hd ? comments : bases;
  const uint64_t *off = hd ? comment_offsets : offsets;
  for (size_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0x7fffffffull) return bad_arg("cfr_read_format_extract: offsets must not decrease, records stay below 2^31 bytes");
  return guarded([&]() -> cfr_status {
    std::string s, q;
    out_offsets[0] = 0;
    for (size_t i = 0; i < n; ++i) {
      const char *p = (const char *)src + off[i];
      const size_t len = (size_t)(off[i + 1] - off[i]);
      const bool with_qual = !hd && qual && out_qual && out_bases;
      if (hd || !inplace) {                                  // Extract(.., needComplement = true, .., bufferId 0) (CentrifugerClass.cpp:182, BarcodeCorrector.hpp:156)
        f->f.extract(p, len, category, true, s);
        if (with_qual) f->f.extract(qual + offsets[i], len, category, false, q);
      } else {                                               // InplaceExtractSeqAndQual (ReadFormatter.hpp:408-422)
        s.assign(p, len);
        f->f.extract_inplace(s, category, true);
        if (with_qual) { q.assign(qual + offsets[i], len); f->f.extract_inplace(q, category, false); }
      }
      if (out_bases) {
        memcpy(out_bases + out_offsets[i], s.data(), s.size());
        if (with_qual) memcpy(out_qual + out_offsets[i], q.data(), std::min(q.size(), s.size()));
      }
      out_offsets[i + 1] = out_offsets[i] + s.size();
    }
    return CFR_OK;
  });
}

void cfr_read_format_destroy(cfr_read_format *f) { delete f; }

cfr_status cfr_barcode_open(const char *whitelist_path, int device, cfr_barcode **out) {
  if (!whitelist_path || !out) return bad_arg("cfr_barcode_open: null argument");
  *out = nullptr;
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_barcode> b(new cfr_barcode{nullptr});
    b->b = new cfr::Barcode(whitelist_path, device);
    *out = b.release();
    return CFR_OK;
  });
}

static cfr_status barcode_args(const char *who, const cfr_barcode *bc, const uint8_t *bases, const uint64_t *offsets, size_t n) {
  if (!bc || (n && (!bases || !offsets))) { g_err = std::string(who) + ": null argument"; return CFR_ERR_ARG; }
  for (size_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) { g_err = std::string(who) + ": offsets must not decrease"; return CFR_ERR_ARG; }
    if (offsets[i + 1] - offsets[i] > cfr::kBarcodeMaxLen) { g_err = std::string(who) + ": a barcode of 256 bytes or more (BarcodeCorrector's buffer holds 255)"; return CFR_ERR_ARG; }
  }
  return CFR_OK;
}

cfr_status cfr_barcode_count(cfr_barcode *bc, const uint8_t *bases, const uint64_t *offsets, size_t n, size_t max_records) {
  if (n > max_records) n = max_records;
  if (cfr_status st = barcode_args("cfr_barcode_count", bc, bases, offsets, n)) return st;
  return guarded([&]() -> cfr_status { bc->b->count(bases, offsets, n, max_records); return CFR_OK; });
}

static cfr_status barcode_correct(const char *who, cfr_barcode *bc, const uint8_t *bases, const uint64_t *offsets, const char *qual, size_t n, int threads,
                                  int8_t *status, uint8_t *out_bases, bool host_only) {
  if (cfr_status st = barcode_args(who, bc, bases, offsets, n)) return st;
  if (n && (!status || !out_bases)) { g_err = std::string(who) + ": null argument"; return CFR_ERR_ARG; }
  return guarded([&]() -> cfr_status { bc->b->correct(bases, offsets, (const int8_t *)qual, n, threads, status, out_bases, host_only); return CFR_OK; });
}

cfr_status cfr_barcode_correct(cfr_barcode *bc, const uint8_t *bases, const uint64_t *offsets, const char *qual, size_t n, int threads, int8_t *status,
                               uint8_t *out_bases) {
  return barcode_correct("cfr_barcode_correct", bc, bases, offsets, qual, n, threads, status, out_bases, false);
}

cfr_status cfr_barcode_correct_host(cfr_barcode *bc, const uint8_t *bases, const uint64_t *offsets, const char *qual, size_t n, int threads, int8_t *status,
                                    uint8_t *out_bases) {
  return barcode_correct("cfr_barcode_correct_host", bc, bases, offsets, qual, n, threads, status, out_bases, true);
}

cfr_status cfr_barcode_counts(cfr_barcode *bc, size_t *n_entries, const uint8_t **bases, const uint64_t **offsets, const uint32_t **counts) {
  if (!bc || !n_entries || !bases || !offsets || !counts) return bad_arg("cfr_barcode_counts: null argument");
  return guarded([&]() -> cfr_status { bc->b->counts(bases, offsets, counts, n_entries); return CFR_OK; });
}

cfr_status cfr_barcode_get_stats(const cfr_barcode *bc, cfr_barcode_stats *st) {
  if (!bc || !st) return bad_arg("cfr_barcode_get_stats: null argument");
  memset(st, 0, sizeof(*st));
  st->whitelist_size = bc->b->whitelist().size();
  st->table_slots = bc->b->table_slots();
  st->host_barcodes = bc->b->host_barcodes;
  st->host_barcodes_total = bc->b->host_barcodes_total;
  st->device_ms = bc->b->device_ms;
  st->barcode_length = bc->b->whitelist().common_length();
  st->on_device = bc->b->on_device() ? 1 : 0;
  return CFR_OK;
}

void cfr_barcode_destroy(cfr_barcode *bc) {
  if (!bc) return;
  delete bc->b;
  delete bc;
}

cfr_status cfr_barcode_translate_open(const char *path, cfr_barcode_translate **out) {
  if (!path || !out) return bad_arg("cfr_barcode_translate_open: null argument");
  *out = nullptr;
  return guarded([&]() -> cfr_status {
    std::unique_ptr<cfr_barcode_translate> t(new cfr_barcode_translate{nullptr});
    t->t = new cfr::BarcodeTranslate(path);
    *out = t.release();
    return CFR_OK;
  });
}

cfr_status cfr_barcode_translate_apply(const cfr_barcode_translate *t, const uint8_t *bases, const uint64_t *offsets, const int8_t *status, size_t n,
                                       uint8_t *out_bases, uint64_t *out_offsets) {
  if (!t || !out_offsets || (n && (!bases || !offsets))) return bad_arg("cfr_barcode_translate_apply: null argument");
  for (size_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return bad_arg("cfr_barcode_translate_apply: offsets must not decrease");
  return guarded([&]() -> cfr_status {
    std::string s, missing;
    out_offsets[0] = 0;
    for (size_t i = 0; i < n; ++i) {
      if (status && status[i] == -1) s = "N";                 // CentrifugerClass.cpp:201-205
      else if (!t->t->translate(bases + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), s, missing))
        throw cfr::FormatError{"Barcode " + missing + " does not exist in the translation table."};   // BarcodeTranslator.hpp:70
      if (out_bases) memcpy(out_bases + out_offsets[i], s.data(), s.size());
      out_offsets[i + 1] = out_offsets[i] + s.size();
    }
    return CFR_OK;
  });
}

void cfr_barcode_translate_destroy(cfr_barcode_translate *t) {
  if (!t) return;
  delete t->t;
  delete t;
}

// ---- --merge-readpair ----
static cfr_status merge_args(const char *who, const void *bases1, const void *offsets1, const void *qual1, const void *bases2, const void *offsets2,
                             const void *qual2, size_t n) {
  if (n && (!bases1 || !offsets1)) { g_err = std::string(who) + ": null argument"; return CFR_ERR_ARG; }
  if ((bases2 == nullptr) != (offsets2 == nullptr)) { g_err = std::string(who) + ": bases2/offsets2 must both be given"; return CFR_ERR_ARG; }
  if (bases2 && (qual1 == nullptr) != (qual2 == nullptr)) {
    g_err = std::string(who) + ": qualities for both mates or for neither (ReadPairMerger::Merge reads both once one is given)";
    return CFR_ERR_ARG;
  }
  return CFR_OK;
}

cfr_status cfr_merge_pairs(const uint8_t *bases1, const uint64_t *offsets1, const char *qual1, const uint8_t *bases2, const uint64_t *offsets2,
                           const char *qual2, size_t n, int threads, uint8_t *out_bases1, uint64_t *out_offsets1, char *out_qual1,
                           uint8_t *out_bases2, uint64_t *out_offsets2, char *out_qual2, int32_t *kind, int32_t *overlap, int32_t *offset) {
  if (!out_offsets1 || !out_offsets2 || (n && (!bases2 || !out_bases1 || !out_bases2))) return bad_arg("cfr_merge_pairs: null argument");
  if (cfr_status st = merge_args("cfr_merge_pairs", bases1, offsets1, qual1, bases2, offsets2, qual2, n)) return st;
  for (size_t i = 0; i < n; ++i)
    if (offsets1[i + 1] - offsets1[i] > 0x7fffffffull || offsets2[i + 1] - offsets2[i] > 0x7fffffffull) return bad_arg("cfr_merge_pairs: a mate of 2^31 bases or more");
  if (threads < 1) threads = 1;
  if ((size_t)threads > n) threads = n ? (int)n : 1;
  // a contiguous slice of pairs per thread: the merged reads of a slice are kept in the thread's buffer until the new offsets are known
  std::vector<int32_t> kd(n, 0);
  std::vector<uint64_t> at(n, 0);
  std::vector<std::vector<uint8_t>> mb((size_t)threads);
  std::vector<std::vector<int8_t>> mq((size_t)threads);
  cfr::parallel_slices(n, threads, [&](size_t lo, size_t hi, int tid) {
    cfr::MergeScratch ws;
    std::vector<uint8_t> rm;
    std::vector<int8_t> qm;
    for (size_t i = lo; i < hi; ++i) {
      const uint64_t a1 = offsets1[i], a2 = offsets2[i];
      const int l1 = (int)(offsets1[i + 1] - a1), l2 = (int)(offsets2[i + 1] - a2);
      rm.resize((size_t)l1 + (size_t)l2 + 1);
      if (qual1) qm.resize((size_t)l1 + (size_t)l2 + 1);
      int mlen = 0, ov = -1, off = -1;
      const int k = cfr::merge_pair(bases1 + a1, qual1 ? (const int8_t *)qual1 + a1 : nullptr, l1, bases2 + a2, qual2 ? (const int8_t *)qual2 + a2 : nullptr, l2,
                                    rm.data(), qual1 ? qm.data() : nullptr, &mlen, &ov, &off, ws);
      kd[i] = k;
      if (kind) kind[i] = k;
      if (overlap) overlap[i] = ov;
      if (offset) offset[i] = off;
      out_offsets1[i + 1] = k ? (uint64_t)mlen : (uint64_t)l1;       // lengths for now
      out_offsets2[i + 1] = k ? 0 : (uint64_t)l2;
      if (k) {
        at[i] = mb[tid].size();
        mb[tid].insert(mb[tid].end(), rm.begin(), rm.begin() + mlen);
        if (qual1) mq[tid].insert(mq[tid].end(), qm.begin(), qm.begin() + mlen);
      }
    }
  });
  out_offsets1[0] = out_offsets2[0] = 0;
  for (size_t i = 0; i < n; ++i) { out_offsets1[i + 1] += out_offsets1[i]; out_offsets2[i + 1] += out_offsets2[i]; }
  cfr::parallel_slices(n, threads, [&](size_t lo, size_t hi, int tid) {
    for (size_t i = lo; i < hi; ++i) {
      const uint64_t d1 = out_offsets1[i], m1 = out_offsets1[i + 1] - d1, d2 = out_offsets2[i], m2 = out_offsets2[i + 1] - d2;
      if (kd[i]) {
        if (m1) memcpy(out_bases1 + d1, mb[tid].data() + at[i], m1);
        if (m1 && qual1 && out_qual1) memcpy(out_qual1 + d1, mq[tid].data() + at[i], m1);
      } else {
        if (m1) memcpy(out_bases1 + d1, bases1 + offsets1[i], m1);
        if (m2) memcpy(out_bases2 + d2, bases2 + offsets2[i], m2);
        if (qual1 && out_qual1 && m1) memcpy(out_qual1 + d1, qual1 + offsets1[i], m1);
        if (qual2 && out_qual2 && m2) memcpy(out_qual2 + d2, qual2 + offsets2[i], m2);
      }
    }
  });
  return CFR_OK;
}

cfr_status cfr_merge_pairs_device(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1, const char *qual1, const uint8_t *bases2,
                                  const uint64_t *offsets2, const char *qual2, size_t n, uint8_t *out_bases1, uint64_t *out_offsets1,
                                  char *out_qual1, uint8_t *out_bases2, uint64_t *out_offsets2, char *out_qual2, int32_t *kind, int32_t *overlap,
                                  int32_t *offset) {
  if (!d || !out_offsets1 || !out_offsets2 || (n && (!bases2 || !out_bases1 || !out_bases2))) return bad_arg("cfr_merge_pairs_device: null argument");
  if (cfr_status st = merge_args("cfr_merge_pairs_device", bases1, offsets1, qual1, bases2, offsets2, qual2, n)) return st;
  for (size_t i = 0; i < n; ++i)
    if (offsets1[i + 1] - offsets1[i] > 0x7fffffffull || offsets2[i + 1] - offsets2[i] > 0x7fffffffull) return bad_arg("cfr_merge_pairs_device: a mate of 2^31 bases or more");
  CFR_ENTER(d, "cfr_merge_pairs_device");
  return guarded([&]() -> cfr_status {
    d->d->merge_pairs_host(bases1, offsets1, (const int8_t *)qual1, bases2, offsets2, (const int8_t *)qual2, n, out_bases1, out_offsets1,
                           (int8_t *)(qual1 ? out_qual1 : nullptr), out_bases2, out_offsets2, (int8_t *)(qual1 ? out_qual2 : nullptr), kind, overlap, offset);
    return CFR_OK;
  });
}

cfr_status cfr_device_index_set_merge(cfr_dev_index *d, int on) {
  if (!d) return bad_arg("cfr_device_index_set_merge: null argument");
  if (d->d->host().prot.enabled) return bad_arg("cfr_device_index_set_merge: a protein index searches the mates translated; a merged pair's empty mate is not covered there");
  CFR_ENTER(d, "cfr_device_index_set_merge");
  d->d->set_merge(on != 0);
  return CFR_OK;
}

cfr_status cfr_classify_batch_merged(cfr_dev_index *d, const uint8_t *bases1, const uint64_t *offsets1, const char *qual1, const uint8_t *bases2,
                                     const uint64_t *offsets2, const char *qual2, size_t n, cfr_result *results, cfr_match *matches,
                                     size_t match_cap, size_t *n_matches, int32_t *merge_kind) {
  if (!d || (n && !results)) return bad_arg("cfr_classify_batch_merged: null argument");
  if (cfr_status st = merge_args("cfr_classify_batch_merged", bases1, offsets1, qual1, bases2, offsets2, qual2, n)) return st;
  CFR_ENTER(d, "cfr_classify_batch_merged");
  return guarded([&]() -> cfr_status {
    d->d->classify_host_merged(bases1, offsets1, (const int8_t *)qual1, bases2, offsets2, (const int8_t *)qual2, n, results, matches, match_cap,
                               n_matches, merge_kind);
    return CFR_OK;
  });
}

cfr_status cfr_classify_batch_resident_merged(cfr_dev_index *d, const void *d_bases1, const void *d_offsets1, const void *d_qual1,
                                              const void *d_bases2, const void *d_offsets2, const void *d_qual2, size_t n,
                                              uint64_t total_bases1, uint64_t total_bases2, cfr_result *results, cfr_match *matches,
                                              size_t match_cap, size_t *n_matches, int32_t *merge_kind) {
  if (!d || (n && !results)) return bad_arg("cfr_classify_batch_resident_merged: null argument");
  if (cfr_status st = merge_args("cfr_classify_batch_resident_merged", d_bases1, d_offsets1, d_qual1, d_bases2, d_offsets2, d_qual2, n)) return st;
  CFR_ENTER(d, "cfr_classify_batch_resident_merged");
  return guarded([&]() -> cfr_status {
    d->d->classify_device_merged((const uint8_t *)d_bases1, (const uint64_t *)d_offsets1, (const int8_t *)d_qual1, (const uint8_t *)d_bases2,
                                 (const uint64_t *)d_offsets2, (const int8_t *)d_qual2, n, total_bases1, total_bases2, results, matches, match_cap,
                                 n_matches, merge_kind);
    return CFR_OK;
  });
}

cfr_status cfr_last_merge_ms(const cfr_dev_index *d, float *ms) {
  if (!d || !ms) return bad_arg("cfr_last_merge_ms: null argument");
  *ms = d->d->last_merge_ms;
  return CFR_OK;
}

const char *cfr_tsv_header(void) {   // ResultWriter::OutputHeader (ResultWriter.hpp:186-197), no barcode/UMI columns
  return "readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\n";
}

const char *cfr_tsv_header_expanded(void) {   // ... with _outputExpandedTaxIds (ResultWriter.hpp:194-195)
  return "readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\texpandedTaxIDs\n";
}

const char *cfr_tsv_header_ex(int has_barcode, int has_umi, int expanded) {   // ... with _hasBarcode / _hasUmi (ResultWriter.hpp:190-193)
#define CFR_TSV_HEAD "readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches"
  static const char *const kHeader[8] = {CFR_TSV_HEAD "\n", CFR_TSV_HEAD "\tbarcode\n", CFR_TSV_HEAD "\tUMI\n", CFR_TSV_HEAD "\tbarcode\tUMI\n",
                                         CFR_TSV_HEAD "\texpandedTaxIDs\n", CFR_TSV_HEAD "\tbarcode\texpandedTaxIDs\n", CFR_TSV_HEAD "\tUMI\texpandedTaxIDs\n",
                                         CFR_TSV_HEAD "\tbarcode\tUMI\texpandedTaxIDs\n"};
#undef CFR_TSV_HEAD
  return kHeader[(has_barcode ? 1 : 0) | (has_umi ? 2 : 0) | (expanded ? 4 : 0)];
}

// the barcode / UMI columns of one row: absent, or PrintExtraCol(s) (ResultWriter.hpp:32-38: a bare tab for a null string)
struct ExtraCols { bool has_barcode = false, has_umi = false; const char *barcode = nullptr, *umi = nullptr; };
static size_t format_tsv(const cfr_index *idx, const char *read_id, const cfr_result *r, const cfr_match *matches, const ExtraCols &x, bool expanded,
                         const cfr_span *spans, const uint64_t *ids, char *buf, size_t cap);
size_t cfr_format_tsv(const cfr_index *idx, const char *read_id, const cfr_result *r, const cfr_match *matches, char *buf, size_t cap) {
  return format_tsv(idx, read_id, r, matches, ExtraCols(), false, nullptr, nullptr, buf, cap);
}
size_t cfr_format_tsv_expanded(const cfr_index *idx, const char *read_id, const cfr_result *r, const cfr_match *matches, const cfr_span *spans,
                               const uint64_t *ids, char *buf, size_t cap) {
  return format_tsv(idx, read_id, r, matches, ExtraCols(), true, spans, ids, buf, cap);
}
size_t cfr_format_tsv_ex(const cfr_index *idx, const char *read_id, const cfr_result *r, const cfr_match *matches, int has_barcode, const char *barcode,
                         int has_umi, const char *umi, int expanded, const cfr_span *spans, const uint64_t *ids, char *buf, size_t cap) {
  ExtraCols x;
  x.has_barcode = has_barcode != 0; x.has_umi = has_umi != 0; x.barcode = barcode; x.umi = umi;
  return format_tsv(idx, read_id, r, matches, x, expanded != 0, spans, ids, buf, cap);
}

static size_t format_tsv(const cfr_index *idx, const char *read_id, const cfr_result *r, const cfr_match *matches, const ExtraCols &x, bool expanded,
                         const cfr_span *spans, const uint64_t *ids, char *buf, size_t cap) {
  // ResultWriter::Output (ResultWriter.hpp:209-240): "%s\t%s\t%lu\t%lu\t%lu\t%d\t%d\t%d" + PrintExtraCol(expandedTaxIdStrings[i]) / PrintExtraCol("")
  // (:226-227, :239-240) - the same bytes, put together by hand: at a hundred million rows per run snprintf's format parsing was the
  // command line's slowest stage (profiles/r5_cli_timing_100m.txt)
  struct Out {
    char *buf; size_t cap, off;
    void put(const char *p, size_t n) { if (buf && off < cap) memcpy(buf + off, p, n < cap - off ? n : cap - off); off += n; }
    void ch(char c) { if (buf && off < cap) buf[off] = c; ++off; }
    void u64(uint64_t v) { char t[24]; int k = 24; do { t[--k] = (char)('0' + v % 10); v /= 10; } while (v); put(t + k, (size_t)(24 - k)); }
    void i32(int32_t v) { if (v < 0) { ch('-'); u64((uint64_t)(-(int64_t)v)); } else u64((uint64_t)v); }
    void extra(const ExtraCols &x) {
      if (x.has_barcode) { ch('\t'); if (x.barcode) put(x.barcode, strlen(x.barcode)); }
      if (x.has_umi) { ch('\t'); if (x.umi) put(x.umi, strlen(x.umi)); }
    }
  } o{buf, cap, 0};
  const cfr::Taxonomy &t = idx->h->tax;
  const size_t idn = strlen(read_id);
  if (r->n_match > 0) {
    for (int i = 0; i < r->n_match; ++i) {
      const cfr_match &m = matches[r->match_begin + (uint64_t)i];
      const char *name;
      if (m.kind == 0) name = m.id < t.seq_name.size() ? t.seq_name[m.id].c_str() : "";
      else name = cfr::tax_rank_string(m.id < t.node_cnt ? t.rank[m.id] : 0);
      o.put(read_id, idn); o.ch('\t'); o.put(name, strlen(name)); o.ch('\t'); o.u64(m.taxid); o.ch('\t'); o.u64(r->score); o.ch('\t');
      o.u64(r->secondary_score); o.ch('\t'); o.i32(r->hit_length); o.ch('\t'); o.i32(r->query_length); o.ch('\t'); o.i32(r->n_match);
      o.extra(x);
      if (expanded) {
        o.ch('\t');
        const cfr_span sp = spans ? spans[r->match_begin + (uint64_t)i] : cfr_span{0, 0};
        for (uint64_t j = 0; j < sp.count; ++j) { if (j) o.ch(','); o.u64(ids[sp.begin + j]); }
      }
      o.ch('\n');
    }
  } else {
    o.put(read_id, idn); { static const char kUn[] = "\tunclassified\t0\t0\t0\t0\t"; o.put(kUn, sizeof(kUn) - 1); } o.i32(r->query_length); o.put("\t1", 2);
    o.extra(x);
    if (expanded) o.ch('\t');
    o.ch('\n');
  }
  if (buf && cap) buf[o.off < cap ? o.off : cap - 1] = '\0';      // always a C string: a truncated call (return value >= cap: retry with that much + 1) ends at cap - 1
  return o.off;
}

}  // extern "C"
