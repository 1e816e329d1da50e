// cfr_barcode.cpp — host twins of ReadFormatter, BarcodeCorrector and BarcodeTranslator (see cfr_barcode.hpp for what is restated and
// for the few places where the reference's behaviour is undefined), and the handle that chooses between the twin and the device table.
#include "cfr_barcode.hpp"
#include "cfr_threads.hpp"

#include <zlib.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>

namespace cfr {

// ---- ReadFormatter ----

// ParseFormatStringAndAppendEffectiveRange (ReadFormatter.hpp:49-139).  avail: bytes of the whole string from s on (the reference
// looks at s[2] whatever len is; past the terminator that is out of bounds, here it is "not a colon")
bool ReadFormat::parse_segment(const char *s, int len, int avail) {
  int i;
  int j = 0;   // start, end, strand section
  char buffer[20];
  int blen = 0;
  int start;
  Seg seg;
  if (avail < 3 || s[2] != ':') return false;
  int category = 0;
  if (s[0] == 'r' && s[1] == '1') category = kFormatRead1;
  else if (s[0] == 'r' && s[1] == '2') category = kFormatRead2;
  else if (s[0] == 'b' && s[1] == 'c') category = kFormatBarcode;
  else if (s[0] == 'u' && s[1] == 'm') category = kFormatUmi;
  else return false;

  start = 3;
  seg.in_comment = false;
  if (len >= 6 && s[3] == 'h' && s[4] == 'd' && s[5] == ':') {   // bc:hd:FIELD:... / bc:hd:PREFIX:...
    seg.in_comment = true;
    blen = 0;
    start = 6;
    for (i = start; i <= len; ++i) {
      if (i == len || s[i] == ':') {
        buffer[blen] = '\0';
        int l;
        for (l = 0; l < blen; ++l)
          if (buffer[l] < '0' || buffer[l] > '9') break;
        if (l == blen) { seg.field = atoi(buffer); seg.prefix.clear(); }
        else { seg.field = -1; seg.prefix = buffer; }
        break;
      }
      if (blen >= 19) return false;
      buffer[blen] = s[i];
      ++blen;
    }
    start = i + 1;
  }

  seg.strand = 1;
  blen = 0;
  for (i = start; i <= len; ++i) {
    if (i == len || s[i] == ':') {
      buffer[blen] = '\0';
      if (j == 0) seg.start = atoi(buffer);
      else if (j == 1) seg.end = atoi(buffer);
      else seg.strand = (buffer[0] == '+' ? 1 : -1);
      blen = 0;
      if (i < len && s[i] == ':') ++j;
    } else {
      if (blen >= 19) return false;
      buffer[blen] = s[i];
      ++blen;
    }
  }
  if (j >= 3 || j < 1) return false;
  segs_[category].push_back(seg);
  return true;
}

bool ReadFormat::init(const char *spec) {   // Init (:202-228)
  const int total = (int)strlen(spec);
  int i, j;
  for (i = 0; spec[i];) {
    for (j = i; spec[j] && spec[j] != ';' && spec[j] != ','; ++j) {}
    if (!parse_segment(spec + i, j - i, total - i)) return false;
    if (spec[j]) i = j + 1;
    else i = j;
  }
  for (int c = 0; c < kFormatCategories; ++c) {   // AreSegmentsSorted (:141-149): the numbers as they were written
    sorted_[c] = true;
    for (size_t k = 1; k < segs_[c].size(); ++k)
      if (segs_[c][k].start <= segs_[c][k - 1].end) sorted_[c] = false;
  }
  return true;
}

int ReadFormat::segment_count(int category) const {
  if (category == kFormatCategories) {
    int ret = 0;
    for (int i = 0; i < kFormatCategories; ++i) ret += (int)segs_[i].size();
    return ret;
  }
  return (int)segs_[category].size();
}

bool ReadFormat::need_extract(int category) const {
  const std::vector<Seg> &s = segs_[category];
  if (s.empty()) return false;
  if (s.size() == 1 && s[0].start == 0 && s[0].end == -1 && s[0].strand == 1 && !s[0].in_comment) return false;
  return true;
}

namespace {
inline char comp_char(uint8_t c) {   // _compChar (:172-177)
  switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return 'N'; }
}
}  // namespace

// the body of Extract (:316-404).  seq == nullptr: in place, the bytes are read from and written to `out` (which holds the sequence);
// otherwise they are read from seq and `out` starts empty
void ReadFormat::run(const char *seq, int len, int category, bool need_complement, std::string *out) const {
  const std::vector<Seg> &seg = segs_[category];
  const bool inplace = seq == nullptr;
  auto at = [&](int p) -> char { return p >= len ? '\0' : (inplace ? (*out)[(size_t)p] : seq[p]); };
  int i = 0, j, k;
  int strand = 1;
  for (k = 0; k < (int)seg.size(); ++k) {
    int start = seg[k].start;
    int end = seg[k].end;
    int lenk = len;
    if (in_comment(category)) {
      int f = 0;
      int fstart = 0, fend = 0;
      if (seg[k].field >= 0) {
        for (j = 0; j <= len; ++j) {
          const char c = at(j);
          if (c == ' ' || c == '\t' || c == '\0') {
            ++f;
            if (f == seg[k].field) fstart = j + 1;
            else if (f == seg[k].field + 1) { fend = j - 1; break; }
          }
        }
        if (f <= seg[k].field) { fstart = len; fend = len - 1; }   // field is not found
      } else {
        const std::string &pre = seg[k].prefix;
        int p = -1;
        for (int a = 0; a + (int)pre.size() <= len && p < 0; ++a) {   // strstr
          size_t b = 0;
          while (b < pre.size() && at(a + (int)b) == pre[b]) ++b;
          if (b == pre.size()) p = a;
        }
        if (p >= 0) {
          fstart = p;
          for (; at(p) != ' ' && at(p) != '\t' && at(p) != '\0'; ++p) {}
          fend = p - 1;
        } else { fstart = len; fend = len - 1; }
      }
      if (start >= 0) start += fstart;
      if (end >= 0) end += fstart;
      lenk = fend + 1;
    }
    if (start < 0) start = lenk + start;
    if (end >= lenk) end = lenk - 1;
    else if (end < 0) end = lenk + end;
    for (j = start; j <= end; ++j) {
      if (j < 0) continue;                       // in front of the string: see the header
      const char c = at(j);
      if ((size_t)i < out->size()) (*out)[(size_t)i] = c;
      else out->push_back(c);
      ++i;
    }
    if (seg[k].strand == -1) strand = -1;
  }
  out->resize((size_t)i);
  if (strand == -1) {
    std::reverse(out->begin(), out->end());
    if (need_complement)
      for (char &c : *out) c = comp_char((uint8_t)c);
  }
}

void ReadFormat::extract(const char *seq, size_t len, int category, bool need_complement, std::string &out) const {
  static const char kEmpty[1] = {0};
  if (!seq) { seq = kEmpty; len = 0; }
  if (!need_extract(category)) { out.assign(seq, len); return; }
  out.clear();
  run(seq, (int)len, category, need_complement, &out);
}

void ReadFormat::extract_inplace(std::string &seq, int category, bool need_complement) const {
  if (!need_extract(category)) return;
  if (sorted_[category]) {
    run(nullptr, (int)seq.size(), category, need_complement, &seq);
  } else {
    std::string out;
    run(seq.data(), (int)seq.size(), category, need_complement, &out);
    seq.swap(out);
  }
}

// ---- Trie / BarcodeCorrector ----

namespace {
inline int nuc_code(uint8_t c) {   // Trie::nucToNum (BarcodeCorrector.hpp:51-55)
  switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}
}  // namespace

BarcodeWhitelist::BarcodeWhitelist(const std::string &path) {
  nodes_.emplace_back();
  char buffer[256];
  gzFile fp = gzopen(path.c_str(), "r");
  if (!fp) throw IoError{"cannot open the barcode whitelist " + path};
  while (gzgets(fp, buffer, sizeof(buffer)) != NULL) {
    int len = (int)strlen(buffer);
    if (len > 0 && buffer[len - 1] == '\n') {
      buffer[len - 1] = '\0';
      --len;
    }
    insert(buffer, 1);
  }
  gzclose(fp);
}

void BarcodeWhitelist::insert(const char *s, int weight) {   // Trie::Insert (:68-92)
  int i;
  for (i = 0; s[i]; ++i)
    if (nuc_code((uint8_t)s[i]) == -1) return;
  uint32_t p = 0;
  for (i = 0; s[i]; ++i) {
    const int tag = nuc_code((uint8_t)s[i]);
    if (nodes_[p].next[tag] == 0) {
      const uint32_t nn = (uint32_t)nodes_.size();
      nodes_.emplace_back();
      nodes_[p].next[tag] = nn;
    }
    p = nodes_[p].next[tag];
  }
  if (!nodes_[p].end) ++n_entries_;
  if (len_seen_ < 0) len_seen_ = i;
  else if (len_seen_ != i) mixed_ = true;
  nodes_[p].end = true;
  nodes_[p].count += weight;
}

int BarcodeWhitelist::search(const uint8_t *s, size_t len) const {
  for (size_t i = 0; i < len; ++i)
    if (nuc_code(s[i]) == -1) return -1;
  uint32_t p = 0;
  for (size_t i = 0; i < len; ++i) {
    p = nodes_[p].next[nuc_code(s[i])];
    if (p == 0) return -1;
  }
  return nodes_[p].count;
}

int BarcodeWhitelist::search_update(const uint8_t *s, size_t len, int weight) {   // SearchAndUpdate (:94-111)
  for (size_t i = 0; i < len; ++i)
    if (nuc_code(s[i]) == -1) return -1;
  uint32_t p = 0;
  for (size_t i = 0; i < len; ++i) {
    p = nodes_[p].next[nuc_code(s[i])];
    if (p == 0) return -1;
  }
  nodes_[p].count += weight;
  return nodes_[p].count;
}

int BarcodeWhitelist::correct(uint8_t *barcode, size_t len, const int8_t *qual) const {   // Correct (:166-234)
  if (search(barcode, len) != -1) return 0;
  struct Triple { int a, b, c; };
  static const char testChr[5] = "ACGT";
  Triple records[4 * kBarcodeMaxLen];
  int recordCnt = 0;
  uint8_t buffer[kBarcodeMaxLen + 1];
  memcpy(buffer, barcode, len);
  for (int i = 0; i < (int)len; ++i) {
    for (int j = 0; j < 4; ++j) {
      if ((uint8_t)testChr[j] == barcode[i]) continue;
      buffer[i] = (uint8_t)testChr[j];
      const int cnt = search(buffer, len);
      buffer[i] = barcode[i];
      if (cnt != -1) records[recordCnt++] = Triple{i, j, cnt};
    }
  }
  int bestCnt = -1;
  int bestTag = -1;
  int bestLowQual = 255;   // the lowest quality score within the best candidates
  if (recordCnt == 0) return -1;
  for (int i = 0; i < recordCnt; ++i) {
    if (records[i].c > bestCnt) {
      bestCnt = records[i].c;
      bestTag = i;
      if (qual != NULL) bestLowQual = qual[records[i].a];
    } else if (records[i].c == bestCnt) {
      if (qual != NULL && qual[records[i].a] < bestLowQual) {
        bestLowQual = qual[records[i].a];
        bestTag = i;
      }
    }
  }
  barcode[records[bestTag].a] = (uint8_t)testChr[records[bestTag].b];
  return 1;
}

void BarcodeWhitelist::entries(std::vector<uint8_t> &bases, std::vector<uint64_t> &offsets, std::vector<uint32_t> &counts) const {
  bases.clear(); offsets.assign(1, 0); counts.clear();
  std::string cur;
  std::function<void(uint32_t)> dfs = [&](uint32_t p) {
    if (nodes_[p].end) {
      bases.insert(bases.end(), cur.begin(), cur.end());
      offsets.push_back(bases.size());
      counts.push_back((uint32_t)nodes_[p].count);
    }
    for (int t = 0; t < 4; ++t)
      if (nodes_[p].next[t]) { cur.push_back("ACGT"[t]); dfs(nodes_[p].next[t]); cur.pop_back(); }
  };
  dfs(0);
}

void BarcodeWhitelist::set_entry_counts(const std::vector<uint32_t> &counts) {
  size_t k = 0;
  std::function<void(uint32_t)> dfs = [&](uint32_t p) {
    if (nodes_[p].end) nodes_[p].count = (int32_t)counts.at(k++);
    for (int t = 0; t < 4; ++t)
      if (nodes_[p].next[t]) dfs(nodes_[p].next[t]);
  };
  dfs(0);
}

// ---- the handle ----

Barcode::Barcode(const std::string &whitelist_path, int device) : wl_(whitelist_path) {
  const int L = wl_.common_length();
  if (device >= 0 && L >= 1 && L <= kBarcodeDeviceMaxLen) {
    wl_.entries(e_bases_, e_off_, e_counts_);
    dev_.reset(make_barcode_device(device, L, e_bases_, e_off_, e_counts_));
  }
}

void Barcode::sync_counts_to_host() {
  if (!dev_ || !dev_counts_newer_) return;
  dev_->download_counts(e_bases_, e_off_, e_counts_);
  wl_.set_entry_counts(e_counts_);
  dev_counts_newer_ = false;
}

// CollectBackgroundDistribution (BarcodeCorrector.hpp:150-163) over barcodes that are already extracted
void Barcode::count(const uint8_t *bases, const uint64_t *offsets, size_t n, size_t max_records) {
  const size_t m = std::min(n, max_records);
  device_ms = 0;
  host_barcodes = 0;
  if (!dev_) {
    for (size_t i = 0; i < m; ++i) wl_.search_update(bases + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), 1);
    host_barcodes = m;
  } else {
    const uint64_t L = (uint64_t)wl_.common_length();
    if (m) { dev_->count(bases, offsets, m); dev_counts_newer_ = true; device_ms = dev_->last_ms; }
    for (size_t i = 0; i < m; ++i)   // a shorter barcode may end on an inner node of the trie, whose count only the twin holds
      if (offsets[i + 1] - offsets[i] != L) { wl_.search_update(bases + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), 1); ++host_barcodes; }
  }
  host_barcodes_total += host_barcodes;
}

void Barcode::correct(const uint8_t *bases, const uint64_t *offsets, const int8_t *qual, size_t n, int threads, int8_t *status, uint8_t *out_bases,
                      bool host_only) {
  device_ms = 0;
  host_barcodes = 0;
  if (n == 0) return;
  if (threads < 1) threads = 1;
  if ((size_t)threads > n) threads = (int)n;
  const bool use_dev = dev_ && !host_only;
  if (use_dev) {
    d_status_.resize(n); d_pos_.resize(n); d_base_.resize(n);
    dev_->correct(bases, offsets, qual, n, d_status_.data(), d_pos_.data(), d_base_.data());
    device_ms = dev_->last_ms;
  } else {
    sync_counts_to_host();
  }
  std::vector<uint64_t> to_host((size_t)threads, 0);
  parallel_slices(n, threads, [&](size_t lo, size_t hi, int tid) {
    if (hi > lo) memcpy(out_bases + offsets[lo], bases + offsets[lo], (size_t)(offsets[hi] - offsets[lo]));
    for (size_t i = lo; i < hi; ++i) {
      const uint64_t a = offsets[i];
      const size_t len = (size_t)(offsets[i + 1] - a);
      if (use_dev && d_status_[i] != kBarcodeToHost) {
        status[i] = d_status_[i];
        if (d_status_[i] == 1) out_bases[a + d_pos_[i]] = d_base_[i];
      } else {
        // on the device path only barcodes whose length is not L come here: they end on inner nodes of the trie or nowhere, never on an
        // entry, so the counts they meet are the ones the host keeps itself and no sync_counts_to_host() is needed
        status[i] = (int8_t)wl_.correct(out_bases + a, len, qual ? qual + a : nullptr);
        ++to_host[(size_t)tid];
      }
    }
  });
  for (uint64_t v : to_host) host_barcodes += v;
  host_barcodes_total += host_barcodes;
}

void Barcode::counts(const uint8_t **bases, const uint64_t **offsets, const uint32_t **counts, size_t *n) {
  sync_counts_to_host();
  wl_.entries(e_bases_, e_off_, e_counts_);
  *bases = e_bases_.data(); *offsets = e_off_.data(); *counts = e_counts_.data(); *n = e_counts_.size();
}

// ---- BarcodeTranslator ----

BarcodeTranslate::BarcodeTranslate(const std::string &path) {
  gzFile fp = gzopen(path.c_str(), "r");
  if (!fp) throw IoError{"cannot open the barcode translation table " + path};
  const uint32_t line_buffer_size = 512;
  char file_line[line_buffer_size];
  while (gzgets(fp, file_line, line_buffer_size) != NULL) {
    int line_len = (int)strlen(file_line);
    if (line_len > 0 && file_line[line_len - 1] == '\n') file_line[line_len - 1] = '\0';
    // ProcessTranslateFileLine (:94-112): TO<sep>FROM; the length of `from` is the last line's; a repeated `from` keeps the last `to`
    const std::string line(file_line);
    const int len = (int)line.length();
    int i;
    for (i = 0; i < len; ++i)
      if (line[i] == ',' || line[i] == '\t' || line[i] == ' ') break;
    if (i >= len - 1) { gzclose(fp); throw FormatError{"barcode translation table " + path + ": a line without `to<separator>from`: " + line}; }
    from_len_ = len - i - 1;
    table_[line.substr((size_t)i + 1, (size_t)(len - i - 1))] = line.substr(0, (size_t)i);
  }
  gzclose(fp);
  if (from_len_ <= 0) throw FormatError{"barcode translation table " + path + " is empty"};
}

bool BarcodeTranslate::translate(const uint8_t *bc, size_t len, std::string &out, std::string &missing) const {   // Translate (:57-83)
  out.clear();
  for (size_t i = 0; i < len / (size_t)from_len_; ++i) {
    std::string bc_from((const char *)bc + i * (size_t)from_len_, (size_t)from_len_);
    bc_from = bc_from.c_str();   // the table is keyed by C strings
    auto it = table_.find(bc_from);
    if (it == table_.end()) { missing = bc_from; return false; }
    if (i == 0) out = it->second;
    else out += "-" + it->second;
  }
  return true;
}

}  // namespace cfr
