// cfr_cli_reads.hpp — the read-file half of the `centrifuger` command line (cfr_cli.cpp): FASTA/FASTQ (optionally gz / BGZF) records
// into the flat buffers of a batch, sequentially or from pieces of a mapped plain file cut at verified record starts.  Needs no
// index and no device; beside cfr_cli.cpp only tools/reads_sanitize.cpp includes it (a program of its own for sanitizer builds,
// which is why everything here sits in an unnamed namespace of the including file).
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cfr_hip.h"

namespace {

void print_log(const char *fmt, ...) {   // Utils::PrintLog (compactds/Utils.hpp:369-381)
  char buffer[1024];
  va_list args;
  va_start(args, fmt);
  vsnprintf(buffer, sizeof(buffer), fmt, args);
  va_end(args);
  time_t now = time(nullptr);
  char stime[128];
  strftime(stime, sizeof(stime), "%c", localtime(&now));
  fprintf(stderr, "[%s] %s\n", stime, buffer);
}

// Growable byte buffer for the bases of a batch; optionally in PINNED host memory (cfr_host_alloc: the bases then go to the
// device at PCIe rate, pageable memory is staged by the runtime at a third of that - but pinning 40 MB per batch object costs
// more than it returns below ~100 M reads, so it is off by default).
class ByteBuf {
 public:
  ByteBuf() = default;
  ByteBuf(const ByteBuf &) = delete;
  ByteBuf &operator=(const ByteBuf &) = delete;
  ~ByteBuf() { release(); }
  uint8_t *data() { return p_; }
  const uint8_t *data() const { return p_; }
  size_t size() const { return n_; }
  void clear() { n_ = 0; }
  void reserve(size_t want) {
    if (want <= cap_) return;
    size_t cap = cap_ ? cap_ : (1u << 20);
    while (cap < want) cap *= 2;
    bool pinned = use_pinned;
    uint8_t *q = pinned ? (uint8_t *)cfr_host_alloc(cap) : nullptr;
    if (!q) { pinned = false; q = (uint8_t *)malloc(cap); }
    if (!q) { fprintf(stderr, "out of memory\n"); exit(EXIT_FAILURE); }
    if (n_) memcpy(q, p_, n_);
    release();
    p_ = q; cap_ = cap; pinned_ = pinned;
  }
  void append(const uint8_t *src, size_t len) {
    if (n_ + len > cap_) { const size_t keep = n_; reserve(n_ + len); n_ = keep; }
    memcpy(p_ + n_, src, len);
    n_ += len;
  }
  static bool use_pinned;
 private:
  void release() {
    if (p_) { if (pinned_) cfr_host_free(p_); else free(p_); }
    p_ = nullptr; cap_ = 0;
  }
  uint8_t *p_ = nullptr;
  size_t n_ = 0, cap_ = 0;
  bool pinned_ = false;
};
bool ByteBuf::use_pinned = false;     // measured: hipHostMalloc of 40 MB per batch costs more than the faster copies return (profiles/r2f_cli_timing.txt); CFR_CLI_PIN=1 turns it on

// ---- FASTA/FASTQ (optionally gz) record reader; id = first word of the header -----------------
// Block reads (16 MB) + memchr line splitting; sequence lines are appended straight into the batch's flat buffers
// (no per-record strings).  Record grammar as in the reference's kseq use (ReadFiles.hpp:94-160): multi-line FASTA and
// FASTQ, '>' or '@' headers, id up to the first blank, trailing /1 or /2 removed (ReadFiles.hpp:82-90).
class SeqReader {
 public:
  explicit SeqReader(const std::vector<std::string> &files) : files_(files), buf_(1u << 24) {}
  bool want_comment = false;           // keep the header's comment (what follows the id's delimiter; kseq's comment) of the last record read
  std::string last_comment;
  static int inflate_threads;          // threads that inflate the blocks of a BGZF file side by side (1: every .gz through gzread)
  // a byte range of a memory-mapped plain file that starts at a record header (the parallel path: ParallelFiles below)
  SeqReader(const char *mem, size_t len) : mem_(mem), pos_(0), end_(len), eof_(true) {}
  ~SeqReader() { close_file(); }

  // offset (in the memory range) at which the next record starts
  size_t next_start() const { return have_header_ ? header_off_ : pos_; }
  bool next_mem(std::vector<char> *ids, ByteBuf &seq, std::vector<char> *qual, bool &has_qual) { return read_record(ids, seq, qual, has_qual); }

  // Appends the next record: id (NUL-terminated) to ids, bases to seq, quality to qual when it is wanted.
  // returns false at the end of all files
  bool next(std::vector<char> *ids, ByteBuf &seq, std::vector<char> *qual, bool &has_qual) {
    for (;;) {
      if (!fp_ && !bgzf_base_) {
        if (file_idx_ >= files_.size()) return false;
        const std::string &f = files_[file_idx_++];
        have_header_ = false;
        pos_ = end_ = 0;
        eof_ = false;
        if (f != "-" && inflate_threads > 1 && open_bgzf(f)) start_bgzf_inflaters();
        else {
          fp_ = f == "-" ? gzdopen(fileno(stdin), "r") : gzopen(f.c_str(), "r");
          if (!fp_) { print_log("ERROR: cannot open read file %s", f.c_str()); exit(EXIT_FAILURE); }
          gzbuffer(fp_, 1 << 20);
          start_inflater();
        }
      }
      if (read_record(ids, seq, qual, has_qual)) return true;
      close_file();
    }
  }

 private:
  // next line without its line terminator; the view is valid until the next call.  false: nothing left.
  bool next_line(const char *&p, size_t &n) {
    for (;;) {
      const char *base = mem_ ? mem_ : buf_.data();
      line_off_ = pos_;
      if (const char *nl = (const char *)memchr(base + pos_, '\n', end_ - pos_)) {
        p = base + pos_;
        n = (size_t)(nl - p);
        pos_ = (size_t)(nl - base) + 1;
        while (n && p[n - 1] == '\r') --n;
        return true;
      }
      if (eof_) {
        if (pos_ == end_) return false;
        p = base + pos_;
        n = end_ - pos_;
        pos_ = end_;
        while (n && p[n - 1] == '\r') --n;
        return n > 0;
      }
      if (pos_) { memmove(buf_.data(), buf_.data() + pos_, end_ - pos_); end_ -= pos_; pos_ = 0; }
      if (end_ == buf_.size()) buf_.resize(buf_.size() * 2);
      const size_t got = pull(buf_.data() + end_, buf_.size() - end_);
      if (got == 0) eof_ = true; else end_ += got;
    }
  }
  bool read_record(std::vector<char> *ids, ByteBuf &seq, std::vector<char> *qual, bool &has_qual) {
    const char *p;
    size_t n;
    if (have_header_) { p = header_.data(); n = header_.size(); }
    else {
      do { if (!next_line(p, n)) return false; } while (n == 0 || (p[0] != '>' && p[0] != '@'));
    }
    have_header_ = false;
    const bool fastq = p[0] == '@';
    size_t e = 1;
    while (e < n && p[e] != ' ' && p[e] != '\t') ++e;
    size_t idn = e - 1;
    if (idn >= 2 && p[e - 2] == '/' && (p[e - 1] == '1' || p[e - 1] == '2')) idn -= 2;
    if (ids) { ids->insert(ids->end(), p + 1, p + 1 + idn); ids->push_back('\0'); }
    if (want_comment) { if (e < n) last_comment.assign(p + e + 1, n - e - 1); else last_comment.clear(); }
    has_qual = false;
    size_t seq_n = 0;
    // kseq's grammar (kseq.h kseq_read): the sequence runs until a line that starts with '>', '@' or '+', whatever the
    // header character was and however many bases have been read; a '+' line switches to the quality block, which is
    // read line by line until it is at least as long as the sequence (at least one line, also for an empty sequence).
    (void)fastq;
    while (next_line(p, n)) {
      if (n == 0) continue;
      if (p[0] == '>' || p[0] == '@') { header_.assign(p, n); have_header_ = true; header_off_ = line_off_; return true; }
      if (p[0] == '+') {
        has_qual = true;
        size_t qn = 0;
        do {
          if (!next_line(p, n)) break;
          if (qual) qual->insert(qual->end(), p, p + n);
          qn += n;
        } while (qn < seq_n);
        return true;
      }
      seq.append((const uint8_t *)p, n);
      seq_n += n;
    }
    return true;
  }
  // ---- the inflater: gzread (one deflate stream is sequential: ~0.4 GB/s of text) runs on a thread of its own, 8 MB chunks ahead of
  // the line splitter, so that decompression and parsing overlap (a .gz input is bound by the inflate rate either way)
  struct Chunk { std::vector<char> data; size_t used = 0; };
  void start_inflater() {
    inf_stop_ = false;
    inf_eof_ = false;
    inflater_ = std::thread([this]() {
      for (;;) {
        Chunk c;
        c.data.resize(8u << 20);
        const int got = gzread(fp_, c.data.data(), (unsigned)c.data.size());
        std::unique_lock<std::mutex> lk(inf_mu_);
        if (got <= 0) { inf_eof_ = true; inf_cv_.notify_all(); return; }
        c.data.resize((size_t)got);
        inf_cv_.wait(lk, [&] { return inf_stop_ || ready_.size() < 4; });
        if (inf_stop_) return;
        ready_.push_back(std::move(c));
        inf_cv_.notify_all();
      }
    });
  }
  // ---- BGZF (bgzip, htslib): a .gz file made of independent deflate blocks of at most 64 KB whose compressed size stands in an extra
  // field of every block's header ('B' 'C', RFC 1952 FEXTRA; SAM specification section 4.1) - so the blocks can be found without
  // inflating anything, and inflated side by side.  The reference reads such a file like any .gz (kseq + gzread, ReadFiles.hpp:337): one
  // thread, ~0.4 GB/s of text; here a dispatcher walks the headers, groups of blocks (~8 MB of text) are inflated by inflate_threads
  // workers (raw inflate + CRC-32 + ISIZE of every block checked, like gzread does) and handed to the line splitter in file order.
  static bool bgzf_header(const uint8_t *b, size_t left, size_t &bsize) {        // b: start of a block; false: not a BGZF block
    if (left < 18 || b[0] != 0x1f || b[1] != 0x8b || b[2] != 8 || !(b[3] & 4)) return false;
    const size_t xlen = (size_t)b[10] | ((size_t)b[11] << 8);
    if (12 + xlen > left) return false;
    for (size_t o = 12; o + 4 <= 12 + xlen;) {
      const size_t slen = (size_t)b[o + 2] | ((size_t)b[o + 3] << 8);
      if (b[o] == 'B' && b[o + 1] == 'C' && slen == 2 && o + 6 <= 12 + xlen) {
        bsize = ((size_t)b[o + 4] | ((size_t)b[o + 5] << 8)) + 1;
        return bsize >= 12 + xlen + 8 && bsize <= left;
      }
      o += 4 + slen;
    }
    return false;
  }
  bool open_bgzf(const std::string &path) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    uint8_t magic[4];
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 28 || pread(fd, magic, 4, 0) != 4 || magic[0] != 0x1f || magic[1] != 0x8b ||
        magic[2] != 8 || !(magic[3] & 4)) { ::close(fd); return false; }
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (m == MAP_FAILED) return false;
    // every member must be a BGZF block: a file that continues as a plain gzip member (`cat a.bgz b.gz`) is read like any .gz below,
    // which is what the reference does with it (kseq + gzread walks concatenated members).  The walk touches one header per block.
    for (size_t o = 0; o < (size_t)st.st_size;) {
      size_t bs = 0;
      if (!bgzf_header((const uint8_t *)m + o, (size_t)st.st_size - o, bs)) { munmap(m, (size_t)st.st_size); return false; }
      o += bs;
    }
    bgzf_base_ = (const uint8_t *)m;
    bgzf_size_ = (size_t)st.st_size;
    bgzf_path_ = path;
    return true;
  }
  struct BgzfTask { size_t id, off, end, text; };                               // blocks [off, end) of the file inflate to `text` bytes
  void start_bgzf_inflaters() {
    inf_stop_ = false;
    inf_eof_ = false;
    bgzf_next_deliver_ = 0;
    bgzf_issued_ = 0;
    bgzf_tasks_done_ = false;
    const int nt = inflate_threads;
    bgzf_workers_.emplace_back([this, nt]() {                                     // the dispatcher
      size_t off = 0, id = 0;
      while (off < bgzf_size_) {
        BgzfTask t{id, off, off, 0};
        while (t.end < bgzf_size_ && t.text < (8u << 20)) {
          size_t bs = 0;
          if (!bgzf_header(bgzf_base_ + t.end, bgzf_size_ - t.end, bs)) { print_log("ERROR: %s is not a well-formed BGZF file at byte %lu", bgzf_path_.c_str(), (unsigned long)t.end); exit(EXIT_FAILURE); }
          const uint8_t *tail = bgzf_base_ + t.end + bs - 4;
          t.text += (size_t)tail[0] | ((size_t)tail[1] << 8) | ((size_t)tail[2] << 16) | ((size_t)tail[3] << 24);
          t.end += bs;
        }
        off = t.end;
        std::unique_lock<std::mutex> lk(inf_mu_);
        inf_cv_.wait(lk, [&] { return inf_stop_ || bgzf_issued_ - bgzf_next_deliver_ < (size_t)(2 * nt + 2); });
        if (inf_stop_) return;
        bgzf_queue_.push_back(t);
        ++bgzf_issued_;
        ++id;
        inf_cv_.notify_all();
      }
      std::lock_guard<std::mutex> lk(inf_mu_);
      bgzf_tasks_done_ = true;
      inf_cv_.notify_all();
    });
    for (int w = 0; w < nt; ++w) bgzf_workers_.emplace_back([this]() {
      z_stream zs;
      memset(&zs, 0, sizeof(zs));
      if (inflateInit2(&zs, -15) != Z_OK) { print_log("ERROR: zlib inflateInit2 failed"); exit(EXIT_FAILURE); }
      for (;;) {
        BgzfTask t;
        {
          std::unique_lock<std::mutex> lk(inf_mu_);
          inf_cv_.wait(lk, [&] { return inf_stop_ || !bgzf_queue_.empty() || bgzf_tasks_done_; });
          if (inf_stop_ || bgzf_queue_.empty()) break;
          t = bgzf_queue_.front();
          bgzf_queue_.pop_front();
        }
        Chunk c;
        c.data.resize(t.text);
        size_t out = 0;
        for (size_t o = t.off; o < t.end;) {
          size_t bs = 0;
          bgzf_header(bgzf_base_ + o, bgzf_size_ - o, bs);
          const uint8_t *b = bgzf_base_ + o;
          const size_t xlen = (size_t)b[10] | ((size_t)b[11] << 8), hdr = 12 + xlen;
          const uint8_t *tail = b + bs - 8;
          const uint32_t crc = (uint32_t)tail[0] | ((uint32_t)tail[1] << 8) | ((uint32_t)tail[2] << 16) | ((uint32_t)tail[3] << 24);
          const size_t isize = (size_t)tail[4] | ((size_t)tail[5] << 8) | ((size_t)tail[6] << 16) | ((size_t)tail[7] << 24);
          inflateReset(&zs);
          zs.next_in = const_cast<Bytef *>(b + hdr);
          zs.avail_in = (uInt)(bs - hdr - 8);
          zs.next_out = (Bytef *)c.data.data() + out;
          zs.avail_out = (uInt)isize;
          const int rc = isize || zs.avail_in > 2 ? inflate(&zs, Z_FINISH) : Z_STREAM_END;
          if ((rc != Z_STREAM_END && !(rc == Z_OK && zs.avail_out == 0)) || zs.total_out != isize ||
              (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)c.data.data() + out, (uInt)isize) != crc) {
            print_log("ERROR: %s: a BGZF block at byte %lu does not inflate to what its trailer says", bgzf_path_.c_str(), (unsigned long)o);
            exit(EXIT_FAILURE);
          }
          out += isize;
          o += bs;
        }
        std::lock_guard<std::mutex> lk(inf_mu_);
        bgzf_done_.emplace(t.id, std::move(c));
        inf_cv_.notify_all();
      }
      inflateEnd(&zs);
    });
  }
  size_t pull_bgzf(char *dst, size_t cap) {
    std::unique_lock<std::mutex> lk(inf_mu_);
    for (;;) {
      inf_cv_.wait(lk, [&] { return bgzf_done_.count(bgzf_next_deliver_) || (bgzf_tasks_done_ && bgzf_next_deliver_ == bgzf_issued_); });
      auto it = bgzf_done_.find(bgzf_next_deliver_);
      if (it == bgzf_done_.end()) return 0;
      Chunk &c = it->second;
      const size_t n = std::min(cap, c.data.size() - c.used);
      memcpy(dst, c.data.data() + c.used, n);
      c.used += n;
      if (c.used == c.data.size()) { bgzf_done_.erase(it); ++bgzf_next_deliver_; inf_cv_.notify_all(); }
      if (n) return n;                                                           // (an empty group - the end-of-file marker block - is skipped)
    }
  }
  size_t pull(char *dst, size_t cap) {                    // up to cap bytes of decompressed text; 0 at the end of the file
    if (bgzf_base_) return pull_bgzf(dst, cap);
    std::unique_lock<std::mutex> lk(inf_mu_);
    inf_cv_.wait(lk, [&] { return !ready_.empty() || inf_eof_; });
    if (ready_.empty()) return 0;
    Chunk &c = ready_.front();
    const size_t n = std::min(cap, c.data.size() - c.used);
    memcpy(dst, c.data.data() + c.used, n);
    c.used += n;
    if (c.used == c.data.size()) { ready_.pop_front(); inf_cv_.notify_all(); }
    return n;
  }
  void close_file() {
    if (inflater_.joinable()) {
      { std::lock_guard<std::mutex> lk(inf_mu_); inf_stop_ = true; }
      inf_cv_.notify_all();
      inflater_.join();
    }
    if (!bgzf_workers_.empty()) {
      { std::lock_guard<std::mutex> lk(inf_mu_); inf_stop_ = true; }
      inf_cv_.notify_all();
      for (auto &t : bgzf_workers_) t.join();
      bgzf_workers_.clear();
      bgzf_queue_.clear();
      bgzf_done_.clear();
    }
    if (bgzf_base_) { munmap((void *)bgzf_base_, bgzf_size_); bgzf_base_ = nullptr; bgzf_size_ = 0; }
    ready_.clear();
    if (fp_) gzclose(fp_);
    fp_ = nullptr;
  }
  const uint8_t *bgzf_base_ = nullptr;
  size_t bgzf_size_ = 0, bgzf_next_deliver_ = 0, bgzf_issued_ = 0;
  bool bgzf_tasks_done_ = false;
  std::string bgzf_path_;
  std::vector<std::thread> bgzf_workers_;
  std::deque<BgzfTask> bgzf_queue_;
  std::map<size_t, Chunk> bgzf_done_;
  std::thread inflater_;
  std::mutex inf_mu_;
  std::condition_variable inf_cv_;
  std::deque<Chunk> ready_;
  bool inf_stop_ = false, inf_eof_ = false;
  std::vector<std::string> files_;
  size_t file_idx_ = 0;
  gzFile fp_ = nullptr;
  std::vector<char> buf_;
  const char *mem_ = nullptr;
  size_t pos_ = 0, end_ = 0, line_off_ = 0, header_off_ = 0;
  bool eof_ = false;
  std::string header_;
  bool have_header_ = false;
};

int SeqReader::inflate_threads = 1;

// The record cutter's search over any buffer of text: the first verified record start at or after `from`, or size.  fmt: '>' or '@',
// the file's first byte.  from = 0 is taken for a line start; elsewhere the search begins behind the next '\n' unless a '\n' stands in
// front.  whole: the buffer ends where the text ends - otherwise a FASTQ record verifies only when its fourth line ends inside the buffer.
inline size_t resync_text(const char *base, size_t size, char fmt, size_t from, bool whole) {
  size_t at = from;
  if (at > 0 && base[at - 1] != '\n') {
    const char *nl = at < size ? (const char *)memchr(base + at, '\n', size - at) : nullptr;
    if (!nl) return size;
    at = (size_t)(nl - base) + 1;
  }
  auto line_end = [&](size_t a) -> size_t { const char *nl = (const char *)memchr(base + a, '\n', size - a); return nl ? (size_t)(nl - base) : size; };
  auto trimmed = [&](size_t a, size_t e) -> size_t { while (e > a && base[e - 1] == '\r') --e; return e - a; };
  while (at < size) {
    const size_t e0 = line_end(at);
    if (base[at] == fmt) {
      if (fmt == '>') return at;
      const size_t l1 = e0 + 1;
      if (l1 < size) {
        const size_t e1 = line_end(l1), l2 = e1 + 1;
        if (l2 < size && base[l2] == '+') {
          const size_t e2 = line_end(l2), l3 = e2 + 1;
          if (l3 <= size) {
            const size_t e3 = l3 < size ? line_end(l3) : size;
            if ((whole || e3 < size) && trimmed(l1, e1) == trimmed(l3, e3) && (e3 + 1 >= size || base[e3 + 1] == '@')) return at;
          }
        }
      }
    }
    at = e0 + 1;
  }
  return size;
}

// A plain (not gz) regular read file mapped into memory, and the offsets at which it can be cut into independently parsable
// pieces.  A cut is a verified record start: FASTA - a line that starts with '>'; FASTQ - a line that starts with '@' whose
// third line starts with '+' and whose second and fourth lines have the same length (a quality line that starts with '@' fails
// that: the line two below it is a sequence).  Multi-line FASTQ never verifies; such files take the sequential reader.
struct MappedFile {
  const char *base = nullptr;
  size_t size = 0;
  int fd = -1;
  ~MappedFile() { if (base) munmap((void *)base, size); if (fd >= 0) close(fd); }
  bool open_plain(const std::string &path) {
    fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 4) return false;
    size = (size_t)st.st_size;
    void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) return false;
    base = (const char *)m;
    if ((unsigned char)base[0] == 0x1f && (unsigned char)base[1] == 0x8b) return false;      // gz
    return base[0] == '@' || base[0] == '>';
  }
  // first verified record start at or after `from` (a line start), or size
  size_t resync(size_t from) const { return resync_text(base, size, base[0], from, true); }
};

// Cuts about every `piece` bytes, each moved on to the next verified record start: cuts = 0, ..., the file size
inline void plan_byte_cuts(const MappedFile &mf, size_t piece, std::vector<size_t> &cuts) {
  cuts.assign(1, 0);
  while (cuts.back() + piece < mf.size) {
    const size_t c = mf.resync(cuts.back() + piece);
    if (c >= mf.size || c <= cuts.back()) break;
    cuts.push_back(c);
  }
  cuts.push_back(mf.size);
}

// --gpu-inflate: a read file that is BGZF throughout, mapped, and the cuts of its TEXT into record-aligned pieces found without the
// text: the members are grouped by their ISIZE into pieces of about `piece` text bytes, and at every boundary a scout inflates members
// on the host (zlib), the boundary's member alone first, one more at a time up to kScoutBytes of text, until the record cutter
// (resync_text) finds a verified record start in that window; a boundary where none is found is dropped.  cut[k]: the text offset of
// piece k's first record; piece k is the text [cut[k], cut[k + 1]).
struct BgzfFile {
  static constexpr size_t kScoutBytes = 4u << 20;
  std::string path;
  const uint8_t *base = nullptr;
  size_t size = 0;
  std::vector<size_t> off, text;       // members + 1 entries: where member m stands in the file, and its text in the file's text
  std::vector<size_t> cut;
  char fmt = 0;
  ~BgzfFile() { if (base) munmap((void *)base, size); }

  static bool header(const uint8_t *b, size_t left, size_t &bsize, size_t &head) {      // the rule of SeqReader::bgzf_header
    if (left < 18 || b[0] != 0x1f || b[1] != 0x8b || b[2] != 8 || !(b[3] & 4)) return false;
    const size_t xlen = (size_t)b[10] | ((size_t)b[11] << 8);
    if (12 + xlen > left) return false;
    for (size_t o = 12; o + 4 <= 12 + xlen;) {
      const size_t slen = (size_t)b[o + 2] | ((size_t)b[o + 3] << 8);
      if (b[o] == 'B' && b[o + 1] == 'C' && slen == 2 && o + 6 <= 12 + xlen) {
        bsize = ((size_t)b[o + 4] | ((size_t)b[o + 5] << 8)) + 1;
        head = 12 + xlen;
        return bsize >= 12 + xlen + 8 && bsize <= left;
      }
      o += 4 + slen;
    }
    return false;
  }
  // true: a regular file made of BGZF members from its first byte to its last
  bool open(const std::string &p) {
    path = p;
    const int fd = ::open(p.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 28) { ::close(fd); return false; }
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (m == MAP_FAILED) return false;
    base = (const uint8_t *)m;
    size = (size_t)st.st_size;
    size_t t = 0;
    for (size_t o = 0; o < size;) {
      size_t bs = 0, head = 0;
      if (!header(base + o, size - o, bs, head)) return false;
      off.push_back(o);
      text.push_back(t);
      const uint8_t *tail = base + o + bs - 4;
      t += (size_t)tail[0] | ((size_t)tail[1] << 8) | ((size_t)tail[2] << 16) | ((size_t)tail[3] << 24);
      o += bs;
    }
    off.push_back(size);
    text.push_back(t);
    return true;
  }
  size_t members() const { return off.size() - 1; }
  size_t member_of(size_t t) const { return (size_t)(std::upper_bound(text.begin(), text.end(), t) - text.begin()) - 1; }   // t below the text's size
  // members [lo, hi) inflated behind out; a member that does not inflate to what its trailer says ends the run, as on the host path
  void inflate_members(size_t lo, size_t hi, std::vector<char> &out) const {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) { print_log("ERROR: zlib inflateInit2 failed"); exit(EXIT_FAILURE); }
    for (size_t m = lo; m < hi; ++m) {
      const uint8_t *b = base + off[m];
      const size_t bs = off[m + 1] - off[m], hdr = 12 + ((size_t)b[10] | ((size_t)b[11] << 8)), isize = text[m + 1] - text[m], at = out.size();
      const uint8_t *tail = b + bs - 8;
      const uint32_t crc = (uint32_t)tail[0] | ((uint32_t)tail[1] << 8) | ((uint32_t)tail[2] << 16) | ((uint32_t)tail[3] << 24);
      out.resize(at + isize);
      inflateReset(&zs);
      zs.next_in = const_cast<Bytef *>(b + hdr);
      zs.avail_in = (uInt)(bs - hdr - 8);
      zs.next_out = (Bytef *)out.data() + at;
      zs.avail_out = (uInt)isize;
      const int rc = isize || zs.avail_in > 2 ? inflate(&zs, Z_FINISH) : Z_STREAM_END;
      if ((rc != Z_STREAM_END && !(rc == Z_OK && zs.avail_out == 0)) || zs.total_out != isize ||
          (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)out.data() + at, (uInt)isize) != crc) bad_member(off[m]);
    }
    inflateEnd(&zs);
  }
  void bad_member(size_t at) const {
    print_log("ERROR: %s: a BGZF block at byte %lu does not inflate to what its trailer says", path.c_str(), (unsigned long)at);
    exit(EXIT_FAILURE);
  }
  // the first verified record start behind the first line end of member m's text, as a text offset;
  // text.back(): none within kScoutBytes
  size_t scout(size_t m, std::vector<char> &win) const {
    win.clear();
    for (size_t hi = m; hi < members();) {
      inflate_members(hi, hi + 1, win);
      ++hi;
      const bool whole = hi == members();
      const size_t at = win.empty() ? 0 : resync_text(win.data(), win.size(), fmt, 1, whole);
      if (at < win.size()) return text[m] + at;
      if (win.size() >= kScoutBytes) break;
    }
    return text.back();
  }
  // false: the text does not begin with a record the cutter verifies.  piece_records: records a piece should hold
  bool plan(size_t piece_records) {
    std::vector<char> win;
    const size_t total = text.back();
    cut.clear();
    if (total == 0) { cut.assign(2, 0); return true; }
    // the first record must verify at the text's first byte; bytes per record from it, as the plain files' cutter takes them
    size_t rec_bytes = 0;
    bool found = false;
    for (size_t hi = 0; hi < members() && !found;) {
      inflate_members(hi, hi + 1, win);
      ++hi;
      if (win.empty()) continue;
      if (!fmt) fmt = win[0];
      if (fmt != '@' && fmt != '>') return false;
      const bool whole = hi == members();
      const size_t first = resync_text(win.data(), win.size(), fmt, 0, whole);
      if (first != 0 && first < win.size()) return false;
      if (first == 0) {
        const size_t second = resync_text(win.data(), win.size(), fmt, 1, whole);
        if (second < win.size() || whole) { rec_bytes = second; found = true; }
      }
      if (!found && win.size() >= kScoutBytes) return false;
    }
    if (!found) return false;
    const size_t piece = std::max<size_t>(16, rec_bytes) * std::max<size_t>(piece_records, 1);
    cut.push_back(0);
    for (size_t from = 0;;) {
      const size_t want = from + piece;
      if (want >= total) break;
      size_t m = member_of(want);
      if (text[m] < want) ++m;                        // the first member that begins at or behind the wanted offset: the floor is one member
      if (m >= members()) break;
      const size_t c = scout(m, win);
      from = want;
      if (c >= total) continue;                       // no start found within the bound: the boundary is dropped, two pieces become one
      if (c > cut.back()) { cut.push_back(c); from = c; }
    }
    cut.push_back(total);
    return true;
  }
};

// Cuts at given RECORD numbers (pairs: both mate files must be cut at the same record, an interleaved file at an even one).
// The structure has to be regular for that - 4-line FASTQ (record r starts at line 4 r), or FASTA where every record starts
// with a '>' line: lines (FASTQ) or '>' lines (FASTA) are counted per chunk by several threads, then the wanted records are
// located inside their chunks.  Every cut is verified as a record start, the parsers check that a piece holds exactly the
// records it was cut for, and the caller falls back to the sequential reader when the file is not of that shape.
// every: records per piece.  cuts: byte offsets of records 0, every, 2 every, ... and the file size.  total: records in the file.
inline bool plan_record_cuts(const MappedFile &mf, size_t every, int threads, std::vector<size_t> &cuts, size_t &total) {
  const char fmt = mf.base[0];
  const bool fastq = fmt == '@';
  const size_t chunk = 4u << 20;       // (small chunks: locating a wanted record scans half a chunk line by line)
  const size_t nchunks = (mf.size + chunk - 1) / chunk;
  std::vector<size_t> units(nchunks + 1, 0);          // FASTQ: newlines in the chunk; FASTA: lines that start with '>'
  {
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    const int nt = (int)std::min<size_t>((size_t)std::max(1, threads), nchunks);
    for (int t = 0; t < nt; ++t) th.emplace_back([&]() {
      std::vector<char> buf(chunk + 1);
      for (;;) {
        const size_t k = next.fetch_add(1);
        if (k >= nchunks) return;
        const size_t lo = k * chunk, len = std::min(chunk, mf.size - lo);
        // one byte before the chunk decides whether its first byte starts a line
        const size_t from = lo ? lo - 1 : 0, want = len + (lo ? 1 : 0);
        size_t got = 0;
        while (got < want) {
          const ssize_t r = pread(mf.fd, buf.data() + got, want - got, (off_t)(from + got));
          if (r <= 0) break;
          got += (size_t)r;
        }
        if (got < want) { units[k + 1] = (size_t)-1; continue; }
        const char *p = buf.data() + (lo ? 1 : 0);
        size_t c = 0;
        if (fastq) { for (size_t i = 0; i < len; ++i) c += p[i] == '\n'; }
        else {
          if (p[0] == '>' && (lo == 0 || buf[0] == '\n')) ++c;
          for (size_t i = 1; i < len; ++i) c += (p[i] == '>') & (p[i - 1] == '\n');
        }
        units[k + 1] = c;
      }
    });
    for (auto &x : th) x.join();
  }
  for (size_t k = 0; k < nchunks; ++k) { if (units[k + 1] == (size_t)-1) return false; units[k + 1] += units[k]; }
  size_t lines = units[nchunks];
  if (fastq) {
    if (mf.base[mf.size - 1] != '\n') ++lines;
    if (lines % 4) return false;
    total = lines / 4;
  } else total = lines;
  auto verified = [&](size_t at) -> bool {
    if (at >= mf.size) return at == mf.size;
    if (mf.base[at] != fmt || (at && mf.base[at - 1] != '\n')) return false;
    if (!fastq) return true;
    const char *l1 = (const char *)memchr(mf.base + at, '\n', mf.size - at);
    if (!l1) return false;
    const char *l2 = (const char *)memchr(l1 + 1, '\n', mf.size - (size_t)(l1 + 1 - mf.base));
    return l2 && (size_t)(l2 + 1 - mf.base) < mf.size && l2[1] == '+';
  };
  cuts.clear();
  for (size_t rec = 0; rec < total; rec += every) {
    const size_t unit = fastq ? 4 * rec : rec;          // FASTQ: the record starts behind newline number `unit`; FASTA: at '>' line number `unit`
    if (fastq && unit == 0) { cuts.push_back(0); continue; }
    // FASTQ: the chunk that holds newline number `unit` (units[k] < unit <= units[k + 1]); FASTA: the chunk with '>' line number `unit`
    const size_t k = fastq ? (size_t)(std::lower_bound(units.begin(), units.end(), unit) - units.begin()) - 1
                           : (size_t)(std::upper_bound(units.begin(), units.end(), unit) - units.begin()) - 1;
    if (k >= nchunks) return false;
    size_t at = k * chunk, have = units[k];
    const size_t end = std::min(mf.size, at + chunk + 1);     // (+ 1: the record may start on the first byte of the next chunk)
    size_t pos = (size_t)-1;
    if (fastq) {
      // the byte behind newline number `unit` (1-based count of newlines seen = unit)
      while (have < unit && at < end) {
        const char *nl = (const char *)memchr(mf.base + at, '\n', end - at);
        if (!nl) break;
        ++have;
        at = (size_t)(nl - mf.base) + 1;
      }
      if (have == unit) pos = at;
    } else {
      while (at < end) {
        if (mf.base[at] == '>' && (at == 0 || mf.base[at - 1] == '\n')) { if (have == unit) { pos = at; break; } ++have; }
        const char *nl = (const char *)memchr(mf.base + at, '\n', end - at);
        if (!nl) break;
        at = (size_t)(nl - mf.base) + 1;
      }
    }
    if (pos == (size_t)-1 || !verified(pos)) return false;
    cuts.push_back(pos);
  }
  cuts.push_back(mf.size);
  return !cuts.empty() && cuts[0] == 0;
}

// One batch of reads on its way through the stages of the command line: as read, as classified, as formatted.
struct Batch {
  size_t n = 0;
  bool paired = false;
  std::vector<char> ids;               // NUL-terminated ids back to back
  std::vector<size_t> id_off;
  std::vector<char> qual1, qual2;      // only filled when reads are dumped (--un / --cl)
  std::vector<size_t> q1_off, q2_off;
  std::vector<uint8_t> has_qual, has_qual2;
  ByteBuf bases1, bases2;
  std::vector<uint64_t> offs1, offs2;
  // --merge-readpair with --un / --cl: the reads after the host merge (what is masked and classified; the dumps take a merged pair's
  // mates from bases1 / bases2, which stay as they were read)
  std::vector<uint8_t> m_bases1, m_bases2;
  std::vector<uint64_t> m_offs1, m_offs2;
  std::vector<int32_t> merge_kind;
  // single-cell input: the barcode / UMI records as read (from their files, or a copy of read 1: CopyBatch), then after extraction;
  // bc_str / um_str: what is printed (after correction and translation), NUL-terminated
  ByteBuf bc_raw, um_raw;
  std::vector<uint64_t> bc_raw_off, um_raw_off, bc_rawq_off, um_rawq_off, bc_cm_off, um_cm_off, r1_cm_off;
  std::vector<char> bc_rawq, um_rawq, bc_cm, um_cm, r1_cm;
  std::vector<uint8_t> bc, bc_q, um;
  std::vector<uint64_t> bc_off, um_off;
  bool bc_has_q = false;
  std::vector<char> bc_str, um_str;
  std::vector<size_t> bc_str_off, um_str_off;
  std::vector<cfr_result> results;
  std::vector<cfr_match> matches;
  std::vector<cfr_span> spans;         // --expand-taxid: per match slot, its list in exp_ids
  std::vector<uint64_t> exp_ids;
  std::vector<std::string> tsv_parts;  // the batch's TSV rows in order, as the formatter's workers made them (written part by part: no concatenation;
  std::vector<size_t> part_hits;       //  the strings keep their capacity across recycling); classified reads per part
  size_t n_parts = 0;
  bool tsv_device = false;             // --gpu-format: tsv_parts[0] is the whole batch, made on the device
  bool dump_device = false;            // --gpu-dump: dump_parts hold the batch's BGZF members, made on the device
  std::string dump_parts[2][4];        //  [0: --un, 1: --cl][read 1, read 2, barcode, UMI]
  bool done = false;
  // --gpu-parse: the piece(s) of the mapped read file(s) this batch stands for, not parsed yet: the device worker tokenises them
  // (cfr_tokenize) or, when they are not regular, parses them with SeqReader.  raw_want: the records the piece was cut for;
  // raw_first: the number of its first record in its file
  bool raw = false;
  const char *raw1 = nullptr, *raw2 = nullptr;
  size_t raw1_len = 0, raw2_len = 0, raw_want = 0, raw_first = 0;
  // --gpu-inflate: raw1 / raw1_len are whole BGZF members of bgzf (a file of the run); the piece is the z_len bytes from byte z_skip
  // of their text, with no record count fixed in advance; z_off: where the members stand in the file
  const struct BgzfFile *bgzf = nullptr;
  size_t z_skip = 0, z_len = 0, z_off = 0, z_m0 = 0, z_m1 = 0;     // (z_m0, z_m1: the members, [first, behind the last))
  std::vector<char> z_text;            // ... inflated on the host, when the piece takes the host parsers
  const char *id(size_t i) const { return ids.data() + id_off[i]; }
  void reset(bool pair) {   // keeps every buffer's capacity: batches are recycled, so steady state allocates (and page-faults) nothing
    n = 0; done = false; tsv_device = false; dump_device = false; raw = false; raw1 = raw2 = nullptr; raw1_len = raw2_len = raw_want = raw_first = 0; bgzf = nullptr; z_skip = z_len = z_off = z_m0 = z_m1 = 0;
    ids.clear(); id_off.clear(); qual1.clear(); qual2.clear(); q1_off.clear(); q2_off.clear(); has_qual.clear(); has_qual2.clear();
    bases1.clear(); bases2.clear(); offs1.clear(); offs2.clear(); n_parts = 0;
    bc_raw.clear(); um_raw.clear(); bc_rawq.clear(); um_rawq.clear(); bc_cm.clear(); um_cm.clear(); r1_cm.clear();
    for (auto *v : {&bc_raw_off, &um_raw_off, &bc_rawq_off, &um_rawq_off, &bc_cm_off, &um_cm_off, &r1_cm_off}) v->assign(1, 0);
    bc_str.clear(); um_str.clear(); bc_str_off.clear(); um_str_off.clear();
    paired = pair;
    offs1.push_back(0);
    if (pair) offs2.push_back(0);
    q1_off.push_back(0);
    q2_off.push_back(0);
  }
};

// What the reader takes from every record, and the barcode / UMI files it reads in step with the reads
struct TakeSpec {
  bool paired = false, interleaved = false;
  bool keep_qual = false;              // the qualities too (--un / --cl, --merge-readpair, single-cell input)
  bool r1_comment = false;             // read 1's header comment (a barcode or UMI cut from it, bc:hd: / um:hd:)
  SeqReader *bc = nullptr, *um = nullptr;
};

// one record of the barcode / UMI file beside the read just taken (GetNextBatch, CentrifugerClass.cpp:129-161)
inline void take_extra(SeqReader *r, ByteBuf &raw, std::vector<uint64_t> &off, std::vector<char> &q, std::vector<uint64_t> &q_off, std::vector<char> &cm,
                       std::vector<uint64_t> &cm_off, const char *what) {
  bool hq = false;
  if (!r->next(nullptr, raw, &q, hq)) { print_log("ERROR: The %s file and read file have different number of reads.", what); exit(EXIT_FAILURE); }
  off.push_back(raw.size()); q_off.push_back(q.size());
  if (r->want_comment) { cm.insert(cm.end(), r->last_comment.begin(), r->last_comment.end()); cm_off.push_back(cm.size()); }
}

// one record (+ mate) into b: 1 - taken; 0 - the end of the input; -1 - a read without its mate (the caller says so in its own words)
inline int take(Batch &b, const TakeSpec &ts, SeqReader *r1, SeqReader *r2, bool from_memory) {
  bool hq = false, hq2 = false;
  const size_t id_at = b.ids.size();
  const bool ok1 = from_memory ? r1->next_mem(&b.ids, b.bases1, ts.keep_qual ? &b.qual1 : nullptr, hq)
                               : r1->next(&b.ids, b.bases1, ts.keep_qual ? &b.qual1 : nullptr, hq);
  if (!ok1) return 0;
  if (ts.paired) {
    SeqReader *rm = ts.interleaved ? r1 : r2;
    const bool ok = from_memory ? rm->next_mem(nullptr, b.bases2, ts.keep_qual ? &b.qual2 : nullptr, hq2)
                                : rm->next(nullptr, b.bases2, ts.keep_qual ? &b.qual2 : nullptr, hq2);
    if (!ok) return -1;
    b.offs2.push_back(b.bases2.size());
    if (ts.keep_qual) { b.q2_off.push_back(b.qual2.size()); b.has_qual2.push_back(hq2 ? 1 : 0); }
  }
  b.id_off.push_back(id_at);
  b.offs1.push_back(b.bases1.size());
  if (ts.keep_qual) { b.q1_off.push_back(b.qual1.size()); b.has_qual.push_back(hq ? 1 : 0); }
  if (ts.r1_comment) { b.r1_cm.insert(b.r1_cm.end(), r1->last_comment.begin(), r1->last_comment.end()); b.r1_cm_off.push_back(b.r1_cm.size()); }
  if (ts.bc) take_extra(ts.bc, b.bc_raw, b.bc_raw_off, b.bc_rawq, b.bc_rawq_off, b.bc_cm, b.bc_cm_off, "barcode");
  if (ts.um) take_extra(ts.um, b.um_raw, b.um_raw_off, b.um_rawq, b.um_rawq_off, b.um_cm, b.um_cm_off, "UMI");
  ++b.n;
  return 1;
}

// The records of one piece of a plain file held in memory (m1; pairs: their mates from m2, or interleaved in m1 when there is no
// m2) appended to b; want: stop after that many records (0: all the piece holds).  A piece is good when it was consumed to its
// end (done1, done2), held the records it was cut for (taken) and no read lacked its mate; what a bad one means is the caller's.
struct PieceResult { size_t taken = 0; bool done1 = false, done2 = true, mate_missing = false; };
inline PieceResult parse_piece(Batch &b, const TakeSpec &ts, const char *m1, size_t n1, const char *m2, size_t n2, size_t want) {
  PieceResult res;
  SeqReader rd1(m1, n1), rd2(m2 ? m2 : m1, m2 ? n2 : 0);
  while (rd1.next_start() < n1 && (!want || res.taken < want)) {
    const int got = take(b, ts, &rd1, m2 ? &rd2 : nullptr, true);
    if (got <= 0) { res.mate_missing = got < 0; break; }
    ++res.taken;
  }
  res.done1 = rd1.next_start() >= n1;
  if (m2) res.done2 = rd2.next_start() >= n2;
  return res;
}

}  // namespace
