// reads_sanitize.cpp — a stand-alone driver of the command line's read-file code (csrc/cfr_cli_reads.hpp) for sanitizer builds:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/reads_sanitize.cpp
//       -o reads_sanitize -lz -lpthread && ./reads_sanitize [-t INFLATE_THREADS] reads.fq more.fa.gz ...
// Every file is read three ways: sequentially (SeqReader::next: plain, gz, BGZF); where it is a plain file that cuts, through
// plan_byte_cuts with 64-byte pieces and parse_piece; where the record cutter accepts it and counts the records the sequential
// reader found, through plan_record_cuts with 7 records per piece and parse_piece.  The record streams must be equal.
// One line per file on stdout: its name, the records, a checksum of them (equal for a file and its .gz).  Exit status 0: no
// report and no difference (tests/test_reads_sanitized_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../centrifuger_amd/csrc/cfr_cli_reads.hpp"

// the pinned allocator of the library is not linked: ByteBuf::use_pinned stays off and these are never called
extern "C" void *cfr_host_alloc(size_t) { return nullptr; }
extern "C" void cfr_host_free(void *) {}

namespace {

using Records = std::vector<std::string>;   // "id<TAB>bases<TAB>q:quality|-" per record

void append_records(const Batch &b, Records &out) {
  for (size_t i = 0; i < b.n; ++i) {
    std::string r = b.id(i);
    r += '\t';
    r.append((const char *)b.bases1.data() + b.offs1[i], b.offs1[i + 1] - b.offs1[i]);
    r += b.has_qual[i] ? "\tq:" : "\t-";
    r.append(b.qual1.data() + b.q1_off[i], b.q1_off[i + 1] - b.q1_off[i]);
    out.push_back(std::move(r));
  }
}

int fail(const char *what, const char *file) {
  fprintf(stderr, "reads_sanitize: %s (%s)\n", what, file);
  return 1;
}

// the pieces [cuts[k], cuts[k + 1]) of mf through parse_piece, `every` records in each (0: whatever they hold)
bool read_pieces(const MappedFile &mf, const std::vector<size_t> &cuts, size_t every, size_t total, const TakeSpec &ts, Records &out) {
  Batch b;
  for (size_t k = 0; k + 1 < cuts.size(); ++k) {
    b.reset(false);
    const size_t want = every ? std::min(every, total - k * every) : 0;
    const PieceResult r = parse_piece(b, ts, mf.base + cuts[k], cuts[k + 1] - cuts[k], nullptr, 0, want);
    append_records(b, out);
    if (!r.done1 || (every && r.taken != want)) return false;
  }
  return true;
}

int one_file(const char *path) {
  TakeSpec ts;
  ts.keep_qual = true;
  Records seq, by_bytes, by_records;
  {
    SeqReader rd(std::vector<std::string>{path});
    Batch b;
    for (int got = 1; got > 0;) {
      b.reset(false);
      while (b.n < 1024 && (got = take(b, ts, &rd, nullptr, false)) > 0) {}
      append_records(b, seq);
    }
  }
  MappedFile mf;
  if (mf.open_plain(path)) {
    std::vector<size_t> cuts;
    size_t total = 0;
    if (mf.resync(0) == 0) {
      plan_byte_cuts(mf, 64, cuts);
      if (!read_pieces(mf, cuts, 0, 0, ts, by_bytes)) return fail("a piece cut by bytes was not consumed to its end", path);
      if (by_bytes != seq) return fail("the byte-cut pieces give other records than the sequential reader", path);
    }
    if (plan_record_cuts(mf, 7, 3, cuts, total) && total == seq.size()) {
      if (!read_pieces(mf, cuts, 7, total, ts, by_records)) return fail("a piece cut by records does not hold the records it was cut for", path);
      if (by_records != seq) return fail("the record-cut pieces give other records than the sequential reader", path);
    }
  }
  unsigned long long sum = 1469598103934665603ull;          // FNV-1a over the records
  for (const std::string &r : seq) for (size_t i = 0; i <= r.size(); ++i) sum = (sum ^ (unsigned char)r.c_str()[i]) * 1099511628211ull;
  printf("%s\t%zu\t%016llx\t%s%s\n", path, seq.size(), sum, by_bytes.empty() ? "" : "bytes", by_records.empty() ? "" : "+records");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  int a = 1;
  if (a + 1 < argc && !strcmp(argv[a], "-t")) { SeqReader::inflate_threads = atoi(argv[a + 1]); a += 2; }
  if (a >= argc) { fprintf(stderr, "usage: %s [-t INFLATE_THREADS] reads...\n", argv[0]); return 2; }
  for (; a < argc; ++a) if (one_file(argv[a])) return 1;
  return 0;
}
