// cfr_promote_cli.cpp — `centrifuger-promote`-compatible command line on top of cfr_promote_* (include/cfr_hip.h).
//
// Positionals of the reference's Perl script: centrifuger_index_name centrifuger_output level.  Added: --gpu N|none (default 0; none =
// the host twin, no GPU is touched) and -t INT (threads that parse and format rows).  The classification file may be plain or gz.
// The first line is copied as the header; consecutive rows with one read id are one read (the script's rule); columns 2 (name), 3
// (tax id) and 8 (numMatches) of the kept rows are rewritten, everything else is copied.  Stdout is the script's byte for byte for
// 8-column files; stderr carries its "Couldn't find parent of taxID ..." lines.
// A deliberate difference: the script writes the match count into the LAST column, which in a file with barcode, UMI or expanded
// columns is not numMatches, so it corrupts those files.  This tool always rewrites column 8 and leaves further columns alone.
#include <getopt.h>
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/cfr_hip.h"
#include "cfr_threads.hpp"

static const char usage[] =
    "Usage: centrifuger-promote [OPTIONS] centrifuger_index_name centrifuger_output level > output\n\n"
    "Promote the taxonomy id to specified level in Centrifuge output.\n"
    "\tIf level equals \"lca\", this will merge the multiassignment to their lowest common ancestor.\n"
    "Options:\n"
    "\t--gpu INT|none: GPU that promotes the assignments [0]; none: on the host\n"
    "\t-t INT: number of threads parsing and formatting rows [up to 16]\n"
    "\t-h: print this usage message\n"
    "centrifuger_output may be plain or gz.  Columns 2, 3 and 8 (numMatches) of the kept rows are rewritten; unlike the Perl script,\n"
    "which writes the count into the last column, columns after the eighth (barcode, UMI, expanded tax ids) are left alone.\n";

enum { ARG_GPU = 256 };

struct Line { uint32_t begin, end, t1, t2, t3, t7, t8; uint64_t taxid; };   // byte offsets into the block: tabs behind columns 1, 2, 3, 7, 8 (end where a column is missing)

int main(int argc, char *argv[]) {
  static struct option long_options[] = {{"gpu", required_argument, 0, ARG_GPU}, {(char *)0, 0, 0, 0}};
  int device = 0, threads = 0, c;
  while ((c = getopt_long(argc, argv, "t:h", long_options, nullptr)) != -1) {
    if (c == 't') threads = atoi(optarg);
    else if (c == 'h') { fprintf(stdout, "%s", usage); return 0; }
    else if (c == ARG_GPU) {
      if (!strcmp(optarg, "none")) device = -1;
      else {
        char *end = nullptr;
        long v = strtol(optarg, &end, 10);
        if (end == optarg || *end || v < 0) { fprintf(stderr, "centrifuger-promote: --gpu takes a device number or none, not '%s'\n", optarg); return EXIT_FAILURE; }
        device = (int)v;
      }
    } else { fprintf(stderr, "%s", usage); return EXIT_FAILURE; }
  }
  if (argc - optind != 3) { fprintf(stderr, "%s", usage); return EXIT_FAILURE; }
  const std::string prefix = argv[optind], tsv = argv[optind + 1], level = argv[optind + 2];
  if (threads <= 0) threads = (int)std::min(std::max(std::thread::hardware_concurrency(), 1u), 16u);
  const bool lca = level == "lca";

  // everything this run opens, closed on every way out; the classification file first: a missing one costs no device handle
  struct Open {
    gzFile gz = nullptr;
    cfr_taxonomy *tax = nullptr;
    cfr_promote *pr = nullptr;
    ~Open() { if (pr) cfr_promote_close(pr); if (tax) cfr_taxonomy_close(tax); if (gz) gzclose(gz); }
  } open;
  open.gz = gzopen(tsv.c_str(), "rb");                     // (zlib hands plain files through as they are)
  if (!open.gz) { fprintf(stderr, "centrifuger-promote: cannot open %s\n", tsv.c_str()); return EXIT_FAILURE; }
  gzbuffer(open.gz, 1u << 20);
  if (cfr_taxonomy_open(prefix.c_str(), 0, &open.tax) != CFR_OK) { fprintf(stderr, "centrifuger-promote: cannot read the index %s: %s\n", prefix.c_str(), cfr_last_error()); return EXIT_FAILURE; }
  cfr_taxonomy_tables T;
  cfr_taxonomy_get_tables(open.tax, &T);
  std::unordered_map<uint64_t, uint32_t> to_compact;
  for (uint64_t i = 0; i < T.node_cnt; ++i) to_compact[T.orig_taxid[i]] = (uint32_t)i;       // (a later duplicate wins, as in the script's hashes)
  if (cfr_promote_open(prefix.c_str(), level.c_str(), device, &open.pr) != CFR_OK) { fprintf(stderr, "centrifuger-promote: %s\n", cfr_last_error()); return EXIT_FAILURE; }
  gzFile gz = open.gz;
  cfr_promote *pr = open.pr;

  auto fail = [&](const char *what) { fprintf(stderr, "centrifuger-promote: %s: %s\n", what, cfr_last_error()); return EXIT_FAILURE; };
  std::vector<char> buf((64u << 20) + 1);
  size_t have = 0;
  bool header = true, eof = false;
  std::vector<Line> lines;
  std::vector<cfr_result> results;
  std::vector<cfr_match> matches;
  std::vector<uint64_t> src, warn;
  std::vector<std::string> outs;
  while (!eof) {
    if (have == buf.size() - 1) {
      if (buf.size() > (1u << 31)) { fprintf(stderr, "centrifuger-promote: more than 2 GB of rows with one read id\n"); return EXIT_FAILURE; }
      buf.resize((buf.size() - 1) * 2 + 1);
    }
    while (have < buf.size() - 1) {
      int got = gzread(gz, buf.data() + have, (unsigned)std::min<size_t>(buf.size() - 1 - have, 1u << 30));
      if (got < 0) { fprintf(stderr, "centrifuger-promote: read error in %s\n", tsv.c_str()); return EXIT_FAILURE; }
      if (got == 0) { eof = true; break; }
      have += (size_t)got;
    }
    size_t begin = 0;
    if (header) {                 // the first line, whatever it holds, is printed as it is
      const char *nl = (const char *)memchr(buf.data(), '\n', have);
      if (!nl && !eof) continue;
      begin = nl ? (size_t)(nl - buf.data()) + 1 : have;
      fwrite(buf.data(), 1, begin, stdout);
      header = false;
    }
    // whole lines
    lines.clear();
    size_t end = begin;
    for (size_t p = begin; p < have;) {
      const char *nl = (const char *)memchr(buf.data() + p, '\n', have - p);
      if (!nl && !eof) break;
      const size_t le = nl ? (size_t)(nl - buf.data()) : have;
      Line l{};
      l.begin = (uint32_t)p; l.end = (uint32_t)le;
      lines.push_back(l);
      p = nl ? le + 1 : have;
      end = p;
    }
    cfr::parallel_slices(lines.size(), lines.size() < 4096 ? 1 : threads, [&](size_t lo, size_t hi, int) {
      for (size_t i = lo; i < hi; ++i) {
        Line &l = lines[i];
        uint32_t tab[8];
        int nt = 0;
        for (uint32_t p = l.begin; p < l.end && nt < 8; ++p) if (buf[p] == '\t') tab[nt++] = p;
        for (int k = nt; k < 8; ++k) tab[k] = l.end;
        l.t1 = tab[0]; l.t2 = tab[1]; l.t3 = tab[2]; l.t7 = tab[6]; l.t8 = tab[7];
        uint64_t v = 0;
        for (uint32_t p = l.t2 + 1; p < l.t3 && buf[p] >= '0' && buf[p] <= '9'; ++p) v = v * 10 + (uint64_t)(buf[p] - '0');
        l.taxid = v;
      }
    });
    // reads: consecutive rows with one read id; the last one stays open until the rows behind it are here
    size_t nl_use = lines.size();
    if (!eof && nl_use) {
      size_t k = nl_use - 1;
      const Line &last = lines[k];
      while (k > 0 && lines[k - 1].t1 - lines[k - 1].begin == last.t1 - last.begin &&
             !memcmp(buf.data() + lines[k - 1].begin, buf.data() + last.begin, last.t1 - last.begin)) --k;
      nl_use = k;
      end = lines[k].begin;                 // (a read that fills the whole block: the block grows at the top of the loop)
    }
    results.clear(); matches.resize(nl_use);
    for (size_t i = 0; i < nl_use; ++i) {
      const Line &l = lines[i];
      const bool same = i > 0 && lines[i - 1].t1 - lines[i - 1].begin == l.t1 - l.begin && !memcmp(buf.data() + lines[i - 1].begin, buf.data() + l.begin, l.t1 - l.begin);
      if (!same) { cfr_result r{}; r.match_begin = i; results.push_back(r); }
      ++results.back().n_match;
      auto it = l.taxid ? to_compact.find(l.taxid) : to_compact.end();
      matches[i].id = it == to_compact.end() ? T.node_cnt : it->second;
      matches[i].taxid = l.taxid; matches[i].kind = 1; matches[i].pad = 0;
    }
    if (!results.empty()) {
      if (lca) {
        size_t nw = 0;
        cfr_status st = cfr_promote_lca_warnings(pr, results.data(), matches.data(), results.size(), nullptr, 0, &nw);
        if (st == CFR_ERR_CAPACITY) { warn.resize(nw); st = cfr_promote_lca_warnings(pr, results.data(), matches.data(), results.size(), warn.data(), nw, &nw); }
        if (st != CFR_OK) return fail("cfr_promote_lca_warnings");
        for (size_t i = 0; i < nw; ++i) fprintf(stderr, "Couldn't find parent of taxID %lu - directly assigned to root.\n", (unsigned long)warn[i]);
      }
      src.resize(matches.size());
      if (cfr_promote_apply(pr, results.data(), matches.data(), results.size(), src.data()) != CFR_OK) return fail("cfr_promote_apply");
      const int nth = results.size() < 4096 ? 1 : threads;
      outs.assign((size_t)nth, std::string());
      cfr::parallel_slices(results.size(), nth, [&](size_t lo, size_t hi, int tid) {
        std::string &o = outs[(size_t)tid];
        char num[32];
        for (size_t i = lo; i < hi; ++i) {
          const cfr_result &r = results[i];
          for (int32_t k = 0; k < r.n_match; ++k) {
            const cfr_match &m = matches[r.match_begin + (uint64_t)k];
            const Line &l = lines[src[r.match_begin + (uint64_t)k]];
            // rank mode: a row whose tax id is a node takes the rank of the node it became; lca mode: the row changes when the LCA is not its own id
            const bool rewrite = lca ? m.taxid != l.taxid : (m.kind == 1 && m.id < T.node_cnt);
            o.append(buf.data() + l.begin, l.t1 - l.begin);
            if (l.t1 < l.end) {
              o.push_back('\t');
              if (rewrite) { if (m.id < T.node_cnt) o.append(cfr_tax_rank_string(T.rank[m.id])); }
              else o.append(buf.data() + l.t1 + 1, l.t2 - l.t1 - 1);
            }
            if (l.t2 < l.end) {
              o.push_back('\t');
              if (rewrite) o.append(num, (size_t)snprintf(num, sizeof(num), "%lu", (unsigned long)m.taxid));
              else o.append(buf.data() + l.t2 + 1, l.t3 - l.t2 - 1);
            }
            if (l.t3 < l.end) o.append(buf.data() + l.t3, (l.t7 < l.end ? l.t7 + 1 : l.end) - l.t3);     // columns 4..7 with their tabs
            if (l.t7 < l.end) {
              o.append(num, (size_t)snprintf(num, sizeof(num), "%d", (int)r.n_match));
              o.append(buf.data() + l.t8, l.end - l.t8);                                                 // whatever stands behind column 8
            }
            o.push_back('\n');
          }
        }
      });
      for (const std::string &o : outs) fwrite(o.data(), 1, o.size(), stdout);
    }
    memmove(buf.data(), buf.data() + end, have - end);
    have -= end;
  }
  fflush(stdout);
  return 0;
}
