// cfr_kreport_cli.cpp — `centrifuger-kreport`-compatible command line on top of cfr_kreport_* (include/cfr_hip.h).
//
// Options and positionals of the reference's Perl script: -x INDEX (required: without it the usage text and exit 64), --no-lca,
// --show-zeros, --is-count-table, --min-score, --min-length, --report-score-data, --help; one classification file, plain or gz, or
// stdin.  Added: --gpu N|none (default 0; none = the host twin, no GPU is touched) and -t INT (threads of the host twin).
// Stdout is the script's byte for byte; stderr carries its "Couldn't find parent of taxID ..." lines in its order (its "Loading ..."
// lines are not reproduced).  --no-lca and --is-count-table add fractions in file order and run on the host for every --gpu.
// Differences (csrc/cfr_kreport_core.hpp): more than one file is refused, and so is an index without a node of tax id 1.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cfr_hip.h"

static const char usage_text[] =
    "\nUsage: centrifuger-kreport -x <index name> OPTIONS <centrifuge output file(s)>\n\n"
    "centrifuger-kreport creates Kraken-style reports from centrifuge out files.\n\n"
    "Options:\n"
    "    -x INDEX            (REQUIRED) Centrifuge index\n\n"
    "    --no-lca             Do not report the LCA of multiple assignments, but report count fractions at the taxa.\n"
    "    --show-zeros         Show clades that have zero reads, too\n"
    "    --is-count-table     The format of the file is 'taxID<tab>COUNT' instead of the standard\n"
    "                         Centrifuge output format\n\n"
    "    --min-score SCORE    Require a minimum score for reads to be counted\n"
    "    --min-length LENGTH  Require a minimum alignment length to the read\n"
    "    --report-score-data  Output an extra column summarizing classification scores and other details \n\n"
    "    --gpu INT|none       GPU that counts the reads [0]; none: on the host\n"
    "    -t INT               threads of the host twin [up to 16]\n"
    "One file, plain or gz, or standard input.\n";

static int usage(int code) {
  fprintf(stderr, "%s", usage_text);
  return code;
}

enum { ARG_GPU = 256, ARG_NO_LCA, ARG_SHOW_ZEROS, ARG_COUNT_TABLE, ARG_MIN_SCORE, ARG_MIN_LENGTH, ARG_SCORE_DATA, ARG_HELP };

int main(int argc, char *argv[]) {
  static struct option long_options[] = {{"gpu", required_argument, 0, ARG_GPU},
                                         {"no-lca", no_argument, 0, ARG_NO_LCA},
                                         {"show-zeros", no_argument, 0, ARG_SHOW_ZEROS},
                                         {"is-count-table", no_argument, 0, ARG_COUNT_TABLE},
                                         {"min-score", required_argument, 0, ARG_MIN_SCORE},
                                         {"min-length", required_argument, 0, ARG_MIN_LENGTH},
                                         {"report-score-data", no_argument, 0, ARG_SCORE_DATA},
                                         {"help", no_argument, 0, ARG_HELP},
                                         {(char *)0, 0, 0, 0}};
  cfr_kreport_options opt;
  cfr_kreport_options_default(&opt);
  std::string prefix;
  bool have_prefix = false, count_table = false;
  int device = 0, c;
  opterr = 0;
  while ((c = getopt_long(argc, argv, "x:t:h", long_options, nullptr)) != -1) {
    if (c == 'x') { prefix = optarg; have_prefix = true; }
    else if (c == 't') opt.threads = atoi(optarg);
    else if (c == 'h' || c == ARG_HELP) return usage(0);
    else if (c == ARG_NO_LCA) opt.no_lca = 1;
    else if (c == ARG_SHOW_ZEROS) opt.show_zeros = 1;
    else if (c == ARG_COUNT_TABLE) count_table = true;
    else if (c == ARG_SCORE_DATA) opt.score_data = 1;
    else if (c == ARG_MIN_SCORE || c == ARG_MIN_LENGTH) {
      char *end = nullptr;
      const long long v = strtoll(optarg, &end, 10);
      if (end == optarg || *end) { fprintf(stderr, "Value \"%s\" invalid for option %s (number expected)\n", optarg, c == ARG_MIN_SCORE ? "min-score" : "min-length"); return usage(64); }
      if (c == ARG_MIN_SCORE) { opt.has_min_score = 1; opt.min_score = v < 0 ? 0 : (uint64_t)v; }      // (no score is below 0)
      else { opt.has_min_length = 1; opt.min_length = v; }
    } else if (c == ARG_GPU) {
      if (!strcmp(optarg, "none")) device = -1;
      else {
        char *end = nullptr;
        long v = strtol(optarg, &end, 10);
        if (end == optarg || *end || v < 0) { fprintf(stderr, "centrifuger-kreport: --gpu takes a device number or none, not '%s'\n", optarg); return EXIT_FAILURE; }
        device = (int)v;
      }
    } else return usage(64);
  }
  if (!have_prefix) return usage(64);
  if (argc - optind > 1) {
    fprintf(stderr, "centrifuger-kreport: one classification file at a time (the header line of a second file would be counted as a row)\n");
    return EXIT_FAILURE;
  }
  const std::string input = argc - optind == 1 ? argv[optind] : "-";
  if (count_table || opt.no_lca) {
    if (device >= 0) fprintf(stderr, "centrifuger-kreport: %s adds fractions in file order: it runs on the host\n", count_table ? "--is-count-table" : "--no-lca");
    device = -1;
  }

  struct Open {
    cfr_kreport *k = nullptr;
    ~Open() { if (k) cfr_kreport_close(k); }
  } open;
  if (cfr_kreport_open(prefix.c_str(), &opt, device, &open.k) != CFR_OK) { fprintf(stderr, "centrifuger-kreport: %s\n", cfr_last_error()); return EXIT_FAILURE; }
  const cfr_status st = count_table ? cfr_kreport_add_count_table(open.k, input.c_str()) : cfr_kreport_add_tsv(open.k, input.c_str());
  const std::string add_error = st != CFR_OK ? cfr_last_error() : "";
  // the script prints its lines while it reads: whatever was read before a failure has printed them
  size_t nw = 0;
  std::vector<uint64_t> warn;
  if (cfr_kreport_warnings(open.k, nullptr, 0, &nw) == CFR_ERR_CAPACITY) { warn.resize(nw); cfr_kreport_warnings(open.k, warn.data(), nw, &nw); }
  for (size_t i = 0; i < nw; ++i) fprintf(stderr, "Couldn't find parent of taxID %lu - directly assigned to root.\n", (unsigned long)warn[i]);
  if (st != CFR_OK) { fprintf(stderr, "centrifuger-kreport: %s\n", add_error.c_str()); return EXIT_FAILURE; }
  if (cfr_kreport_write(open.k, nullptr) != CFR_OK) {
    const char *msg = cfr_last_error();
    if (!strncmp(msg, "No sequence matches", 19)) { fprintf(stderr, "%s at centrifuger-kreport.\n", msg); return 255; }     // (Perl's die: 255)
    fprintf(stderr, "centrifuger-kreport: %s\n", msg);
    return EXIT_FAILURE;
  }
  return 0;
}
