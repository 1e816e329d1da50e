// cfr_quant_cli.cpp — `centrifuger-quant`-compatible command line on top of cfr_quant_* (include/cfr_hip.h).
//
// Options of the reference (CentrifugerQuant.cpp:9-34): -x -c --min-score --min-length --output-format -h.  Added: --gpu N|none
// (default 0; none = the host twin, no GPU is touched) and -t INT (threads of the TSV reader).  The mode without -x
// (--taxonomy-tree / --name-table / --size-table) is not supported and says so.  The report goes to stdout, the log lines
// (Utils::PrintLog format) to stderr.
#include <getopt.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>

#include "../../include/cfr_hip.h"

static const char usage[] =
    "./centrifuger-quant [OPTIONS]:\n"
    "Required:\n"
    "\t-c FILE: classification result file (plain or gz; - for stdin)\n"
    "\t-x FILE: index prefix (reads FILE.2.cfr and FILE.3.cfr)\n"
    "Optional:\n"
    "\t--min-score INT: only consider reads with score at least <int> \n"
    "\t--min-length INT: only consider reads with classified length at least <int>\n"
    "\t--output-format INT: output format. (0:centrifuge,default, 1:metaphlan, 2:CAMI, 3:kraken-report)\n"
    "\t--gpu INT|none: GPU that coalesces the assignments and runs the E-step [0]; none: on the host\n"
    "\t-t INT: number of threads reading the classification file [up to 16]\n"
    "\t-h: print this usage message\n"
    "Not supported: --taxonomy-tree, --name-table, --size-table (quantification without -x)\n";

enum { ARG_TAXONOMY_TREE = 256, ARG_NAME_TABLE, ARG_SIZE_TABLE, ARG_MINSCORE, ARG_MINLENGTH, ARG_OUTPUT_FORMAT, ARG_GPU };
static const char *short_options = "x:c:t:h";
static struct option long_options[] = {{"taxonomy-tree", required_argument, 0, ARG_TAXONOMY_TREE},
                                       {"name-table", required_argument, 0, ARG_NAME_TABLE},
                                       {"size-table", required_argument, 0, ARG_SIZE_TABLE},
                                       {"min-score", required_argument, 0, ARG_MINSCORE},
                                       {"min-length", required_argument, 0, ARG_MINLENGTH},
                                       {"output-format", required_argument, 0, ARG_OUTPUT_FORMAT},
                                       {"gpu", required_argument, 0, ARG_GPU},
                                       {(char *)0, 0, 0, 0}};

static void print_log(const char *fmt, ...) {   // Utils::PrintLog (compactds/Utils.hpp:369-381)
  va_list args;
  va_start(args, fmt);
  char buffer[2048];
  vsnprintf(buffer, sizeof(buffer), fmt, args);
  va_end(args);
  time_t mytime = time(NULL);
  char stime[500];
  strftime(stime, sizeof(stime), "%c", localtime(&mytime));
  fprintf(stderr, "[%s] %s\n", stime, buffer);
}

int main(int argc, char *argv[]) {
  if (argc <= 1) { fprintf(stderr, "%s", usage); return 0; }
  std::string prefix, tsv;
  cfr_quant_options opt;
  cfr_quant_options_default(&opt);
  int format = 0, c, option_index = 0;
  while ((c = getopt_long(argc, argv, short_options, long_options, &option_index)) != -1) {
    if (c == 'x') prefix = optarg;
    else if (c == 'c') tsv = optarg;
    else if (c == 't') opt.threads = atoi(optarg);
    else if (c == ARG_MINSCORE) opt.min_score = (uint64_t)atoi(optarg);
    else if (c == ARG_MINLENGTH) opt.min_length = atoi(optarg);
    else if (c == ARG_OUTPUT_FORMAT) format = atoi(optarg);
    else if (c == ARG_GPU) {
      if (!strcmp(optarg, "none")) opt.device = -1;
      else {
        char *end = nullptr;
        long v = strtol(optarg, &end, 10);
        if (end == optarg || *end || v < 0) { fprintf(stderr, "centrifuger-quant: --gpu takes a device number or none, not '%s'\n", optarg); return EXIT_FAILURE; }
        opt.device = (int32_t)v;
      }
    } else if (c == ARG_TAXONOMY_TREE || c == ARG_NAME_TABLE || c == ARG_SIZE_TABLE) {
      fprintf(stderr, "centrifuger-quant: --%s is not supported: quantification needs an index prefix (-x)\n", long_options[option_index].name);
      return EXIT_FAILURE;
    } else if (c == 'h') { fprintf(stdout, "%s", usage); return 0; }
    else { fprintf(stderr, "%s", usage); return EXIT_FAILURE; }
  }
  print_log("Centrifuger-quant (%s) starts.", cfr_version());
  if (prefix.empty()) { print_log("Need to use -x to specify index prefix."); return EXIT_FAILURE; }
  if (tsv.empty()) { print_log("Need to use -c to specify the classification result file."); return EXIT_FAILURE; }
  if (format < 0 || format > 3) { print_log("Warning: unknown output format, will output in Centrifuger format."); format = 0; }

  cfr_quant *q = nullptr;
  auto fail = [&](const char *what) { print_log("%s: %s", what, cfr_last_error()); if (q) cfr_quant_destroy(q); return EXIT_FAILURE; };
  if (cfr_quant_open(prefix.c_str(), &opt, &q) != CFR_OK) return fail("cannot open the index");
  if (cfr_quant_add_tsv(q, tsv.c_str()) != CFR_OK) return fail("cannot read the classification result");
  print_log("Finish loading the read classification result.");
  int32_t rounds = 0;
  if (cfr_quant_run(q, &rounds) != CFR_OK) return fail("quantification failed");
  if (cfr_quant_write(q, format, "-") != CFR_OK) return fail("cannot write the report");
  cfr_quant_stats st;
  cfr_quant_get_stats(q, &st);
  cfr_quant_destroy(q);
  print_log("Centrifuger-quant finishes (%s; reader %.1f ms, coalesce %.1f ms, EM %d rounds in %.1f ms).", opt.device < 0 ? "host" : "device",
            st.reader_ms, st.coalesce_ms, (int)rounds, st.em_ms);
  return 0;
}
