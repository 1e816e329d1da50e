// cfr_inspect_cli.cpp — `centrifuger-inspect`-compatible command line on top of cfr_taxonomy_* (include/cfr_hip.h).  Host only.
//
// Options of the reference (CentrifugerInspect.cpp:10-35): -x, --summary, --seq-name, --conversion-table, --taxonomy-tree,
// --name-table, --size-table, -h; the last item given counts.  Stdout is the reference's byte for byte (:96-135,
// Taxonomy.hpp:1289-1313).  Reads <prefix>.2.cfr and <prefix>.3.cfr only, never .1.cfr.  --seq-name prints nothing, as there.
// Differences: a missing or malformed index file is a message and a non-zero exit (the reference dereferences a null FILE *), and
// --index-size is refused: it prints the sizes of the reference's in-memory structures (FMIndex::PrintSpace), which this project's
// image does not have.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/cfr_hip.h"

static const char usage[] =
    "./centrifuger-inspect [OPTIONS]:\n"
    "Required:\n"
    "\t-x STRING: index prefix\n"
    "One of:\n"
    "\t--summary: print the summary information for each strain in the database\n"
    "\t--conversion-table: print the seqID to taxonomy ID translation information\n"
    "\t--taxonomy-tree: print the taxonomy tree\n"
    "\t--name-table: print the scientific name for each strain in the database\n"
    "\t--size-table: print the lengths of the sequences belonging to the same taxonomic ID\n"
    "\t-h: print this usage message\n"
    "Not supported: --index-size (the sizes of the reference's in-memory FM index structures)\n";

enum { ARG_SUMMARY = 256, ARG_SEQNAME, ARG_CONVERSION_TABLE, ARG_TAXONOMY_TREE, ARG_NAME_TABLE, ARG_SIZE_TABLE, ARG_INDEXSIZE };
static const char *short_options = "x:h";
static struct option long_options[] = {{"summary", no_argument, 0, ARG_SUMMARY},
                                       {"seq-name", no_argument, 0, ARG_SEQNAME},
                                       {"conversion-table", no_argument, 0, ARG_CONVERSION_TABLE},
                                       {"taxonomy-tree", no_argument, 0, ARG_TAXONOMY_TREE},
                                       {"name-table", no_argument, 0, ARG_NAME_TABLE},
                                       {"size-table", no_argument, 0, ARG_SIZE_TABLE},
                                       {"index-size", no_argument, 0, ARG_INDEXSIZE},
                                       {(char *)0, 0, 0, 0}};

int main(int argc, char *argv[]) {
  std::string prefix;
  bool have_prefix = false;
  int item = -1, c, option_index = 0;
  while ((c = getopt_long(argc, argv, short_options, long_options, &option_index)) != -1) {
    if (c == 'x') { prefix = optarg; have_prefix = true; }
    else if (c == 'h') { fprintf(stdout, "%s", usage); return 0; }
    else if (c == '?') { fprintf(stderr, "%s", usage); return EXIT_FAILURE; }
    else item = c;
  }
  if (item == ARG_INDEXSIZE) {
    fprintf(stderr, "centrifuger-inspect: --index-size is not supported: it prints the sizes of the reference's in-memory FM index structures, which this build does not have\n");
    return EXIT_FAILURE;
  }
  if (!have_prefix) { fprintf(stderr, "Need -x to specify index.\n%s", usage); return EXIT_FAILURE; }
  if (item == -1) { fprintf(stderr, "Use inspect options from %s", usage); return EXIT_FAILURE; }

  cfr_taxonomy *t = nullptr;
  if (cfr_taxonomy_open(prefix.c_str(), 1, &t) != CFR_OK) {
    fprintf(stderr, "centrifuger-inspect: cannot read the index %s: %s\n", prefix.c_str(), cfr_last_error());
    return EXIT_FAILURE;
  }
  cfr_taxonomy_tables T;
  cfr_taxonomy_get_tables(t, &T);
  auto seq_tax = [&](uint64_t id) { return id < T.seq_cnt ? T.seq_to_tax[id] : T.node_cnt; };        // Taxonomy::SeqIdToTaxId
  auto orig = [&](uint64_t ctid) { return (unsigned long)T.orig_taxid[ctid < T.node_cnt ? ctid : T.root]; };   // GetOrigTaxId

  if (item == ARG_SUMMARY) {
    for (uint64_t k = 0; k < T.n_seq_lengths; ++k) {
      const uint64_t id = T.length_seq_id[k], ctid = seq_tax(id);
      const char *name = cfr_taxonomy_seq_name(t, id);
      fprintf(stdout, "%s\t%lu\t%lu\t%s\n", name ? name : "", orig(ctid), (unsigned long)T.length_value[k], cfr_taxonomy_tax_name(t, ctid));
    }
  } else if (item == ARG_CONVERSION_TABLE) {
    for (uint64_t i = 0; i < T.n_seq_names; ++i) fprintf(stdout, "%s\t%lu\n", cfr_taxonomy_seq_name(t, i), orig(seq_tax(i)));
  } else if (item == ARG_TAXONOMY_TREE) {
    for (uint64_t i = 0; i < T.node_cnt; ++i) fprintf(stdout, "%lu\t|\t%lu\t|\t%s\t|\n", orig(i), orig(T.parent[i]), cfr_tax_rank_string(T.rank[i]));
  } else if (item == ARG_NAME_TABLE) {
    for (uint64_t i = 0; i < T.node_cnt; ++i) fprintf(stdout, "%lu\t|\t%s\t|\tscientific name\t|\n", orig(i), cfr_taxonomy_tax_name(t, i));
  } else if (item == ARG_SIZE_TABLE) {
    for (uint64_t i = 0; i < T.node_cnt; ++i)
      if (T.taxid_length[i] != 0) fprintf(stdout, "%lu\t%lu\n", orig(i), (unsigned long)T.taxid_length[i]);
  }                                        // (--seq-name: nothing, CentrifugerInspect.cpp:92-95)
  cfr_taxonomy_close(t);
  return 0;
}
