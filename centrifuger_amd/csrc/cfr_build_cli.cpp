// cfr_build_cli.cpp — `centrifuger-build`-compatible command line on top of cfr_build_index (include/cfr_hip.h).
//
// Same option names as the reference's builder (CentrifugerBuild.cpp:34-52) for what the MI355X writer covers: nucleotide and protein
// references, sequence-level conversion tables or a two-column -l list (file name, tax id: the list is the conversion table, a file's
// base name is the name of all its records and they add into one genome), --subset-tax, --concat-tax-genome, default layout or
// --rbbwt-b / --offrate / --ftabchars.  --bmax / --dcv / --build-mem steer the reference's blockwise sorter (FMBuilder.hpp:444-811) and
// have no meaning here (the suffix array is built in HBM): accepted and ignored.  --protein writes the amino-acid index
// (FMIndex<Sequence_RunBlockOneTree>, '$' behind every sequence).  --checkpoint is rejected with a message.
// The front end: the files are read front to back (gzread: gz or plain) in chunks and handed to cfr_refseq_feed - nucleotide input to
// the kernels of cfr_refseq.hip on the GPU that sorts the suffixes, --protein to the host twin; the input decides.  The handle drops
// what the index does not keep and delivers one record per header; cfr_build_select turns the records into genomes (Builder::Build,
// Builder.hpp:104-211, and Taxonomy::ReadSeqNameFile, Taxonomy.hpp:303-368): a conversion table may name sequences the FASTA does not
// hold (they keep their ids and tax ids in .2.cfr, have no length in .3.cfr); a FASTA sequence the table does not name is added as an
// extra name with a warning (or skipped under --ignore-uncategorized-genome); a repeated sequence id is taken once; a sequence shorter
// than --ftabchars + 1 after dropping non-ACGT characters is filtered with a warning; a name listed twice in the table gets the lowest
// common ancestor of its tax ids; --subset-tax keeps the records under one node; --concat-tax-genome makes one genome per tax id.
// cfr_refseq_assemble then writes the text of the index in HBM, and cfr_build_index_assembled sorts it where it lies.
#include <getopt.h>
#include <zlib.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <string>
#include <vector>

#include "../../include/cfr_hip.h"

namespace {

const char *kUsage =
    "./centrifuger-build [OPTIONS]:\n"
    "Required:\n"
    "\t-r FILE: reference sequence file (can use multiple -r to specify more than one input file)\n"
    "\t\tor\n"
    "\t-l FILE: list of reference sequence file stored in <file>, one sequence file per row. Can be a two-column file, where the second column is the taxonomy ID of the file.\n"
    "\t--taxonomy-tree FILE: taxonomy tree, i.e., nodes.dmp file\n"
    "\t--name-table FILE: name table, i.e., names.dmp file\n"
    "\t--conversion-table FILE: a table that converts reference sequence id to taxonomy id. No need for this if -l is a two-column file\n"
    "Optional:\n"
    "\t-o STRING: output prefix [centrifuger]\n"
    "\t-t INT: number of host threads [automatic]\n"
    "\t--offrate INT: SA/offset is sampled every (2^<int>) BWT chars [4]\n"
    "\t--ftabchars INT: # of chars consumed in initial lookup [10]\n"
    "\t--rbbwt-b INT: block size for run-block compressed BWT. 0 for auto. 1 for no compression [0]\n"
    "\t--protein: the input is protein sequences [off]\n"
    "\t--subset-tax INT: only consider the subset of input genomes under taxonomy node INT [0]\n"
    "\t--concat-tax-genome: concatenate the genomes with the same taxID and discard the seqID information [not used]\n"
    "\t--ignore-uncategorized-genome: do not index a sequence that is missing from the conversion table\n"
    "\t--gpu INT: MI355X ordinal that builds the suffix array [0]\n"
    "\t--bmax / --dcv / --build-mem: accepted and ignored (they steer the reference's blockwise sorter)\n"
    "\t-h: print this usage message\n";

enum { O_BMAX = 1000, O_DCV, O_MEM, O_OFFRATE, O_FTAB, O_RBB, O_TREE, O_CONV, O_NAMES, O_GPU, O_IGNORE_UNCAT, O_PROTEIN, O_SUBSET, O_CONCAT, O_UNSUPPORTED };

void print_log(const char *fmt, ...) {
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

std::vector<std::string> split_dmp(const std::string &line) {     // "a\t|\tb\t|\t..." -> fields, blanks trimmed
  std::vector<std::string> f;
  size_t at = 0;
  for (;;) {
    const size_t bar = line.find('|', at);
    std::string x = line.substr(at, bar == std::string::npos ? std::string::npos : bar - at);
    const size_t a = x.find_first_not_of(" \t\r\n"), b = x.find_last_not_of(" \t\r\n");
    f.push_back(a == std::string::npos ? "" : x.substr(a, b - a + 1));
    if (bar == std::string::npos) break;
    at = bar + 1;
  }
  return f;
}

bool read_lines(const char *path, std::vector<std::string> &lines) {
  gzFile fp = gzopen(path, "r");
  if (!fp) return false;
  std::string cur;
  char buf[1 << 16];
  int got;
  while ((got = gzread(fp, buf, sizeof(buf))) > 0) {
    for (int i = 0; i < got; ++i) {
      if (buf[i] == '\n') { lines.push_back(cur); cur.clear(); }
      else cur += buf[i];
    }
  }
  if (!cur.empty()) lines.push_back(cur);
  gzclose(fp);
  return true;
}

}  // namespace

int main(int argc, char *argv[]) {
  if (argc <= 1) { fprintf(stderr, "%s", kUsage); return 0; }
  static const char *short_options = "r:l:o:t:h";
  static struct option long_options[] = {
      {"bmax", required_argument, 0, O_BMAX}, {"dcv", required_argument, 0, O_DCV}, {"build-mem", required_argument, 0, O_MEM},
      {"offrate", required_argument, 0, O_OFFRATE}, {"ftabchars", required_argument, 0, O_FTAB}, {"rbbwt-b", required_argument, 0, O_RBB},
      {"taxonomy-tree", required_argument, 0, O_TREE}, {"conversion-table", required_argument, 0, O_CONV}, {"name-table", required_argument, 0, O_NAMES},
      {"gpu", required_argument, 0, O_GPU}, {"subset-tax", required_argument, 0, O_SUBSET}, {"concat-tax-genome", no_argument, 0, O_CONCAT},
      {"checkpoint", no_argument, 0, O_UNSUPPORTED}, {"protein", no_argument, 0, O_PROTEIN},
      {"ignore-uncategorized-genome", no_argument, 0, O_IGNORE_UNCAT}, {0, 0, 0, 0}};
  std::vector<std::string> fasta;
  std::string out_prefix = "centrifuger", tree, names_dmp, conv, file_list;
  bool ignore_uncategorized = false, ftab_given = false, concat = false;
  int list_columns = 0;
  unsigned long subset_tax = 0;
  cfr_build_options opt;
  cfr_build_options_default(&opt);
  opt.verbose = 1;
  int c, option_index = 0;
  while ((c = getopt_long(argc, argv, short_options, long_options, &option_index)) != -1) {
    switch (c) {
      case 'r': fasta.push_back(optarg); break;
      case 'l': {
        std::vector<std::string> lines;
        if (!read_lines(optarg, lines)) { print_log("ERROR: cannot open %s", optarg); return EXIT_FAILURE; }
        file_list = optarg;
        for (const std::string &ln : lines) {
          char name[4096];
          if (sscanf(ln.c_str(), "%4095s", name) != 1) continue;
          fasta.push_back(name);
          if (list_columns == 0) {      // the first row decides (CentrifugerBuild.cpp:106-112): one more column per blank or tab
            list_columns = 1;
            for (char ch : ln) if (ch == ' ' || ch == '\t') ++list_columns;
          }
        }
        break;
      }
      case 'o': out_prefix = optarg; break;
      case 't': opt.threads = atoi(optarg); break;
      case 'h': fprintf(stderr, "%s", kUsage); return 0;
      case O_BMAX: case O_DCV: case O_MEM: break;
      case O_OFFRATE: opt.offrate = atoi(optarg); break;
      case O_FTAB: opt.ftab_chars = atoi(optarg); ftab_given = true; break;
      case O_RBB: opt.rbbwt_b = strtoull(optarg, nullptr, 10); break;
      case O_TREE: tree = optarg; break;
      case O_CONV: conv = optarg; break;
      case O_NAMES: names_dmp = optarg; break;
      case O_GPU: opt.device = atoi(optarg); break;
      case O_IGNORE_UNCAT: ignore_uncategorized = true; break;
      case O_PROTEIN: opt.protein = 1; break;
      case O_SUBSET: sscanf(optarg, "%lu", &subset_tax); break;
      case O_CONCAT: concat = true; break;
      case O_UNSUPPORTED:
        print_log("ERROR: option --%s belongs to a part of centrifuger-build outside the MI355X writer and is not available in this build.",
                  long_options[option_index].name);
        return EXIT_FAILURE;
      default: fprintf(stderr, "%s", kUsage); return EXIT_FAILURE;
    }
  }
  // --protein: alphabet "$ARNDCEQGHILKMFPSTWYV", 4 characters in the initial lookup unless --ftabchars says otherwise (CentrifugerBuild.cpp:221-227:
  // the reference tests "width == 10", so an explicit --ftabchars 10 becomes 4 there too)
  if (opt.protein && (!ftab_given || opt.ftab_chars == 10)) opt.ftab_chars = 4;
  if (fasta.empty()) { print_log("Need to use -r/-l to specify the reference sequences."); return EXIT_FAILURE; }
  if (tree.empty() || names_dmp.empty()) { print_log("Need to use --taxonomy-tree, --name-table and --conversion-table."); return EXIT_FAILURE; }
  // without --conversion-table a two-column -l list is the table, at file level (CentrifugerBuild.cpp:200-212)
  const bool file_level = conv.empty();
  if (file_level && (file_list.empty() || list_columns < 2)) {
    fprintf(stderr, "Should use two-column file to specify the file name to taxonomy id mapping through the \"-l\" option. Otherwise, need to use --conversion-table to specify sequence id to taxonomy id mapping.\n");
    return EXIT_FAILURE;
  }
  if (file_level) conv = file_list;

  // ---- taxonomy files (Taxonomy::Init, Taxonomy.hpp:146-180)
  std::vector<uint64_t> node_taxid, node_parent, name_taxid, seq_taxid, present_taxid;
  std::vector<std::string> node_rank, name_text, seq_name;
  {
    std::vector<std::string> lines;
    if (!read_lines(tree.c_str(), lines)) { print_log("ERROR: cannot open %s", tree.c_str()); return EXIT_FAILURE; }
    for (const std::string &ln : lines) {
      if (ln.empty() || ln[0] == '#') continue;
      const auto f = split_dmp(ln);
      if (f.size() < 3) continue;
      node_taxid.push_back(strtoull(f[0].c_str(), nullptr, 10));
      node_parent.push_back(strtoull(f[1].c_str(), nullptr, 10));
      node_rank.push_back(f[2]);
    }
    lines.clear();
    if (!read_lines(names_dmp.c_str(), lines)) { print_log("ERROR: cannot open %s", names_dmp.c_str()); return EXIT_FAILURE; }
    for (const std::string &ln : lines) {
      if (ln.find("scientific name") == std::string::npos) continue;
      const auto f = split_dmp(ln);
      if (f.size() < 2) continue;
      name_taxid.push_back(strtoull(f[0].c_str(), nullptr, 10));
      name_text.push_back(f[1]);
    }
    lines.clear();
    if (!read_lines(conv.c_str(), lines)) { print_log("ERROR: cannot open %s", conv.c_str()); return EXIT_FAILURE; }
    // a name listed with two tax ids keeps their lowest common ancestor (Taxonomy.hpp:327-352): lineages to the root, compared
    // from the root down; the root itself when even the top nodes differ
    std::map<uint64_t, uint64_t> parent_of;
    for (size_t i = 0; i < node_taxid.size(); ++i) parent_of.emplace(node_taxid[i], node_parent[i]);
    auto lineage = [&](uint64_t t) {
      std::vector<uint64_t> path;
      for (size_t guard = 0; guard <= parent_of.size(); ++guard) {
        path.push_back(t);
        auto it = parent_of.find(t);
        if (it == parent_of.end() || it->second == t) break;
        t = it->second;
      }
      return path;
    };
    uint64_t tree_root = 1;                  // Taxonomy::FindRoot (Taxonomy.hpp:426-433): the first node that is its own parent
    for (const auto &kv : parent_of) if (kv.second == kv.first) { tree_root = kv.first; break; }
    std::map<std::string, size_t> first_at;
    for (const std::string &ln : lines) {   // (every tax id the table mentions keeps its lineage in the tree, Taxonomy.hpp:275-300)
      if (ln.empty() || ln[0] == '#') continue;
      char nm[4096];
      unsigned long long tid;
      if (sscanf(ln.c_str(), "%4095s %llu", nm, &tid) != 2) continue;
      if (file_level) { char base[4096]; cfr_file_base_name(nm, base, sizeof(base)); memcpy(nm, base, sizeof(base)); }      // (Taxonomy.hpp:319-324)
      present_taxid.push_back(tid);
      auto it = first_at.find(nm);
      if (it == first_at.end()) {
        first_at.emplace(nm, seq_name.size());
        seq_name.push_back(nm);
        seq_taxid.push_back(tid);
      } else {
        // (an id the tree does not hold has the root as its whole lineage there, Taxonomy.hpp:977-984, and two lineages that part
        // at the very top meet in the root, :345-348)
        const uint64_t a = seq_taxid[it->second];
        if (!parent_of.count(a) || !parent_of.count(tid)) seq_taxid[it->second] = tree_root;
        else {
          const auto pa = lineage(a), pb = lineage(tid);
          long i = (long)pa.size() - 1, j = (long)pb.size() - 1;
          for (; i >= 0 && j >= 0; --i, --j) if (pa[(size_t)i] != pb[(size_t)j]) break;
          seq_taxid[it->second] = (i == (long)pa.size() - 1) ? tree_root : pa[(size_t)i + 1];
        }
      }
    }
  }
  const size_t n_table = seq_name.size();

  // ---- sequences: the bytes of every file, in chunks, to the front end (cfr_refseq_core.hpp); what comes back is one record per header
  // with the place of its kept symbols in the stream U.  The reader is sequential (gzread reads plain files too).
  cfr_refseq *rs = nullptr;
  if (cfr_refseq_open(opt.protein ? -1 : opt.device, opt.protein, &rs) != CFR_OK) { print_log("ERROR: %s", cfr_last_error()); return EXIT_FAILURE; }
  struct timespec ts0, ts1;
  clock_gettime(CLOCK_MONOTONIC, &ts0);
  std::vector<std::string> rec_id;
  std::vector<uint32_t> rec_file;
  std::vector<cfr_select_record> recs;
  std::vector<cfr_select_piece> pieces;
  {
    size_t chunk = (size_t)1 << 27;
    // (test hook, behind CFR_DEBUG_ENV like the writer's other hooks: small chunks make small files take many of them)
    if (getenv("CFR_DEBUG_ENV") && atoi(getenv("CFR_DEBUG_ENV")) && getenv("CFR_REFSEQ_CHUNK_LOG2")) chunk = (size_t)1 << std::min(31, std::max(6, atoi(getenv("CFR_REFSEQ_CHUNK_LOG2"))));
    uint8_t *buf = opt.protein ? nullptr : (uint8_t *)cfr_host_alloc(chunk);      // pinned for the copy to the device
    const bool pinned = buf != nullptr;
    if (!buf) buf = (uint8_t *)malloc(chunk);
    if (!buf) { print_log("ERROR: out of memory"); return EXIT_FAILURE; }
    auto done = [&](int rc) { if (pinned) cfr_host_free(buf); else free(buf); return rc; };
    std::vector<cfr_refseq_record> chunk_recs;
    for (size_t fi = 0; fi < fasta.size(); ++fi) {
      gzFile fp = gzopen(fasta[fi].c_str(), "r");
      if (!fp) { print_log("ERROR: cannot open %s", fasta[fi].c_str()); return done(EXIT_FAILURE); }
      gzbuffer(fp, 1 << 20);
      size_t have = 0;
      int line_start = 1;
      bool eof = false, file_has_record = false;
      while (!eof) {
        while (have < chunk) {
          const int got = gzread(fp, buf + have, (unsigned)std::min<size_t>(chunk - have, (size_t)1 << 30));
          if (got < 0) { print_log("ERROR: cannot read %s", fasta[fi].c_str()); gzclose(fp); return done(EXIT_FAILURE); }
          if (got == 0) { eof = true; break; }
          have += (size_t)got;
        }
        cfr_refseq_info info;
        if (cfr_refseq_feed(rs, buf, have, line_start, eof ? 1 : 0, &info) != CFR_OK) { print_log("ERROR: %s: %s", fasta[fi].c_str(), cfr_last_error()); gzclose(fp); return done(EXIT_FAILURE); }
        chunk_recs.resize(info.n_records);
        if (info.n_records && cfr_refseq_fetch(rs, chunk_recs.data()) != CFR_OK) { print_log("ERROR: %s", cfr_last_error()); gzclose(fp); return done(EXIT_FAILURE); }
        uint64_t src = info.u_start;
        if (info.lead_kept && file_has_record) { pieces.push_back(cfr_select_piece{src, info.lead_kept}); ++recs.back().n_pieces; }   // (bytes before a file's first header belong to no record)
        src += info.lead_kept;
        for (const cfr_refseq_record &r : chunk_recs) {
          rec_id.emplace_back((const char *)buf + r.header + 1, r.id_len);
          rec_file.push_back((uint32_t)fi);
          recs.push_back(cfr_select_record{nullptr, nullptr, pieces.size(), 0});
          if (r.kept) { pieces.push_back(cfr_select_piece{src, r.kept}); recs.back().n_pieces = 1; }
          src += r.kept;
          file_has_record = true;
        }
        have -= (size_t)info.consumed;
        if (have) memmove(buf, buf + info.consumed, have);
        line_start = info.at_line_start;
      }
      gzclose(fp);
    }
    done(0);
  }
  for (size_t k = 0; k < recs.size(); ++k) { recs[k].id = rec_id[k].c_str(); recs[k].file = fasta[rec_file[k]].c_str(); }
  seq_taxid.resize(seq_name.size(), 0);

  auto cptrs = [](const std::vector<std::string> &v) { std::vector<const char *> p; for (const auto &s : v) p.push_back(s.c_str()); return p; };
  const auto p_seq = cptrs(seq_name), p_rank = cptrs(node_rank), p_names = cptrs(name_text);
  cfr_build_input in;
  memset(&in, 0, sizeof(in));
  in.n_seqs = seq_name.size(); in.seq_names = p_seq.data(); in.seq_taxids = seq_taxid.data();
  in.n_present_taxids = present_taxid.size(); in.present_taxids = present_taxid.data();
  in.n_nodes = node_taxid.size(); in.node_taxid = node_taxid.data(); in.node_parent = node_parent.data(); in.node_rank = p_rank.data();
  in.n_names = name_taxid.size(); in.name_taxid = name_taxid.data(); in.name_text = p_names.data();
  // ---- which records become which genomes, and where their symbols go in the text
  cfr_select_options so;
  memset(&so, 0, sizeof(so));
  so.file_level = file_level; so.concat_tax_genome = concat; so.ignore_uncategorized = ignore_uncategorized; so.protein = opt.protein;
  so.subset_tax = subset_tax; so.ftab_chars = opt.ftab_chars;
  cfr_build_selection *sel = nullptr;
  if (cfr_build_select(&in, &so, recs.data(), recs.size(), pieces.data(), pieces.size(), &sel) != CFR_OK) {
    const std::string why = cfr_last_error();
    if (why.find("found 0 genomes") != std::string::npos) fprintf(stderr, "ERROR: %s\n", why.c_str());      // (the reference's words, Builder.hpp:218-222)
    else print_log("ERROR: %s", why.c_str());
    return EXIT_FAILURE;
  }
  const cfr_refseq_segment *segs = nullptr;
  uint64_t n_segs = 0, n_text = 0, n_genomes = 0, n_extra = 0;
  cfr_build_selection_get(sel, &segs, &n_segs, &n_text, &n_genomes, &n_extra);
  if (cfr_refseq_assemble(rs, segs, n_segs, n_text) != CFR_OK) { print_log("ERROR: %s", cfr_last_error()); return EXIT_FAILURE; }
  clock_gettime(CLOCK_MONOTONIC, &ts1);
  cfr_refseq_stats rst;
  cfr_refseq_get_stats(rs, &rst);
  print_log("Read %lu sequences, %lu bases (%lu names in the conversion table, %lu extra names).", (unsigned long)n_genomes,
            (unsigned long)n_text, (unsigned long)n_table, (unsigned long)n_extra);
  print_log("Front end: %.3f s (%lu records; filter %.3f s of which copy in %.3f s, assemble %.3f s).", (double)(ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double)(ts1.tv_nsec - ts0.tv_nsec),
            (unsigned long)recs.size(), rst.feed_ms * 1e-3, rst.copy_in_ms * 1e-3, rst.assemble_ms * 1e-3);
  in.selection = sel;
  cfr_build_report rep;
  const cfr_status st = cfr_build_index_assembled(rs, &in, &opt, out_prefix.c_str(), &rep);
  cfr_build_selection_free(sel);
  cfr_refseq_close(rs);
  if (st != CFR_OK) { print_log("ERROR: index build failed (status %d): %s", st, cfr_last_error()); return EXIT_FAILURE; }
  print_log("Index of %lu bases written to %s.*.cfr (run-block size %lu, suffix array %.1f s, total %.1f s).", (unsigned long)rep.n, out_prefix.c_str(),
            (unsigned long)rep.block_size, rep.seconds_sa, rep.seconds_total);
  return 0;
}
