// cfr_cli.cpp — `centrifuger`-compatible command line on top of the C-ABI (include/cfr_hip.h).
//
// Drop-in for the reference's classification driver (CentrifugerClass.cpp:342-968) for the options that
// touch the accelerated path: same option names, same TSV on stdout (ResultWriter.hpp:186-242), same
// --un/--cl read dumps, same stderr summary lines.  What the reference does with
// pthread_create(ClassifyReads_Thread) per batch (CentrifugerClass.cpp:681-688) is one
// cfr_classify_batch call per batch here; batches round-robin over the GPUs given by --gpu, output stays
// in input order.  --merge-readpair (CentrifugerClass.cpp:256-335) merges the pairs on the device inside
// cfr_classify_batch_merged (on the host when --un / --cl need the reads).  Additive options: --gpu LIST|all,
// --gpu-batch N, --gpu-throughput, --quant FILE, and --promote LEVEL (cfr_device_index_set_promote: what centrifuger-promote does
// to the output afterwards, done in HBM before the rows are written), and --gpu-parse (plain files are handed to the device workers as
// unparsed pieces; cfr_tokenize makes the flat reads in HBM and cfr_classify_batch_resident takes them from there).  The single-cell
// options (--barcode, --UMI, --read-format, --barcode-whitelist, --barcode-translate; CentrifugerClass.cpp:457-466, 516-590) are
// implemented; --sample-sheet is outside this build and is rejected with a message instead of being silently ignored.
//
// Layout: reading the read files is cfr_cli_reads.hpp.  Here: parse_options, the parser self-test hook (run_parse_only), BatchQueue,
// the single-cell steps, one function or struct per stage (Reader, dust_stage, DeviceWorker, format_stage, write_stage), and main.
#include <getopt.h>
#include <cerrno>

#include <chrono>
#include <functional>
#include <iostream>
#include <memory>

#include "cfr_cli_reads.hpp"

namespace {

const char *kUsage =
    "./centrifuger [OPTIONS] > output.tsv:\n"
    "Required:\n"
    "\t-x FILE: index prefix\n"
    "\t-1 FILE -2 FILE: paired-end read\n"
    "\t\tor\n"
    "\t-u FILE: single-end read\n"
    "\t\tor\n"
    "\t-i FILE: interleaved read file\n"
    "Optional:\n"
    "\t-t INT: number of host threads (dust masking, TSV formatting) [1]\n"
    "\t-k INT: report upto <int> distinct, primary assignments for each read pair [1]\n"
    "\t--un STR: output unclassified reads to files with the prefix of <str>\n"
    "\t--cl STR: output classified reads to files with the prefix of <str>\n"
    "\t--no-dust: do not DUST-mask low-complexity regions of reads [mask]\n"
    "\t--merge-readpair: merge overlapped paired-end reads and trim adapters [no merge]\n"
    "\t--min-hitlen INT: minimum length of partial hits [auto]\n"
    "\t--hitk-factor INT: resolve at most <int>*k entries for each hit [40; use 0 for no restriction]\n"
    "\t--consider-secondary STR: in the format INT,FLOAT consider the secondary hit if its hitlen>=INT,score>=FLOAT*best_score [2000,0.995]\n"
    "\t--expand-taxid: output the tax IDs that are promoted to the final report tax ID [no]\n"
    "\t--barcode STR: path to the barcode file\n"
    "\t--UMI STR: path to the UMI file\n"
    "\t--read-format STR: format for read, barcode and UMI files, e.g. r1:0:-1,r2:0:-1,bc:0:15,um:16:-1 for paired-end files with barcode and UMI\n"
    "\t--barcode-whitelist STR: path to the barcode whitelist file\n"
    "\t--barcode-translate STR: path to the barcode translation file\n"
    "\t--quant FILE: also write the abundance report of centrifuger-quant for this run to FILE (equal to centrifuger-quant -x IDX -c\n"
    "\t\tthis output, when no two adjacent reads share a read id: there every read is an assignment of its own) [no report]\n"
    "\t--quant-format INT: format of that report (0:centrifuge, 1:metaphlan, 2:CAMI, 3:kraken-report) [0]\n"
    "\t--promote STR: promote every assignment to the rank <str> (genus, species, ...), or merge a read's assignments into their lowest\n"
    "\t\tcommon ancestor (lca), on the GPU before the rows are written (equal to centrifuger-promote IDX this-output-without-it STR when no two\n"
    "\t\tadjacent reads share a read id); not together with --quant or --expand-taxid [no promotion]\n"
    "\t--kreport FILE: also write the Kraken-style report of centrifuger-kreport for this run to FILE, the reads counted per taxon on the GPU\n"
    "\t\t(equal to centrifuger-kreport -x IDX this-output-without---promote); with --gpu LIST every GPU counts its own reads and the counts\n"
    "\t\tare summed after the last batch; not together with --expand-taxid [no report]\n"
    "\t--gpu LIST: comma separated MI355X ordinals, or 'all' [0]\n"
    "\t--gpu-batch INT: reads per device batch [262144]\n"
    "\t--gpu-balanced: also derive the text-mode tables and the locate memo on the device (+0.4 s load per Gbp, faster kernels)\n"
    "\t--gpu-throughput: ... and the 68 GB K-mer table (longest load, fastest kernels) [default: neither, shortest load]\n"
    "\t--parse-threads INT: threads that parse plain single-end read files in pieces [min(-t,8); 1 = sequential reader]\n"
    "\t--gpu-parse: tokenise plain FASTA/FASTQ files (-u, -1/-2) on the GPU that classifies them; the run falls back to the host parsers, with one log line, for what that does not cover [host parsers]\n"
    "\t--gpu-inflate: inflate -u files that are BGZF throughout on the GPU that classifies them and tokenise the text there (implies --gpu-parse); every other file is inflated on the host, with one log line [host inflaters]\n"
    "\t--gpu-format: make the TSV rows on the GPU that classified the reads (with --gpu-parse the read ids never leave it); the rows are formatted on the host, with one log line, for what that does not cover [host formatter]\n"
    "\t--gpu-dump: make and compress the --un / --cl read dumps on the GPU that classified the reads; the files are BGZF (gzip in members of at most 64 KiB, read by every gunzip); --merge-readpair keeps the host writer, with one log line [host writer, zlib level 1]\n"
    "\t--gpu-dump-codes fixed|dynamic: the Huffman codes of --gpu-dump's members: the fixed code of deflate, or each member's own codes where they make it smaller (smaller files, more work on the GPU) [fixed]\n"
    "\t-h: print this usage message\n"
    "\t-v: print the version information and quit\n";

enum { OPT_UN = 1000, OPT_CL, OPT_NO_DUST, OPT_MIN_HITLEN, OPT_HITK, OPT_SECONDARY, OPT_GPU, OPT_GPU_BATCH, OPT_GPU_THROUGHPUT, OPT_GPU_FASTLOAD, OPT_GPU_BALANCED, OPT_PARSE_THREADS, OPT_GPU_PARSE, OPT_GPU_INFLATE, OPT_GPU_FORMAT, OPT_GPU_DUMP, OPT_GPU_DUMP_CODES, OPT_EXPAND_TAXID, OPT_MERGE_READPAIR, OPT_QUANT, OPT_QUANT_FORMAT, OPT_PROMOTE, OPT_KREPORT, OPT_BARCODE, OPT_UMI, OPT_READ_FORMAT, OPT_BARCODE_WHITELIST, OPT_BARCODE_TRANSLATE, OPT_UNSUPPORTED };

// Persistent workers for the dust and the format stage: a 256 k-read batch is 6 ms of work on 64 threads, less than
// what starting 64 threads costs, so the threads are started once.
class WorkerPool {
 public:
  explicit WorkerPool(int n) : n_(n < 1 ? 1 : n) {
    for (int t = 1; t < n_; ++t) th_.emplace_back([this, t]() { loop(t); });
  }
  ~WorkerPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; ++gen_; }
    cv_.notify_all();
    for (auto &x : th_) x.join();
  }
  int size() const { return n_; }
  // fn(t) for t in [0, parts): parts <= size(); the caller runs part 0 itself and returns when all are done
  void run(int parts, const std::function<void(int)> &fn) {
    if (parts <= 1) { fn(0); return; }
    { std::lock_guard<std::mutex> lk(mu_); fn_ = &fn; parts_ = parts; pending_ = parts - 1; ++gen_; }
    cv_.notify_all();
    fn(0);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&]() { return pending_ == 0; });
  }

 private:
  void loop(int t) {
    unsigned long seen = 0;
    for (;;) {
      const std::function<void(int)> *fn;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&]() { return gen_ != seen; });
        seen = gen_;
        if (stop_) return;
        if (t >= parts_) continue;
        fn = fn_;
      }
      (*fn)(t);
      std::lock_guard<std::mutex> lk(mu_);
      if (--pending_ == 0) done_.notify_all();
    }
  }
  int n_;
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_;
  const std::function<void(int)> *fn_ = nullptr;
  int parts_ = 0, pending_ = 0;
  unsigned long gen_ = 0;
  bool stop_ = false;
};

struct Options {
  std::string idx;
  std::vector<std::string> u, m1, m2, inter;
  int threads = 1;
  cfr_params params;
  bool dust = true;
  bool merge = false;                  // --merge-readpair
  std::string quant_path;              // --quant: the abundance report of this run
  int quant_format = 0;                // --quant-format
  std::string kreport_path;            // --kreport: the Kraken-style report of this run
  std::string promote;                 // --promote: the level
  bool has_promote = false;
  std::string un_prefix, cl_prefix;
  std::vector<int> gpus{0};
  bool all_gpus = false;
  size_t gpu_batch = 1u << 18;
  bool throughput_profile = false;
  int parse_threads = 0;               // 0 = automatic
  bool balanced_profile = false;
  bool gpu_parse = false;              // --gpu-parse: cfr_tokenize on the device instead of SeqReader, where it applies
  bool gpu_inflate = false;            // --gpu-inflate: BGZF -u files go to the device compressed (cfr_inflate_bgzf, cfr_tokenize_resident), where it applies
  bool gpu_format = false;             // --gpu-format: the rows of a batch made on the device (cfr_device_index_tsv_last), where it applies
  bool gpu_dump_dynamic = false;       // --gpu-dump-codes dynamic: cfr_gz_options.codes = 1 for those dumps
  bool gpu_dump = false;               // --gpu-dump: the --un / --cl dumps made and compressed on the device (cfr_gz_dump), where it applies
  // single-cell input (CentrifugerClass.cpp:374-381)
  std::vector<std::string> bc_files, um_files;
  std::string read_format, whitelist, translate;
  bool has_read_format = false;
  // what parse_options derives from the above
  bool paired = false;                 // -1/-2 or -i
  cfr_read_format *fmt = nullptr;
  cfr_barcode_translate *translate_table = nullptr;
  bool has_barcode = false, has_umi = false, bc_hd = false, um_hd = false, single_cell = false;
};

// the files of a read dump (ResultWriter::SetOutputReads, ResultWriter.hpp:126-176): slot 0 read 1, 1 read 2, 2 barcode, 3 UMI; "" - the
// run does not write that one.  Always 'fa' for barcode and umi (ResultWriter.hpp:161-171).
std::string dump_file_name(const std::string &prefix, int slot, bool mate, bool has_barcode, bool has_umi) {
  switch (slot) {
    case 0: return prefix + (mate ? "_1.fq.gz" : ".fq.gz");
    case 1: return mate ? prefix + "_2.fq.gz" : "";
    case 2: return has_barcode ? prefix + "_bc.fa.gz" : "";
    default: return has_umi ? prefix + "_um.fa.gz" : "";
  }
}

// gz read dumps written record by record on the host
struct ReadDump {
  gzFile fp[4] = {nullptr, nullptr, nullptr, nullptr};
  void open(const std::string &prefix, bool mate, bool has_barcode, bool has_umi) {
    for (int k : {2, 3, 0, 1}) {
      const std::string name = dump_file_name(prefix, k, mate, has_barcode, has_umi);
      if (!name.empty()) fp[k] = gzopen(name.c_str(), "w1");
    }
  }
  // (gzprintf, like ResultWriter.hpp:254-265: zlib formats into its 8192-byte buffer and writes NOTHING for a record that does
  // not fit - the reference's dumps silently lack reads of ~8 kbp and more, and so do these; tests/test_gpu_cli.py)
  void put(int k, const char *id, const uint8_t *s, size_t n, const char *q, size_t qn) {
    if (!fp[k]) return;
    if (!q) gzprintf(fp[k], ">%s\n%.*s\n", id, (int)n, (const char *)s);
    else gzprintf(fp[k], "@%s\n%.*s\n+\n%.*s\n", id, (int)n, (const char *)s, (int)qn, q);
  }
  void put_extra(int k, const char *id, const char *s) { if (fp[k]) gzprintf(fp[k], ">%s\n%s\n", id, s); }   // ResultWriter.hpp:267-275
  void close() { for (auto &f : fp) if (f) { gzclose(f); f = nullptr; } }
};

// --gpu-dump: the same files taken as BGZF members from the device workers; close() ends each with the end-of-file member
struct RawDump {
  FILE *fp[4] = {nullptr, nullptr, nullptr, nullptr};
  bool on() const { return fp[0] != nullptr; }
  void open(const std::string &prefix, bool mate, bool has_barcode, bool has_umi) {
    for (int k = 0; k < 4; ++k) {
      const std::string name = dump_file_name(prefix, k, mate, has_barcode, has_umi);
      if (name.empty()) continue;
      if (!(fp[k] = fopen(name.c_str(), "wb"))) { print_log("ERROR: cannot write %s (%s).", name.c_str(), strerror(errno)); exit(EXIT_FAILURE); }
    }
  }
  void put(int k, const std::string &members) { if (fp[k] && !members.empty()) fwrite(members.data(), 1, members.size(), fp[k]); }
  void close() {
    const uint8_t *eof = nullptr;
    size_t n = 0;
    cfr_gz_eof(&eof, &n);
    for (auto &f : fp) if (f) {
      const bool ok = fwrite(eof, 1, n, f) == n;
      if (fclose(f) != 0 || !ok) { print_log("ERROR: writing a read dump failed (%s).", strerror(errno)); exit(EXIT_FAILURE); }
      f = nullptr;
    }
  }
};

// CFR_CLI_TIMING=1: per-stage busy seconds on stderr at exit (stage threads overlap, so they do not add up to the wall clock)
struct StageClock {
  std::atomic<long long> ns[8];
  StageClock() { for (auto &x : ns) x = 0; }
  void add(int k, std::chrono::steady_clock::time_point t0) {
    ns[k] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  }
};
enum { T_OPEN = 0, T_DEVICE, T_PARSE, T_DUST, T_CLASSIFY, T_FORMAT, T_WRITE, T_WALL };
inline std::chrono::steady_clock::time_point tick() { return std::chrono::steady_clock::now(); }

// .4.cfr says sequence_type amino_acid (Classifier::IsProteinDatabase); asked before the index itself is loaded
bool index_is_protein(const std::string &prefix) {
  bool protein = false;
  if (FILE *f4 = fopen((prefix + ".4.cfr").c_str(), "r")) {
    char key[128], val[128];
    while (fscanf(f4, "%127s %127s", key, val) == 2) if (!strcmp(key, "sequence_type") && !strcmp(val, "amino_acid")) protein = true;
    fclose(f4);
  }
  return protein;
}

[[noreturn]] void die_status(const char *what, cfr_status st) {
  print_log("ERROR: %s failed (status %d): %s", what, st, cfr_last_error());
  exit(EXIT_FAILURE);
}

[[noreturn]] void die_mates() { print_log("ERROR: The two mate-pair read files have different number of reads."); exit(EXIT_FAILURE); }

int32_t format_info(const cfr_read_format *fmt, int cat, int which) {   // 0: segments, 1: NeedExtract, 2: IsInComment
  int32_t v[3] = {0, 0, 0};
  cfr_read_format_info(fmt, cat, &v[0], &v[1], &v[2]);
  return v[which];
}

// single-cell input: --barcode, --UMI, --read-format, --barcode-whitelist, --barcode-translate (CentrifugerClass.cpp:457-466, 516-590).
// Returns -1 to go on, or the exit status.
int single_cell_options(Options &opt) {
  if (cfr_read_format_parse(opt.read_format.c_str(), &opt.fmt) != CFR_OK) {     // ReadFormatter::Init (ReadFormatter.hpp:212-213)
    fprintf(stderr, "%s\n", cfr_last_error());
    return 1;
  }
  opt.has_barcode = !opt.bc_files.empty() || format_info(opt.fmt, CFR_FORMAT_BARCODE, 0) > 0;   // :560-563
  opt.has_umi = !opt.um_files.empty() || format_info(opt.fmt, CFR_FORMAT_UMI, 0) > 0;
  opt.bc_hd = format_info(opt.fmt, CFR_FORMAT_BARCODE, 2) != 0;
  opt.um_hd = format_info(opt.fmt, CFR_FORMAT_UMI, 2) != 0;
  opt.single_cell = opt.has_barcode || opt.has_umi || opt.has_read_format;
  if (!opt.whitelist.empty() && opt.bc_files.empty()) {                      // :565-574
    print_log("Barcode whitelist has to be used with --barcode option, so cases like piping input is not supported.");
    return EXIT_FAILURE;
  }
  if (!opt.whitelist.empty() && opt.bc_hd) {
    // (the reference's background pass hands the barcode record's sequence to a format that describes its comment, BarcodeCorrector.hpp:156)
    print_log("ERROR: --barcode-whitelist cannot be combined with a barcode taken from the header comment (bc:hd:) in this build.");
    return EXIT_FAILURE;
  }
  const size_t read_files = std::max(opt.u.size(), std::max(opt.m1.size(), opt.inter.size()));
  if ((!opt.bc_files.empty() && opt.bc_files.size() != read_files) || (!opt.um_files.empty() && opt.um_files.size() != read_files)) {
    print_log("ERROR: --barcode / --UMI must be given once per read file.");
    return EXIT_FAILURE;
  }
  if (!opt.translate.empty() && cfr_barcode_translate_open(opt.translate.c_str(), &opt.translate_table) != CFR_OK) {
    print_log("ERROR: %s", cfr_last_error());
    return EXIT_FAILURE;
  }
  if (opt.single_cell) opt.parse_threads = 1;      // the barcode and UMI files are read in step with the reads: the sequential reader
  return -1;
}

// The getopt loop and every check that needs neither the index nor a device.  Returns -1 to go on, or the exit status.
int parse_options(int argc, char *argv[], Options &opt) {
  if (argc <= 1) { fprintf(stderr, "%s", kUsage); return 0; }
  cfr_params_default(&opt.params);
  static const char *short_options = "x:1:2:u:i:o:t:k:hv";
  static struct option long_options[] = {
      {"un", required_argument, 0, OPT_UN}, {"cl", required_argument, 0, OPT_CL}, {"no-dust", no_argument, 0, OPT_NO_DUST},
      {"min-hitlen", required_argument, 0, OPT_MIN_HITLEN}, {"hitk-factor", required_argument, 0, OPT_HITK},
      {"consider-secondary", required_argument, 0, OPT_SECONDARY}, {"gpu", required_argument, 0, OPT_GPU},
      {"gpu-batch", required_argument, 0, OPT_GPU_BATCH}, {"gpu-throughput", no_argument, 0, OPT_GPU_THROUGHPUT},
      {"gpu-fast-load", no_argument, 0, OPT_GPU_FASTLOAD}, {"gpu-balanced", no_argument, 0, OPT_GPU_BALANCED},
      {"parse-threads", required_argument, 0, OPT_PARSE_THREADS}, {"gpu-parse", no_argument, 0, OPT_GPU_PARSE}, {"gpu-inflate", no_argument, 0, OPT_GPU_INFLATE}, {"gpu-format", no_argument, 0, OPT_GPU_FORMAT}, {"gpu-dump", no_argument, 0, OPT_GPU_DUMP}, {"gpu-dump-codes", required_argument, 0, OPT_GPU_DUMP_CODES},
      {"sample-sheet", required_argument, 0, OPT_UNSUPPORTED}, {"merge-readpair", no_argument, 0, OPT_MERGE_READPAIR},
      {"quant", required_argument, 0, OPT_QUANT}, {"quant-format", required_argument, 0, OPT_QUANT_FORMAT},
      {"promote", required_argument, 0, OPT_PROMOTE}, {"kreport", required_argument, 0, OPT_KREPORT},
      {"expand-taxid", no_argument, 0, OPT_EXPAND_TAXID}, {"read-format", required_argument, 0, OPT_READ_FORMAT},
      {"barcode", required_argument, 0, OPT_BARCODE}, {"UMI", required_argument, 0, OPT_UMI},
      {"barcode-whitelist", required_argument, 0, OPT_BARCODE_WHITELIST}, {"barcode-translate", required_argument, 0, OPT_BARCODE_TRANSLATE},
      {0, 0, 0, 0}};
  int c, option_index = 0;
  while ((c = getopt_long(argc, argv, short_options, long_options, &option_index)) != -1) {
    switch (c) {
      case 'x': opt.idx = optarg; break;
      case 'u': opt.u.push_back(optarg); break;
      case '1': opt.m1.push_back(optarg); break;
      case '2': opt.m2.push_back(optarg); break;
      case 'i': opt.inter.push_back(optarg); break;
      case 'o': break;   // accepted and unused, like the reference
      case 't': opt.threads = atoi(optarg); break;
      case 'k': opt.params.max_result = atoi(optarg); break;
      case 'v': printf("Centrifuger-MI355X %s\n", cfr_version()); return 0;
      case OPT_UN: opt.un_prefix = optarg; break;
      case OPT_CL: opt.cl_prefix = optarg; break;
      case OPT_NO_DUST: opt.dust = false; break;
      case OPT_MERGE_READPAIR: opt.merge = true; break;                    // CentrifugerClass.cpp:445-447
      case OPT_QUANT: opt.quant_path = optarg; break;
      case OPT_QUANT_FORMAT: opt.quant_format = atoi(optarg); break;
      case OPT_PROMOTE: opt.promote = optarg; opt.has_promote = true; break;
      case OPT_KREPORT: opt.kreport_path = optarg; break;
      case OPT_EXPAND_TAXID: opt.params.output_expanded = 1; break;       // CentrifugerClass.cpp:453-455
      case OPT_BARCODE: opt.bc_files.push_back(optarg); break;             // CentrifugerClass.cpp:457-466
      case OPT_UMI: opt.um_files.push_back(optarg); break;
      case OPT_READ_FORMAT: opt.read_format = optarg; opt.has_read_format = true; break;
      case OPT_BARCODE_WHITELIST: opt.whitelist = optarg; break;
      case OPT_BARCODE_TRANSLATE: opt.translate = optarg; break;
      case OPT_MIN_HITLEN: opt.params.min_hit_len = atoi(optarg); break;
      case OPT_HITK: opt.params.max_result_per_hit_factor = atoi(optarg); break;
      case OPT_SECONDARY: {
        unsigned long hl; double f;
        if (sscanf(optarg, "%lu,%lf", &hl, &f) != 2) {
          print_log("Invalid format for --consider-secondary option. It should be in the format of INT,FLOAT");
          return EXIT_FAILURE;
        }
        opt.params.consider_secondary_hit_len = hl;
        opt.params.consider_secondary_score_factor = f;
        break;
      }
      case OPT_GPU:
        if (!strcmp(optarg, "all")) opt.all_gpus = true;
        else {
          opt.gpus.clear();
          for (char *tok = strtok(optarg, ","); tok; tok = strtok(nullptr, ",")) opt.gpus.push_back(atoi(tok));
        }
        break;
      case OPT_GPU_BATCH: opt.gpu_batch = strtoull(optarg, nullptr, 10); break;
      case OPT_GPU_THROUGHPUT: opt.throughput_profile = true; break;
      case OPT_GPU_FASTLOAD: break;                      // the default; accepted for symmetry
      case OPT_GPU_BALANCED: opt.balanced_profile = true; break;
      case OPT_PARSE_THREADS: opt.parse_threads = atoi(optarg); break;
      case OPT_GPU_PARSE: opt.gpu_parse = true; break;
      case OPT_GPU_INFLATE: opt.gpu_inflate = true; break;
      case OPT_GPU_FORMAT: opt.gpu_format = true; break;
      case OPT_GPU_DUMP: opt.gpu_dump = true; break;
      case OPT_GPU_DUMP_CODES:
        if (!strcmp(optarg, "dynamic")) opt.gpu_dump_dynamic = true;
        else if (!strcmp(optarg, "fixed")) opt.gpu_dump_dynamic = false;
        else { print_log("ERROR: --gpu-dump-codes is 'fixed' or 'dynamic', not '%s'.", optarg); return EXIT_FAILURE; }
        break;
      case OPT_UNSUPPORTED:
        print_log("ERROR: option --%s belongs to a part of Centrifuger outside the MI355X classification path and is not available in this build.",
                  long_options[option_index].name);
        return EXIT_FAILURE;
      default: fprintf(stderr, "%s", kUsage); return EXIT_FAILURE;
    }
  }
  print_log("Centrifuger-MI355X (%s) starts.", cfr_version());
  if (opt.idx.empty()) { print_log("Need to use -x to specify index prefix."); return EXIT_FAILURE; }
  if (opt.threads < 1) opt.threads = 1;
  SeqReader::inflate_threads = std::max(1, std::min(opt.threads, 16));
  if (opt.gpu_batch < 1) opt.gpu_batch = 1;
  {
    // a batch's match (24 B) and --expand-taxid span (16 B) buffers have max_result slots per read, on the host and on the device: with
    // -k 4096 the default batch of 262144 reads would be 43 GB of them, zero-filled per recycled batch.  Large -k therefore runs smaller
    // batches (2 GB of slots at most); the rows do not depend on where a batch ends.
    const size_t k_slots = (size_t)(opt.params.max_result > 0 ? opt.params.max_result : 4);
    const size_t by_k = std::max<size_t>(1024, (size_t)(2e9 / (40.0 * (double)k_slots)));
    if (opt.gpu_batch > by_k) opt.gpu_batch = by_k;
  }
  if (opt.has_promote && !opt.quant_path.empty()) {      // (the quantifier must see the assignments as the classifier made them)
    print_log("ERROR: --promote cannot be combined with --quant: the abundance report is estimated from unpromoted assignments. Run centrifuger-quant on the unpromoted output instead.");
    return EXIT_FAILURE;
  }
  if (opt.has_promote && opt.params.output_expanded) {   // (the reference's centrifuger-promote cannot process the expandedTaxIDs column either)
    print_log("ERROR: --promote cannot be combined with --expand-taxid: promotion does not cover the expanded tax id lists.");
    return EXIT_FAILURE;
  }
  if (!opt.kreport_path.empty() && opt.params.output_expanded) {   // (--expand-taxid has a classify entry of its own, which the report's hook does not cover)
    print_log("ERROR: --kreport cannot be combined with --expand-taxid: the report is made by the wide classify entries. Run centrifuger-kreport on the output instead.");
    return EXIT_FAILURE;
  }
  if (!opt.quant_path.empty() && (opt.quant_format < 0 || opt.quant_format > 3)) { print_log("ERROR: --quant-format takes 0, 1, 2 or 3."); return EXIT_FAILURE; }
  opt.paired = !opt.m1.empty() || !opt.inter.empty();
  if (opt.merge && !opt.paired) {      // (the reference calls ReadPairMerger::Merge with a null mate there and does not survive it, ReadPairMerger.hpp:135-141)
    print_log("ERROR: option --merge-readpair needs paired-end reads (-1 / -2 or -i); with single-end reads it is not available in this build.");
    return EXIT_FAILURE;
  }
  if (opt.m1.size() != opt.m2.size()) { print_log("ERROR: -1 and -2 must be given the same number of times."); return EXIT_FAILURE; }
  if (opt.u.empty() && !opt.paired) { print_log("Need to use -u/-1/-2/-i to specify input reads."); return EXIT_FAILURE; }
  if ((int)!opt.u.empty() + (int)!opt.m1.empty() + (int)!opt.inter.empty() > 1) {
    // the reference would walk a mixed file list; this build processes one kind of input per run and says so instead of dropping files
    print_log("ERROR: -u, -1/-2 and -i cannot be combined in one run of this build.");
    return EXIT_FAILURE;
  }
  return single_cell_options(opt);
}

int parse_workers(const Options &opt) { return opt.parse_threads > 0 ? opt.parse_threads : std::min(opt.threads, 8); }

// bytes of read input: plain files as they are on disk, .gz files times gz_factor; stdin is unknown and counts nothing
unsigned long long input_bytes(const Options &opt, unsigned long long gz_factor) {
  unsigned long long bytes = 0;
  for (const auto *lst : {&opt.u, &opt.m1, &opt.m2, &opt.inter})
    for (const std::string &f : *lst) {
      struct stat st;
      if (f != "-" && stat(f.c_str(), &st) == 0 && S_ISREG(st.st_mode)) {
        const bool gz = f.size() > 3 && f.compare(f.size() - 3, 3, ".gz") == 0;
        bytes += (unsigned long long)st.st_size * (gz ? gz_factor : 1ull);
      }
    }
  return bytes;
}

// the sequential readers of -i, -1/-2 or -u
void open_readers(const Options &opt, std::unique_ptr<SeqReader> &r1, std::unique_ptr<SeqReader> &r2) {
  if (!opt.inter.empty()) r1.reset(new SeqReader(opt.inter));
  else if (opt.paired) { r1.reset(new SeqReader(opt.m1)); r2.reset(new SeqReader(opt.m2)); }
  else r1.reset(new SeqReader(opt.u));
}

// ---- CFR_CLI_PARSE_ONLY: parser self-test hook (tests/test_host_cpu.py) on the reader's own pieces; no index, no device ------------

// records as "id<TAB>bases[<TAB>mate bases]<TAB>q|-" lines
void print_records(const Batch &b) {
  for (size_t i = 0; i < b.n; ++i) {
    printf("%s\t%.*s", b.id(i), (int)(b.offs1[i + 1] - b.offs1[i]), (const char *)b.bases1.data() + b.offs1[i]);
    if (b.paired) printf("\t%.*s", (int)(b.offs2[i + 1] - b.offs2[i]), (const char *)b.bases2.data() + b.offs2[i]);
    printf("\t%s%.*s\n", b.has_qual[i] ? "q:" : "-", (int)(b.q1_off[i + 1] - b.q1_off[i]), b.qual1.data() + b.q1_off[i]);
  }
}

size_t env_size(const char *name, size_t otherwise) { const char *e = getenv(name); return e ? strtoull(e, nullptr, 10) : otherwise; }

int run_parse_only(const Options &opt, int mode) {
  ByteBuf::use_pinned = false;
  const bool interleaved = !opt.inter.empty();
  TakeSpec ts;
  ts.paired = opt.paired; ts.interleaved = interleaved; ts.keep_qual = mode != 2;
  Batch b;
  if (mode == 3 && !opt.paired) {   // the parallel cutter on every -u file: the records piece by piece
    for (const std::string &f : opt.u) {
      MappedFile mf;
      if (!mf.open_plain(f) || mf.resync(0) != 0) { puts("NOT_CUTTABLE"); continue; }
      std::vector<size_t> cuts;
      plan_byte_cuts(mf, env_size("CFR_CLI_PIECE_BYTES", 64), cuts);
      for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        b.reset(false);
        const PieceResult r = parse_piece(b, ts, mf.base + cuts[k], cuts[k + 1] - cuts[k], nullptr, 0, 0);
        print_records(b);
        if (!r.done1) puts("CUT_MISMATCH");
      }
    }
    return 0;
  }
  if (mode == 4 && opt.paired) {   // the pair cutter (plan_record_cuts): pieces of CFR_CLI_PIECE_RECORDS pairs, records piece by piece
    const size_t every = env_size("CFR_CLI_PIECE_RECORDS", 7);
    MappedFile f1, f2;
    std::vector<size_t> c1, c2;
    size_t t1 = 0, t2 = 0;
    const bool ok = interleaved ? (f1.open_plain(opt.inter[0]) && plan_record_cuts(f1, 2 * every, 3, c1, t1) && t1 % 2 == 0)
                                : (f1.open_plain(opt.m1[0]) && f2.open_plain(opt.m2[0]) && plan_record_cuts(f1, every, 3, c1, t1) && plan_record_cuts(f2, every, 3, c2, t2) && t1 == t2);
    if (!ok) { puts("NOT_CUTTABLE"); return 0; }
    for (size_t k = 0; k + 1 < c1.size(); ++k) {
      b.reset(true);
      const PieceResult r = parse_piece(b, ts, f1.base + c1[k], c1[k + 1] - c1[k], interleaved ? nullptr : f2.base + c2[k], interleaved ? 0 : c2[k + 1] - c2[k], 0);
      print_records(b);
      if (r.mate_missing) puts("MATE_MISSING");
      if (k + 2 < c1.size() && r.taken != every) puts("PIECE_SIZE_MISMATCH");
    }
    return 0;
  }
  std::unique_ptr<SeqReader> r1, r2;
  open_readers(opt, r1, r2);
  if (mode == 2) {       // count only (parser throughput)
    size_t nrec = 0;
    const auto tp = tick();
    b.reset(opt.paired);
    for (;;) {
      if (b.bases1.size() > (1u << 26)) b.reset(opt.paired);
      if (take(b, ts, r1.get(), r2.get(), false) <= 0) break;
      ++nrec;
    }
    const double sec = std::chrono::duration<double>(tick() - tp).count();
    printf("%zu records in %.3f s = %.2f M records/s (%zu)\n", nrec, sec, (double)nrec / sec * 1e-6, b.bases1.size());
    return 0;
  }
  for (int got = 1; got > 0;) {
    b.reset(opt.paired);
    while (b.n < 4096 && (got = take(b, ts, r1.get(), r2.get(), false)) > 0) {}
    print_records(b);
    if (got < 0) fputs("MATE_MISSING\n", stdout);
  }
  return 0;
}

// ---- pipeline: reader -> dust -> device workers (one per GPU) -> TSV formatter -> ordered writer (the main thread) -----------------

// The hand-off between two stages.  pop waits for a batch and returns nothing once every producer has closed the queue and it is
// empty: that is how a stage learns that the one before it has finished.  The writer's queue (in_order: every batch in input order)
// also makes push wait while `limit` batches are in flight, and hands a batch out only once the formatter has marked it done.
class BatchQueue {
 public:
  explicit BatchQueue(size_t limit = (size_t)-1, bool wait_done = false) : limit_(limit), wait_done_(wait_done) {}
  void producers(size_t n) { std::lock_guard<std::mutex> lk(mu_); open_ = n; }   // more than the one a queue starts with (before they start)
  void push(const std::shared_ptr<Batch> &b) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&]() { return q_.size() < limit_; });
    q_.push_back(b);
    cv_.notify_all();
  }
  std::shared_ptr<Batch> pop(bool wait = true) {   // wait = false: what is there now
    std::unique_lock<std::mutex> lk(mu_);
    auto ready = [&]() { return !q_.empty() && (!wait_done_ || q_.front()->done); };
    if (wait) cv_.wait(lk, [&]() { return ready() || (open_ == 0 && q_.empty()); });
    if (!ready()) return nullptr;
    std::shared_ptr<Batch> b = q_.front();
    q_.pop_front();
    cv_.notify_all();
    return b;
  }
  void mark_done(Batch &b) { std::lock_guard<std::mutex> lk(mu_); b.done = true; cv_.notify_all(); }
  void close() { std::lock_guard<std::mutex> lk(mu_); if (open_) --open_; cv_.notify_all(); }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<Batch>> q_;
  const size_t limit_;
  const bool wait_done_;
  size_t open_ = 1;
};

// What the stages of one run share: the options and what follows from them, the queues between the stages, and (once loaded) the
// index and its device images
struct Run {
  explicit Run(Options &o) : opt(o), t_wall(tick()) {}
  Options &opt;
  StageClock clk;
  const std::chrono::steady_clock::time_point t_wall;
  ReadDump un, cl;
  RawDump raw_un, raw_cl;              // --gpu-dump, where it applies: the same files, written as the devices' members
  bool gpu_dump = false;
  std::atomic<long long> dump_ns{0}, dump_kernel_ns{0};   // ... the workers' time in cfr_gz_dump, and the device time of its kernels
  bool gpu_parse = false;              // --gpu-parse, where it applies
  bool gpu_inflate = false;            // --gpu-inflate, where it applies (then gpu_parse is on as well)
  std::vector<std::unique_ptr<BgzfFile>> bgzf_files;   // (mapped until the end of the run: batches point into them)
  bool gpu_format = false;             // --gpu-format, where it applies
  std::atomic<long long> tsv_kernel_ns{0};   // ... and the device time of its kernels (cfr_last_tsv_ms), all batches
  bool protein = false, dumps = false, host_dust = false, host_merge = false, expand = false;
  BatchQueue pending;                  // parsed, waiting for the dust stage
  BatchQueue dusted;                   // masked, waiting for a device
  BatchQueue classified;               // classified, waiting for the TSV formatter
  BatchQueue recycled;                 // written out; their buffers serve the next batches
  BatchQueue in_order{16, true};       // parsed batches waiting: the reader runs ahead of the index load
  std::vector<std::unique_ptr<MappedFile>> raw_files;   // (mapped until the end of the run: batches point into them)
  std::atomic<bool> raw_broken{false};                 // a piece came back irregular: it and every later one go through SeqReader
  cfr_index *idx = nullptr;
  std::vector<cfr_dev_index *> devs;
  std::vector<cfr_barcode *> whitelists;
  cfr_quant *quant = nullptr;
  std::mutex quant_mu;
  cfr_kreport *kreport = nullptr;      // --kreport: the host handle that takes the devices' bins and writes the report
  std::mutex kreport_mu;
  size_t total = 0, classified_reads = 0;
};

// ---- single-cell input: the reformatting of a batch, the whitelist's background pass, the barcode correction and translation ------

// one category over n records (cfr_read_format_extract: once for the sizes, once for the bytes)
void extract(const cfr_read_format *fmt, int cat, int inplace, const uint8_t *bases, const uint64_t *off, const char *q, const uint8_t *cm, const uint64_t *cm_off,
             size_t n, std::vector<uint8_t> &out, std::vector<uint64_t> &out_off, std::vector<uint8_t> *out_q) {
  static const uint8_t kNone[1] = {0};
  out_off.resize(n + 1);
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) { out.resize(out_off[n] + 1); if (out_q) out_q->resize(out_off[n] + 1); }
    const cfr_status s = cfr_read_format_extract(fmt, cat, inplace, bases ? bases : kNone, off, q, cm, cm_off, n, pass ? out.data() : nullptr, out_off.data(),
                                                 pass && out_q && q ? (char *)out_q->data() : nullptr);
    if (s != CFR_OK) die_status("cfr_read_format_extract", s);
  }
}

// NUL-terminated strings of n flat records; status (may be null): -1 prints as "N" (CentrifugerClass.cpp:189-205)
void strings(const uint8_t *bases, const uint64_t *off, size_t n, const int8_t *status, std::vector<char> &str, std::vector<size_t> &str_off) {
  str.clear(); str_off.clear();
  for (size_t i = 0; i < n; ++i) {
    str_off.push_back(str.size());
    if (status && status[i] == -1) str.push_back('N');
    else str.insert(str.end(), bases + off[i], bases + off[i + 1]);
    str.push_back('\0');
  }
}

void check_barcode_lengths(const uint64_t *off, size_t n) {
  for (size_t i = 0; i < n; ++i) if (off[i + 1] - off[i] > 255) { print_log("ERROR: a barcode of 256 bases or more cannot be looked up in the whitelist."); exit(EXIT_FAILURE); }
}

bool uniform_qual(const std::vector<uint64_t> &off, const std::vector<uint64_t> &q_off, size_t n) {   // qualities for every record, as long as the bases
  bool same = q_off.size() == n + 1 && q_off[n] > 0;
  for (size_t i = 0; same && i <= n; ++i) same = q_off[i] == off[i];
  return same;
}

// Reformat everything (CentrifugerClass.cpp:163-224) up to the correction, which waits for the GPU that classifies the batch
void reformat(const Options &opt, Batch &b) {
  if (!opt.single_cell || b.n == 0) return;
  static const uint8_t kNone[1] = {0};
  std::vector<uint8_t> tmp, tmp_q;
  std::vector<uint64_t> tmp_off;
  std::vector<uint64_t> q1o(b.q1_off.begin(), b.q1_off.end()), q2o(b.q2_off.begin(), b.q2_off.end());
  const bool q1_ok = uniform_qual(b.offs1, q1o, b.n), q2_ok = b.paired && uniform_qual(b.offs2, q2o, b.n);
  // barcode and UMI first: without a file of their own they are cut from read 1 as it was read (CopyBatch, :140-160)
  auto side = [&](int cat, bool hd, bool own_file, ByteBuf &raw, std::vector<uint64_t> &raw_off, std::vector<char> &rawq, std::vector<uint64_t> &rawq_off,
                  std::vector<char> &cm, std::vector<uint64_t> &cm_off, std::vector<uint8_t> &out, std::vector<uint64_t> &out_off, std::vector<uint8_t> *out_q,
                  bool *has_q) {
    const uint8_t *src = own_file ? raw.data() : b.bases1.data();
    const std::vector<uint64_t> &src_off = own_file ? raw_off : b.offs1;
    const bool q_ok = own_file ? uniform_qual(raw_off, rawq_off, b.n) : q1_ok;
    const char *q = !q_ok || hd ? nullptr : own_file ? rawq.data() : b.qual1.data();
    const char *comments = own_file ? cm.data() : b.r1_cm.data();
    extract(opt.fmt, cat, 1, src, src_off.data(), q, comments ? (const uint8_t *)comments : kNone, (own_file ? cm_off : b.r1_cm_off).data(), b.n, out, out_off, out_q);
    if (has_q) *has_q = q != nullptr;
  };
  if (opt.has_barcode) side(CFR_FORMAT_BARCODE, opt.bc_hd, !opt.bc_files.empty(), b.bc_raw, b.bc_raw_off, b.bc_rawq, b.bc_rawq_off, b.bc_cm, b.bc_cm_off, b.bc, b.bc_off, &b.bc_q, &b.bc_has_q);
  if (opt.has_umi) {
    side(CFR_FORMAT_UMI, opt.um_hd, !opt.um_files.empty(), b.um_raw, b.um_raw_off, b.um_rawq, b.um_rawq_off, b.um_cm, b.um_cm_off, b.um, b.um_off, nullptr, nullptr);
    strings(b.um.data(), b.um_off.data(), b.n, nullptr, b.um_str, b.um_str_off);
  }
  auto mate = [&](int cat, ByteBuf &bases, std::vector<uint64_t> &off, std::vector<char> &qual, std::vector<size_t> &q_off, bool q_ok) {
    if (!format_info(opt.fmt, cat, 1)) return;                       // NeedExtract
    static const uint64_t none[1] = {0};
    extract(opt.fmt, cat, 1, bases.data(), off.data(), q_ok ? qual.data() : nullptr, kNone, none, b.n, tmp, tmp_off, &tmp_q);
    bases.clear(); bases.append(tmp.data(), tmp_off[b.n]);
    off = tmp_off;
    if (q_ok) { qual.assign((const char *)tmp_q.data(), (const char *)tmp_q.data() + tmp_off[b.n]); q_off.assign(tmp_off.begin(), tmp_off.end()); }
  };
  mate(CFR_FORMAT_READ1, b.bases1, b.offs1, b.qual1, b.q1_off, q1_ok);
  if (b.paired) mate(CFR_FORMAT_READ2, b.bases2, b.offs2, b.qual2, b.q2_off, q2_ok);
}

// The whitelist: one table per GPU in use, then the background counts of the first 2 000 000 barcode records on each of them
// (SetWhitelist + CollectBackgroundDistribution, CentrifugerClass.cpp:521-523, 565-569), before any batch is corrected
void open_whitelists(Run &run) {
  const Options &opt = run.opt;
  cfr_status st;
  for (int g : opt.gpus) {
    cfr_barcode *w = nullptr;
    if ((st = cfr_barcode_open(opt.whitelist.c_str(), g, &w)) != CFR_OK) die_status("cfr_barcode_open", st);
    run.whitelists.push_back(w);
  }
  SeqReader rd(opt.bc_files);
  ByteBuf raw;
  std::vector<uint64_t> off, out_off;
  std::vector<uint8_t> out;
  size_t left = 2000000;
  bool more = true;
  while (more && left) {
    raw.clear(); off.assign(1, 0);
    bool hq = false;
    while (off.size() - 1 < std::min<size_t>(left, 1u << 18)) { if (!rd.next(nullptr, raw, nullptr, hq)) { more = false; break; } off.push_back(raw.size()); }
    const size_t n = off.size() - 1;
    if (!n) break;
    extract(opt.fmt, CFR_FORMAT_BARCODE, 0, raw.data(), off.data(), nullptr, nullptr, nullptr, n, out, out_off, nullptr);   // Extract into a buffer, as the background pass does (BarcodeCorrector.hpp:156)
    check_barcode_lengths(out_off.data(), n);
    for (cfr_barcode *w : run.whitelists) if ((st = cfr_barcode_count(w, out.data(), out_off.data(), n, n)) != CFR_OK) die_status("cfr_barcode_count", st);
    left -= n;
  }
}

// Correct, Translate or "N" (CentrifugerClass.cpp:186-206), on the GPU that classifies the batch: b.bc_str is what is printed
void correct_barcodes(const Run &run, size_t dev_no, Batch &b) {
  const Options &opt = run.opt;
  std::vector<int8_t> status(b.n, 0);
  std::vector<uint8_t> fixed;
  const uint8_t *bc = b.bc.data();
  if (!run.whitelists.empty()) {
    check_barcode_lengths(b.bc_off.data(), b.n);
    fixed.resize(b.bc_off[b.n] + 1);
    const cfr_status s = cfr_barcode_correct(run.whitelists[dev_no], b.bc.data(), b.bc_off.data(), b.bc_has_q ? (const char *)b.bc_q.data() : nullptr, b.n,
                                             std::max(1, opt.threads / (int)run.devs.size()), status.data(), fixed.data());
    if (s != CFR_OK) die_status("cfr_barcode_correct", s);
    bc = fixed.data();
  }
  if (!opt.translate_table) { strings(bc, b.bc_off.data(), b.n, status.data(), b.bc_str, b.bc_str_off); return; }
  std::vector<uint64_t> t_off(b.n + 1);
  std::vector<uint8_t> t;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) t.resize(t_off[b.n] + 1);
    if (cfr_barcode_translate_apply(opt.translate_table, bc, b.bc_off.data(), status.data(), b.n, pass ? t.data() : nullptr, t_off.data()) != CFR_OK) {
      std::cerr << cfr_last_error() << std::endl;          // BarcodeTranslator.hpp:70-72
      fflush(stdout);
      _exit(255);
    }
  }
  strings(t.data(), t_off.data(), b.n, nullptr, b.bc_str, b.bc_str_off);
}

// ---- reader stage: needs no index; it runs ahead of the index load ------------------------------------------------------------------
struct Reader {
  Run &run;
  const Options &opt;
  TakeSpec ts;
  std::unique_ptr<SeqReader> bc_reader, um_reader;
  std::atomic<size_t> bases_hint{0};

  explicit Reader(Run &r) : run(r), opt(r.opt) {
    ts.paired = opt.paired;
    ts.interleaved = !opt.inter.empty();
    ts.keep_qual = !opt.un_prefix.empty() || !opt.cl_prefix.empty() || opt.merge || opt.single_cell;   // (ReadPairMerger and BarcodeCorrector read the qualities)
    if (!opt.bc_files.empty()) { bc_reader.reset(new SeqReader(opt.bc_files)); bc_reader->want_comment = opt.bc_hd; }
    if (!opt.um_files.empty()) { um_reader.reset(new SeqReader(opt.um_files)); um_reader->want_comment = opt.um_hd; }
    ts.bc = bc_reader.get(); ts.um = um_reader.get();
    ts.r1_comment = (opt.has_barcode && !bc_reader && opt.bc_hd) || (opt.has_umi && !um_reader && opt.um_hd);
  }

  std::shared_ptr<Batch> fresh_batch() {
    std::shared_ptr<Batch> b = run.recycled.pop(false);
    if (!b) b = std::make_shared<Batch>();
    b->reset(opt.paired);
    b->bases1.reserve(bases_hint.load());                 // one allocation per batch object instead of a doubling series
    if (opt.paired) b->bases2.reserve(bases_hint.load());
    return b;
  }
  void publish(const std::shared_ptr<Batch> &b) {
    const size_t want = std::max(b->bases1.size(), b->bases2.size()) + (std::max(b->bases1.size(), b->bases2.size()) >> 3);
    size_t cur = bases_hint.load();
    while (want > cur && !bases_hint.compare_exchange_weak(cur, want)) {}
    run.in_order.push(b);
    run.pending.push(b);
  }

  void read_sequential(SeqReader *r1, SeqReader *r2) {
    bool more = true;
    while (more) {
      const auto tp = tick();
      std::shared_ptr<Batch> b = fresh_batch();
      while (b->n < opt.gpu_batch) {
        const int got = take(*b, ts, r1, r2, false);
        if (got < 0) die_mates();
        if (!got) { more = false; break; }
      }
      ByteBuf extra;
      bool hq2 = false;
      if (!more && opt.paired && !ts.interleaved && r2->next(nullptr, extra, nullptr, hq2)) die_mates();
      if (!more) for (SeqReader *r : {ts.bc, ts.um})
        if (r && r->next(nullptr, extra, nullptr, hq2)) { print_log("ERROR: The %s file and read file have different number of reads.", r == ts.bc ? "barcode" : "UMI"); exit(EXIT_FAILURE); }
      reformat(opt, *b);
      run.clk.add(T_PARSE, tp);
      if (b->n == 0) break;
      publish(b);
    }
  }

  // a worker's private copy of its piece: pread, not page faults on a mapping every thread shares
  static size_t fetch(const MappedFile &mf, size_t lo, size_t hi, std::vector<char> &dst) {
    const size_t span = hi - lo;
    if (dst.size() < span) dst.resize(span + (span >> 3));
    for (size_t got = 0; got < span;) {
      const ssize_t r = pread(mf.fd, dst.data() + got, span - got, (off_t)(lo + got));
      if (r <= 0) { print_log("ERROR: cannot read the read file."); exit(EXIT_FAILURE); }
      got += (size_t)r;
    }
    return span;
  }
  // The pieces of plain files, parsed by several threads and published in file order.  Single-end files are cut at verified
  // record starts about every batch's worth of bytes (plan_byte_cuts): every = 0, a piece holds what it holds.  Pairs: both mate
  // files (f2), or the interleaved file (no f2), are cut at the same RECORD numbers (plan_record_cuts), `every` pairs per piece of
  // `total`; a piece that does not hold exactly the records it was cut for stops the run (never a silent shift between mates).
  // die: the message for a piece that does not parse as it was cut, with one %lu (the byte, or the pair, where).
  void read_pieces(const MappedFile &f1, const std::vector<size_t> &c1, const MappedFile *f2, const std::vector<size_t> &c2, size_t every, size_t total,
                   const char *die) {
    const size_t npieces = c1.size() - 1;
    std::atomic<size_t> next_piece{0};
    std::mutex turn_mu;
    std::condition_variable turn_cv;
    size_t publish_next = 0;
    const int workers = std::max(1, std::min<int>(parse_workers(opt), (int)npieces));
    std::vector<std::thread> th;
    for (int w = 0; w < workers; ++w) th.emplace_back([&]() {
      std::vector<char> p1, p2;
      for (;;) {
        const size_t k = next_piece.fetch_add(1);
        if (k >= npieces) return;
        const auto tp = tick();
        std::shared_ptr<Batch> b = fresh_batch();
        const size_t want = every ? std::min(every, total - k * every) : 0;
        const size_t s1 = fetch(f1, c1[k], c1[k + 1], p1), s2 = f2 ? fetch(*f2, c2[k], c2[k + 1], p2) : 0;
        const PieceResult r = parse_piece(*b, ts, p1.data(), s1, f2 ? p2.data() : nullptr, s2, want);
        if (r.mate_missing) die_mates();
        if ((every && r.taken != want) || !r.done1 || !r.done2) {
          print_log(die, (unsigned long)(every ? k * every + b->n : c1[k + 1]));
          exit(EXIT_FAILURE);
        }
        run.clk.add(T_PARSE, tp);
        std::unique_lock<std::mutex> lk(turn_mu);
        turn_cv.wait(lk, [&]() { return publish_next == k; });
        if (b->n) publish(b);
        ++publish_next;
        turn_cv.notify_all();
      }
    });
    for (auto &x : th) x.join();
  }

  // --gpu-parse: every file must be a plain file that the record cutter accepts (pieces of --gpu-batch records that start and end at
  // verified record starts); otherwise nothing of the run takes this path.  The pieces go to the device workers unparsed.
  bool publish_raw() {
    struct RawPlan { const MappedFile *f1, *f2; std::vector<size_t> c1, c2; size_t total; const BgzfFile *z; };
    std::vector<RawPlan> plans;
    const char *why = nullptr;
    const std::vector<std::string> &first = opt.paired ? opt.m1 : opt.u;
    // --gpu-inflate: every -u file is planned by its own kind, plain or BGZF throughout; one file of neither kind and the run is what
    // it is without the switch
    std::vector<const BgzfFile *> zfile(first.size(), nullptr);
    if (run.gpu_inflate) {
      const char *why_z = nullptr;
      for (size_t i = 0; i < first.size() && !why_z; ++i) {
        MappedFile probe;
        if (first[i] != "-" && probe.open_plain(first[i])) continue;
        run.bgzf_files.emplace_back(new BgzfFile());
        BgzfFile &z = *run.bgzf_files.back();
        if (first[i] == "-" || !z.open(first[i])) why_z = "an input is neither a plain file nor BGZF throughout (plain gzip, stdin, or BGZF followed by plain members)";
        else if (!z.plan(opt.gpu_batch)) why_z = "the text of a BGZF file does not begin with a regular record (4-line FASTQ, or FASTA)";
        else {
          for (size_t k = 0; k + 1 < z.cut.size() && !why_z; ++k)
            if ((z.cut[k + 1] - z.cut[k] + 2 * 65536) >> 32) why_z = "a piece of the text has 4 GB or more";
          zfile[i] = &z;
        }
      }
      if (why_z) {
        print_log("--gpu-inflate is not used, the file is inflated on the host: %s.", why_z);
        run.gpu_inflate = false;
        if (!opt.gpu_parse) { run.gpu_parse = false; return false; }
        zfile.assign(first.size(), nullptr);
      }
    }
    for (size_t i = 0; i < first.size() && !why; ++i) {
      RawPlan p{nullptr, nullptr, {}, {}, 0, zfile[i]};
      if (p.z) { plans.push_back(std::move(p)); continue; }
      size_t t2 = 0;
      auto plan = [&](const std::string &f, const MappedFile *&mf, std::vector<size_t> &cuts, size_t &total) {
        run.raw_files.emplace_back(new MappedFile());
        mf = run.raw_files.back().get();
        if (f == "-" || !run.raw_files.back()->open_plain(f)) { why = "an input is not a plain FASTA/FASTQ file (gz, stdin, or too short)"; return; }
        if (!plan_record_cuts(*mf, opt.gpu_batch, parse_workers(opt), cuts, total)) { why = "a file is not made of regular records (4-line FASTQ, or FASTA)"; return; }
        for (size_t k = 0; k + 1 < cuts.size(); ++k) if ((cuts[k + 1] - cuts[k]) >> 32) why = "a piece of --gpu-batch records has 4 GB or more";
      };
      plan(first[i], p.f1, p.c1, p.total);
      if (!why && opt.paired) {
        plan(opt.m2[i], p.f2, p.c2, t2);
        if (!why && (t2 != p.total || p.c2.size() != p.c1.size())) why = "the mate files have different numbers of records";
      }
      plans.push_back(std::move(p));
    }
    if (why) {
      if (opt.gpu_parse) print_log("--gpu-parse is not used, the reads are parsed on the host: %s.", why);
      else print_log("--gpu-inflate is not used, the file is inflated on the host: %s.", why);
      run.gpu_inflate = false;
      return false;
    }
    for (const RawPlan &p : plans) {
      if (p.z) {                                         // the members that hold the piece's text, and where the piece lies in it
        const BgzfFile &z = *p.z;
        for (size_t k = 0; k + 1 < z.cut.size(); ++k) {
          if (z.cut[k + 1] == z.cut[k]) continue;
          std::shared_ptr<Batch> b = fresh_batch();
          b->raw = true;
          b->bgzf = &z;
          b->z_m0 = z.member_of(z.cut[k]); b->z_m1 = z.member_of(z.cut[k + 1] - 1) + 1;
          b->z_off = z.off[b->z_m0];
          b->raw1 = (const char *)z.base + b->z_off; b->raw1_len = z.off[b->z_m1] - b->z_off;
          b->z_skip = z.cut[k] - z.text[b->z_m0]; b->z_len = z.cut[k + 1] - z.cut[k];
          publish(b);
        }
        continue;
      }
      for (size_t k = 0; k + 1 < p.c1.size(); ++k) {
        std::shared_ptr<Batch> b = fresh_batch();
        b->raw = true;
        b->raw_first = k * opt.gpu_batch;
        b->raw_want = std::min(opt.gpu_batch, p.total - b->raw_first);
        b->raw1 = p.f1->base + p.c1[k]; b->raw1_len = p.c1[k + 1] - p.c1[k];
        if (p.f2) { b->raw2 = p.f2->base + p.c2[k]; b->raw2_len = p.c2[k + 1] - p.c2[k]; }
        publish(b);
      }
    }
    return true;
  }

  // one pair of mate files, or one interleaved file, in pieces; false: not plain files of regular shape, nothing was read
  bool read_pairs_in_pieces() {
    MappedFile f1, f2;
    std::vector<size_t> c1, c2;
    size_t t1 = 0, t2 = 0;
    const int pt = parse_workers(opt);
    if (ts.interleaved) {
      if (!(opt.inter.size() == 1 && opt.inter[0] != "-" && f1.open_plain(opt.inter[0]) && plan_record_cuts(f1, 2 * opt.gpu_batch, pt, c1, t1) && t1 % 2 == 0 && c1.size() >= 3)) return false;
      read_pieces(f1, c1, nullptr, c2, opt.gpu_batch, t1 / 2, "ERROR: the interleaved file is not made of regular records around pair %lu; rerun with --parse-threads 1.");
    } else {
      if (!(opt.m1.size() == 1 && opt.m2.size() == 1 && opt.m1[0] != "-" && opt.m2[0] != "-" && f1.open_plain(opt.m1[0]) && f2.open_plain(opt.m2[0]) &&
            plan_record_cuts(f1, opt.gpu_batch, pt, c1, t1) && plan_record_cuts(f2, opt.gpu_batch, pt, c2, t2) && c1.size() >= 3)) return false;
      if (t1 != t2) die_mates();
      read_pieces(f1, c1, &f2, c2, opt.gpu_batch, t1, "ERROR: the mate files are not made of regular records around pair %lu; rerun with --parse-threads 1.");
    }
    return true;
  }

  // Plain files are read in pieces by several threads; anything else (gz, stdin, files that do not verify, --parse-threads 1,
  // single-cell input) takes the sequential reader.
  void read_all() {
    const bool in_pieces = opt.parse_threads != 1;
    if (run.gpu_parse && publish_raw()) return;
    if (opt.paired && in_pieces && read_pairs_in_pieces()) return;
    if (opt.paired || !in_pieces) {
      std::unique_ptr<SeqReader> r1, r2;
      open_readers(opt, r1, r2);
      r1->want_comment = ts.r1_comment;
      read_sequential(r1.get(), r2.get());
      return;
    }
    for (const std::string &f : opt.u) {
      MappedFile mf;
      std::vector<size_t> cuts;
      if (f != "-" && mf.open_plain(f) && mf.resync(0) == 0) {
        // pieces of about one device batch: bytes per record from the first record
        const size_t rec_bytes = std::max<size_t>(16, mf.resync(1));
        plan_byte_cuts(mf, std::max<size_t>(1u << 16, rec_bytes * opt.gpu_batch), cuts);
      }
      if (cuts.size() >= 3) read_pieces(mf, cuts, nullptr, cuts, 0, 0, "ERROR: read file could not be cut at byte %lu; rerun with --parse-threads 1.");
      else { SeqReader r1(std::vector<std::string>{f}); read_sequential(&r1, nullptr); }
    }
  }
  void operator()() {
    read_all();
    run.pending.close();
    run.in_order.close();
  }
};

// the qualities of a batch as cfr_merge_pairs / cfr_classify_batch_merged take them: laid out by the bases' offsets, or none at all
void batch_quals(const Batch &b, const char *&q1, const char *&q2) {
  size_t with = 0;
  for (size_t i = 0; i < b.n; ++i) with += (b.has_qual[i] ? 1 : 0) + (b.has_qual2[i] ? 1 : 0);
  q1 = q2 = nullptr;
  if (with == 0) return;
  bool same = with == 2 * b.n;
  for (size_t i = 0; same && i <= b.n; ++i) same = b.q1_off[i] == b.offs1[i] && b.q2_off[i] == b.offs2[i];
  if (!same) {
    print_log("ERROR: --merge-readpair needs qualities for every read of both files (FASTQ, as long as the sequences) or for none (FASTA).");
    exit(EXIT_FAILURE);
  }
  q1 = b.qual1.data(); q2 = b.qual2.data();
}

// ---- dust stage (CentrifugerClass.cpp:276-316): needs no index either -------------------------------------------------------------
// The masking itself runs on the device inside the classify call (cfr_device_index_set_dust); the host stage only works
// when the masked reads are needed on the host as well (--un / --cl write them).
void dust_stage(Run &run, WorkerPool &pool) {
  const Options &opt = run.opt;
  while (std::shared_ptr<Batch> b = run.pending.pop()) {
    const auto ts = tick();
    uint8_t *dust1 = b->bases1.data(), *dust2 = b->paired ? b->bases2.data() : nullptr;
    const uint64_t *dust_o1 = b->offs1.data(), *dust_o2 = b->offs2.data();
    if (run.host_merge && b->n) {         // CentrifugerClass.cpp:271-273: the merge comes first
      const char *q1, *q2;
      batch_quals(*b, q1, q2);
      b->m_bases1.resize(b->offs1[b->n] + b->offs2[b->n] + 1); b->m_bases2.resize(b->offs2[b->n] + 1);
      b->m_offs1.resize(b->n + 1); b->m_offs2.resize(b->n + 1); b->merge_kind.resize(b->n);
      const cfr_status ms = cfr_merge_pairs(b->bases1.data(), b->offs1.data(), q1, b->bases2.data(), b->offs2.data(), q2, b->n, opt.threads,
                                            b->m_bases1.data(), b->m_offs1.data(), nullptr, b->m_bases2.data(), b->m_offs2.data(), nullptr,
                                            b->merge_kind.data(), nullptr, nullptr);
      if (ms != CFR_OK) die_status("cfr_merge_pairs", ms);
      dust1 = b->m_bases1.data(); dust2 = b->m_bases2.data(); dust_o1 = b->m_offs1.data(); dust_o2 = b->m_offs2.data();
    }
    if (run.host_dust) {      // slices of the batch on the stage's own workers (offsets are absolute, so a slice is just an offset window)
      const int parts = (int)std::min<size_t>((size_t)pool.size(), std::max<size_t>(1, b->n / 2048));
      pool.run(parts, [&](int t) {
        const size_t lo = b->n * (size_t)t / (size_t)parts, hi = b->n * (size_t)(t + 1) / (size_t)parts;
        cfr_dust_mask_batch(dust1, dust_o1 + lo, hi - lo, 1);
        if (b->paired) cfr_dust_mask_batch(dust2, dust_o2 + lo, hi - lo, 1);
      });
    }
    run.clk.add(T_DUST, ts);
    run.dusted.push(b);
  }
  run.dusted.close();
}

// ---- device stage: one worker per GPU takes dust-masked batches ---------------------------------------------------------------------
struct DeviceWorker {
  Run &run;
  cfr_dev_index *dev;
  size_t dev_no;
  cfr_tokenizer *tok1 = nullptr, *tok2 = nullptr;       // --gpu-parse: opened with the first raw batch, on this worker's GPU
  cfr_token_info tk1, tk2;
  cfr_inflate *inf = nullptr;                           // --gpu-inflate: opened with the first BGZF batch, beside the tokeniser
  std::vector<char> z_ids;
  std::vector<uint64_t> z_id_off;
  std::vector<cfr_read_record> recs;
  std::vector<char> id_bytes;                           // --gpu-format: the batch's ids without their terminators, and their n + 1 offsets
  std::vector<uint64_t> id_offs;
  size_t tsv_guess = 1 << 16;                           // ... and the size the text buffer starts with: the largest text so far, and a little
  cfr_gz *gz = nullptr;                                 // --gpu-dump: opened with the first batch, on this worker's GPU
  std::vector<uint8_t> dump_select;
  std::vector<char> dump_ids, dump_extra[2];
  std::vector<uint64_t> dump_id_off, dump_extra_off[2];

  // --gpu-parse: a raw batch on the worker's own tokeniser(s).  true: the reads are in HBM (ids in b.ids); false: the piece is not
  // regular, nothing was taken from it
  bool tokenize_raw(Batch &b) {
    for (cfr_tokenizer **t : {&tok1, &tok2})
      if (!*t && (t == &tok1 || b.raw2)) { const cfr_status s = cfr_tokenizer_open(run.opt.gpus[dev_no], t); if (s != CFR_OK) die_status("cfr_tokenizer_open", s); }
    cfr_status s = cfr_tokenize(tok1, (const uint8_t *)b.raw1, b.raw1_len, 1, b.raw_want, &tk1);
    if (s != CFR_OK) die_status("cfr_tokenize", s);
    bool ok = !tk1.irregular && tk1.n_records == b.raw_want && tk1.consumed == b.raw1_len;
    if (ok && b.raw2) {
      if ((s = cfr_tokenize(tok2, (const uint8_t *)b.raw2, b.raw2_len, 1, b.raw_want, &tk2)) != CFR_OK) die_status("cfr_tokenize", s);
      ok = !tk2.irregular && tk2.n_records == b.raw_want && tk2.consumed == b.raw2_len;
    }
    if (!ok) return false;
    b.n = b.raw_want;
    if (run.gpu_format) return true;               // the ids stay in HBM: the rows are made there (format_on_device), nothing else reads them
    recs.resize(b.raw_want);
    if ((s = cfr_tokenizer_fetch(tok1, recs.data(), nullptr, nullptr)) != CFR_OK) die_status("cfr_tokenizer_fetch", s);
    for (size_t i = 0; i < b.raw_want; ++i) {      // the ids for the TSV: from the record table and the mapped text
      const char *id = b.raw1 + recs[i].header + 1;
      b.id_off.push_back(b.ids.size());
      b.ids.insert(b.ids.end(), id, id + recs[i].id_len);
      b.ids.push_back('\0');
    }
    return true;
  }
  // --gpu-inflate: the batch's members are inflated in HBM and the piece of their text is tokenised where it lies.  true: the reads
  // are in HBM; false: the piece is not regular.  A member that does not inflate ends the run, as it does on the host path.
  bool tokenize_bgzf(Batch &b) {
    cfr_status s;
    if (!tok1 && (s = cfr_tokenizer_open(run.opt.gpus[dev_no], &tok1)) != CFR_OK) die_status("cfr_tokenizer_open", s);
    if (!inf && (s = cfr_inflate_open(run.opt.gpus[dev_no], &inf)) != CFR_OK) die_status("cfr_inflate_open", s);
    const uint8_t *text = nullptr;
    uint64_t text_n = 0;
    cfr_inflate_info info;
    if ((s = cfr_inflate_bgzf(inf, (const uint8_t *)b.raw1, b.raw1_len, 0, &text, &text_n, &info)) != CFR_OK) die_status("cfr_inflate_bgzf", s);
    if (info.bad_members) b.bgzf->bad_member(b.bgzf->off[b.z_m0 + info.first_bad]);
    const void *d_text = nullptr;
    if ((s = cfr_inflate_device_text(inf, &d_text, &text_n)) != CFR_OK) die_status("cfr_inflate_device_text", s);
    if ((s = cfr_tokenize_resident(tok1, (const uint8_t *)d_text + b.z_skip, b.z_len, 1, 0, &tk1)) != CFR_OK) die_status("cfr_tokenize_resident", s);
    if (tk1.irregular || tk1.consumed != b.z_len) return false;
    b.n = tk1.n_records;
    if (run.gpu_format) return true;               // the ids stay in HBM
    z_ids.resize(b.z_len + 1);                     // (no id is longer than its header line)
    z_id_off.resize(b.n + 1);
    if ((s = cfr_tokenizer_fetch_ids(tok1, z_ids.data(), z_ids.size(), z_id_off.data())) != CFR_OK) die_status("cfr_tokenizer_fetch_ids", s);
    for (size_t i = 0; i < b.n; ++i) {
      b.id_off.push_back(b.ids.size());
      b.ids.insert(b.ids.end(), z_ids.data() + z_id_off[i], z_ids.data() + z_id_off[i + 1]);
      b.ids.push_back('\0');
    }
    return true;
  }
  // ... and such a piece inflated with zlib and parsed with SeqReader
  void parse_bgzf_on_host(Batch &b) {
    b.z_text.clear();
    b.bgzf->inflate_members(b.z_m0, b.z_m1, b.z_text);
    TakeSpec ts;
    parse_piece(b, ts, b.z_text.data() + b.z_skip, b.z_len, nullptr, 0, 0);
  }
  // ... and the same pieces through SeqReader, as the parallel readers of the host path take them
  void parse_raw_on_host(Batch &b) {
    TakeSpec ts;
    ts.paired = b.raw2 != nullptr;
    const PieceResult r = parse_piece(b, ts, b.raw1, b.raw1_len, b.raw2, b.raw2_len, 0);
    if (r.mate_missing) die_mates();
    if (b.raw2 && (b.n != b.raw_want || !r.done2)) {
      print_log("ERROR: the mate files are not made of regular records around pair %lu; rerun without --gpu-parse and with --parse-threads 1.", (unsigned long)(b.raw_first + b.n));
      exit(EXIT_FAILURE);
    }
  }
  // true: the batch's reads are resident in HBM, made by the tokeniser(s)
  bool take_raw(Batch &b) {
    bool resident = false;
    if (!run.raw_broken.load()) {
      resident = b.bgzf ? tokenize_bgzf(b) : tokenize_raw(b);
      if (!resident && !run.raw_broken.exchange(true)) {
        if (run.gpu_inflate) print_log("--gpu-inflate stops here, the rest is inflated and parsed on the host: a piece of the input is not made of regular records.");
        else print_log("--gpu-parse stops here, the rest is parsed on the host: a piece of the input is not made of regular records.");
      }
    }
    if (!resident) { if (b.bgzf) parse_bgzf_on_host(b); else parse_raw_on_host(b); }
    return resident;
  }

  void classify(Batch &b, bool resident) {
    const Options &opt = run.opt;
    b.results.resize(b.n);
    size_t cap = b.n * (size_t)(opt.params.max_result > 0 ? opt.params.max_result : 4) + 16, used = 0;
    size_t ids_cap = run.expand ? std::max<size_t>(b.exp_ids.size(), 4 * b.n + 16) : 0, ids_used = 0;
    // the reads the device gets: the batch as it was read (and masked), or what the host merge made of it
    const bool merged_here = run.host_merge && b.n;
    const uint8_t *in1 = merged_here ? b.m_bases1.data() : b.bases1.data();
    const uint8_t *in2 = !b.paired ? nullptr : merged_here ? b.m_bases2.data() : b.bases2.data();
    const uint64_t *in_o1 = merged_here ? b.m_offs1.data() : b.offs1.data();
    const uint64_t *in_o2 = !b.paired ? nullptr : merged_here ? b.m_offs2.data() : b.offs2.data();
    const char *mq1 = nullptr, *mq2 = nullptr;
    const bool device_merge = opt.merge && !run.host_merge && b.paired && b.n;
    if (device_merge) batch_quals(b, mq1, mq2);
    for (;;) {
      b.matches.resize(cap);
      cfr_status s;
      if (run.expand) {
        b.spans.resize(cap);
        b.exp_ids.resize(ids_cap);
        s = cfr_classify_batch_expanded(dev, in1, in_o1, in2, in_o2, b.n, b.results.data(), b.matches.data(), b.spans.data(), cap, &used,
                                        b.exp_ids.data(), ids_cap, &ids_used);
      } else if (resident) {
        const void *d_b1 = nullptr, *d_o1 = nullptr, *d_b2 = nullptr, *d_o2 = nullptr;
        cfr_tokenizer_device_reads(tok1, &d_b1, &d_o1);
        if (b.raw2) cfr_tokenizer_device_reads(tok2, &d_b2, &d_o2);
        s = cfr_classify_batch_resident(dev, d_b1, d_o1, d_b2, d_o2, b.n, tk1.total_bases, b.raw2 ? tk2.total_bases : 0, b.results.data(), b.matches.data(), cap, &used);
      } else if (device_merge)
        s = cfr_classify_batch_merged(dev, in1, in_o1, mq1, in2, in_o2, mq2, b.n, b.results.data(), b.matches.data(), cap, &used, nullptr);
      else
        s = cfr_classify_batch(dev, in1, in_o1, in2, in_o2, b.n, b.results.data(), b.matches.data(), cap, &used);
      if (s == CFR_ERR_CAPACITY) { if (used > cap) cap = used + 16; if (ids_used > ids_cap) ids_cap = ids_used + 16; continue; }
      if (s != CFR_OK) die_status("cfr_classify_batch", s);
      break;
    }
    // --quant: the quantifier of centrifuger-quant beside the classifier (Quantifier::AddReadAssignment, Quantifier.hpp:624-637): every
    // batch's results go into it on the worker that holds them; it coalesces them in the HBM of the first GPU of the run
    if (run.quant) {
      std::lock_guard<std::mutex> ql(run.quant_mu);
      const cfr_status s = cfr_quant_add_results(run.quant, b.results.data(), b.matches.data(), b.n);
      if (s != CFR_OK) die_status("cfr_quant_add_results", s);
    }
    // --kreport: the reads were counted in HBM by the call above; the script's warning lines come from a host scan of the reads that
    // carry a tax id without a node (none under --promote: the host then holds promoted assignments)
    if (run.kreport && !opt.has_promote) {
      std::lock_guard<std::mutex> kl(run.kreport_mu);
      const cfr_status s = cfr_kreport_scan_warnings(run.kreport, b.results.data(), b.matches.data(), b.n);
      if (s != CFR_OK) die_status("cfr_kreport_scan_warnings", s);
    }
  }

  // --gpu-format: the rows of the batch the device has just classified, as the batch's single TSV part.  The ids come from the
  // tokeniser's tables in HBM (a resident batch) or go up as bytes.
  void format_on_device(Batch &b, bool resident) {
    if (b.tsv_parts.empty()) { b.tsv_parts.resize(1); b.part_hits.resize(1); }
    std::string &out = b.tsv_parts[0];
    b.n_parts = 1;
    b.tsv_device = true;
    if (!b.n) { out.clear(); return; }
    const void *d_text = nullptr, *d_rec = nullptr;
    if (resident) {
      const cfr_status s = cfr_tokenizer_device_records(tok1, &d_text, &d_rec);
      if (s != CFR_OK) die_status("cfr_tokenizer_device_records", s);
    } else {
      id_bytes.clear(); id_offs.clear();
      for (size_t i = 0; i < b.n; ++i) {
        const char *id = b.id(i);
        id_offs.push_back(id_bytes.size());
        id_bytes.insert(id_bytes.end(), id, id + strlen(id));
      }
      id_offs.push_back(id_bytes.size());
    }
    uint64_t len = 0;
    if (out.size() < tsv_guess) out.resize(tsv_guess);
    for (;;) {
      const cfr_status s = resident ? cfr_device_index_tsv_last_resident(dev, d_text, d_rec, &out[0], out.size(), &len, nullptr)
                                    : cfr_device_index_tsv_last(dev, id_bytes.data(), id_offs.data(), &out[0], out.size(), &len, nullptr);
      if (s == CFR_ERR_CAPACITY && len > out.size()) { out.resize(len + len / 16); continue; }
      if (s != CFR_OK) die_status("cfr_device_index_tsv_last", s);
      break;
    }
    tsv_guess = std::max<size_t>(tsv_guess, len + len / 16);
    out.resize(len);
    float ms = 0.f;
    if (cfr_last_tsv_ms(dev, &ms) == CFR_OK) run.tsv_kernel_ns += (long long)((double)ms * 1e6);
  }

  // --gpu-dump: the records of the batch's classified and unclassified reads made and compressed on this worker's GPU, from the arrays
  // write_stage prints them from (masked bases, as the dust stage left them); the members wait on the batch for the writer
  void dump_on_device(Batch &b) {
    const Options &opt = run.opt;
    b.dump_device = true;
    for (auto &set : b.dump_parts) for (auto &s : set) s.clear();
    if (!b.n) return;
    if (!gz) {
      cfr_gz_options gz_opt;
      cfr_gz_options_default(&gz_opt);
      gz_opt.codes = opt.gpu_dump_dynamic ? 1 : 0;
      const cfr_status s = cfr_gz_open(opt.gpus[dev_no], &gz_opt, &gz);
      if (s != CFR_OK) die_status("cfr_gz_open", s);
    }
    static const char kNone[1] = {0};
    auto strings = [&](const std::vector<char> &text, const std::vector<size_t> &at, std::vector<char> &bytes, std::vector<uint64_t> &off) {   // NUL-terminated -> bytes + offsets
      bytes.clear(); off.clear();
      for (size_t i = 0; i < b.n; ++i) {
        const char *s = text.data() + at[i];
        off.push_back(bytes.size());
        bytes.insert(bytes.end(), s, s + strlen(s));
      }
      off.push_back(bytes.size());
    };
    strings(b.ids, b.id_off, dump_ids, dump_id_off);
    cfr_gz_file files[4];
    int slot_of[4], n_files = 0;
    auto reads = [&](int slot, const ByteBuf &bases, const std::vector<uint64_t> &offs, const std::vector<char> &qual, const std::vector<size_t> &q_off, const std::vector<uint8_t> &has) {
      static_assert(sizeof(size_t) == sizeof(uint64_t), "the quality offsets are handed over as they are");
      files[n_files] = cfr_gz_file{bases.data(), offs.data(), qual.empty() ? kNone : qual.data(), reinterpret_cast<const uint64_t *>(q_off.data()), has.data()};
      slot_of[n_files++] = slot;
    };
    reads(0, b.bases1, b.offs1, b.qual1, b.q1_off, b.has_qual);
    if (b.paired) reads(1, b.bases2, b.offs2, b.qual2, b.q2_off, b.has_qual2);
    if (opt.has_barcode) {
      strings(b.bc_str, b.bc_str_off, dump_extra[0], dump_extra_off[0]);
      files[n_files] = cfr_gz_file{(const uint8_t *)dump_extra[0].data(), dump_extra_off[0].data(), nullptr, nullptr, nullptr};
      slot_of[n_files++] = 2;
    }
    if (opt.has_umi) {
      strings(b.um_str, b.um_str_off, dump_extra[1], dump_extra_off[1]);
      files[n_files] = cfr_gz_file{(const uint8_t *)dump_extra[1].data(), dump_extra_off[1].data(), nullptr, nullptr, nullptr};
      slot_of[n_files++] = 3;
    }
    dump_select.resize(b.n);
    for (int set = 0; set < 2; ++set) {                 // 0: --un, 1: --cl
      if (!(set ? run.raw_cl.on() : run.raw_un.on())) continue;
      for (size_t i = 0; i < b.n; ++i) dump_select[i] = (b.results[i].n_match > 0) == (set == 1) ? 1 : 0;
      const uint8_t *out[4];
      uint64_t out_n[4];
      const cfr_status s = cfr_gz_dump(gz, dump_ids.data(), dump_id_off.data(), dump_select.data(), b.n, files, n_files, out, out_n);
      if (s != CFR_OK) die_status("cfr_gz_dump", s);
      for (int f = 0; f < n_files; ++f) b.dump_parts[set][slot_of[f]].assign((const char *)out[f], out_n[f]);
      cfr_gz_stats st;
      if (cfr_gz_get_stats(gz, &st) == CFR_OK) run.dump_kernel_ns += (long long)((double)(st.format_ms + st.deflate_ms + st.pack_ms) * 1e6);
    }
  }

  void operator()() {
    while (std::shared_ptr<Batch> b = run.dusted.pop()) {
      auto ts = tick();
      bool resident = false;
      if (b->raw) {
        resident = take_raw(*b);
        run.clk.add(T_PARSE, ts);
        ts = tick();
      }
      if (run.opt.has_barcode && b->n) correct_barcodes(run, dev_no, *b);
      classify(*b, resident);
      run.clk.add(T_CLASSIFY, ts);
      if (run.gpu_format) {
        ts = tick();
        format_on_device(*b, resident);
        run.clk.add(T_FORMAT, ts);
      }
      if (run.gpu_dump) {
        ts = tick();
        dump_on_device(*b);
        run.dump_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(tick() - ts).count();
      }
      run.classified.push(b);
    }
    cfr_gz_close(gz);
    cfr_tokenizer_close(tok1);
    cfr_tokenizer_close(tok2);
    cfr_inflate_close(inf);
    run.classified.close();
  }
};

// ---- format stage: TSV rows (ResultWriter::Output), formatted in parallel slices; the writer puts them out in order -------------------
void format_stage(Run &run, WorkerPool &pool) {
  const Options &opt = run.opt;
  while (std::shared_ptr<Batch> b = run.classified.pop()) {
    const auto ts = tick();
    if (b->tsv_device) {                     // --gpu-format: the device worker made the rows; what is left is the count of classified reads
      size_t hits = 0;
      for (size_t i = 0; i < b->n; ++i) hits += b->results[i].n_match > 0 ? 1 : 0;
      b->part_hits[0] = hits;
      run.clk.add(T_FORMAT, ts);
      run.in_order.mark_done(*b);
      continue;
    }
    const int nt = (int)std::min<size_t>((size_t)pool.size(), std::max<size_t>(1, b->n / 4096));
    if (b->tsv_parts.size() < (size_t)nt) { b->tsv_parts.resize((size_t)nt); b->part_hits.resize((size_t)nt); }
    b->n_parts = (size_t)nt;
    pool.run(nt, [&](int t) {
      const size_t lo = b->n * (size_t)t / (size_t)nt, hi = b->n * (size_t)(t + 1) / (size_t)nt;
      std::string &out = b->tsv_parts[(size_t)t];
      out.clear();
      if (out.capacity() < (hi - lo) * 64) out.reserve((hi - lo) * 96);
      size_t hits = 0;
      for (size_t i = lo; i < hi; ++i) hits += b->results[i].n_match > 0 ? 1 : 0;
      b->part_hits[(size_t)t] = hits;
      char buf[8192];
      auto row = [&](size_t i, char *dst, size_t cap) {
        if (opt.single_cell)
          return cfr_format_tsv_ex(run.idx, b->id(i), &b->results[i], b->matches.data(), opt.has_barcode, opt.has_barcode ? b->bc_str.data() + b->bc_str_off[i] : nullptr, opt.has_umi,
                                   opt.has_umi ? b->um_str.data() + b->um_str_off[i] : nullptr, run.expand, b->spans.data(), b->exp_ids.data(), dst, cap);
        return run.expand ? cfr_format_tsv_expanded(run.idx, b->id(i), &b->results[i], b->matches.data(), b->spans.data(), b->exp_ids.data(), dst, cap)
                          : cfr_format_tsv(run.idx, b->id(i), &b->results[i], b->matches.data(), dst, cap);
      };
      for (size_t i = lo; i < hi; ++i) {
        size_t w = row(i, buf, sizeof(buf));
        if (w < sizeof(buf)) out.append(buf, w);
        else {
          std::string big(w + 1, '\0');
          row(i, &big[0], big.size());
          out.append(big.data(), w);
        }
      }
    });
    run.clk.add(T_FORMAT, ts);
    run.in_order.mark_done(*b);
  }
}

// ---- writer: the batches in input order to stdout and to the --un / --cl dumps; then their buffers go back to the reader -----------
void write_stage(Run &run) {
  const Options &opt = run.opt;
  ReadDump &un = run.un, &cl = run.cl;
  while (std::shared_ptr<Batch> b = run.in_order.pop()) {
    const auto tw = tick();
    for (size_t t = 0; t < b->n_parts; ++t) { fwrite(b->tsv_parts[t].data(), 1, b->tsv_parts[t].size(), stdout); run.classified_reads += b->part_hits[t]; }
    run.total += b->n;
    if (b->dump_device) {                    // --gpu-dump: the device worker made the members of every file
      for (int k = 0; k < 4; ++k) { run.raw_un.put(k, b->dump_parts[0][k]); run.raw_cl.put(k, b->dump_parts[1][k]); }
    } else if (cl.fp[0] || un.fp[0]) for (size_t i = 0; i < b->n; ++i) {
      const bool hit = b->results[i].n_match > 0;
      ReadDump *dump = hit ? (cl.fp[0] ? &cl : nullptr) : (un.fp[0] ? &un : nullptr);
      if (!dump) continue;
      // --merge-readpair: a merged pair is dumped as its original mates (only the merged read was masked, CentrifugerClass.cpp:304-315),
      // every other pair as the masked mates (which the host merge left in its own buffers)
      const bool from_merge = run.host_merge && !b->merge_kind[i];
      const uint8_t *s1 = from_merge ? b->m_bases1.data() + b->m_offs1[i] : b->bases1.data() + b->offs1[i];
      dump->put(0, b->id(i), s1, b->offs1[i + 1] - b->offs1[i],
                b->has_qual[i] ? b->qual1.data() + b->q1_off[i] : nullptr, b->q1_off[i + 1] - b->q1_off[i]);
      if (b->paired) {
        const uint8_t *s2 = from_merge ? b->m_bases2.data() + b->m_offs2[i] : b->bases2.data() + b->offs2[i];
        dump->put(1, b->id(i), s2, b->offs2[i + 1] - b->offs2[i],
                  b->has_qual2[i] ? b->qual2.data() + b->q2_off[i] : nullptr, b->q2_off[i + 1] - b->q2_off[i]);
      }
      if (opt.has_barcode) dump->put_extra(2, b->id(i), b->bc_str.data() + b->bc_str_off[i]);
      if (opt.has_umi) dump->put_extra(3, b->id(i), b->um_str.data() + b->um_str_off[i]);
    }
    run.clk.add(T_WRITE, tw);
    run.recycled.push(b);
  }
}

// ---- what is decided before any stage starts: the devices, the dumps, which stages work on the host -----------------------------
int plan_run(Run &run) {
  Options &opt = run.opt;
  // ---- --gpu-dump: the dumps are made and compressed by the device workers; the rule of --gpu-parse and --gpu-format for what is not covered
  run.gpu_dump = opt.gpu_dump;
  if (run.gpu_dump) {
    if (opt.un_prefix.empty() && opt.cl_prefix.empty()) { print_log("--gpu-dump has no effect: neither --un nor --cl is given."); run.gpu_dump = false; }
    else if (opt.merge) {
      print_log("--gpu-dump is not used, the dumps are written on the host: --merge-readpair takes every mate from one of two buffers.");
      run.gpu_dump = false;
    }
  }
  if (opt.gpu_dump_dynamic && !run.gpu_dump) { print_log("--gpu-dump-codes dynamic has no effect: the dumps are not made on the GPU."); opt.gpu_dump_dynamic = false; }
  if (run.gpu_dump) {
    if (!opt.un_prefix.empty()) run.raw_un.open(opt.un_prefix, opt.paired, opt.has_barcode, opt.has_umi);
    if (!opt.cl_prefix.empty()) run.raw_cl.open(opt.cl_prefix, opt.paired, opt.has_barcode, opt.has_umi);
  } else {
    if (!opt.un_prefix.empty()) run.un.open(opt.un_prefix, opt.paired, opt.has_barcode, opt.has_umi);
    if (!opt.cl_prefix.empty()) run.cl.open(opt.cl_prefix, opt.paired, opt.has_barcode, opt.has_umi);
  }
  if (!opt.all_gpus && opt.gpus.empty()) { print_log("ERROR: no MI355X device selected."); return EXIT_FAILURE; }
  if (opt.all_gpus) {
    int cnt = 0;
    cfr_device_count(&cnt);
    opt.gpus.clear();
    for (int g = 0; g < cnt; ++g) opt.gpus.push_back(g);
    if (opt.gpus.empty()) { print_log("ERROR: no MI355X device found (this build has no CPU fallback)."); return EXIT_FAILURE; }
  }
  // a protein index (.4.cfr says sequence_type amino_acid, Classifier::IsProteinDatabase) is searched translated and never
  // dust-masked (CentrifugerClass.cpp:248, 276); the stages must know before the index itself is loaded
  run.protein = index_is_protein(opt.idx);
  // ---- --gpu-parse: where it applies the reader hands out unparsed pieces of the mapped files and the device workers tokenise them;
  // everywhere else the run is what it is without the switch, and one log line says why
  run.gpu_parse = opt.gpu_parse;
  {
    const char *why = nullptr;
    if (!opt.un_prefix.empty() || !opt.cl_prefix.empty()) why = "--un / --cl need the reads and their qualities on the host";
    else if (opt.merge) why = "--merge-readpair needs the qualities";
    else if (opt.params.output_expanded) why = "--expand-taxid has a classify entry of its own";
    else if (!opt.inter.empty()) why = "interleaved files (-i) are not covered";
    else if (opt.single_cell) why = "the single-cell options read several files in step";
    else if (run.protein) why = "a protein index is not covered";
    if (run.gpu_parse && why) { print_log("--gpu-parse is not used, the reads are parsed on the host: %s.", why); run.gpu_parse = false; }
    // ---- --gpu-inflate: the same rule, under the conditions of --gpu-parse, which it implies; -u files only (the reader decides per file)
    if (opt.gpu_inflate) {
      if (!why && opt.paired) why = "two BGZF mate files (-1/-2) cannot be cut at the same pair without inflating them";
      if (why) print_log("--gpu-inflate is not used, the file is inflated on the host: %s.", why);
      else run.gpu_inflate = run.gpu_parse = true;
    }
  }
  // ---- --gpu-format: the same rule
  run.gpu_format = opt.gpu_format;
  if (run.gpu_format) {
    const char *why = nullptr;
    if (opt.params.output_expanded) why = "the expandedTaxIDs column of --expand-taxid is not made on the device";
    else if (opt.single_cell) why = "the barcode and UMI columns are not made on the device";
    else if (opt.params.max_result <= 0) why = "the device keeps -k result slots per read, -k must be positive";
    if (why) { print_log("--gpu-format is not used, the rows are formatted on the host: %s.", why); run.gpu_format = false; }
  }
  if (run.protein) opt.dust = false;
  if (run.protein && opt.merge) {
    print_log("ERROR: --merge-readpair is not available with a protein index in this build: a merged pair is searched as one read with an "
              "empty mate, and the translated search of an empty mate is not verified.");
    return EXIT_FAILURE;
  }
  run.dumps = !opt.un_prefix.empty() || !opt.cl_prefix.empty();
  run.host_dust = opt.dust && run.dumps;
  // the dumps need to know which pairs merged before the masking: merge, then SDUST, on the host.  (--expand-taxid has its own classify
  // entry, which takes reads that are merged already)
  run.expand = opt.params.output_expanded != 0;
  run.host_merge = opt.merge && (run.dumps || run.expand);
  run.classified.producers(opt.gpus.size());
  return -1;
}

// ---- index load and device images, while the reader and dust threads already work on the first batches ---------------------------
void load_index_and_devices(Run &run) {
  const Options &opt = run.opt;
  auto t0 = tick();
  cfr_status st = cfr_index_open(opt.idx.c_str(), &opt.params, &run.idx);
  if (st != CFR_OK) die_status("loading the index", st);
  run.clk.add(T_OPEN, t0);
  cfr_index_info info;
  cfr_index_get_info(run.idx, &info);
  if (info.is_protein) print_log("This is a protein database and will use translated search.");
  print_log("Finishes loading index.");
  if (opt.params.min_hit_len <= 0) print_log("Inferred --min-hitlen: %d", info.min_hit_len);
  t0 = tick();
  cfr_device_options dopt;
  cfr_device_options_default(&dopt);
  // default: the fast-load image.  This program hands the device pageable host buffers, which bounds the device stage at
  // ~30 M reads/s whatever the tables (profiles/r2f_cli_timing.txt): what a run feels is the load time.  --gpu-balanced adds the
  // text-mode tables and the locate memo (+0.4 s per Gbp), --gpu-throughput the 68 GB K-mer table as well.
  dopt.profile = opt.throughput_profile ? CFR_PROFILE_THROUGHPUT : opt.balanced_profile ? CFR_PROFILE_BALANCED : CFR_PROFILE_FAST_LOAD;
  // no profile asked for: by the size of the input.  The fast-load image classifies ~30 M reads/s; the text-mode tables of the
  // balanced image cost ~0.4 s per Gbp of index once and lift that several-fold, which pays from a few GB of reads on (plain
  // files: bytes on disk; gz: ~4x that when inflated; stdin: unknown, stays fast-load).
  if (!opt.throughput_profile && !opt.balanced_profile && input_bytes(opt, 4) >= (8ull << 30)) dopt.profile = CFR_PROFILE_BALANCED;
  for (int g : opt.gpus) {
    cfr_dev_index *d = nullptr;
    st = cfr_device_index_create_ex(run.idx, g, &dopt, &d);
    if (st != CFR_OK) die_status("creating the device index (this build has no CPU fallback)", st);
    if (opt.dust && !run.host_dust) cfr_device_index_set_dust(d, 1);
    if (opt.merge && !run.host_merge && (st = cfr_device_index_set_merge(d, 1)) != CFR_OK) die_status("cfr_device_index_set_merge", st);
    if (opt.has_promote && (st = cfr_device_index_set_promote(d, opt.promote.c_str())) != CFR_OK) die_status("cfr_device_index_set_promote", st);
    if (!opt.kreport_path.empty()) {
      cfr_kreport_options ko;
      cfr_kreport_options_default(&ko);
      if ((st = cfr_device_index_set_kreport(d, &ko)) != CFR_OK) die_status("cfr_device_index_set_kreport", st);
    }
    if (run.gpu_format && (st = cfr_device_index_set_tsv(d, 1)) != CFR_OK) die_status("cfr_device_index_set_tsv", st);
    run.devs.push_back(d);
  }
  run.clk.add(T_DEVICE, t0);
  if (!opt.whitelist.empty()) open_whitelists(run);
  fputs(opt.single_cell ? cfr_tsv_header_ex(opt.has_barcode, opt.has_umi, run.expand) : run.expand ? cfr_tsv_header_expanded() : cfr_tsv_header(), stdout);   // only once the index and the devices are up: a failed load prints no TSV at all
  if (!opt.quant_path.empty()) {
    cfr_quant_options qo;
    cfr_quant_options_default(&qo);
    qo.device = opt.gpus[0];
    const cfr_status s = cfr_quant_open(opt.idx.c_str(), &qo, &run.quant);
    if (s != CFR_OK) die_status("cfr_quant_open", s);
  }
  if (!opt.kreport_path.empty()) {
    cfr_kreport_options ko;
    cfr_kreport_options_default(&ko);
    const cfr_status s = cfr_kreport_open(opt.idx.c_str(), &ko, -1, &run.kreport);      // (host handle: the roll-up and the writer; the counting is the devices')
    if (s != CFR_OK) die_status("cfr_kreport_open", s);
  }
}

// ---- after the last batch: the summary line, the --quant report, and the exit status ---------------------------------------------
[[noreturn]] void finish(Run &run) {
  const Options &opt = run.opt;
  run.un.close();
  run.cl.close();
  run.raw_un.close();
  run.raw_cl.close();
  fflush(stdout);
  // ResultWriter::Finalize (ResultWriter.hpp:279-283)
  print_log("Processed %lu read fragments, and %lu (%.2lf%%) can be classified.", (unsigned long)run.total, (unsigned long)run.classified_reads,
            run.total ? (double)run.classified_reads / (double)run.total * 100.0 : 0.0);
  if (run.quant) {
    cfr_status s = cfr_quant_run(run.quant, nullptr);
    if (s != CFR_OK) die_status("cfr_quant_run", s);
    s = cfr_quant_write(run.quant, opt.quant_format, opt.quant_path.c_str());
    if (s != CFR_OK) die_status("cfr_quant_write", s);
    cfr_quant_destroy(run.quant);
  }
  if (run.kreport) {                        // every device's bins summed into the host handle, then the script's report
    size_t nb = 0;
    cfr_kreport_bins(run.kreport, &nb);
    std::vector<uint64_t> own(nb), score(nb);
    for (auto *d : run.devs) {
      cfr_status s = cfr_device_index_kreport_counts(d, own.data(), score.data(), nb, nullptr);
      if (s != CFR_OK) die_status("cfr_device_index_kreport_counts", s);
      if ((s = cfr_kreport_add_counts(run.kreport, own.data(), score.data(), nb)) != CFR_OK) die_status("cfr_kreport_add_counts", s);
    }
    size_t nw = 0;
    (void)cfr_kreport_warnings(run.kreport, nullptr, 0, &nw);
    if (opt.has_promote) print_log("--kreport: tax ids without a node are counted at the root; their lines are not counted under --promote.");
    else if (nw) print_log("--kreport: %lu tax ids without a node were assigned to the root (centrifuger-kreport prints a line for each).", (unsigned long)nw);
    if (run.total == 0) print_log("--kreport: no reads, no report (centrifuger-kreport: No sequence matches with given settings).");
    else {
      const cfr_status s = cfr_kreport_write(run.kreport, opt.kreport_path.c_str());
      if (s != CFR_OK) die_status("cfr_kreport_write", s);
    }
    cfr_kreport_close(run.kreport);
  }
  for (auto *w : run.whitelists) cfr_barcode_destroy(w);
  for (auto *d : run.devs) cfr_device_index_destroy(d);
  cfr_index_destroy(run.idx);
  run.clk.add(T_WALL, run.t_wall);
  if (const char *e = getenv("CFR_CLI_TIMING")) if (atoi(e)) {
    static const char *names[] = {"index_open", "device_index", "parse", "dust", "classify", "format", "write", "wall"};
    for (int k = 0; k < 8; ++k) fprintf(stderr, "[timing] %-12s %8.3f s\n", names[k], (double)run.clk.ns[k].load() * 1e-9);
    if (run.gpu_format) fprintf(stderr, "[timing] %-12s %8.3f s\n", "tsv_kernels", (double)run.tsv_kernel_ns.load() * 1e-9);
    if (run.gpu_dump) {
      fprintf(stderr, "[timing] %-12s %8.3f s\n", "dump", (double)run.dump_ns.load() * 1e-9);
      fprintf(stderr, "[timing] %-12s %8.3f s\n", "dump_kernels", (double)run.dump_kernel_ns.load() * 1e-9);
    }
  }
  // the TSV must have reached its destination before success is reported (a full disk or a closed pipe otherwise ends in a
  // truncated file with exit status 0); only then is the runtime's teardown skipped (~0.3 s of a sub-second run)
  if (fflush(stdout) != 0 || ferror(stdout)) {
    print_log("ERROR: writing the classification output failed (%s).", strerror(errno));
    fflush(stderr);
    _exit(EXIT_FAILURE);
  }
  print_log("Centrifuger finishes.");
  fflush(stderr);
  _exit(0);
}

}  // namespace

int main(int argc, char *argv[]) {
  Options opt;
  int status = parse_options(argc, argv, opt);
  if (status >= 0) return status;
  if (const char *e = getenv("CFR_CLI_PARSE_ONLY")) if (atoi(e)) return run_parse_only(opt, atoi(e));
  // pinned batch buffers pay off once the input is large (they cost ~0.4 s of allocation per GB of buffers)
  ByteBuf::use_pinned = input_bytes(opt, 1) > 20ull << 30;
  if (const char *e = getenv("CFR_CLI_PIN")) ByteBuf::use_pinned = atoi(e) != 0;
  Run run(opt);
  if ((status = plan_run(run)) >= 0) return status;

  Reader read_stage(run);
  std::thread reader(std::ref(read_stage));
  WorkerPool dust_pool(run.host_dust || run.host_merge ? opt.threads : 1), format_pool(opt.threads);
  std::thread duster(dust_stage, std::ref(run), std::ref(dust_pool));

  load_index_and_devices(run);

  std::vector<DeviceWorker> device_stage;
  for (size_t k = 0; k < run.devs.size(); ++k) device_stage.push_back(DeviceWorker{run, run.devs[k], k});
  std::vector<std::thread> workers;
  for (DeviceWorker &w : device_stage) workers.emplace_back(std::ref(w));
  std::thread formatter(format_stage, std::ref(run), std::ref(format_pool));
  write_stage(run);

  reader.join();
  duster.join();
  for (auto &w : workers) w.join();
  formatter.join();
  finish(run);
}
