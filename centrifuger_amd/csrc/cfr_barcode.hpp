// cfr_barcode.hpp — single-cell input: read formats, barcode whitelist correction and barcode translation.
//
// Host twins: literal restatements of ReadFormatter (ReadFormatter.hpp:49-422), Trie / BarcodeCorrector (BarcodeCorrector.hpp:10-235)
// and BarcodeTranslator (BarcodeTranslator.hpp:40-112); cfr_barcode.cpp.  The device side of the whitelist (cfr_barcode.hip) is a
// hash table in HBM that is tested against the twin.
//
// Where the reference's behaviour is undefined, the twins do this instead (all of it outside what the reference's own tests reach):
//   * a byte outside 'A'..'Z' indexes Trie::nucToNum out of bounds (BarcodeCorrector.hpp:74, :99): here it is any other byte that is
//     not A, C, G or T - the whitelist entry is skipped, the barcode is not found;
//   * Trie::Insert reads `newElem` uninitialised (:71, :90): the whitelist size here is the number of distinct valid entries;
//   * Correct copies the barcode into char[256] (:168, :179): a barcode of 256 bytes or more is refused;
//   * a segment that starts before the first byte (a negative start on a short read) reads in front of the string
//     (ReadFormatter.hpp:380-392): those positions are left out;
//   * the output of unsorted segments may outgrow the reference's buffer of len + 1 bytes (:318): here it grows;
//   * a number of 20 characters or more in a format string overflows buffer[20] (:52): the format is refused;
//   * a translation line without separator, or with an empty `from`, throws or divides by zero (BarcodeTranslator.hpp:65, :103):
//     the table is refused.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "cfr_index.hpp"

namespace cfr {

enum { kFormatRead1 = 0, kFormatRead2 = 1, kFormatBarcode = 2, kFormatUmi = 3, kFormatCategories = 4 };

class ReadFormat {
 public:
  struct Seg { int start = 0, end = 0, strand = 1; bool in_comment = false; int field = -1; std::string prefix; };
  // Init (ReadFormatter.hpp:202-228); false: "Format description error in <spec>"
  bool init(const char *spec);
  int segment_count(int category) const;       // GetSegmentCount; kFormatCategories: all of them
  bool need_extract(int category) const;       // NeedExtract (:261-275)
  bool in_comment(int category) const { return !segs_[category].empty() && segs_[category][0].in_comment; }   // IsInComment (:277-282)
  // Extract (:288-405) with a buffer of its own (bufferId >= 0): seq is left as it is
  void extract(const char *seq, size_t len, int category, bool need_complement, std::string &out) const;
  // one half of InplaceExtractSeqAndQual (:408-422): sorted segments are copied inside seq itself (bufferId -1), so a later segment
  // reads what an earlier one has written
  void extract_inplace(std::string &seq, int category, bool need_complement) const;

 private:
  bool parse_segment(const char *s, int len, int avail);
  void run(const char *seq, int len, int category, bool need_complement, std::string *out) const;
  std::vector<Seg> segs_[kFormatCategories];
  bool sorted_[kFormatCategories] = {true, true, true, true};
};

// Trie + BarcodeCorrector
class BarcodeWhitelist {
 public:
  explicit BarcodeWhitelist(const std::string &path);                  // SetWhitelist (:122-143); IoError
  uint64_t size() const { return n_entries_; }
  int common_length() const { return mixed_ || len_seen_ < 1 ? 0 : len_seen_; }                 // L when every valid entry has L bytes, else 0
  // SearchAndUpdate(s, weight) (:94-111): the count after the update, -1: not found
  int search_update(const uint8_t *s, size_t len, int weight);
  int search(const uint8_t *s, size_t len) const;
  // Correct (:166-234) on bc[0..len) in place; qual may be null.  -1 / 0 / 1
  int correct(uint8_t *bc, size_t len, const int8_t *qual) const;
  // every entry (a node with end = true) in the order A < C < G < T, a prefix before its extensions
  void entries(std::vector<uint8_t> &bases, std::vector<uint64_t> &offsets, std::vector<uint32_t> &counts) const;
  void set_entry_counts(const std::vector<uint32_t> &counts);          // in the order of entries()

 private:
  struct Node { uint32_t next[4] = {0, 0, 0, 0}; int32_t count = 0; bool end = false; };
  void insert(const char *s, int weight);
  std::vector<Node> nodes_;
  uint64_t n_entries_ = 0;
  int len_seen_ = -1;
  bool mixed_ = false;
};
constexpr size_t kBarcodeMaxLen = 255;   // char buffer[256] of Correct
constexpr int kBarcodeDeviceMaxLen = 32; // 2 bits per base in 64

// the whitelist in HBM (cfr_barcode.hip); throws HipError
class BarcodeDevice {
 public:
  virtual ~BarcodeDevice() {}
  // exact hits among the first n barcodes of length L add 1 to their count; the others are left to the caller
  virtual void count(const uint8_t *bases, const uint64_t *offsets, size_t n) = 0;
  // status: -1 / 0 / 1, or 2 for a barcode whose length is not L (left to the caller); pos / base: the change of a status 1
  virtual void correct(const uint8_t *bases, const uint64_t *offsets, const int8_t *qual, size_t n, int8_t *status, uint8_t *pos, uint8_t *base) = 0;
  virtual void download_counts(const std::vector<uint8_t> &bases, const std::vector<uint64_t> &offsets, std::vector<uint32_t> &counts) = 0;
  virtual uint64_t table_slots() const = 0;
  double last_ms = 0;                    // stream time of the last call: copies in, kernels, copies out
};
BarcodeDevice *make_barcode_device(int device, int L, const std::vector<uint8_t> &bases, const std::vector<uint64_t> &offsets, const std::vector<uint32_t> &counts);
constexpr int8_t kBarcodeToHost = 2;

// whitelist + the path of the handle
class Barcode {
 public:
  Barcode(const std::string &whitelist_path, int device);
  void count(const uint8_t *bases, const uint64_t *offsets, size_t n, size_t max_records);
  void correct(const uint8_t *bases, const uint64_t *offsets, const int8_t *qual, size_t n, int threads, int8_t *status, uint8_t *out_bases, bool host_only);
  void counts(const uint8_t **bases, const uint64_t **offsets, const uint32_t **counts, size_t *n);
  const BarcodeWhitelist &whitelist() const { return wl_; }
  bool on_device() const { return dev_ != nullptr; }
  uint64_t table_slots() const { return dev_ ? dev_->table_slots() : 0; }
  double device_ms = 0;
  uint64_t host_barcodes = 0, host_barcodes_total = 0;

 private:
  void sync_counts_to_host();
  BarcodeWhitelist wl_;
  std::unique_ptr<BarcodeDevice> dev_;
  bool dev_counts_newer_ = false;
  std::vector<uint8_t> e_bases_;
  std::vector<uint64_t> e_off_;
  std::vector<uint32_t> e_counts_;
  std::vector<int8_t> d_status_;
  std::vector<uint8_t> d_pos_, d_base_;
};

// BarcodeTranslator
class BarcodeTranslate {
 public:
  explicit BarcodeTranslate(const std::string &path);                  // SetTranslateTable (:40-55); IoError, FormatError
  // Translate (:57-83); false: `missing` is the piece that is not in the table
  bool translate(const uint8_t *bc, size_t len, std::string &out, std::string &missing) const;
  int from_length() const { return from_len_; }

 private:
  std::unordered_map<std::string, std::string> table_;
  int from_len_ = -1;
};

}  // namespace cfr
