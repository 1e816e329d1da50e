// cfr_gz.hpp — the handle behind cfr_gz_*: a text as BGZF members, and the records of a read dump made and compressed in one call
// (semantics: cfr_gz_core.hpp).  Two makers of one interface: the host twin (cfr_gz.cpp: plain C++, no HIP header, so that a sanitizer
// build of it stands alone) and the device form (cfr_gz.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#include "cfr_gz_core.hpp"

namespace cfr {

constexpr int kGzMaxFiles = 4;                 // read 1, read 2, barcode, UMI

class Gz {
 public:
  virtual ~Gz() {}
  // host text in; the members in a buffer of the handle's, good until its next call
  virtual void compress(const uint8_t *text, uint64_t n, const uint8_t **out, uint64_t *out_n) = 0;
  // the records of the selected reads of n_files files, each file's members in a buffer of the handle's
  virtual void dump(const char *id_bytes, const uint64_t *id_off, const uint8_t *select, size_t n, const cfr_gz_file *files, int n_files,
                    const uint8_t **out, uint64_t *out_n) = 0;
  virtual void stats(cfr_gz_stats *st) const = 0;
};

// the argument checks of cfr_gz_dump, before anything is launched: throws std::invalid_argument
void gz_check_dump(const char *id_bytes, const uint64_t *id_off, const uint8_t *select, size_t n, const cfr_gz_file *files, int n_files,
                   const uint8_t *const *out, const uint64_t *out_n);
uint32_t gz_block_bytes(const cfr_gz_options &o);      // the option checked; 0 is the default
bool gz_dynamic(const cfr_gz_options &o);              // codes checked: 1 is dynamic mode

Gz *make_gz_host(const cfr_gz_options &o);                 // cfr_gz.cpp
Gz *make_gz_device(int device, const cfr_gz_options &o);   // cfr_gz.hip; throws HipError{.., -1} without that GPU

}  // namespace cfr
