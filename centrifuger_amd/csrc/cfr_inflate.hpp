// cfr_inflate.hpp — the handle behind cfr_inflate_*: BGZF members back into text (semantics: cfr_inflate_core.hpp).  Two makers of
// one interface: the host twin (cfr_inflate.cpp: plain C++, no HIP header and no zlib call, so that a sanitizer build of it stands
// alone) and the device form (cfr_inflate.hip).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "cfr_inflate_core.hpp"

namespace cfr {

class Inflate {
 public:
  virtual ~Inflate() {}
  // whole members in; the text in a buffer of the handle's (fetch_text = 0 on the device: in HBM only, *text = nullptr)
  virtual void inflate(const uint8_t *members, uint64_t n, int fetch_text, const uint8_t **text, uint64_t *text_n, cfr_inflate_info *info) = 0;
  // the last call's members: status[i], i < members; text_off[i], i <= members; false: cap is below the members
  virtual bool member_status(uint8_t *status, uint64_t *text_off, uint64_t cap) const = 0;
  virtual bool device_text(const void **d_text, uint64_t *n) { (void)d_text; (void)n; return false; }
  virtual void stats(cfr_inflate_stats *st) const = 0;
};

// the host's walk over the headers, before anything is inflated or launched: the members, their text offsets (members + 1 entries) and
// the statuses the framing alone decides (ISIZE above 65536); throws std::invalid_argument for input that does not frame or for
// 4 GiB of text
void inf_walk(const uint8_t *members, uint64_t n, std::vector<InfMember> &out, std::vector<uint64_t> &text_off, std::vector<uint8_t> &status);
// info from the statuses
void inf_fill_info(const std::vector<uint8_t> &status, uint64_t bytes_in, uint64_t bytes_out, cfr_inflate_info *info);

Inflate *make_inflate_host(int threads = 0);     // cfr_inflate.cpp; threads 0: up to 16
Inflate *make_inflate_device(int device);        // cfr_inflate.hip; throws HipError{.., -1} without that GPU

}  // namespace cfr
