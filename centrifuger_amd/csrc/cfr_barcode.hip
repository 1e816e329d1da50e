// cfr_barcode.hip — the barcode whitelist in HBM (gfx950): exact lookup, background counts and single-substitution correction.
//
// The reference walks a pointer trie: one dependent load per base for a lookup, 3 L more lookups for a barcode that misses
// (BarcodeCorrector.hpp:94-111, :180-200).  Here the whitelist is an open-addressing table (linear probing, load factor <= 0.5) of
// 16-byte slots { key: the barcode, 2 bits per base, base j in bits 2j..2j+1 | count | pad }: a lookup is one 16-byte load of one
// random line.  A present entry has count >= 1 (its lines in the whitelist), so count 0 marks an empty slot and every key, all-T at
// L = 32 included, is a valid one.  Only whitelists whose entries share one length L <= 32 come here (cfr_barcode.cpp).
//
//   k_bc_build     one lane per distinct entry (the host has added up repeated lines): claims the first free slot of its probe
//                  sequence with a compare-and-swap on the count, then writes the key.  The entries are distinct, so no lane ever
//                  compares keys while the table is being built.
//   k_bc_count     one lane per barcode: pack, probe, atomicAdd on the count of an exact hit (CollectBackgroundDistribution)
//   k_bc_lookup    one lane per entry: its count, for the download
//   k_bc_correct   Correct.  Pass 1, one lane per barcode: pack and one probe; a hit is status 0, two or more non-ACGT bytes are
//                  status -1 (every substitution still holds one of them).  The block's misses are compacted into LDS (key, mask of the
//                  non-ACGT position, lane).  Pass 2: each of the block's four waves takes one miss at a time and spreads its
//                  candidates over the lanes: candidate c = 4 * position + base in the reference's order (position, then A C G T), two
//                  rounds of 64 lanes for L = 32; with one non-ACGT byte only the four candidates at that position.  Every lane
//                  probes once; the choice - largest count, then lowest quality at the changed position, then first in order
//                  (:202-227) - is one max-reduction over the wave of (count << 32 | (127 - quality) << 8 | (127 - c)).
//                  So the common case costs one line fetch per barcode and the rare 4 L probes of a miss run side by side instead of
//                  one after the other in a lane.  256 lanes per block, 4 KB of LDS, no scratch: eight waves per SIMD hide the
//                  latency of the random fetches.
// A barcode whose length is not L gets status 2 and is left to the host twin.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "cfr_barcode.hpp"
#include "cfr_hip_util.hpp"

namespace cfr {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct alignas(16) BcSlot { unsigned long long key; uint32_t count; uint32_t pad; };

__device__ inline uint64_t bc_hash(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

// count of `key`, 0: not in the table; *where: its slot
__device__ inline uint32_t bc_probe(const BcSlot *table, uint64_t mask, uint64_t key, uint64_t *where) {
  uint64_t pos = bc_hash(key) & mask;
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    const uint4 v = *reinterpret_cast<const uint4 *>(table + pos);
    if (v.z == 0) return 0;
    if ((((uint64_t)v.y << 32) | v.x) == key) { *where = pos; return v.z; }
    pos = (pos + 1) & mask;
  }
  return 0;
}

// 2 bits per base; *nmask: bit j set where byte j is not A, C, G or T (its two key bits stay 0)
__device__ inline uint64_t bc_pack(const uint8_t *b, int L, uint32_t *nmask) {
  uint64_t key = 0;
  uint32_t nm = 0;
  for (int j = 0; j < L; ++j) {
    const uint8_t c = b[j];
    const uint32_t code = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
    if (code == 4u) nm |= 1u << j;
    else key |= (uint64_t)code << (2 * j);
  }
  *nmask = nm;
  return key;
}

__global__ __launch_bounds__(kBlock) void k_bc_build(BcSlot *table, uint64_t mask, const unsigned long long *keys, const uint32_t *weights, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  uint64_t pos = bc_hash(key) & mask;
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    if (atomicCAS(&table[pos].count, 0u, weights[i]) == 0u) { table[pos].key = key; return; }
    pos = (pos + 1) & mask;
  }
}

__global__ __launch_bounds__(kBlock) void k_bc_count(BcSlot *table, uint64_t mask, int L, const uint8_t *bases, const uint64_t *offsets, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t a = offsets[i];
  if (offsets[i + 1] - a != (uint64_t)L) return;
  uint32_t nm;
  const uint64_t key = bc_pack(bases + a, L, &nm);
  if (nm) return;
  uint64_t where = 0;
  if (bc_probe(table, mask, key, &where)) atomicAdd(&table[where].count, 1u);
}

__global__ __launch_bounds__(kBlock) void k_bc_lookup(const BcSlot *table, uint64_t mask, const unsigned long long *keys, uint64_t n, uint32_t *counts) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint64_t where = 0;
  counts[i] = bc_probe(table, mask, keys[i], &where);
}

__global__ __launch_bounds__(kBlock) void k_bc_correct(const BcSlot *table, uint64_t mask, int L, const uint8_t *bases, const uint64_t *offsets,
                                                       const int8_t *qual, uint64_t n, int8_t *status, uint8_t *out_pos, uint8_t *out_base) {
  __shared__ unsigned long long s_key[kBlock];
  __shared__ uint32_t s_nm[kBlock];
  __shared__ uint32_t s_lane[kBlock];
  __shared__ uint32_t s_n;
  const uint32_t tid = threadIdx.x;
  const uint64_t base_i = (uint64_t)blockIdx.x * kBlock;
  const uint64_t i = base_i + tid;
  if (tid == 0) s_n = 0;
  __syncthreads();
  if (i < n) {
    const uint64_t a = offsets[i];
    if (offsets[i + 1] - a != (uint64_t)L) status[i] = kBarcodeToHost;
    else {
      uint32_t nm;
      const uint64_t key = bc_pack(bases + a, L, &nm);
      uint64_t where = 0;
      if (nm == 0 && bc_probe(table, mask, key, &where)) status[i] = 0;
      else if (__popc(nm) >= 2) status[i] = -1;
      else {
        const uint32_t k = atomicAdd(&s_n, 1u);
        s_key[k] = key; s_nm[k] = nm; s_lane[k] = tid;
      }
    }
  }
  __syncthreads();
  const uint32_t n_miss = s_n;
  const uint32_t lane = tid & 63u;
  for (uint32_t m = tid >> 6; m < n_miss; m += kWaves) {
    const uint64_t key = s_key[m];
    const uint32_t nm = s_nm[m];
    const uint64_t gi = base_i + s_lane[m];
    unsigned long long best = 0;
    for (uint32_t c = lane; c < 4u * (uint32_t)L; c += 64u) {
      const uint32_t pos = c >> 2, j = c & 3u;
      const bool valid = nm ? ((nm >> pos) & 1u) != 0 : (uint32_t)((key >> (2 * pos)) & 3u) != j;
      if (!valid) continue;
      const uint64_t cand = (key & ~(3ull << (2 * pos))) | ((uint64_t)j << (2 * pos));
      uint64_t where = 0;
      const uint32_t cnt = bc_probe(table, mask, cand, &where);
      if (!cnt) continue;
      const int q = qual ? (int)qual[offsets[gi] + pos] : 0;
      const unsigned long long score = ((unsigned long long)cnt << 32) | ((unsigned long long)(uint32_t)(127 - q) << 8) | (unsigned long long)(127u - c);
      best = score > best ? score : best;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(best, d, 64);
      best = o > best ? o : best;
    }
    if (lane == 0) {
      if (best == 0) status[gi] = -1;
      else {
        const uint32_t c = 127u - (uint32_t)(best & 0xffu);
        status[gi] = 1;
        out_pos[gi] = (uint8_t)(c >> 2);
        out_base[gi] = (uint8_t)("ACGT"[c & 3u]);
      }
    }
  }
}

class DeviceWhitelist : public BarcodeDevice {
 public:
  DeviceWhitelist(int device, int L, const std::vector<uint8_t> &bases, const std::vector<uint64_t> &offsets, const std::vector<uint32_t> &counts)
      : device_(device), L_(L), n_entries_(counts.size()) {
    if (!device_exists(device)) throw HipError{"cfr_barcode: no HIP device " + std::to_string(device), -1};
    DeviceScope scope(device);
    stream_.create();
    ev0_.create();
    ev1_.create();
    slots_ = 64;
    while (slots_ < 2 * n_entries_) slots_ <<= 1;
    std::vector<unsigned long long> keys(n_entries_);
    for (uint64_t e = 0; e < n_entries_; ++e) {
      unsigned long long k = 0;
      for (int j = 0; j < L; ++j) {
        const uint8_t c = bases[offsets[e] + (uint64_t)j];
        k |= (unsigned long long)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3) << (2 * j);
      }
      keys[e] = k;
    }
    table_.alloc(slots_);
    d_keys_.alloc(n_entries_);
    d_counts_.alloc(n_entries_);
    HIP_CHECK(hipMemsetAsync(table_, 0, slots_ * sizeof(BcSlot), stream_));
    if (n_entries_) {
      HIP_CHECK(hipMemcpyAsync(d_keys_, keys.data(), n_entries_ * 8, hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipMemcpyAsync(d_counts_, counts.data(), n_entries_ * 4, hipMemcpyHostToDevice, stream_));
      hipLaunchKernelGGL(k_bc_build, dim3(grid_for(n_entries_)), dim3(kBlock), 0, stream_, table_.get(), slots_ - 1, (const unsigned long long *)d_keys_,
                         (const uint32_t *)d_counts_, n_entries_);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(stream_));   // (keys is a local)
  }
  ~DeviceWhitelist() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }

  void count(const uint8_t *bases, const uint64_t *offsets, size_t n) override {
    if (n == 0) { last_ms = 0; return; }
    DeviceScope scope(device_);
    HIP_CHECK(hipEventRecord(ev0_, stream_));
    upload(bases, offsets, nullptr, n);
    hipLaunchKernelGGL(k_bc_count, dim3(grid_for(n)), dim3(kBlock), 0, stream_, table_.get(), slots_ - 1, L_, (const uint8_t *)d_bases_, (const uint64_t *)d_off_, (uint64_t)n);
    HIP_CHECK(hipGetLastError());
    finish();
  }

  void correct(const uint8_t *bases, const uint64_t *offsets, const int8_t *qual, size_t n, int8_t *status, uint8_t *pos, uint8_t *base) override {
    if (n == 0) { last_ms = 0; return; }
    DeviceScope scope(device_);
    HIP_CHECK(hipEventRecord(ev0_, stream_));
    upload(bases, offsets, qual, n);
    hipLaunchKernelGGL(k_bc_correct, dim3(grid_for(n)), dim3(kBlock), 0, stream_, (const BcSlot *)table_, slots_ - 1, L_, (const uint8_t *)d_bases_,
                       (const uint64_t *)d_off_, (const int8_t *)(qual ? d_qual_.get() : nullptr), (uint64_t)n, d_status_.get(), d_pos_.get(), d_base_.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(status, d_status_, n, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(pos, d_pos_, n, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(base, d_base_, n, hipMemcpyDeviceToHost, stream_));
    finish();
  }

  void download_counts(const std::vector<uint8_t> &, const std::vector<uint64_t> &, std::vector<uint32_t> &counts) override {
    counts.resize(n_entries_);
    if (!n_entries_) return;
    DeviceScope scope(device_);
    hipLaunchKernelGGL(k_bc_lookup, dim3(grid_for(n_entries_)), dim3(kBlock), 0, stream_, (const BcSlot *)table_, slots_ - 1, (const unsigned long long *)d_keys_,
                       n_entries_, d_counts_.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(counts.data(), d_counts_, n_entries_ * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  uint64_t table_slots() const override { return slots_; }

 private:
  // the barcodes of one call: the bytes offsets[0] .. offsets[n) and the n + 1 offsets, rebased to the first byte.  A size class grows
  // into fresh buffers that replace the old ones only when all of them exist.
  void upload(const uint8_t *bases, const uint64_t *offsets, const int8_t *qual, size_t n) {
    const uint64_t first = offsets[0], total = offsets[n] - first;
    if (total > cap_bytes_) {
      DevBuf<uint8_t> b(total);
      d_bases_ = std::move(b); d_qual_.reset(); cap_bytes_ = total;      // the qualities follow the bases' size, when they are asked for
    }
    if (qual && !d_qual_) d_qual_.alloc(cap_bytes_);
    if (n > cap_n_) {
      DevBuf<uint64_t> off(n + 1);
      DevBuf<int8_t> st(n);
      DevBuf<uint8_t> pos(n), base(n);
      d_off_ = std::move(off); d_status_ = std::move(st); d_pos_ = std::move(pos); d_base_ = std::move(base); cap_n_ = n;
    }
    const uint64_t *src = offsets;
    if (first) {
      rebased_.resize(n + 1);
      for (size_t i = 0; i <= n; ++i) rebased_[i] = offsets[i] - first;
      src = rebased_.data();
    }
    if (total) HIP_CHECK(hipMemcpyAsync(d_bases_, bases + first, total, hipMemcpyHostToDevice, stream_));
    if (total && qual) HIP_CHECK(hipMemcpyAsync(d_qual_, qual + first, total, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(d_off_, src, (n + 1) * 8, hipMemcpyHostToDevice, stream_));
  }
  void finish() {
    HIP_CHECK(hipEventRecord(ev1_, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev0_, ev1_));
    last_ms = ms;
  }

  int device_, L_;
  uint64_t n_entries_, slots_ = 0;
  Stream stream_;                  // first: the last to go
  Event ev0_, ev1_;
  DevBuf<BcSlot> table_;
  DevBuf<unsigned long long> d_keys_;
  DevBuf<uint32_t> d_counts_;
  DevBuf<uint8_t> d_bases_, d_pos_, d_base_;
  DevBuf<int8_t> d_qual_, d_status_;
  DevBuf<uint64_t> d_off_;
  uint64_t cap_bytes_ = 0;
  size_t cap_n_ = 0;
  std::vector<uint64_t> rebased_;
};

}  // namespace

BarcodeDevice *make_barcode_device(int device, int L, const std::vector<uint8_t> &bases, const std::vector<uint64_t> &offsets, const std::vector<uint32_t> &counts) {
  return new DeviceWhitelist(device, L, bases, offsets, counts);
}

}  // namespace cfr
