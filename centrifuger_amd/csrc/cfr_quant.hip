// cfr_quant.hip — the device side of centrifuger-quant (gfx950): the coalesce of read assignments and the E-step of the EM.
//
//   k_quant_coalesce      one lane per record: hash of (n_targets, targets in order), open-addressing table in HBM whose key is
//                         the full list (keys in a side arena, compared word for word), integer atomics on a match.  The sums are
//                         integers (weights in units of 2^-22), so they do not depend on the order the lanes arrive in.
//   k_quant_rehash        after the host has grown the table: one lane per entry puts its index into the new slot array
//   k_quant_estep_terms   one lane per assignment slot: sum = left-to-right sum of abund0 over the assignment, term = (w * abund0[t]) / sum,
//                         stored at the slot's place in the node-major order
//   k_quant_estep_sum     one lane per node: adds the node's terms in that order, starting from 0.0 - one lane per segment, whatever
//                         its length, because splitting a segment changes the rounding
// The last two restate the E-step loop of EMupdate (Quantifier.hpp:196-208; host twin: HostEStep in cfr_quant.cpp) and must give its
// bits: no contraction into fused multiply-adds (the pragma below and -ffp-contract=off), IEEE division (what clang emits for fp64).
//
// Hand-off between lanes inside k_quant_coalesce: nobody waits for anybody.  A lane that finds its list missing writes key and
// entry first and then puts the entry into the empty slot with one compare-and-swap (release); if another lane's entry got there
// first it compares with that one, and its own entry stays behind unused (marked dead, skipped by the rehash and the download).
// Everything another lane may read before the kernel ends - slots, keys, entry headers - is written and read with agent-scope
// atomics, which go past the per-CU cache.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "cfr_hip_util.hpp"
#include "cfr_quant.hpp"

#pragma clang fp contract(off)

namespace cfr {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kSlotEmpty = 0, kEntryDead = 0xffffffffu;
enum { CTL_ENTRIES = 0, CTL_ARENA = 1, CTL_FULL = 2, CTL_WORDS = 4 };

struct QuantTable {
  uint32_t *slots;                 // n_slots (a power of two): 0 empty, else entry + 1
  uint64_t n_slots;
  uint64_t *e_hash, *e_off;        // per entry: hash, first word of its key in the arena
  uint32_t *e_len;                 //            words of the key; 0xffffffff: an entry that lost the race for its slot (never read)
  unsigned long long *e_acc;       //            3 sums: weight units, count, uniq
  uint64_t max_entries;            // n_slots / 2: the table never fills beyond half
  uint32_t *arena;
  uint64_t arena_cap;
  unsigned long long *ctl;         // CTL_*
};

#define Q_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define Q_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ inline uint64_t quant_hash(const uint32_t *t, uint32_t n) {
  uint64_t h = 0x9e3779b97f4a7c15ull ^ n;
  for (uint32_t j = 0; j < n; ++j) { h = (h ^ t[j]) * 0xff51afd7ed558ccdull; h ^= h >> 32; }
  return h;
}

__global__ __launch_bounds__(kBlock) void k_quant_coalesce(QuantTable T, const uint32_t *words, const uint32_t *off, uint32_t n, uint8_t *done) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || done[i]) return;
  const uint32_t *w = words + off[i];
  const uint32_t nt = w[0];
  const uint32_t *t = w + 1;
  const uint32_t meta = w[1 + nt];
  const uint64_t h = quant_hash(t, nt);
  const uint64_t mask = T.n_slots - 1;
  uint64_t pos = h & mask;
  uint64_t entry = ~0ull, mine = ~0ull;                    // mine: an entry this lane has written and not yet put into a slot
  for (uint64_t probes = 0; probes < T.n_slots; ++probes) {
    uint32_t v = __hip_atomic_load(T.slots + pos, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    if (v == kSlotEmpty) {
      if (mine == ~0ull) {
        // room for the key first, then an entry (a key claimed for nothing is only lost room; the host grows the table next)
        const uint64_t a = atomicAdd(T.ctl + CTL_ARENA, (unsigned long long)nt);
        uint64_t e = ~0ull;
        if (a + nt <= T.arena_cap) {
          e = atomicAdd(T.ctl + CTL_ENTRIES, 1ull);
          if (e >= T.max_entries) e = ~0ull;
        }
        if (e == ~0ull) { Q_STORE(T.ctl + CTL_FULL, 1ull); return; }   // done[i] stays 0: the batch runs again on the grown table
        for (uint32_t j = 0; j < nt; ++j) Q_STORE(T.arena + a + j, t[j]);
        Q_STORE(T.e_hash + e, h); Q_STORE(T.e_off + e, a); Q_STORE(T.e_len + e, nt);
        mine = e;
      }
      uint32_t expect = kSlotEmpty;
      if (__hip_atomic_compare_exchange_strong(T.slots + pos, &expect, (uint32_t)mine + 1, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) {
        entry = mine; mine = ~0ull;
        break;
      }
      v = expect;                                          // another lane's entry got there first: is it this list?
    }
    const uint64_t e = v - 1;
    bool same = Q_LOAD(T.e_hash + e) == h && Q_LOAD(T.e_len + e) == nt;
    if (same) {
      const uint32_t *k = T.arena + Q_LOAD(T.e_off + e);
      for (uint32_t j = 0; j < nt && same; ++j) same = Q_LOAD(k + j) == t[j];
    }
    if (same) { entry = e; break; }
    pos = (pos + 1) & mask;
  }
  if (mine != ~0ull) Q_STORE(T.e_len + mine, kEntryDead);   // the same list was entered by another lane meanwhile
  if (entry == ~0ull) { Q_STORE(T.ctl + CTL_FULL, 1ull); return; }
  atomicAdd(T.e_acc + 3 * entry + 0, 1ull << (kQuantWeightShift - 2 * (int)(meta & 0xff)));
  atomicAdd(T.e_acc + 3 * entry + 1, 1ull);
  if (meta & 256u) atomicAdd(T.e_acc + 3 * entry + 2, 1ull);
  done[i] = 1;
}

__global__ __launch_bounds__(kBlock) void k_quant_rehash(QuantTable T, uint64_t n_entries) {
  const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_entries) return;
  const uint64_t mask = T.n_slots - 1;
  if (T.e_len[e] == kEntryDead) return;
  uint64_t pos = T.e_hash[e] & mask;
  for (uint64_t probes = 0; probes < T.n_slots; ++probes) {   // the entries are distinct: the first free slot is the place
    if (atomicCAS(T.slots + pos, kSlotEmpty, (uint32_t)e + 1) == kSlotEmpty) return;
    pos = (pos + 1) & mask;
  }
}

__global__ __launch_bounds__(kBlock) void k_quant_estep_terms(const uint64_t *a_begin, const uint32_t *a_target, const double *a_weight, const uint32_t *slot_assign,
                                                              const uint64_t *slot_pos, const double *abund, int init, double *terms, uint64_t n_slots) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_slots) return;
  const uint32_t a = slot_assign[s];
  const uint64_t b = a_begin[a], e = a_begin[a + 1];
  const double w = a_weight[a];
  double term;
  if (init) term = w / (double)(e - b);
  else {
    double sum = 0;
    for (uint64_t j = b; j < e; ++j) sum += abund[a_target[j]];
    term = w * abund[a_target[s]] / sum;
  }
  terms[slot_pos[s]] = term;
}

__global__ __launch_bounds__(kBlock) void k_quant_estep_sum(const uint64_t *node_begin, const double *terms, double *read_count, uint64_t n_nodes) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_nodes) return;
  double acc = 0.0;
  for (uint64_t p = node_begin[v], e = node_begin[v + 1]; p < e; ++p) acc += terms[p];
  read_count[v] = acc;
}

template <class T> DevBuf<T> upload(const std::vector<T> &v, hipStream_t st) {
  DevBuf<T> d(v.size());
  if (!v.empty()) HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return d;
}
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the memory a QuantTable points into (all but the control block, which outlives every growth); slots and sums start cleared on st
struct QuantTableMem {
  uint64_t n_slots = 0, arena_cap = 0;
  DevBuf<uint32_t> slots;
  DevBuf<uint64_t> e_hash, e_off;
  DevBuf<uint32_t> e_len;
  DevBuf<unsigned long long> e_acc;
  DevBuf<uint32_t> arena;
  QuantTableMem() = default;
  QuantTableMem(uint64_t n, uint64_t cap, hipStream_t st)
      : n_slots(n), arena_cap(cap), slots(n), e_hash(n / 2), e_off(n / 2), e_len(n / 2), e_acc(3 * (n / 2)), arena(cap) {
    HIP_CHECK(hipMemsetAsync(slots, 0, n * 4, st));
    HIP_CHECK(hipMemsetAsync(e_acc, 0, 24 * (n / 2), st));
  }
  uint64_t max_entries() const { return n_slots / 2; }
  QuantTable view(unsigned long long *ctl) const { return QuantTable{slots, n_slots, e_hash, e_off, e_len, e_acc, max_entries(), arena, arena_cap, ctl}; }
};

class DeviceCoalescer : public QuantCoalescer {
 public:
  DeviceCoalescer(int device, uint64_t table_slots) : device_(device) {
    if (!device_exists(device)) throw HipError{"cfr_quant: no HIP device " + std::to_string(device), -1};
    DeviceScope scope(device);
    stream_.create();
    uint64_t slots = 64;
    const uint64_t want = table_slots ? table_slots : (1ull << 21);
    while (slots < want && slots < (1ull << 31)) slots <<= 1;
    ctl_.alloc(CTL_WORDS);
    HIP_CHECK(hipMemsetAsync(ctl_, 0, CTL_WORDS * 8, stream_));
    mem_ = QuantTableMem(slots, slots * 4, stream_);
  }
  ~DeviceCoalescer() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }
  // Batches are double-buffered on the stream: batch k is copied into its pinned buffer while the device works on batch k - 1; the
  // outcome of k - 1 (did the table or the arena fill?) is looked at before k is launched.
  void add(const QuantRecords &r) override {
    if (r.n() == 0) return;
    const double t0 = now_ms();
    DeviceScope scope(device_);
    Buf &b = buf_[next_ & 1];
    ++next_;
    reserve(b, r.words.size(), r.n());
    memcpy(b.h_words, r.words.data(), r.words.size() * 4);
    memcpy(b.h_off, r.off.data(), r.off.size() * 4);
    b.n = (uint32_t)r.n();
    resolve();
    HIP_CHECK(hipMemcpyAsync(b.d_words, b.h_words, r.words.size() * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(b.d_off, b.h_off, r.off.size() * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemsetAsync(b.d_done, 0, b.n, stream_));
    launch(b);
    live_ = &b;
    stats.coalesce_ms += now_ms() - t0;
  }
  void finish(QuantAssignments &out) override {
    const double t0 = now_ms();
    DeviceScope scope(device_);
    resolve();
    unsigned long long ctl[CTL_WORDS];
    HIP_CHECK(hipMemcpy(ctl, ctl_, sizeof(ctl), hipMemcpyDeviceToHost));
    const uint64_t ne = ctl[CTL_ENTRIES], na = std::min<uint64_t>(ctl[CTL_ARENA], mem_.arena_cap);
    std::vector<uint64_t> e_off(ne), acc(3 * ne);
    std::vector<uint32_t> e_len(ne), arena(na);
    if (ne) {
      HIP_CHECK(hipMemcpy(e_off.data(), mem_.e_off, ne * 8, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(e_len.data(), mem_.e_len, ne * 4, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(acc.data(), mem_.e_acc, ne * 24, hipMemcpyDeviceToHost));
    }
    if (na) HIP_CHECK(hipMemcpy(arena.data(), mem_.arena, na * 4, hipMemcpyDeviceToHost));
    out = QuantAssignments();
    for (uint64_t e = 0; e < ne; ++e) {
      if (e_len[e] == kEntryDead) continue;
      if (e_off[e] + e_len[e] > na) throw HipError{"cfr_quant: a key of the coalesce table lies outside its arena", 0};
      out.targets.insert(out.targets.end(), arena.begin() + e_off[e], arena.begin() + e_off[e] + e_len[e]);
      out.begin.push_back(out.targets.size());
      out.weight_units.push_back(acc[3 * e]); out.count.push_back(acc[3 * e + 1]); out.uniq.push_back(acc[3 * e + 2]);
    }
    stats.table_slots = mem_.n_slots;
    stats.coalesce_ms += now_ms() - t0;
  }
  QuantDeviceStats stats;

 private:
  struct Buf { PinnedBuf<uint32_t> h_words, h_off; DevBuf<uint32_t> d_words, d_off; DevBuf<uint8_t> d_done; size_t cap_words = 0, cap_n = 0; uint32_t n = 0; };

  // a size class grows into fresh buffers that replace the old ones only when all of them exist
  void reserve(Buf &b, size_t words, size_t n) {
    if (words > b.cap_words) {
      const size_t cap = std::max<size_t>(words, 1u << 16);
      PinnedBuf<uint32_t> h(cap);
      DevBuf<uint32_t> d(cap);
      b.h_words = std::move(h); b.d_words = std::move(d); b.cap_words = cap;
    }
    if (n > b.cap_n) {
      const size_t cap = std::max<size_t>(n, 1u << 12);
      PinnedBuf<uint32_t> h(cap + 1);
      DevBuf<uint32_t> d(cap + 1);
      DevBuf<uint8_t> done(cap);
      b.h_off = std::move(h); b.d_off = std::move(d); b.d_done = std::move(done); b.cap_n = cap;
    }
  }
  void launch(const Buf &b) {
    hipLaunchKernelGGL(k_quant_coalesce, dim3(grid_for(b.n)), dim3(kBlock), 0, stream_, mem_.view(ctl_), (const uint32_t *)b.d_words, (const uint32_t *)b.d_off, b.n, b.d_done.get());
    HIP_CHECK(hipGetLastError());
  }
  // waits for the batch in flight; while it left the FULL flag: a table of twice the slots and twice the arena, the entries moved and
  // hashed into it on the device, and the records of that batch that are not done yet once more
  void resolve() {
    if (!live_) return;
    for (;;) {
      HIP_CHECK(hipStreamSynchronize(stream_));
      unsigned long long ctl[CTL_WORDS];
      HIP_CHECK(hipMemcpy(ctl, ctl_, sizeof(ctl), hipMemcpyDeviceToHost));
      if (!ctl[CTL_FULL]) break;
      if (mem_.n_slots >= (1ull << 31)) throw CapacityError{"cfr_quant: more than 2^30 distinct target lists"};
      const uint64_t ne = std::min<uint64_t>(ctl[CTL_ENTRIES], mem_.max_entries()), na = std::min<uint64_t>(ctl[CTL_ARENA], mem_.arena_cap);
      QuantTableMem N(mem_.n_slots * 2, mem_.arena_cap * 2, stream_);
      if (ne) {
        HIP_CHECK(hipMemcpyAsync(N.e_hash, mem_.e_hash, ne * 8, hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(N.e_off, mem_.e_off, ne * 8, hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(N.e_len, mem_.e_len, ne * 4, hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(N.e_acc, mem_.e_acc, ne * 24, hipMemcpyDeviceToDevice, stream_));
      }
      if (na) HIP_CHECK(hipMemcpyAsync(N.arena, mem_.arena, na * 4, hipMemcpyDeviceToDevice, stream_));
      const unsigned long long fixed[CTL_WORDS] = {ne, na, 0, 0};
      HIP_CHECK(hipMemcpyAsync(ctl_, fixed, sizeof(fixed), hipMemcpyHostToDevice, stream_));
      if (ne) { hipLaunchKernelGGL(k_quant_rehash, dim3(grid_for(ne)), dim3(kBlock), 0, stream_, N.view(ctl_), ne); HIP_CHECK(hipGetLastError()); }
      HIP_CHECK(hipStreamSynchronize(stream_));
      mem_ = std::move(N);      // (the old table goes with N)
      ++stats.grow_count;
      launch(*live_);
    }
    live_ = nullptr;
  }

  int device_;
  Stream stream_;                  // first: the last to go
  DevBuf<unsigned long long> ctl_; // CTL_*
  QuantTableMem mem_;
  Buf buf_[2];
  Buf *live_ = nullptr;
  size_t next_ = 0;
};

class DeviceEStep : public QuantEStep {
 public:
  DeviceEStep(int device, const QuantCsr &c) : device_(device), n_nodes_(c.n_nodes), n_slots_(c.n_slots) {
    if (!device_exists(device)) throw HipError{"cfr_quant: no HIP device " + std::to_string(device), -1};
    DeviceScope scope(device);
    stream_.create();
    std::vector<uint32_t> slot_assign(c.n_slots);
    for (size_t a = 0; a + 1 < c.a_begin.size(); ++a) for (uint64_t s = c.a_begin[a]; s < c.a_begin[a + 1]; ++s) slot_assign[s] = (uint32_t)a;
    a_begin_ = upload(c.a_begin, stream_); a_target_ = upload(c.a_target, stream_); a_weight_ = upload(c.a_weight, stream_);
    slot_assign_ = upload(slot_assign, stream_); slot_pos_ = upload(c.slot_pos, stream_); node_begin_ = upload(c.node_begin, stream_);
    terms_.alloc(c.n_slots); d_abund_.alloc(c.n_nodes); d_rc_.alloc(c.n_nodes);
    h_pin_.alloc(std::max<size_t>(c.n_nodes, 1) * 2);
    HIP_CHECK(hipStreamSynchronize(stream_));   // (slot_assign is a local)
  }
  ~DeviceEStep() override {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }
  // one round: abund goes up and readCount comes down, each n_nodes doubles through pinned memory
  void run(const double *abund, bool init, double *read_count) override {
    DeviceScope scope(device_);
    if (!init) {
      memcpy(h_pin_, abund, n_nodes_ * 8);
      HIP_CHECK(hipMemcpyAsync(d_abund_, h_pin_, n_nodes_ * 8, hipMemcpyHostToDevice, stream_));
    }
    if (n_slots_) {
      hipLaunchKernelGGL(k_quant_estep_terms, dim3(grid_for(n_slots_)), dim3(kBlock), 0, stream_, (const uint64_t *)a_begin_, (const uint32_t *)a_target_,
                         (const double *)a_weight_, (const uint32_t *)slot_assign_, (const uint64_t *)slot_pos_, (const double *)d_abund_, init ? 1 : 0, terms_.get(), n_slots_);
      HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_quant_estep_sum, dim3(grid_for(n_nodes_)), dim3(kBlock), 0, stream_, (const uint64_t *)node_begin_, (const double *)terms_, d_rc_.get(), n_nodes_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_pin_ + n_nodes_, d_rc_, n_nodes_ * 8, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    memcpy(read_count, h_pin_ + n_nodes_, n_nodes_ * 8);
  }

 private:
  int device_;
  uint64_t n_nodes_, n_slots_;
  Stream stream_;                  // first: the last to go
  DevBuf<uint64_t> a_begin_, slot_pos_, node_begin_;
  DevBuf<uint32_t> a_target_, slot_assign_;
  DevBuf<double> a_weight_, terms_, d_abund_, d_rc_;
  PinnedBuf<double> h_pin_;
};

}  // namespace

QuantCoalescer *make_device_coalescer(int device, uint64_t table_slots) { return new DeviceCoalescer(device, table_slots); }
QuantEStep *make_device_estep(int device, const QuantCsr &c) { return new DeviceEStep(device, c); }
QuantDeviceStats device_coalescer_stats(const QuantCoalescer *c) {
  const DeviceCoalescer *d = dynamic_cast<const DeviceCoalescer *>(c);
  return d ? d->stats : QuantDeviceStats();
}

}  // namespace cfr
