// cfr_threads.hpp — the host fan-out every batch helper uses: a contiguous slice of [0, n) per thread, spawn, join.
// Header-only and free of library types, so that a plain client of the C ABI may include it too.
#pragma once

#include <cstddef>
#include <thread>
#include <vector>

namespace cfr {

// fn(lo, hi, tid) for tid in [0, threads): lo = n * tid / threads, hi = n * (tid + 1) / threads (slices may be empty when
// threads > n).  threads < 1 counts as 1, and one thread runs on the caller's.  Whether a piece of work is worth several threads
// at all is the caller's decision.
template <class F> void parallel_slices(size_t n, int threads, F &&fn) {
  if (threads < 1) threads = 1;
  if (threads == 1) { fn((size_t)0, n, 0); return; }
  const size_t nt = (size_t)threads;
  std::vector<std::thread> th;
  for (size_t t = 0; t < nt; ++t) th.emplace_back([&fn, n, nt, t]() { fn(n * t / nt, n * (t + 1) / nt, (int)t); });
  for (auto &x : th) x.join();
}

}  // namespace cfr
