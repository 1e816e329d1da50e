#!/usr/bin/env python3
"""The --merge-readpair pre-step on the device, next to the step it sits in front of: 10 M synthetic 2 x 150 bp pairs on the 1 Gbp
index of bench.py (same cache), fragment lengths uniform in 100..500, -k 5, reads and qualities resident in HBM.  Prints one JSON line:
  merge_ms            (a) the merge kernels alone (HIP events around decide + scans + write)
  step_merge_on_ms    (b) cfr_classify_batch_resident_merged with the merge switched on
  step_merge_off_ms   (c) cfr_classify_batch_resident on the same pairs, same process
and, for scale, the search kernel time of (b) and (c), (c) with SDUST on the device, the share of merged pairs, and the host twin's
pairs/s on 16 threads.  One warm-up call, then the median of --steps timed ones."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (index cache and read generator of the flagship benchmark)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ins-lo", type=int, default=100)
    ap.add_argument("--ins-hi", type=int, default=500)
    ap.add_argument("--host-pairs", type=int, default=1_000_000, help="pairs the host twin is timed on")
    ap.add_argument("--cache", default=os.environ.get("CFR_BENCH_CACHE", "/tmp/cfr_bench"))
    a = ap.parse_args()
    import torch
    from centrifuger_amd import capi
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    args = argparse.Namespace(species=50, strains=5, genome_len=4_000_000, seed=20260928, builder="own", divergence_step=0.01, index_gbp=0.0,
                              divergence_model="star", build_threads=16)
    cache = os.path.join(a.cache, bench.cache_key(args))
    prefix = bench.build_index(args, cache, device)
    torch.cuda.empty_cache()
    cat_d = torch.from_numpy(np.ascontiguousarray(np.load(os.path.join(cache, "genome_cat.npy"), mmap_mode="r"))).to(device)
    starts = np.load(os.path.join(cache, "genome_starts.npy"))
    n, L = a.pairs, 150
    r1, r2 = bench.make_pairs_gpu(torch, cat_d, starts, n, L, args.seed + 3000, device, ins_lo=a.ins_lo, ins_hi=a.ins_hi)
    del cat_d
    gen = torch.Generator(device=device)
    gen.manual_seed(7)
    q1 = torch.randint(33, 74, (n, L), generator=gen, device=device, dtype=torch.uint8)
    q2 = torch.randint(33, 74, (n, L), generator=gen, device=device, dtype=torch.uint8)
    offs = torch.arange(n + 1, device=device, dtype=torch.int64) * L
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    idx = capi.Index(prefix, capi.default_params(max_result=5))
    dev = capi.DeviceIndex(idx, 0)
    res = capi.PinnedArray(n, capi.RESULT_DTYPE)
    mat = capi.PinnedArray(5 * n, capi.MATCH_DTYPE)
    ptr = dict(d_bases1=r1.data_ptr(), d_offsets1=offs.data_ptr(), n=n, total1=n * L, d_bases2=r2.data_ptr(), d_offsets2=offs.data_ptr(), total2=n * L,
               results=res.array, matches=mat.array)

    def timed(fn):
        ms, extra = [], None
        for k in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            extra = fn()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), ms, extra

    off_ms, off_all, _ = timed(lambda: dev.classify_resident(**ptr))
    off_search = dev.last_stats().search_ms
    dev.set_dust(True)
    dust_ms, _, _ = timed(lambda: dev.classify_resident(**ptr))
    dev.set_dust(False)
    dev.set_merge(True)
    merge_only = []

    def on():
        out = dev.classify_resident_merged(d_qual1=q1.data_ptr(), d_qual2=q2.data_ptr(), **ptr)
        merge_only.append(dev.last_merge_ms())
        return out
    on_ms, on_all, (_, _, kind) = timed(on)
    on_search = dev.last_stats().search_ms
    dev.set_merge(False)
    h = min(a.host_pairs, n)
    hb1, hb2 = r1[:h].cpu().numpy().reshape(-1), r2[:h].cpu().numpy().reshape(-1)
    hq1, hq2 = q1[:h].cpu().numpy().reshape(-1), q2[:h].cpu().numpy().reshape(-1)
    ho = np.arange(h + 1, dtype=np.uint64) * np.uint64(L)
    t0 = time.perf_counter()
    hm = capi.merge_pairs(hb1, ho, hb2, ho, hq1, hq2, threads=16)
    host_s = time.perf_counter() - t0
    assert np.array_equal(hm["kind"], kind[:h]), "device and host twin disagree on which pairs merge"
    out = {"bench": "merge_readpair", "pairs": n, "read_len": L, "insert": [a.ins_lo, a.ins_hi], "k": 5, "steps": a.steps, "warmup": a.warmup,
           "merge_ms": round(statistics.median(merge_only[a.warmup:]), 3), "step_merge_on_ms": round(on_ms, 3), "step_merge_off_ms": round(off_ms, 3),
           "step_merge_on_all_ms": [round(x, 3) for x in on_all], "step_merge_off_all_ms": [round(x, 3) for x in off_all],
           "search_ms_merge_on": round(on_search, 3), "search_ms_merge_off": round(off_search, 3), "step_sdust_on_merge_off_ms": round(dust_ms, 3),
           "merged_fraction": {"overlap": round(float((kind == 1).mean()), 4), "read_through": round(float((kind == 2).mean()), 4)},
           "pairs_per_s_merge_on": round(n / on_ms * 1e3), "pairs_per_s_merge_off": round(n / off_ms * 1e3),
           "host_twin_pairs_per_s_16_threads": round(h / host_s)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
