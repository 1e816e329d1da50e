#!/usr/bin/env python3
"""Barcode whitelist correction, device table against the host twin: a synthetic whitelist of 737 280 16-mers and 10 M barcodes, 90 %
exact, 8 % one substitution away, 2 % random.  Prints one JSON line and writes it to profiles/barcode_bench.json (--out):
  count_device_ms / correct_device_ms     stream time of one call (copies in, kernels, copies out: cfr_barcode_get_stats)
  count_call_ms / correct_call_ms         wall time of the same calls, the host's share (copy, patch, the twin for odd lengths) included
  host_count_ms / host_correct_ms         the host twin (the reference's trie) in the same process; correct on 16 threads, count on
                                          one (the reference's background pass is serial)
One warm-up call, then the median of --steps timed ones.  Device and twin must agree on every status and byte."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=737_280)
    ap.add_argument("--barcodes", type=int, default=10_000_000)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "barcode_bench.json"))
    a = ap.parse_args()
    from centrifuger_amd import capi
    rng = np.random.default_rng(20261018)
    L, n = a.length, a.barcodes
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    keys = np.unique(rng.integers(0, 4 ** L, size=a.entries * 2, dtype=np.uint64))
    keys = rng.permutation(keys)[:a.entries]
    wl = acgt[(keys[:, None] >> (2 * np.arange(L, dtype=np.uint64))[None, :]) & np.uint64(3)]           # entries x L
    tmp = tempfile.mkdtemp(prefix="cfr_bench_barcode_")
    path = os.path.join(tmp, "whitelist.txt")
    with open(path, "wb") as f:
        f.write(np.concatenate([wl, np.full((len(wl), 1), 10, dtype=np.uint8)], axis=1).tobytes())
    bc = wl[rng.integers(0, len(wl), size=n)].copy()
    cls = rng.random(n)
    sub = np.nonzero((cls >= 0.90) & (cls < 0.98))[0]
    pos = rng.integers(0, L, size=len(sub))
    bc[sub, pos] = acgt[(np.searchsorted(acgt, bc[sub, pos]) + rng.integers(1, 4, size=len(sub))) & 3]
    rand = np.nonzero(cls >= 0.98)[0]
    bc[rand] = acgt[rng.integers(0, 4, size=(len(rand), L))]
    bases = bc.reshape(-1)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    qual = rng.integers(33, 74, size=n * L).astype(np.uint8)

    def timed(fn, stat=None):
        wall, dev = [], []
        for k in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            out = fn()
            if k >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                if stat:
                    dev.append(stat())
        return statistics.median(wall), (statistics.median(dev) if dev else None), out

    t0 = time.perf_counter()
    d = capi.Barcode(path, device=0)
    open_ms = (time.perf_counter() - t0) * 1e3
    h = capi.Barcode(path, device=None)
    cap = 2_000_000
    cnt_wall, cnt_dev, _ = timed(lambda: d.count(bases, offs, max_records=cap), lambda: d.stats().device_ms)
    cor_wall, cor_dev, (s_dev, b_dev) = timed(lambda: d.correct(bases, offs, qual, threads=a.threads), lambda: d.stats().device_ms)
    hcnt_wall, _, _ = timed(lambda: h.count(bases, offs, max_records=cap))
    hcor_wall, _, (s_host, b_host) = timed(lambda: h.correct(bases, offs, qual, threads=a.threads))
    assert np.array_equal(d.counts()[1], h.counts()[1]), "device and host twin disagree on the counts"
    assert np.array_equal(s_dev, s_host) and np.array_equal(b_dev, b_host), "device and host twin disagree on the corrections"
    st = d.stats()
    out = {"bench": "barcode_whitelist", "entries": int(len(wl)), "barcodes": n, "length": L, "steps": a.steps, "warmup": a.warmup,
           "table_slots": int(st.table_slots), "open_ms_with_table_build": round(open_ms, 1),
           "count_records": cap, "count_device_ms": round(cnt_dev, 3), "count_call_ms": round(cnt_wall, 3), "host_count_ms_1_thread": round(hcnt_wall, 3),
           "correct_device_ms": round(cor_dev, 3), "correct_call_ms": round(cor_wall, 3), f"host_correct_ms_{a.threads}_threads": round(hcor_wall, 3),
           "barcodes_per_s_device_call": round(n / cor_wall * 1e3), f"barcodes_per_s_host_twin_{a.threads}_threads": round(n / hcor_wall * 1e3),
           "status_share": {str(v): round(float((s_dev == v).mean()), 4) for v in (-1, 0, 1)}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    os.remove(path)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
