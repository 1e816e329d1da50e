#!/usr/bin/env python
"""The tokeniser alone (cfr_tokenize): 10 M x 150 bp reads as FASTQ and as FASTA, handed over in chunks of about 256 MB.
Per format and per chunk: the device handle's device_ms (copy in, kernels, the small copies out), its parts from the events inside the call
(cfr_tokenizer_get_stats: copy_in_ms, kernel_ms, and the kernels' share of device_ms), the call's wall time, and the host twin on 16
threads over the same chunks in the same process (every chunk cut into 16 parts at record starts, one handle per thread).
Writes profiles/parse_bench.json (or --out).  Needs an MI355X; --reads N for a shorter run."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from centrifuger_amd import capi  # noqa: E402


def make_chunk(first, n, fastq, rng):
    """n records with ids read.<9 digits>, 150 bases, as one uint8 array (every record has the same length)"""
    head = np.frombuffer((b"@" if fastq else b">") + b"read.000000000/1\n", dtype=np.uint8)
    rec_len = len(head) + 151 + (2 + 151 if fastq else 0)
    a = np.empty((n, rec_len), dtype=np.uint8)
    a[:, :len(head)] = head
    ids = np.arange(first, first + n, dtype=np.int64)
    for d in range(9):
        a[:, 6 + 8 - d] = 48 + (ids // 10 ** d) % 10
    a[:, len(head):len(head) + 150] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 150))]
    a[:, len(head) + 150] = 10
    if fastq:
        a[:, len(head) + 151] = ord("+")
        a[:, len(head) + 152] = 10
        a[:, len(head) + 153:len(head) + 303] = ord("I")
        a[:, len(head) + 303] = 10
    return a.reshape(-1), rec_len


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--chunk-mb", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(5)
    dev = capi.Tokenizer(args.device)
    hosts = [capi.Tokenizer(None) for _ in range(args.threads)]
    pool = ThreadPoolExecutor(args.threads)
    result = {"reads": args.reads, "read_length": 150, "chunk_mb": args.chunk_mb, "host_threads": args.threads, "formats": {}}
    for fastq in (True, False):
        rec_len = make_chunk(0, 1, fastq, rng)[1]
        per_chunk = (args.chunk_mb << 20) // rec_len
        rows, done = [], 0
        while done < args.reads:
            n = min(per_chunk, args.reads - done)
            text, _ = make_chunk(done, n, fastq, rng)
            dev.tokenize(text)                                  # (first touch of the chunk's pages and of grown buffers)
            t0 = time.perf_counter()
            info = dev.tokenize(text)
            wall = (time.perf_counter() - t0) * 1e3
            assert info.n_records == n and info.irregular == 0 and info.total_bases == 150 * n
            st = dev.stats()
            cuts = [(n * k // args.threads) * rec_len for k in range(args.threads + 1)]
            t0 = time.perf_counter()
            got = list(pool.map(lambda k: hosts[k].tokenize(text[cuts[k]:cuts[k + 1]]).n_records, range(args.threads)))
            host_ms = (time.perf_counter() - t0) * 1e3
            assert sum(got) == n
            rows.append({"records": n, "bytes": int(len(text)), "device_ms": round(info.device_ms, 3), "copy_in_ms": round(st.copy_in_ms, 3), "kernel_ms": round(st.kernel_ms, 3),
                         "kernel_share": round(st.kernel_ms / info.device_ms, 4), "device_call_wall_ms": round(wall, 3), "host_twin_ms": round(host_ms, 3)})
            done += n
        tot = {k: sum(r[k] for r in rows) for k in ("records", "bytes", "device_ms", "copy_in_ms", "kernel_ms", "device_call_wall_ms", "host_twin_ms")}
        result["formats"]["fastq" if fastq else "fasta"] = {
            "chunks": rows,
            "device_reads_per_s": tot["records"] / (tot["device_ms"] * 1e-3), "device_gb_per_s": tot["bytes"] / (tot["device_ms"] * 1e-3) / 1e9,
            "kernel_share_of_device_ms": tot["kernel_ms"] / tot["device_ms"],
            "device_call_reads_per_s": tot["records"] / (tot["device_call_wall_ms"] * 1e-3),
            "host_twin_reads_per_s": tot["records"] / (tot["host_twin_ms"] * 1e-3)}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {m: (round(v, 3) if isinstance(v, float) else v) for m, v in r.items() if m != "chunks"} for k, r in result["formats"].items()}))


if __name__ == "__main__":
    main()
