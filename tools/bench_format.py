#!/usr/bin/env python3
"""tools/bench_format.py - what making the TSV rows on the device costs (profiles/format_bench.json; nothing in the test suite depends on it).

Workload: the reads of tools/bench_promote.py - a synthetic taxonomy of 102 101 nodes, 10 M reads with lists of 1-5 strains, one id in
a hundred in no tree - with read ids of 20 bytes.  The handle wants a whole index: the FM index of tests/golden/f6 stands under the
synthetic taxonomy (the formatter reads names and rank codes only).

  --api    in one process: len_ms, scan_ms and write_ms of the kernels by HIP events and direct_blocks (cfr_tsv_get_stats), the wall
           time of cfr_tsv_format around them (host arrays in, text out: its copies included), and the host twin on 16 threads over the
           same arrays (the yardstick for the kernels); texts compared byte for byte
  --cli FILE...  bin/centrifuger end to end on the given read file(s) (-u FILE, or -1 FILE -2 FILE with two), index --cli-index, -t 16:
           the default command line, --gpu-format, --gpu-parse and --gpu-parse --gpu-format, --cli-runs alternating runs each, every
           run's wall time, the md5 of its TSV and the stages' busy seconds (CFR_CLI_TIMING) appended to
           profiles/gpu_format_cli_timing.txt; --cli-parent BINARY adds the parent commit's default command line to the series
Every part merges its figures into the JSON file given by --out."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_promote as bp  # noqa: E402

F6 = os.path.join(ROOT, "tests", "golden", "f6")


def make_ids(n):
    """n ids of 20 bytes, `SRR12345678.` and 8 digits -> (bytes uint8[20 n], offsets uint64[n + 1])"""
    ids = np.empty((n, 20), dtype=np.uint8)
    ids[:, :12] = np.frombuffer(b"SRR12345678.", dtype=np.uint8)
    k = np.arange(n, dtype=np.int64)
    for d in range(8):
        ids[:, 19 - d] = 48 + (k // 10 ** d) % 10
    return ids.reshape(-1), np.arange(n + 1, dtype=np.uint64) * 20


def part_api(prefix, res, mat, reps):
    from centrifuger_amd import capi
    n = len(res)
    idb, ido = make_ids(n)
    idx = capi.Index(prefix)
    host, dev = capi.Tsv(idx, device=None, threads=16), capi.Tsv(idx, device=0)
    status, need, _t, _o = host.format_raw(res, mat, idb, ido, 0, want_offsets=False)
    assert status == capi.CFR_ERR_CAPACITY
    rows = {"reads": n, "rows": int(res["n_match"].clip(1).sum()), "text_bytes": need}
    keep = {}
    for name, h in (("device", dev), ("host_16_threads", host)):
        ms = {k: [] for k in ("upload_ms", "len_ms", "scan_ms", "write_ms", "download_ms", "wall_ms")}
        for r in range(reps + 1):
            t = time.perf_counter()
            status, ln, text, _o = h.format_raw(res, mat, idb, ido, need, want_offsets=False)
            w = (time.perf_counter() - t) * 1e3
            assert status == capi.CFR_OK and ln == need
            if r:                                               # (the first call allocates)
                st = h.stats()
                for k in ms:
                    ms[k].append(w if k == "wall_ms" else getattr(st, k))
        keep[name] = hashlib.md5(text[:need].tobytes()).hexdigest()
        st = h.stats()
        row = {k: bp.median(v) for k, v in ms.items()}
        row["md5"] = keep[name]
        if name == "device":
            row["blocks"], row["direct_blocks"] = int(st.blocks), int(st.direct_blocks)
            row["reads_per_s_kernels"] = n / (row["len_ms"] + row["scan_ms"] + row["write_ms"]) * 1e3
            row["wall_ms_note"] = "cfr_tsv_format with its copies: results, matches and ids up from pageable memory, the text down into a numpy array"
        else:
            row["reads_per_s"] = n / (row["len_ms"] + row["write_ms"]) * 1e3
        rows[name] = row
    assert keep["device"] == keep["host_16_threads"]
    dev.close(); host.close(); idx.close()
    return rows


def part_cli(files, index, runs, log, parent=None):
    cli = os.path.join(bp.BIN, "centrifuger")
    reads = ["-u", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]
    variants = {"default": (cli, []), "gpu_format": (cli, ["--gpu-format"]), "gpu_parse": (cli, ["--gpu-parse"]),
                "gpu_parse_gpu_format": (cli, ["--gpu-parse", "--gpu-format"])}
    if parent:
        variants["parent_default"] = (parent, [])       # the parent commit's binary in the same alternating series
    env = dict(os.environ, CFR_CLI_TIMING="1")
    out = {k: {"seconds": [], "md5": []} for k in variants}
    with open(log, "a") as lf:
        lf.write(f"# {' '.join(reads)}  index {index}  -t 16  ({time.strftime('%Y-%m-%d %H:%M:%S')})\n")
        for r in range(runs):
            for name, (exe, extra) in variants.items():
                t = time.perf_counter()
                p = subprocess.run([exe, "-x", index, "-t", "16"] + reads + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, env=env)
                w = time.perf_counter() - t
                md5 = hashlib.md5(p.stdout).hexdigest()
                out[name]["seconds"].append(round(w, 3)); out[name]["md5"].append(md5)
                clocks = " ".join("%s %s" % tuple(l.split()[1:3]) for l in p.stderr.decode().splitlines() if l.startswith("[timing]"))
                lf.write(f"run {r} {name:22s} {w:8.3f} s  md5 {md5}  busy s: {clocks}\n")
    for v in out.values():
        v["median_seconds"] = bp.median(v["seconds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "format_bench.json"))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--api", action="store_true")
    ap.add_argument("--cli", nargs="+", metavar="FILE")
    ap.add_argument("--cli-index")
    ap.add_argument("--cli-runs", type=int, default=4)
    ap.add_argument("--cli-parent", metavar="BINARY", help="the parent commit's bin/centrifuger: its default command line joins the series")
    ap.add_argument("--cli-log", default=os.path.join(ROOT, "profiles", "gpu_format_cli_timing.txt"))
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    tmp = tempfile.mkdtemp(prefix="cfr_bench_format_")

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    try:
        if a.api:
            prefix = os.path.join(tmp, "tax")
            orig, t0 = bp.write_taxonomy(prefix)
            for ext in ("1", "4"):
                os.symlink(F6 + f".{ext}.cfr", prefix + f".{ext}.cfr")
            res, mat = bp.make_reads(a.reads, 1, orig, t0)
            doc["workload"] = {"nodes": 1 + bp.FAM + bp.GEN + bp.SPE + bp.STR, "reads": a.reads, "list_lengths": "1-5", "unknown_id_rate": 0.01, "id_bytes": 20}
            doc["api"] = part_api(prefix, res, mat, a.reps)
            save()
        if a.cli:
            if not a.cli_index:
                ap.error("--cli needs --cli-index")
            doc.setdefault("cli", {})[" ".join(os.path.basename(f) for f in a.cli)] = part_cli(a.cli, a.cli_index, a.cli_runs, a.cli_log, a.cli_parent)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    save()
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
