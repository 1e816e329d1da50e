#!/usr/bin/env python3
"""tools/bench_dump.py - what making and compressing the --un / --cl read dumps on the device costs (profiles/dump_bench.json; nothing in
the test suite depends on it).

Workload: --reads FASTQ records (10 M) of 150 bases with ids of 20 bytes (`SRR12345678.` and 8 digits): reads drawn from a random
genome of 4 Mbp with one substitution in a hundred, qualities from seven symbols with a geometric distribution (what an Illumina run
binned to few quality values looks like); every read selected, one file.

  --api    in one process: the device times of the record step (format_ms: length kernel, scan, write kernel), of the compressor
           (deflate_ms) and of scan + pack (pack_ms) by HIP events (cfr_gz_get_stats); the wall time of cfr_gz_dump around them (host
           arrays in from pageable memory, members out: its copies included); the host twin on 16 threads over the same arrays (bytes
           compared); zlib level 1 on one thread over the same text (what gzprintf into a "w1" stream costs at the least), in the same
           process; and the compressed size against zlib level 1.
  --cli FILE   bin/centrifuger -u FILE --un A --cl B -t 16 end to end, index --cli-index, with and without --gpu-dump, --cli-runs
           alternating runs each: every run's wall time, the md5 of its TSV, the size of its dump files, the md5 of what they inflate
           to (first run only) and the stages' busy seconds (CFR_CLI_TIMING) appended to profiles/gpu_dump_cli_timing.txt.
  --codes dynamic   the same two parts for dynamic Huffman codes (cfr_gz_options.codes = 1, --gpu-dump-codes dynamic) beside the fixed code:
           --api runs a fixed and a dynamic device handle in one process, their calls alternating, and reports both kernels' event
           times, both sizes and the sizes against zlib level 1 under the key "api_dynamic"; --cli runs --gpu-dump with the fixed code
           and with dynamic codes alternately, under "cli_dynamic".  The keys of the default --codes fixed stay as they are.
Every part merges its figures into the JSON file given by --out."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "centrifuger_amd", "bin")


def make_ids(n):
    """n ids of 20 bytes, `SRR12345678.` and 8 digits -> (bytes uint8[20 n], offsets uint64[n + 1])"""
    ids = np.empty((n, 20), dtype=np.uint8)
    ids[:, :12] = np.frombuffer(b"SRR12345678.", dtype=np.uint8)
    k = np.arange(n, dtype=np.int64)
    for d in range(8):
        ids[:, 19 - d] = 48 + (k // 10 ** d) % 10
    return ids.reshape(-1), np.arange(n + 1, dtype=np.uint64) * 20


def make_reads(n, read_len=150, seed=7):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, 4_000_000)]
    seq = np.empty((n, read_len), dtype=np.uint8)
    qual = np.empty((n, read_len), dtype=np.uint8)
    qsym = np.frombuffer(b"FFFF:,#", dtype=np.uint8)
    step = 500_000
    for lo in range(0, n, step):
        m = min(step, n - lo)
        at = rng.integers(0, len(genome) - read_len, m)
        s = genome[at[:, None] + np.arange(read_len)[None, :]]
        flip = rng.random((m, read_len)) < 0.01
        s[flip] = acgt[rng.integers(0, 4, int(flip.sum()))]
        seq[lo:lo + m] = s
        qual[lo:lo + m] = qsym[np.minimum(rng.geometric(0.6, (m, read_len)) - 1, 6)]
    off = np.arange(n + 1, dtype=np.uint64) * read_len
    return seq.reshape(-1), off, qual.reshape(-1), off.copy()


def inflate_members(data):
    """BGZF members -> text, member by member along their BSIZE fields"""
    out, at, view = [], 0, memoryview(data)
    while at < len(data):
        size = int.from_bytes(data[at + 16:at + 18], "little") + 1
        out.append(zlib.decompress(view[at + 18:at + size - 8], -15))
        at += size
    return b"".join(out)


def say(*a):
    print("[bench_dump]", time.strftime("%H:%M:%S"), *a, flush=True)


def part_api(n, reps):
    from centrifuger_amd import capi
    idb, ido = make_ids(n)
    seq, so, qual, qo = make_reads(n)
    say("reads made")
    select, has = np.ones(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)
    files = [(seq, so, qual, qo, has)]
    rows = {"reads": n, "read_len": 150, "id_bytes": 20}
    keep = {}
    for name, h in (("device", capi.Gz(device=0)), ("host_16_threads", capi.Gz(threads=16))):
        ms = {k: [] for k in ("upload_ms", "format_ms", "deflate_ms", "pack_ms", "download_ms", "wall_ms")}
        for r in range(reps + 1):
            t = time.perf_counter()
            if r == 0:
                members = h.dump_arrays(idb, ido, select, files)[0]
                keep[name] = hashlib.md5(members).hexdigest()
                if name == "device":
                    text = inflate_members(members)
                rows["compressed_bytes"] = len(members)
                del members
            else:
                h.dump_arrays(idb, ido, select, files, copy=False)
            w = (time.perf_counter() - t) * 1e3
            if r:                                               # (the first call allocates, and copies the members into Python)
                st = h.stats()
                for k in ms:
                    ms[k].append(w if k == "wall_ms" else getattr(st, k))
        st = h.stats()
        row = {k: statistics.median(v) for k, v in ms.items()}
        row["md5"] = keep[name]
        row["blocks"], row["stored_blocks"], row["bytes_in"], row["bytes_out"] = int(st.blocks), int(st.stored_blocks), int(st.bytes_in), int(st.bytes_out)
        if name == "device":
            row["gb_per_s_record_kernels"] = st.bytes_in / row["format_ms"] / 1e6
            row["gb_per_s_deflate_kernel"] = st.bytes_in / row["deflate_ms"] / 1e6
            row["gb_per_s_call"] = st.bytes_in / row["wall_ms"] / 1e6
            row["wall_ms_note"] = "cfr_gz_dump with its copies: ids, sequences and qualities up from pageable memory, the members down into the handle's pinned buffer"
        else:
            row["gb_per_s"] = st.bytes_in / (row["format_ms"] + row["deflate_ms"]) / 1e6
        rows[name] = row
        h.close()
        say(name, json.dumps(row))
    assert keep["device"] == keep["host_16_threads"]
    rows["text_bytes"] = len(text)
    say("zlib level 1 over", len(text), "bytes")
    t = time.perf_counter()
    z = zlib.compress(text, 1)
    w = time.perf_counter() - t
    rows["zlib_level_1_one_thread"] = {"seconds": w, "gb_per_s": len(text) / w / 1e9, "compressed_bytes": len(z)}
    rows["size_against_zlib_level_1"] = rows["compressed_bytes"] / len(z)
    rows["ratio"] = {"fixed_huffman_bgzf": len(text) / rows["compressed_bytes"], "zlib_level_1": len(text) / len(z)}
    return rows


def part_api_dynamic(n, reps):
    """a fixed and a dynamic device handle over the same arrays, their calls alternating; the dynamic host twin for the bytes; zlib level 1"""
    from centrifuger_amd import capi
    idb, ido = make_ids(n)
    seq, so, qual, qo = make_reads(n)
    say("reads made")
    select, has = np.ones(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)
    files = [(seq, so, qual, qo, has)]
    rows = {"reads": n, "read_len": 150, "id_bytes": 20}
    handles = {"fixed": capi.Gz(device=0), "dynamic": capi.Gz(device=0, codes="dynamic")}
    ms = {name: {k: [] for k in ("format_ms", "deflate_ms", "pack_ms", "download_ms", "wall_ms")} for name in handles}
    md5, text = {}, None
    for r in range(reps + 1):
        for name, h in handles.items():
            t = time.perf_counter()
            if r == 0:
                members = h.dump_arrays(idb, ido, select, files)[0]
                md5[name] = hashlib.md5(members).hexdigest()
                got = inflate_members(members)
                assert text is None or got == text
                text = got
                del members, got
                continue
            h.dump_arrays(idb, ido, select, files, copy=False)
            w = (time.perf_counter() - t) * 1e3
            st = h.stats()
            for k in ms[name]:
                ms[name][k].append(w if k == "wall_ms" else getattr(st, k))
    for name, h in handles.items():
        st = h.stats()
        row = {k: statistics.median(v) for k, v in ms[name].items()}
        row["deflate_ms_all"] = ms[name]["deflate_ms"]
        row["md5"] = md5[name]
        row["blocks"], row["stored_blocks"], row["dynamic_blocks"], row["bytes_in"], row["bytes_out"] = (int(st.blocks), int(st.stored_blocks), int(st.dynamic_blocks),
                                                                                                         int(st.bytes_in), int(st.bytes_out))
        row["gb_per_s_deflate_kernel"] = st.bytes_in / row["deflate_ms"] / 1e6
        rows[name] = row
        h.close()
        say(name, json.dumps(row))
    host = capi.Gz(threads=16, codes="dynamic")
    t = time.perf_counter()
    members = host.dump_arrays(idb, ido, select, files)[0]
    rows["host_16_threads_dynamic"] = {"wall_ms": (time.perf_counter() - t) * 1e3, "deflate_ms": host.stats().deflate_ms, "md5": hashlib.md5(members).hexdigest()}
    assert rows["host_16_threads_dynamic"]["md5"] == md5["dynamic"]
    del members
    host.close()
    rows["text_bytes"] = len(text)
    say("zlib level 1 over", len(text), "bytes")
    t = time.perf_counter()
    z = zlib.compress(text, 1)
    w = time.perf_counter() - t
    rows["zlib_level_1_one_thread"] = {"seconds": w, "gb_per_s": len(text) / w / 1e9, "compressed_bytes": len(z)}
    rows["size_against_zlib_level_1"] = {k: rows[k]["bytes_out"] / len(z) for k in handles}
    rows["size_dynamic_against_fixed"] = rows["dynamic"]["bytes_out"] / rows["fixed"]["bytes_out"]
    rows["deflate_time_dynamic_against_fixed"] = rows["dynamic"]["deflate_ms"] / rows["fixed"]["deflate_ms"]
    rows["ratio"] = {"fixed_huffman_bgzf": len(text) / rows["fixed"]["bytes_out"], "dynamic_huffman_bgzf": len(text) / rows["dynamic"]["bytes_out"], "zlib_level_1": len(text) / len(z)}
    return rows


def part_cli(reads_file, index, runs, log, dynamic=False):
    cli = os.path.join(BIN, "centrifuger")
    env = dict(os.environ, CFR_CLI_TIMING="1")
    variants = {"host_dump": [], "gpu_dump": ["--gpu-dump"]}
    if dynamic:
        variants = {"gpu_dump": ["--gpu-dump"], "gpu_dump_dynamic": ["--gpu-dump", "--gpu-dump-codes", "dynamic"]}
    out = {k: {"seconds": [], "md5": [], "dump_bytes": []} for k in variants}
    with open(log, "a") as lf:
        lf.write(f"# -u {reads_file} --un A --cl B  index {index}  -t 16  ({time.strftime('%Y-%m-%d %H:%M:%S')})\n")
        for r in range(runs):
            for name, extra in variants.items():
                work = tempfile.mkdtemp(prefix="cfr_bench_dump_")
                t = time.perf_counter()
                p = subprocess.run([cli, "-x", index, "-t", "16", "-u", reads_file, "--un", os.path.join(work, "A"), "--cl", os.path.join(work, "B")] + extra,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, env=env)
                w = time.perf_counter() - t
                md5 = hashlib.md5(p.stdout).hexdigest()
                sizes = {f: os.path.getsize(os.path.join(work, f)) for f in sorted(os.listdir(work))}
                out[name]["seconds"].append(round(w, 3)); out[name]["md5"].append(md5); out[name]["dump_bytes"].append(sizes)
                clocks = " ".join("%s %s" % tuple(l.split()[1:3]) for l in p.stderr.decode().splitlines() if l.startswith("[timing]"))
                lf.write(f"run {r} {name:{16 if dynamic else 10}s} {w:8.3f} s  md5 {md5}  dumps {sizes}  busy s: {clocks}\n")
                lf.flush()
                say(f"run {r} {name} {w:.3f} s")
                if r == 0:                                      # what the dumps inflate to: gzip reads both framings
                    inflated = {}
                    for f in sizes:
                        h, z = hashlib.md5(), subprocess.Popen(["gzip", "-dc", os.path.join(work, f)], stdout=subprocess.PIPE)
                        for chunk in iter(lambda: z.stdout.read(1 << 24), b""):
                            h.update(chunk)
                        assert z.wait() == 0
                        inflated[f] = h.hexdigest()
                    out[name]["inflated_md5"] = inflated
                    lf.write(f"run {r} {name:{16 if dynamic else 10}s} inflated md5 {inflated}\n")
                    lf.flush()
                shutil.rmtree(work)
    first, second = list(variants)
    assert out[first]["inflated_md5"] == out[second]["inflated_md5"] and set(out[first]["md5"]) == set(out[second]["md5"])
    for v in out.values():
        v["median_seconds"] = statistics.median(v["seconds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dump_bench.json"))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--api", action="store_true")
    ap.add_argument("--cli", metavar="FILE")
    ap.add_argument("--cli-index")
    ap.add_argument("--cli-runs", type=int, default=4)
    ap.add_argument("--cli-log", default=os.path.join(ROOT, "profiles", "gpu_dump_cli_timing.txt"))
    ap.add_argument("--codes", choices=("fixed", "dynamic"), default="fixed")
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    dynamic = a.codes == "dynamic"
    if a.api:
        if dynamic:
            doc["api_dynamic"] = part_api_dynamic(a.reads, a.reps)
        else:
            doc["api"] = part_api(a.reads, a.reps)
        save()
    if a.cli:
        if not a.cli_index:
            ap.error("--cli needs --cli-index")
        doc.setdefault("cli_dynamic" if dynamic else "cli", {})[os.path.basename(a.cli)] = part_cli(a.cli, a.cli_index, a.cli_runs, a.cli_log, dynamic)
        save()
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
