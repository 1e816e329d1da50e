#!/usr/bin/env python3
"""tools/bench_inflate.py - what inflating BGZF read files on the device costs (profiles/inflate_bench.json; nothing in the test suite
depends on it).

Workload: --reads FASTQ records (10 M; the records of tools/bench_dump.py: 150 bases, ids of 20 bytes, 326 bytes a record) as one
text, cut into members of 65280 bytes three ways: zlib level 6 (what bgzip writes), and this project's own compressor with the fixed
code and with dynamic codes.  The text goes through the inflater in calls of --call-mb MB of text (a call takes less than 4 GiB).

Per kind, in one process: the device times by HIP events (cfr_inflate_get_stats: upload_ms, inflate_ms = k_bgzf_inflate) and the
wall time of cfr_inflate_bgzf with the text left in HBM; the host twin on 16 threads and zlib on one thread over the same members;
then the comparison the feature exists for: cfr_inflate_bgzf + cfr_tokenize_resident (compressed bytes in) against cfr_tokenize of
the host text (text in), wall time both.  Medians over --reps repetitions behind one warm-up call each.
The figures are merged into the JSON file given by --out under the key "api".

  --cli   end to end: tests/golden/se.fq 25 000 times over (10 M reads, 3.1 GB) as BGZF of 65280 bytes per member, zlib level 6;
          bin/centrifuger -u 10M.fq.gz -t 16 on the golden index f10 with and without --gpu-inflate, --cli-runs alternating runs
          each: every run's wall time, the md5 of its TSV and the stages' busy seconds (CFR_CLI_TIMING) appended to
          profiles/gpu_inflate_cli_timing.txt, the wall times under the key "cli"."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BLOCK = 65280


def say(*a):
    print("[bench_inflate]", time.strftime("%H:%M:%S"), *a, flush=True)


def make_text(n):
    import bench_dump as bd
    idb, _ = bd.make_ids(n)
    seq, _, qual, _ = bd.make_reads(n)
    rec = np.empty((n, 326), dtype=np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1:21] = idb.reshape(n, 20)
    rec[:, 21] = 10
    rec[:, 22:172] = seq.reshape(n, 150)
    rec[:, 172:175] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 175:325] = qual.reshape(n, 150)
    rec[:, 325] = 10
    return rec.reshape(-1)


def _bgzip(piece):
    out = []
    for at in range(0, len(piece), BLOCK):
        t = piece[at:at + BLOCK]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        d = c.compress(t) + c.flush()
        size = 18 + len(d) + 8
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (size - 1).to_bytes(2, "little") + d + zlib.crc32(t).to_bytes(4, "little") + len(t).to_bytes(4, "little"))
    return b"".join(out)


def zlib_members(text, call_bytes):
    """the calls' members, made on 16 processes"""
    calls = [bytes(text[a:a + call_bytes]) for a in range(0, len(text), call_bytes)]
    step = BLOCK * 256
    with ProcessPoolExecutor(16) as ex:
        return [b"".join(ex.map(_bgzip, [c[a:a + step] for a in range(0, len(c), step)])) for c in calls]


def zlib_inflate(members):
    at, n, view = 0, 0, memoryview(members)
    while at < len(members):
        size = int.from_bytes(members[at + 16:at + 18], "little") + 1
        n += len(zlib.decompress(view[at + 18:at + size - 8], -15))
        at += size
    return n


def med(v):
    return statistics.median(v)


def part_api(n, reps, call_mb):
    from centrifuger_amd import capi
    text = make_text(n)
    call_bytes = call_mb * 1000000 // 326 * 326                        # whole records per call
    calls_text = [text[a:a + call_bytes] for a in range(0, len(text), call_bytes)]
    say(f"text made: {len(text)} bytes in {len(calls_text)} calls")
    kinds = {"zlib_level_6": zlib_members(text, call_bytes)}
    for codes in ("fixed", "dynamic"):
        g = capi.Gz(device=0, codes=codes)
        kinds[f"own_{codes}"] = [g.compress(t) for t in calls_text]
        g.close()
    say("members made")
    dev, host, tok = capi.Inflate(device=0), capi.Inflate(), capi.Tokenizer(device=0)
    rows = {"reads": n, "text_bytes": int(len(text)), "call_text_bytes": call_bytes, "reps": reps}
    for kind, calls in kinds.items():
        arrs = [np.frombuffer(c, dtype=np.uint8) for c in calls]
        row = {"compressed_bytes": sum(len(c) for c in calls), "members": 0}
        ms = {k: [] for k in ("upload_ms", "inflate_ms", "wall_ms", "inflate_tokenize_wall_ms", "host_16_threads_ms")}
        for r in range(reps + 1):
            acc = dict.fromkeys(ms, 0.0)
            for a, t in zip(arrs, calls_text):
                w = time.perf_counter()
                size, info = dev.inflate(a, fetch_text=False, copy=False)
                acc["wall_ms"] += (time.perf_counter() - w) * 1e3
                assert size == len(t) and info.bad_members == 0
                st = dev.stats()
                acc["upload_ms"] += st.upload_ms
                acc["inflate_ms"] += st.inflate_ms
                if r == 0:
                    row["members"] += int(info.members)
                    got, _ = dev.inflate(a)                             # the bytes, once
                    assert got == t.tobytes()
                w = time.perf_counter()
                dev.inflate(a, fetch_text=False, copy=False)
                d_text, size = dev.device_text()
                ti = tok.tokenize_resident(d_text, size)
                acc["inflate_tokenize_wall_ms"] += (time.perf_counter() - w) * 1e3
                assert ti.irregular == 0 and ti.n_records == len(t) // 326
                w = time.perf_counter()
                host.inflate(a, copy=False)
                acc["host_16_threads_ms"] += (time.perf_counter() - w) * 1e3
            if r:
                for k in ms:
                    ms[k].append(acc[k])
        row.update({k: med(v) for k, v in ms.items()})
        w = time.perf_counter()
        assert sum(zlib_inflate(c) for c in calls) == len(text)
        row["zlib_1_thread_ms"] = (time.perf_counter() - w) * 1e3
        row["gb_per_s_k_bgzf_inflate"] = len(text) / row["inflate_ms"] / 1e6
        row["gb_per_s_call"] = len(text) / row["wall_ms"] / 1e6
        row["gb_per_s_host_16_threads"] = len(text) / row["host_16_threads_ms"] / 1e6
        row["gb_per_s_zlib_1_thread"] = len(text) / row["zlib_1_thread_ms"] / 1e6
        rows[kind] = row
        say(kind, json.dumps(row))
    tms = []
    for r in range(reps + 1):
        w = time.perf_counter()
        for t in calls_text:
            tok.tokenize(t)
        if r:
            tms.append((time.perf_counter() - w) * 1e3)
    rows["tokenize_from_host_text_wall_ms"] = med(tms)
    rows["note"] = ("inflate_tokenize_wall_ms: cfr_inflate_bgzf (members up from pageable memory, text left in HBM) + cfr_tokenize_resident; "
                    "tokenize_from_host_text_wall_ms: cfr_tokenize of the same text from pageable host memory")
    return rows


def part_cli(runs, log, copies):
    import gzip
    import hashlib
    import shutil
    import subprocess
    import tempfile
    golden = os.path.join(ROOT, "tests", "golden")
    tmp = tempfile.mkdtemp(prefix="cfr_inflate_cli_")
    for f in ("f10.2.cfr", "f10.4.cfr", "f10.3.cfr"):
        if os.path.exists(os.path.join(golden, f)):
            shutil.copy(os.path.join(golden, f), tmp)
    with gzip.open(os.path.join(golden, "f10.1.cfr.gz"), "rb") as fi, open(os.path.join(tmp, "f10.1.cfr"), "wb") as fo:
        shutil.copyfileobj(fi, fo)
    se = open(os.path.join(golden, "se.fq"), "rb").read()
    reads = os.path.join(tmp, "reads.fq.gz")
    per = 500                                                           # copies of se.fq a process compresses at a time
    with ProcessPoolExecutor(16) as ex, open(reads, "wb") as f:
        # (members are cut per process piece: every piece but the last of a piece has 65280 bytes of text)
        for part in ex.map(_bgzip, [se * min(per, copies - a) for a in range(0, copies, per)]):
            f.write(part)
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    say("reads made:", os.path.getsize(reads), "bytes")
    cli = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
    env = dict(os.environ, CFR_CLI_TIMING="1")
    variants = {"host_inflate": [], "gpu_inflate": ["--gpu-inflate"]}
    rows = {k: [] for k in variants}
    md5 = set()
    with open(log, "a") as lf:
        lf.write(f"# -u reads.fq.gz ({copies} x tests/golden/se.fq, BGZF, zlib level 6, 65280 bytes per member)  index f10  -t 16  ({time.strftime('%Y-%m-%d %H:%M:%S')})\n")
        for r in range(runs):
            for name, extra in variants.items():
                w = time.perf_counter()
                p = subprocess.run([cli, "-x", os.path.join(tmp, "f10"), "-u", reads, "-t", "16"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, check=True)
                wall = time.perf_counter() - w
                h = hashlib.md5(p.stdout).hexdigest()
                md5.add(h)
                busy = [l for l in p.stderr.decode().split("\n") if "busy" in l or "--gpu-inflate" in l]
                lf.write(f"run {r} {name:13s} {wall:7.3f} s  md5 {h}  {' | '.join(b.split('] ', 1)[-1] for b in busy)}\n")
                rows[name].append(wall)
                say(r, name, f"{wall:.3f} s")
    shutil.rmtree(tmp)
    return {"reads": 400 * copies, "wall_s": rows, "same_tsv": len(md5) == 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--call-mb", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_bench.json"))
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-runs", type=int, default=4)
    ap.add_argument("--cli-copies", type=int, default=25000)
    ap.add_argument("--cli-log", default=os.path.join(ROOT, "profiles", "gpu_inflate_cli_timing.txt"))
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.cli:
        res["cli"] = part_cli(a.cli_runs, a.cli_log, a.cli_copies)
    else:
        res["api"] = part_api(a.reads, a.reps, a.call_mb)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    say("written", a.out)


if __name__ == "__main__":
    main()
