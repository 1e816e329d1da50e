#!/usr/bin/env python3
"""tools/bench_promote.py - what promotion costs (profiles/promote_bench.json; nothing in the test suite depends on it).

Workload: a synthetic taxonomy of ~1e5 nodes (root / 100 families / 2 000 genera / 20 000 species / 80 000 strains, written straight
into a .2.cfr), 10 M reads with lists of 1-5 strains - the strains of one read lie close together, as a classifier's ties do, and one
id in a hundred is in no tree - promoted to `genus` and folded with `lca`.

  --api       device time of k_promote_table and k_promote_reads / k_promote_lca by HIP events (cfr_promote_get_stats), the wall time
              of cfr_promote_apply around them (host buffers in and out), and the host twin on 16 threads in the same process
  --tool      bin/centrifuger-promote end to end on a TSV of the same shape (10 M reads), --gpu 0 and --gpu none, output to /dev/null
  --pipeline  the classifier on bench.py's default index and reads (10 M x 150 bp, -k 1, wide results): device time of a step with the
              switch off and with --promote genus, and the promotion kernels' own time (cfr_last_promote_ms)
  --perl      the reference's Perl script on a 1 M-row sample, on the CPU, where perl and the script exist (CFR_REFERENCE_SRC); it
              starts bin/centrifuger-inspect, whose output is the reference's byte for byte
  --bench-line TAG=FILE (repeatable)  the last JSON line of a `bench.py --gpus 1` run kept in FILE, recorded under bench_py_default_line[TAG]:
              the default line of this commit and of the parent commit, run in turn on one box in one session (bench.py's default entry is
              the compact one, which promotion never touches)
Every part merges its figures into the JSON file given by --out."""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "centrifuger_amd", "bin")
FAM, GEN, SPE, STR = 100, 2000, 20000, 80000


def write_taxonomy(prefix):
    """root 1; families 100+; genera 10 000+; species 100 000+; strains 1 000 000+ (children of a node are consecutive)"""
    orig = np.concatenate([[1], 100 + np.arange(FAM), 10_000 + np.arange(GEN), 100_000 + np.arange(SPE), 1_000_000 + np.arange(STR)]).astype(np.uint64)
    f0, g0, s0, t0 = 1, 1 + FAM, 1 + FAM + GEN, 1 + FAM + GEN + SPE
    parent = np.concatenate([[0], np.zeros(FAM, dtype=np.int64), f0 + np.arange(GEN) // (GEN // FAM), g0 + np.arange(SPE) // (SPE // GEN),
                             s0 + np.arange(STR) // (STR // SPE)]).astype(np.uint64)
    rank = np.concatenate([[0], np.full(FAM, 4), np.full(GEN, 3), np.full(SPE, 2), np.full(STR, 1)]).astype(np.uint8)
    n = len(orig)
    nodes = np.zeros(n, dtype=np.dtype([("parent", "<u8"), ("rank", "u1"), ("leaf", "u1"), ("pad", "u1", 6)]))
    nodes["parent"], nodes["rank"], nodes["leaf"] = parent, rank, (rank == 1)
    with open(prefix + ".2.cfr", "wb") as f:
        f.write(struct.pack("<QQQ", n, 1, 0))
        f.write(nodes.tobytes())
        f.write(struct.pack("<Q", n)); f.write(orig.tobytes())
        for i in range(n):
            name = b"t%d" % orig[i]
            f.write(struct.pack("<Q", len(name))); f.write(name)
        f.write(struct.pack("<Q", t0))                       # the one sequence belongs to the first strain
        f.write(struct.pack("<Q", 4)); f.write(b"seq0")
    with open(prefix + ".3.cfr", "wb") as f:
        f.write(struct.pack("<QQ", 0, 1000))
    return orig, t0


def make_reads(n, seed, orig, t0):
    from centrifuger_amd import capi
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 6, size=n)
    begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(begin[-1])
    first = np.repeat(rng.integers(0, STR - 64, size=n), lens)
    node = t0 + first + rng.integers(0, 64, size=total)         # within 64 strains: same species, genus or family
    unknown = rng.random(total) < 0.01
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    res["score"], res["hit_length"], res["query_length"], res["n_match"], res["match_begin"] = 5000, 148, 150, lens, begin[:-1]
    mat = np.zeros(total, dtype=capi.MATCH_DTYPE)
    mat["kind"] = 1
    mat["id"] = np.where(unknown, len(orig), node)
    mat["taxid"] = np.where(unknown, 99_999_999, orig[node])
    return res, mat


def median(xs):
    return float(np.median(xs))


def part_api(prefix, res0, mat0, reps):
    from centrifuger_amd import capi
    out = {}
    n = len(res0)
    for level in ("genus", "lca"):
        row = {}
        for name, device in (("device", 0), ("host_16_threads", None)):
            p = capi.Promote(prefix, level, device=device)
            kern, wall, table = [], [], p.stats().table_ms
            for k in range(reps + 1):
                res, mat = res0.copy(), mat0.copy()
                t = time.perf_counter()
                p.apply(res, mat)
                w = (time.perf_counter() - t) * 1e3
                if k:                                           # (the first call allocates)
                    wall.append(w); kern.append(p.stats().reads_ms)
            p.close()
            if device is None:
                row[name] = {"apply_ms": median(kern), "reads_per_s": n / median(kern) * 1e3}
                host = (res, mat)
            else:
                row[name] = {"k_promote_table_ms": table, "per_read_kernel_ms": median(kern), "reads_per_s_kernel": n / median(kern) * 1e3,
                             "apply_wall_ms_with_copies": median(wall)}
                dev = (res, mat)
        assert np.array_equal(host[0], dev[0])
        row["kept_matches"] = int(dev[0]["n_match"].sum())
        out[level] = row
    return out


def write_tsv(path, res, mat, block_reads=100_000):
    """the rows of the first block_reads reads, written as often as it takes (read ids differ between neighbours; that is all the tools look at)"""
    lines = []
    for i in range(block_reads):
        b, k = int(res["match_begin"][i]), int(res["n_match"][i])
        for j in range(k):
            lines.append(f"r{i}\tseq\t{int(mat['taxid'][b + j])}\t5000\t5000\t148\t150\t{k}\n")
    block = "".join(lines).encode()
    times = len(res) // block_reads
    with open(path, "wb") as f:
        f.write(b"readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\n")
        for _ in range(times):
            f.write(block)
    return times * block_reads, times * len(lines)


def part_tool(prefix, tsv, reads, rows):
    out = {"reads": reads, "rows": rows, "tsv_bytes": os.path.getsize(tsv)}
    for level in ("genus", "lca"):
        for name, gpu in (("gpu_0", "0"), ("gpu_none", "none")):
            best = None
            for _ in range(2):
                t = time.perf_counter()
                with open(os.devnull, "wb") as sink:
                    subprocess.run([os.path.join(BIN, "centrifuger-promote"), "--gpu", gpu, prefix, tsv, level], check=True, stdout=sink, stderr=subprocess.DEVNULL)
                w = time.perf_counter() - t
                best = w if best is None else min(best, w)
            out[f"{level}_{name}"] = {"seconds": best, "rows_per_s": rows / best}
    return out


def part_perl(prefix, tsv_rows=1_000_000):
    src = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
    script = os.path.join(src, "centrifuger-promote")
    if not (shutil.which("perl") and os.path.exists(script)):
        return None
    d = tempfile.mkdtemp(prefix="cfr_bench_promote_perl_")
    os.makedirs(os.path.join(d, "bin"))                   # the script starts centrifuger-inspect from its own directory; ours finds the library one up
    shutil.copy(script, os.path.join(d, "bin", "centrifuger-promote"))
    shutil.copy(os.path.join(BIN, "centrifuger-inspect"), os.path.join(d, "bin", "centrifuger-inspect"))
    shutil.copy(os.path.join(ROOT, "centrifuger_amd", "libcfr_hip.so"), d)
    orig, t0 = write_taxonomy(os.path.join(d, "tax"))
    res, mat = make_reads(400_000, 7, orig, t0)
    sample = os.path.join(d, "sample.tsv")
    lines = 0
    with open(sample, "w") as f:
        f.write("readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\n")
        for i in range(len(res)):
            b, k = int(res["match_begin"][i]), int(res["n_match"][i])
            for j in range(k):
                f.write(f"r{i}\tseq\t{int(mat['taxid'][b + j])}\t5000\t5000\t148\t150\t{k}\n")
                lines += 1
            if lines >= tsv_rows:
                break
    out = {"rows": lines}
    for level in ("genus", "lca"):
        t = time.perf_counter()
        with open(os.devnull, "wb") as sink:
            subprocess.run(["perl", os.path.join(d, "bin", "centrifuger-promote"), os.path.join(d, "tax"), sample, level], check=True, stdout=sink, stderr=subprocess.DEVNULL)
        w = time.perf_counter() - t
        out[level] = {"seconds": w, "rows_per_s": lines / w}       # (includes the two centrifuger-inspect runs that load the tree)
    shutil.rmtree(d)
    return out


def part_pipeline(reps):
    import torch
    import bench
    from centrifuger_amd import capi
    args = argparse.Namespace(species=50, strains=5, genome_len=4_000_000, seed=20260928, divergence_step=0.01, index_gbp=0.0, builder="own",
                              divergence_model="star", read_len=150, reads=10_000_000)
    device = torch.device("cuda:0")
    cache = os.path.join(os.environ.get("CFR_BENCH_CACHE", "/tmp/cfr_bench"), bench.cache_key(args))
    prefix = bench.build_index(args, cache, device)
    cat = np.load(os.path.join(cache, "genome_cat.npy"), mmap_mode="r")
    starts = np.load(os.path.join(cache, "genome_starts.npy"))
    cat_d = torch.from_numpy(np.ascontiguousarray(cat)).to(device)
    reads_d = bench.make_reads_gpu(torch, cat_d, starts, args.reads, args.read_len, args.seed + 1000, device)
    del cat_d
    torch.cuda.empty_cache()
    offs_d = torch.arange(args.reads + 1, device=device, dtype=torch.int64) * args.read_len
    torch.cuda.synchronize()
    idx = capi.Index(prefix, capi.default_params(max_result=1))
    dev = capi.DeviceIndex(idx, 0, capi.default_device_options(profile=capi.PROFILE_FAST_LOAD))
    res = capi.PinnedArray(args.reads, capi.RESULT_DTYPE)
    mat = capi.PinnedArray(args.reads, capi.MATCH_DTYPE)

    def steps(level):
        dev.set_promote(level)
        total, promo = [], []
        for k in range(reps + 1):
            dev.classify_resident(reads_d.data_ptr(), offs_d.data_ptr(), args.reads, args.reads * args.read_len, results=res.array, matches=mat.array)
            if k:
                total.append(dev.last_stats().total_ms); promo.append(dev.last_promote_ms())
        return total, promo
    off, _ = steps(None)
    on, promo = steps("genus")
    off2, _ = steps(None)
    dev.set_promote(None)
    out = {"reads": args.reads, "entry": "cfr_classify_batch_resident (wide results, -k 1, fast-load image)",
           "step_ms_switch_off": median(off + off2), "step_ms_switch_off_runs": [round(x, 3) for x in off + off2],
           "step_ms_promote_genus": median(on), "step_ms_promote_genus_runs": [round(x, 3) for x in on],
           "promotion_kernels_ms_per_10M_reads": median(promo) * 1e7 / args.reads}
    dev.close(); idx.close(); res.free(); mat.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "promote_bench.json"))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-line", action="append", default=[], metavar="TAG=FILE")
    for part in ("api", "tool", "pipeline", "perl"):
        ap.add_argument("--" + part, action="store_true")
    a = ap.parse_args()
    if a.pipeline:            # torch initialises HIP before the library makes the process's first HIP call (the order tests/conftest.py keeps)
        import torch
        torch.cuda.init()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["workload"] = {"nodes": 1 + FAM + GEN + SPE + STR, "reads": a.reads, "list_lengths": "1-5", "unknown_id_rate": 0.01, "levels": ["genus", "lca"]}
    for item in a.bench_line:
        tag, path = item.split("=", 1)
        lines = [l for l in open(path).read().splitlines() if l.lstrip().startswith("{")]
        j = json.loads(lines[-1])
        keep = {k: j[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "reads_per_step") if k in j}
        doc.setdefault("bench_py_default_line", {})[tag] = keep or j
    tmp = tempfile.mkdtemp(prefix="cfr_bench_promote_")

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    try:
        prefix = os.path.join(tmp, "tax")
        orig, t0 = write_taxonomy(prefix)
        if a.api or a.tool:
            res, mat = make_reads(a.reads, 1, orig, t0)
        if a.api:
            doc["api"] = part_api(prefix, res, mat, a.reps)
            save()
        if a.tool:
            tsv = os.path.join(tmp, "reads.tsv")
            reads, rows = write_tsv(tsv, res, mat)
            doc["offline_tool"] = part_tool(prefix, tsv, reads, rows)
            save()
        if a.pipeline:
            doc["classifier"] = part_pipeline(a.reps)
        if a.perl:
            doc["perl_script_cpu"] = part_perl(prefix)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    save()
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
