#!/usr/bin/env python3
"""tools/bench_kreport.py - what the Kraken-style report costs (profiles/kreport_bench.json; nothing in the test suite depends on it).

Workload: that of tools/bench_promote.py - a synthetic taxonomy of 102 101 nodes, 10 M reads with lists of 1-5 strains that lie close
together, one id in a hundred in no tree - in two distributions of the reads over the taxa: `uniform` (as generated) and `skewed`
(half of the reads, picked at random, moved into the four strains of one species).

  --api    device time of k_kreport_fold and k_kreport_accumulate by HIP events (cfr_kreport_get_stats), the wall time of
           cfr_kreport_add_results around them (host buffers in), the host twin on 16 threads in the same process, and for orientation
           the device time of k_promote_lca over the same reads (the fold does the same walks)
  --tool   bin/centrifuger-kreport end to end on a TSV of the same shape (10 M reads), --gpu 0 and --gpu none, output to /dev/null
  --pipeline  the classifier on bench.py's default index and reads (10 M x 150 bp, -k 1, wide results): device time of a step with the
           switch off and with the report on, and the report kernels' own time (cfr_last_kreport_ms: the folds of all sub-batches and
           the one accumulate of the call)
  --bench-line TAG=FILE (repeatable)  the last JSON line of a `bench.py --gpus 1` run kept in FILE, recorded under bench_py_default_line[TAG]:
           this commit and the parent commit, run in turn on one box in one session (bench.py's default entry is the compact one, which
           the report never touches)
  --perl   the reference's Perl script on a 1 M-row sample, on the CPU, where perl and the script exist (CFR_REFERENCE_SRC); it
           starts bin/centrifuger-inspect, whose output is the reference's byte for byte
Every part merges its figures into the JSON file given by --out."""
import argparse
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

BIN = bp.BIN


def skew(res, mat, orig, t0, seed):
    """half of the reads, at random, into the four strains below the first species"""
    rng = np.random.default_rng(seed)
    res, mat = res.copy(), mat.copy()
    hot = np.nonzero(rng.random(len(res)) < 0.5)[0]
    lens = res["n_match"][hot].astype(np.int64)
    slots = np.repeat(res["match_begin"][hot].astype(np.int64), lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
    node = t0 + rng.integers(0, bp.STR // bp.SPE, size=len(slots))
    mat["id"][slots], mat["taxid"][slots] = node, orig[node]
    return res, mat


def part_api(prefix, loads, reps):
    from centrifuger_amd import capi
    out = {}
    for name, (res, mat) in loads.items():
        n = len(res)
        row = {}
        k = capi.Kreport(prefix, device=0)
        fold, acc, wall = [], [], []
        for r in range(reps + 1):
            t = time.perf_counter()
            k.add_results(res, mat)
            w = (time.perf_counter() - t) * 1e3
            if r:                                               # (the first call allocates)
                st = k.stats()
                fold.append(st.fold_ms); acc.append(st.accumulate_ms); wall.append(w)
        own_d, _c, sc_d, _cs, seq_d = k.counts()
        k.close()
        row["device"] = {"k_kreport_fold_ms": bp.median(fold), "k_kreport_accumulate_ms": bp.median(acc), "add_results_wall_ms_with_copies": bp.median(wall),
                         "reads_per_s_kernels": n / (bp.median(fold) + bp.median(acc)) * 1e3}
        h = capi.Kreport(prefix, device=None, threads=16)
        host = []
        for r in range(reps + 1):
            h.add_results(res, mat)
            if r:
                host.append(h.stats().fold_ms)
        own_h, _c, sc_h, _cs, seq_h = h.counts()
        h.close()
        assert np.array_equal(own_d, own_h) and np.array_equal(sc_d, sc_h) and seq_d == seq_h == n * (reps + 1)
        row["host_16_threads"] = {"add_results_ms": bp.median(host), "reads_per_s": n / bp.median(host) * 1e3}
        row["largest_bin_share"] = float(own_d.max()) / float(own_d.sum())
        p = capi.Promote(prefix, "lca", device=0)
        lca = []
        for r in range(reps + 1):
            a, b = res.copy(), mat.copy()
            p.apply(a, b)
            if r:
                lca.append(p.stats().reads_ms)
        p.close()
        row["k_promote_lca_ms_same_process"] = bp.median(lca)
        out[name] = row
    return out


def part_tool(prefix, tsv, reads, rows):
    out = {"reads": reads, "rows": rows, "tsv_bytes": os.path.getsize(tsv)}
    for name, gpu in (("gpu_0", "0"), ("gpu_none", "none")):
        best = None
        for _ in range(2):
            t = time.perf_counter()
            with open(os.devnull, "wb") as sink:
                subprocess.run([os.path.join(BIN, "centrifuger-kreport"), "--gpu", gpu, "-x", prefix, tsv], check=True, stdout=sink, stderr=subprocess.DEVNULL)
            w = time.perf_counter() - t
            best = w if best is None else min(best, w)
        out[name] = {"seconds": best, "rows_per_s": rows / best}
    return out


def part_perl(tsv_rows=1_000_000):
    src = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
    script = os.path.join(src, "centrifuger-kreport")
    if not (shutil.which("perl") and os.path.exists(script)):
        return None
    d = tempfile.mkdtemp(prefix="cfr_bench_kreport_perl_")
    os.makedirs(os.path.join(d, "bin"))                   # the script starts centrifuger-inspect from its own directory; ours finds the library one up
    shutil.copy(script, os.path.join(d, "bin", "centrifuger-kreport"))
    shutil.copy(os.path.join(BIN, "centrifuger-inspect"), os.path.join(d, "bin", "centrifuger-inspect"))
    shutil.copy(os.path.join(ROOT, "centrifuger_amd", "libcfr_hip.so"), d)
    orig, t0 = bp.write_taxonomy(os.path.join(d, "tax"))
    res, mat = bp.make_reads(400_000, 7, orig, t0)
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
    t = time.perf_counter()
    with open(os.devnull, "wb") as sink:
        subprocess.run(["perl", os.path.join(d, "bin", "centrifuger-kreport"), "-x", os.path.join(d, "tax"), sample], check=True, stdout=sink, stderr=subprocess.DEVNULL)
    w = time.perf_counter() - t
    out.update({"seconds": w, "rows_per_s": lines / w})            # (includes the two centrifuger-inspect runs that load the tree)
    t = time.perf_counter()
    with open(os.devnull, "wb") as sink:
        subprocess.run([os.path.join(BIN, "centrifuger-kreport"), "--gpu", "none", "-x", os.path.join(d, "tax"), sample], check=True, stdout=sink, stderr=subprocess.DEVNULL)
    out["this_tool_gpu_none_same_file_seconds"] = time.perf_counter() - t
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

    def steps(on):
        dev.set_kreport(on)
        total, rep = [], []
        for k in range(reps + 1):
            dev.classify_resident(reads_d.data_ptr(), offs_d.data_ptr(), args.reads, args.reads * args.read_len, results=res.array, matches=mat.array)
            if k:
                total.append(dev.last_stats().total_ms); rep.append(dev.last_kreport_ms())
        return total, rep
    off, _ = steps(False)
    on, rep = steps(True)
    off2, _ = steps(False)
    out = {"reads": args.reads, "entry": "cfr_classify_batch_resident (wide results, -k 1, fast-load image)",
           "step_ms_switch_off": bp.median(off + off2), "step_ms_switch_off_runs": [round(x, 3) for x in off + off2],
           "step_ms_kreport_on": bp.median(on), "step_ms_kreport_on_runs": [round(x, 3) for x in on],
           "note": "step_ms is the device span first search to last tail; the one accumulate of the call runs behind it and is in report_kernels_ms only",
           "report_kernels_ms_per_10M_reads": bp.median(rep) * 1e7 / args.reads}
    dev.close(); idx.close(); res.free(); mat.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kreport_bench.json"))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-line", action="append", default=[], metavar="TAG=FILE")
    for part in ("api", "tool", "perl", "pipeline"):
        ap.add_argument("--" + part, action="store_true")
    a = ap.parse_args()
    if a.pipeline:            # torch initialises HIP before the library makes the process's first HIP call (the order tests/conftest.py keeps)
        import torch
        torch.cuda.init()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for item in a.bench_line:
        tag, path = item.split("=", 1)
        lines = [l for l in open(path).read().splitlines() if l.lstrip().startswith("{")]
        j = json.loads(lines[-1])
        doc.setdefault("bench_py_default_line", {})[tag] = {k: j[k] for k in ("metric", "value", "unit", "ms_per_step", "steps") if k in j}
    doc["workload"] = {"nodes": 1 + bp.FAM + bp.GEN + bp.SPE + bp.STR, "reads": a.reads, "list_lengths": "1-5", "unknown_id_rate": 0.01,
                       "distributions": {"uniform": "as tools/bench_promote.py draws them", "skewed": "half of the reads in the four strains of one species"}}
    tmp = tempfile.mkdtemp(prefix="cfr_bench_kreport_")

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    try:
        prefix = os.path.join(tmp, "tax")
        orig, t0 = bp.write_taxonomy(prefix)
        if a.api or a.tool:
            res, mat = bp.make_reads(a.reads, 1, orig, t0)
        if a.api:
            doc["api"] = part_api(prefix, {"uniform": (res, mat), "skewed": skew(res, mat, orig, t0, 2)}, a.reps)
            save()
        if a.tool:
            tsv = os.path.join(tmp, "reads.tsv")
            reads, rows = bp.write_tsv(tsv, res, mat)
            doc["offline_tool"] = part_tool(prefix, tsv, reads, rows)
            save()
        if a.pipeline:
            doc["classifier"] = part_pipeline(a.reps)
            save()
        if a.perl:
            doc["perl_script_cpu"] = part_perl()
            doc["perl_script_cpu"]["where"] = "a development machine that holds the reference's source; not reproducible where it is absent (None there)"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    save()
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
