#!/usr/bin/env python3
"""centrifuger-quant, three ways, on two synthetic classification files (writes profiles/quant_bench.json and prints it):
  k1   10 M rows, one per read (`-k 1`): strains, species and genera of a taxonomy of 50 species x 20 strains (synth.make_genomes)
  k5   10 M reads with 1..5 rows each (`-k 5`): strains of one species, the strain-rich case where the EM has work to do
Timed, wall clock of the whole command each: the reference quantifier (oracle/_ref/centrifuger-quant or $CFR_REF_QUANT when present,
else null), the host twin on 16 threads (`--gpu none -t 16`) and the device path (`--gpu 0 -t 16`); the twin and the device path also
report their split into reader, coalesce and EM (rounds, ms per round) through cfr_quant_get_stats.  The three reports must be
byte-equal.  The small index (genomes of 2 kbp) is written by the product's own writer on the GPU; only its taxonomy matters here."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
QUANT = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger-quant")
HEADER = "readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\n"


def write_tsv(path, g, reads, k, seed, block=200_000):
    """`reads` reads; a block of `block` distinct reads is generated once and written over and over (read ids differ inside a block and
    across its seam, which is all the grouping looks at)"""
    rng = np.random.default_rng(seed)
    strains = {}
    for (tid, par, rank) in g.nodes:
        if rank == "strain":
            strains.setdefault(par, []).append(tid)
    species = sorted(strains)
    parent = {tid: par for tid, par, _r in g.nodes}
    rows = []
    for i in range(block):
        sp = species[int(rng.zipf(1.6)) % len(species)]
        hit = 150 - int(rng.integers(0, 14)) if rng.random() < 0.3 else 150
        if k == 1:
            r = rng.random()
            tid = strains[sp][int(rng.integers(0, len(strains[sp])))] if r < 0.6 else (sp if r < 0.9 else parent[sp])
            rows.append(f"b{i}\tseq\t{tid}\t{hit * hit}\t{0 if r < 0.6 else hit * hit}\t{hit}\t150\t1\n")
        else:
            m = int(rng.integers(1, k + 1))
            first = int(rng.integers(0, len(strains[sp])))
            for j in range(m):
                rows.append(f"b{i}\tseq\t{strains[sp][(first + j * 3) % len(strains[sp])]}\t{hit * hit}\t{0 if m == 1 else hit * hit}\t{hit}\t150\t{m}\n")
    text = "".join(rows).encode()
    with open(path, "wb") as f:
        f.write(HEADER.encode())
        for _ in range(max(1, reads // block)):
            f.write(text)
    return max(1, reads // block) * len(rows)


def timed(cmd, out_path):
    t0 = time.perf_counter()
    with open(out_path, "wb") as fo:
        r = subprocess.run(cmd, stdout=fo, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return wall, r.stderr.decode()


def split(prefix, tsv, device):
    """reader / coalesce / EM of one in-process run through the C-ABI"""
    from centrifuger_amd import capi
    q = capi.Quant(prefix, device=device, threads=16)
    q.add_tsv(tsv)
    n = len(q.assignments()[0])
    rounds = q.run()
    st = q.stats()
    q.close()
    return {"reader_ms": round(st.reader_ms, 1), "coalesce_ms": round(st.coalesce_ms, 1), "em_ms": round(st.em_ms, 2), "em_rounds": rounds,
            "em_ms_per_round": round(st.em_ms / max(rounds, 1), 3), "distinct_lists": n, "table_grown": int(st.grow_count)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_bench.json"))
    ap.add_argument("--ref", default=os.environ.get("CFR_REF_QUANT", os.path.join(ROOT, "oracle", "_ref", "centrifuger-quant")))
    a = ap.parse_args()
    from centrifuger_amd import capi, synth
    tmp = tempfile.mkdtemp(prefix="cfr_bench_quant_")
    g = synth.make_genomes(n_species=50, n_strains=20, genome_len=2000, seed=20261101)
    prefix = os.path.join(tmp, "strains20")
    capi.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, prefix, ftab_chars=6)
    out = {"bench": "quant", "reads": a.reads, "taxonomy": "50 species x 20 strains", "reference_binary": os.path.exists(a.ref), "cases": {}}
    for key, k in (("k1", 1), ("k5", 5)):
        tsv = os.path.join(tmp, key + ".tsv")
        rows = write_tsv(tsv, g, a.reads, k, 7 + k)
        case = {"rows": rows, "tsv_bytes": os.path.getsize(tsv)}
        rep = {}
        if os.path.exists(a.ref):
            case["reference_s"], _ = timed([a.ref, "-x", prefix, "-c", tsv], os.path.join(tmp, "ref.txt"))
            rep["reference"] = open(os.path.join(tmp, "ref.txt"), "rb").read()
        else:
            case["reference_s"] = None
        case["host_twin_16_threads_s"], _ = timed([QUANT, "--gpu", "none", "-t", "16", "-x", prefix, "-c", tsv], os.path.join(tmp, "host.txt"))
        case["device_s"], _ = timed([QUANT, "--gpu", "0", "-t", "16", "-x", prefix, "-c", tsv], os.path.join(tmp, "dev.txt"))
        rep["host"] = open(os.path.join(tmp, "host.txt"), "rb").read()
        rep["device"] = open(os.path.join(tmp, "dev.txt"), "rb").read()
        case["device_equals_host_twin"] = rep["device"] == rep["host"]
        case["host_twin_equals_reference"] = (rep["host"] == rep["reference"]) if "reference" in rep else None
        case["host_twin_split"] = split(prefix, tsv, None)
        case["device_split"] = split(prefix, tsv, 0)
        for name in ("reference_s", "host_twin_16_threads_s", "device_s"):
            if case[name] is not None:
                case[name] = round(case[name], 3)
        if case["reference_s"]:
            case["speedup_vs_reference"] = {"host_twin": round(case["reference_s"] / case["host_twin_16_threads_s"], 1),
                                            "device": round(case["reference_s"] / case["device_s"], 1)}
        out["cases"][key] = case
        os.remove(tsv)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    assert all(c["device_equals_host_twin"] and c["host_twin_equals_reference"] is not False for c in out["cases"].values()), "reports differ"


if __name__ == "__main__":
    main()
