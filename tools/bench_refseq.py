"""The front end of bin/centrifuger-build, timed against another build of the same command line (the parent commit's): one plain FASTA
generated from a seed (centrifuger_amd/synth.py, as bench.py makes its genomes), the two builders run alternately on it, `runs` times
each.  Per run: the wall time of the whole command, the writer's own total from its last log line, the front end = wall - writer (what
happens before cfr_build_index: reading, filtering, and - in the parent - nothing of the upload, which its writer does), and from the
new builder's "Front end:" line the front end on its own clock with cfr_refseq_feed / cfr_refseq_assemble from device events.

  python tools/bench_refseq.py --parent-bin PATH/centrifuger-build [--bases 1000000000] [--runs 3] [--out profiles/refseq_bench.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centrifuger_amd import synth  # noqa: E402


def run(binary, args):
    t0 = time.perf_counter()
    r = subprocess.run([binary] + args, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    err = r.stderr.decode()
    if r.returncode != 0:
        raise SystemExit(f"{binary} failed:\n{err[-2000:]}")
    out = {"wall_s": round(wall, 3)}
    m = re.search(r"suffix array ([0-9.]+) s, total ([0-9.]+) s", err)
    out["suffix_array_s"], out["writer_s"] = float(m.group(1)), float(m.group(2))
    out["front_end_s"] = round(wall - out["writer_s"], 3)
    m = re.search(r"Front end: ([0-9.]+) s \((\d+) records; filter ([0-9.]+) s of which copy in ([0-9.]+) s, assemble ([0-9.]+) s\)", err)
    if m:
        out.update(front_end_own_clock_s=float(m.group(1)), feed_device_s=float(m.group(3)), feed_copy_in_s=float(m.group(4)), assemble_device_s=float(m.group(5)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", required=True)
    ap.add_argument("--bases", type=float, default=1e9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20240229)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refseq_bench.json"))
    a = ap.parse_args()
    genome_len = 4_000_000
    n_genomes = max(2, int(a.bases // genome_len))
    n_species = max(1, n_genomes // 2)
    new_bin = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger-build")
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        g, _ = synth.make_genomes_fast(n_species, 2, genome_len, seed=a.seed, threads=16)
        synth.write_reference_inputs(g, tmp)
        print(f"input: {g.total_len} bases in {len(g.names)} sequences, {os.path.getsize(os.path.join(tmp, 'ref.fa'))} bytes of FASTA ({time.perf_counter() - t0:.1f} s)", flush=True)
        args = ["-r", os.path.join(tmp, "ref.fa"), "--taxonomy-tree", os.path.join(tmp, "nodes.dmp"), "--name-table", os.path.join(tmp, "names.dmp"),
                "--conversion-table", os.path.join(tmp, "seqid.map"), "-t", "16"]
        res = {"parent": [], "this": []}
        for k in range(a.runs):
            for who, binary in (("parent", a.parent_bin), ("this", new_bin)):
                r = run(binary, args + ["-o", os.path.join(tmp, who)])
                res[who].append(r)
                print(who, k, json.dumps(r), flush=True)
        same = all(open(os.path.join(tmp, f"parent.{k}.cfr"), "rb").read() == open(os.path.join(tmp, f"this.{k}.cfr"), "rb").read() for k in (1, 2, 3))
    fe_p, fe_t = [r["front_end_s"] for r in res["parent"]], [r["front_end_s"] for r in res["this"]]
    summary = {"bases": g.total_len, "sequences": len(g.names), "seed": a.seed, "runs": res, "files_equal": same,
               "front_end_parent_s": {"min": min(fe_p), "max": max(fe_p)}, "front_end_this_s": {"min": min(fe_t), "max": max(fe_t)},
               "parent_spread_s": round(max(fe_p) - min(fe_p), 3), "gain_s": round(min(fe_p) - max(fe_t), 3),
               "device_front_end_is_faster_than_the_parents_spread": min(fe_p) - max(fe_t) > max(fe_p) - min(fe_p)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in summary.items() if k != "runs"}))


if __name__ == "__main__":
    main()
