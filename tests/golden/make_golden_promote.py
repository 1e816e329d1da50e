#!/usr/bin/env python3
"""Regenerate tests/golden/inspect/* and tests/golden/promote/*: what the REAL reference's centrifuger-inspect and centrifuger-promote
print for the indexes and classification files the quantifier's fixtures already hold.  Dev container only (needs the reference's
source, g++ and perl):  python tests/golden/make_golden_promote.py

  inspect/<q8|qw>.<summary|conversion-table|taxonomy-tree|name-table|size-table>.txt   the reference centrifuger-inspect's stdout
  promote/<se_k1|pe_k5|edge|wide>.<level>.tsv.gz                                     the Perl script's stdout; levels genus, species,
                                                                                     strain, subspecies, "no rank" (file name no_rank),
                                                                                     lca and bogus (a string that names no rank)
  promote/manifest.json                                                              arguments, warning counts and md5 of every file
Inputs are quant/se_k1.tsv.gz, quant/pe_k5.tsv.gz, quant/edge.tsv (index quant/q8) and quant_wide/wide.tsv.gz (index quant_wide/qw)
as they stand; nothing is copied.  CentrifugerInspect.cpp is compiled where the reference's source lies into a temporary directory,
and the script is copied beside it there (it starts `centrifuger-inspect` from its own directory).  Committed: data only.

The in-pipeline comparison of tests/test_gpu_promote.py (bin/centrifuger --promote against these files) rests on neighbouring reads
of quant/reads_*.fq.gz carrying different ids - the script takes consecutive rows with one id for one read - which is asserted here."""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
INSPECT_MODES = ["summary", "conversion-table", "taxonomy-tree", "name-table", "size-table"]
INDEXES = {"q8": os.path.join(HERE, "quant", "q8"), "qw": os.path.join(HERE, "quant_wide", "qw")}
INPUTS = {"se_k1": ("q8", os.path.join("quant", "se_k1.tsv.gz")), "pe_k5": ("q8", os.path.join("quant", "pe_k5.tsv.gz")),
          "edge": ("q8", os.path.join("quant", "edge.tsv")), "wide": ("qw", os.path.join("quant_wide", "wide.tsv.gz"))}
LEVELS = ["genus", "species", "strain", "subspecies", "no rank", "lca", "bogus"]


def run(cmd, **kw):
    print("+", " ".join(cmd), file=sys.stderr)
    return subprocess.run(cmd, check=True, **kw)


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def gz_write(path, data):
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(data)


def read_ids(path):
    with gzip.open(path, "rb") as f:
        return [line.split()[0][1:] for k, line in enumerate(f) if k % 4 == 0]


def main():
    for name in ("reads_se.fq.gz", "reads_1.fq.gz", "reads_2.fq.gz"):
        ids = read_ids(os.path.join(HERE, "quant", name))
        assert all(a != b for a, b in zip(ids, ids[1:])), f"{name}: two neighbouring reads share an id"
    tmp = tempfile.mkdtemp(prefix="cfr_golden_promote_")
    inspect = os.path.join(tmp, "centrifuger-inspect")
    run(["g++", "-O3", "-msse4.2", "-w", f"-I{REF_SRC}", "-o", inspect, os.path.join(REF_SRC, "CentrifugerInspect.cpp"), "-lpthread", "-lz"])
    script = os.path.join(tmp, "centrifuger-promote")
    shutil.copy(os.path.join(REF_SRC, "centrifuger-promote"), script)

    out_i = os.path.join(HERE, "inspect")
    out_p = os.path.join(HERE, "promote")
    for d in (out_i, out_p):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
    for idx, prefix in INDEXES.items():
        for mode in INSPECT_MODES:
            with open(os.path.join(out_i, f"{idx}.{mode}.txt"), "wb") as fo:
                run([inspect, "-x", prefix, "--" + mode], stdout=fo)

    outputs = {}
    for key, (idx, rel) in INPUTS.items():
        src = os.path.join(HERE, rel)
        plain = os.path.join(tmp, key + ".tsv")               # (the script opens the file as it is: no gz)
        with (gzip.open(src, "rb") if src.endswith(".gz") else open(src, "rb")) as fi, open(plain, "wb") as fo:
            shutil.copyfileobj(fi, fo)
        for level in LEVELS:
            r = run(["perl", script, INDEXES[idx], plain, level], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            name = f"{key}.{level.replace(' ', '_')}.tsv.gz"
            gz_write(os.path.join(out_p, name), r.stdout)
            warnings = [l for l in r.stderr.decode().splitlines() if l.startswith("Couldn't find parent of taxID")]
            outputs[name] = {"index": idx, "input": rel.replace(os.sep, "/"), "level": level, "warnings": len(warnings), "rows": r.stdout.count(b"\n") - 1}
    manifest = {"levels": LEVELS, "inspect_modes": INSPECT_MODES, "outputs": outputs,
                "md5": {os.path.relpath(os.path.join(d, f), HERE).replace(os.sep, "/"): md5(os.path.join(d, f))
                        for top in (out_i, out_p) for d, _s, fs in os.walk(top) for f in sorted(fs) if f != "manifest.json"}}
    with open(os.path.join(out_p, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    shutil.rmtree(tmp)
    print("wrote", out_i, out_p, file=sys.stderr)


if __name__ == "__main__":
    main()
