#!/usr/bin/env python3
"""Regenerate tests/golden/kreport/*: what the REAL reference's centrifuger-kreport (a Perl script) prints for the classification files
the quantifier's fixtures already hold.  Dev container only (needs the reference's source, g++ and perl):
    python tests/golden/make_golden_kreport.py

  kreport/<se_k1|pe_k5|edge|wide>.<set>.txt.gz   the script's stdout for an option set (SETS below); empty where it died
  kreport/count_table.txt                         the one --is-count-table input: a repeated id, an id no tree holds, id 0, a fraction
  kreport/count_table.<set>.txt.gz                the script's stdout for it
  kreport/manifest.json                           per output: index, input, arguments, exit status, the tax ids of the "Couldn't find
                                                  parent of taxID" lines on stderr in order, lines of stdout; md5 of every file
Inputs are quant/se_k1.tsv.gz, quant/pe_k5.tsv.gz, quant/edge.tsv (index quant/q8) and quant_wide/wide.tsv.gz (index quant_wide/qw)
as they stand; nothing is copied.  CentrifugerInspect.cpp is compiled where the reference's source lies into a temporary directory,
and the script is copied beside it there (it starts `centrifuger-inspect` from its own directory).  Committed: data only."""
import gzip
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
INDEXES = {"q8": os.path.join(HERE, "quant", "q8"), "qw": os.path.join(HERE, "quant_wide", "qw")}
INPUTS = {"se_k1": ("q8", os.path.join("quant", "se_k1.tsv.gz")), "pe_k5": ("q8", os.path.join("quant", "pe_k5.tsv.gz")),
          "edge": ("q8", os.path.join("quant", "edge.tsv")), "wide": ("qw", os.path.join("quant_wide", "wide.tsv.gz"))}
# --min-score / --min-length values that drop some reads of every input and not all of them (asserted below through seq_count)
FILTER = {"se_k1": ["--min-score", "10000", "--min-length", "100"], "pe_k5": ["--min-score", "10000", "--min-length", "100"],
          "edge": ["--min-score", "3000", "--min-length", "76"], "wide": ["--min-score", "5000", "--min-length", "140"]}
SETS = {"default": [], "show_zeros": ["--show-zeros"], "score": ["--report-score-data"], "filter": None,
        "filter_score_zeros": None, "no_lca": ["--no-lca"], "no_lca_filter": None, "drop_all": ["--min-score", "1000000000000"]}
COUNT_TABLE = "61\t10\n62\t5\n61\t7\n9999\t3\n0\t4\n90\t2.5\n\n50 1\n"
WARN = re.compile(r"^Couldn't find parent of taxID (\d+) - directly assigned to root\.$")


def run(cmd, **kw):
    print("+", " ".join(cmd), file=sys.stderr)
    return subprocess.run(cmd, **kw)


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def gz_write(path, data):
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(data)


def args_of(key, name):
    if name == "filter":
        return FILTER[key]
    if name == "filter_score_zeros":
        return FILTER[key] + ["--report-score-data", "--show-zeros"]
    if name == "no_lca_filter":
        return ["--no-lca"] + FILTER[key]
    return SETS[name]


def seq_count(stdout):
    """unclassified + the clade of node 1 (reads under another root are in neither; the fixtures have none)"""
    rows = [l.split(b"\t") for l in stdout.split(b"\n") if l]
    return int(rows[0][1]) + (int(rows[1][1]) if len(rows) > 1 else 0)


def main():
    tmp = tempfile.mkdtemp(prefix="cfr_golden_kreport_")
    inspect = os.path.join(tmp, "centrifuger-inspect")
    run(["g++", "-O3", "-msse4.2", "-w", f"-I{REF_SRC}", "-o", inspect, os.path.join(REF_SRC, "CentrifugerInspect.cpp"), "-lpthread", "-lz"], check=True)
    script = os.path.join(tmp, "centrifuger-kreport")
    shutil.copy(os.path.join(REF_SRC, "centrifuger-kreport"), script)
    out = os.path.join(HERE, "kreport")
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    with open(os.path.join(out, "count_table.txt"), "w") as f:
        f.write(COUNT_TABLE)

    outputs = {}

    def one(name, idx, rel, path, args):
        r = run(["perl", script, "-x", INDEXES[idx]] + args + [path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        gz_write(os.path.join(out, name), r.stdout)
        warn = [int(m.group(1)) for m in map(WARN.match, r.stderr.decode().splitlines()) if m]
        outputs[name] = {"index": idx, "input": rel.replace(os.sep, "/"), "args": args, "status": r.returncode, "warnings": warn,
                         "lines": r.stdout.count(b"\n"), "died": "No sequence matches with given settings" in r.stderr.decode()}
        return r

    for key, (idx, rel) in INPUTS.items():
        src = os.path.join(HERE, rel)
        plain = os.path.join(tmp, key + ".tsv")               # (the script opens the file as it is: no gz)
        with (gzip.open(src, "rb") if src.endswith(".gz") else open(src, "rb")) as fi, open(plain, "wb") as fo:
            shutil.copyfileobj(fi, fo)
        total = None
        for name in SETS:
            r = one(f"{key}.{name}.txt.gz", idx, rel, plain, args_of(key, name))
            if name == "default":
                total = seq_count(r.stdout)
            elif name == "filter":
                assert 0 < seq_count(r.stdout) < total, (key, seq_count(r.stdout), total)
                outputs[f"{key}.{name}.txt.gz"]["kept"] = seq_count(r.stdout)
            elif name == "drop_all":
                assert r.returncode != 0 and r.stdout == b""
    for name, args in (("default", []), ("show_zeros_score", ["--show-zeros", "--report-score-data"])):
        one(f"count_table.{name}.txt.gz", "q8", os.path.join("kreport", "count_table.txt"), os.path.join(out, "count_table.txt"), ["--is-count-table"] + args)
    r = run(["perl", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    manifest = {"outputs": outputs, "usage_status": r.returncode,
                "md5": {f: md5(os.path.join(out, f)) for f in sorted(os.listdir(out)) if f != "manifest.json"}}
    with open(os.path.join(out, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    shutil.rmtree(tmp)
    print("wrote", out, file=sys.stderr)


if __name__ == "__main__":
    main()
