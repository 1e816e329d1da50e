#!/usr/bin/env python3
"""Regenerate tests/golden/quant/*: a small index whose taxonomy exercises the quantifier, classification TSVs, and what the REAL
reference quantifier prints for them.  Dev container only:  make -C oracle ref && python tests/golden/make_golden_quant.py

  q8.{1,2,3,4}.cfr     written by the reference's centrifuger-build (oracle/_ref) from the inputs made below (8 sequences):
                         1 root / 10 superkingdom / 20 clade / 30 phylum / 40 no rank / 50, 80 genus / 60, 70, 90, 91 species /
                         61, 62 strain (two genomes of one species, 6000 and 9000 bases) / 71 subspecies
                         species 70 holds a sequence of its own AND a child with one (a node with sequences that is not a leaf)
                         species 90: NC_000101.1 + NC_000102.1 are one genome (consecutive accessions), NC_000110.1 another
                         species 91: NZ_000300.1, NZ_000305.1 are two genomes (not consecutive)
  reads_se.fq.gz, reads_1.fq.gz, reads_2.fq.gz   3000 single reads, 2000 pairs (what bin/centrifuger --quant is run on)
  se_k1.tsv.gz, pe_k5.tsv.gz                     the reference centrifuger's output for them (-k 1, -k 5)
  edge.tsv, header_only.tsv                      hand-made rows, one for every branch of LoadReadAssignments
  report/<tsv>.<f|n><format>.txt                 the reference centrifuger-quant's stdout: format 0..3, n = no filter,
                                                 f = --min-score 300 --min-length 40
  manifest.json                                  arguments and md5 of every file
The reference quantifier is compiled where its source lies into a temporary directory.  Committed: data only."""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "quant")
REF = os.path.join(ROOT, "oracle", "_ref")
REF_SRC = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
SEED = 20261101
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGTN")] = list(b"TGCAN")

NODES = [(1, 1, "no rank"), (10, 1, "superkingdom"), (20, 10, "clade"), (30, 20, "phylum"), (40, 30, "no rank"), (50, 40, "genus"),
         (60, 50, "species"), (61, 60, "strain"), (62, 60, "strain"), (70, 50, "species"), (71, 70, "subspecies"), (80, 40, "genus"),
         (90, 80, "species"), (91, 80, "species")]
NAMES = {1: "root", 10: "Bacteria", 20: "Terra group", 30: "Examplota", 40: "unclassified Examplota", 50: "Alphagenus", 60: "Alphagenus primus",
         61: "Alphagenus primus str. A", 62: "Alphagenus primus str. B", 70: "Alphagenus secundus", 71: "Alphagenus secundus subsp. minor",
         80: "Betagenus", 90: "Betagenus tertius", 91: "Betagenus quartus"}
# name, tax id, length, (name of the sequence it is derived from, divergence) or None
SEQS = [("NC_000001.1", 61, 6000, None), ("NC_000003.1", 62, 9000, ("NC_000001.1", 0.01)), ("NC_000010.1", 70, 5000, None),
        ("NC_000020.1", 71, 7000, ("NC_000010.1", 0.02)), ("NC_000101.1", 90, 4000, None), ("NC_000102.1", 90, 3000, None),
        ("NC_000110.1", 90, 5000, ("NC_000101.1", 0.03)), ("NZ_000300.1", 91, 3500, ("NC_000102.1", 0.02)), ("NZ_000305.1", 91, 2500, None)]
FILTER = ["--min-score", "300", "--min-length", "40"]

HEADER = "readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\n"
EDGE_ROWS = [
    # plain unique reads
    ("r1", "NC_000001.1", 61, 18225, 0, 150, 150, 1),
    ("r2", "NC_000003.1", 62, 18225, 0, 150, 150, 1),
    # adjacent reads with the same id: ONE assignment [61, 62, 61]; weight and uniq from the first row
    ("dup", "NC_000001.1", 61, 10000, 400, 140, 150, 1),
    ("dup", "NC_000003.1", 62, 18225, 0, 150, 150, 1),
    ("dup", "NC_000001.1", 61, 18225, 0, 150, 150, 1),
    # two targets, both orders
    ("ab", "NC_000001.1", 61, 12000, 12000, 130, 150, 2),
    ("ab", "NC_000003.1", 62, 12000, 12000, 130, 150, 2),
    ("ba", "NC_000003.1", 62, 12000, 12000, 130, 150, 2),
    ("ba", "NC_000001.1", 61, 12000, 12000, 130, 150, 2),
    ("ab2", "NC_000001.1", 61, 12000, 12000, 149, 150, 2),
    ("ab2", "NC_000003.1", 62, 12000, 12000, 149, 150, 2),
    # unclassified
    ("u1", "unclassified", 0, 0, 0, 0, 150, 1),
    # a tax id the tree does not hold: counted for the root; twice in one list, and beside a real one
    ("x1", "foreign", 9999, 5000, 0, 100, 100, 1),
    ("x2", "foreign", 9999, 5000, 5000, 100, 100, 2),
    ("x2", "foreign2", 8888, 5000, 5000, 100, 100, 2),
    ("x3", "foreign", 9999, 5000, 5000, 100, 100, 2),
    ("x3", "NC_000101.1", 90, 5000, 5000, 100, 100, 2),
    # rows that only the filter removes (score 299 / hitLength 39), and rows that just pass it
    ("f1", "NC_000010.1", 70, 299, 0, 150, 150, 1),
    ("f2", "NC_000010.1", 70, 5000, 0, 39, 150, 1),
    ("f3", "NC_000010.1", 70, 300, 0, 40, 45, 1),
    # a group whose first row the filter removes and whose second it keeps: weight and uniq come from the second
    ("g1", "NC_000020.1", 71, 200, 100, 150, 150, 2),
    ("g1", "NC_000010.1", 70, 400, 400, 60, 70, 2),
    # a dropped row between two rows of one id does not split the group
    ("g2", "NC_000101.1", 90, 900, 0, 80, 80, 3),
    ("g2", "none", 0, 900, 0, 80, 80, 3),
    ("g2", "NZ_000300.1", 91, 900, 0, 80, 80, 3),
    # a read shorter than 100 bases: int(readLength * 0.01) == 0, so one missing base already costs a factor of 4
    ("s1", "NZ_000305.1", 91, 3000, 0, 75, 76, 1),
    ("s2", "NZ_000305.1", 91, 3000, 0, 76, 76, 1),
    # longer than 100: one missing base is free
    ("s3", "NZ_000305.1", 91, 3000, 0, 149, 150, 1),
    # d = 10, 11, far more than 11, and a hit longer than the read
    ("d10", "NC_000110.1", 90, 2000, 0, 139, 150, 1),
    ("d11", "NC_000110.1", 90, 2000, 0, 138, 150, 1),
    ("d99", "NC_000110.1", 90, 2000, 0, 41, 150, 1),
    ("neg", "NC_000110.1", 90, 2000, 0, 160, 150, 1),
    # species with a sequence of its own, an internal node, the genus
    ("i1", "species", 60, 4000, 4000, 120, 150, 1),
    ("i2", "genus", 50, 4000, 4000, 120, 150, 1),
    ("i3", "NC_000020.1", 71, 9000, 0, 150, 150, 1),
    ("i4", "NC_000010.1", 70, 9000, 0, 150, 150, 1),
    ("r1", "NC_000001.1", 61, 18225, 0, 150, 150, 1),
]


def run(cmd, **kw):
    print("+", " ".join(cmd), file=sys.stderr)
    return subprocess.run(cmd, check=True, **kw)


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def gz_write(path, data):
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(data)


def main():
    rng = np.random.default_rng(SEED)
    tmp = tempfile.mkdtemp(prefix="cfr_golden_quant_")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(os.path.join(OUT, "report"))

    seqs = {}
    for name, _tid, L, derived in SEQS:
        if derived is None:
            s = ACGT[rng.integers(0, 4, size=L)]
        else:
            base, div = derived
            src = seqs[base]
            s = np.concatenate([src, ACGT[rng.integers(0, 4, size=max(0, L - len(src)))]])[:L].copy()
            hit = np.nonzero(rng.random(L) < div)[0]
            s[hit] = ACGT[rng.integers(0, 4, size=len(hit))]
        seqs[name] = s
    with open(os.path.join(tmp, "ref.fa"), "w") as f:
        for name, _tid, _L, _d in SEQS:
            s = seqs[name].tobytes().decode()
            f.write(f">{name}\n" + "\n".join(s[i:i + 80] for i in range(0, len(s), 80)) + "\n")
    with open(os.path.join(tmp, "nodes.dmp"), "w") as f:
        for tid, par, rank in NODES:
            f.write(f"{tid}\t|\t{par}\t|\t{rank}\t|\n")
    with open(os.path.join(tmp, "names.dmp"), "w") as f:
        for tid, _par, _rank in NODES:
            f.write(f"{tid}\t|\t{NAMES[tid]}\t|\t\t|\tscientific name\t|\n")
    with open(os.path.join(tmp, "seqid.map"), "w") as f:
        for name, tid, _L, _d in SEQS:
            f.write(f"{name}\t{tid}\n")
    run([os.path.join(REF, "centrifuger-build"), "-t", "2", "-r", os.path.join(tmp, "ref.fa"), "--taxonomy-tree", os.path.join(tmp, "nodes.dmp"),
         "--name-table", os.path.join(tmp, "names.dmp"), "--conversion-table", os.path.join(tmp, "seqid.map"), "--ftabchars", "6",
         "-o", os.path.join(tmp, "q8")])
    for k in (1, 2, 3, 4):
        shutil.copy(os.path.join(tmp, f"q8.{k}.cfr"), OUT)

    # reads: fragments of the sequences, 1 % substitutions, a tenth of them random
    names = [s[0] for s in SEQS]

    def fragment(L):
        s = seqs[names[int(rng.integers(0, len(names)))]]
        p = int(rng.integers(0, len(s) - L))
        r = s[p:p + L].copy()
        hit = np.nonzero(rng.random(L) < 0.01)[0]
        r[hit] = ACGT[rng.integers(0, 4, size=len(hit))]
        return r

    def fastq(reads, prefix):
        return "".join(f"@{prefix}{i}\n{r.tobytes().decode()}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()

    se = []
    for i in range(3000):
        L = int(rng.integers(60, 151))
        se.append(ACGT[rng.integers(0, 4, size=L)] if i % 10 == 9 else (fragment(L) if rng.random() < 0.5 else COMP[fragment(L)][::-1]))
    p1, p2 = [], []
    for i in range(2000):
        if i % 10 == 9:
            p1.append(ACGT[rng.integers(0, 4, size=100)]); p2.append(ACGT[rng.integers(0, 4, size=100)])
            continue
        f = fragment(int(rng.integers(220, 400)))
        p1.append(f[:100].copy()); p2.append(COMP[f[-100:]][::-1].copy())
    for fname, data in (("reads_se.fq", fastq(se, "s")), ("reads_1.fq", fastq(p1, "p")), ("reads_2.fq", fastq(p2, "p"))):
        open(os.path.join(tmp, fname), "wb").write(data)
        gz_write(os.path.join(OUT, fname + ".gz"), data)

    cf = os.path.join(REF, "centrifuger")
    runs = {"se_k1": ["-u", "reads_se.fq", "-k", "1"], "pe_k5": ["-1", "reads_1.fq", "-2", "reads_2.fq", "-k", "5"]}
    tsvs = {}
    for key, args in runs.items():
        full = [a if a.startswith("-") or a.isdigit() else os.path.join(tmp, a) for a in args]
        p = os.path.join(tmp, key + ".tsv")
        with open(p, "wb") as fo:
            run([cf, "-x", os.path.join(tmp, "q8"), "-t", "1"] + full, stdout=fo)
        gz_write(os.path.join(OUT, key + ".tsv.gz"), open(p, "rb").read())
        tsvs[key] = p
    edge = HEADER + "".join("\t".join(str(x) for x in row) + "\n" for row in EDGE_ROWS)
    for key, text in (("edge", edge), ("header_only", HEADER)):
        p = os.path.join(OUT, key + ".tsv")
        open(p, "w").write(text)
        tsvs[key] = p

    quant = os.path.join(tmp, "centrifuger-quant")
    run(["g++", "-O3", "-msse4.2", "-w", f"-I{REF_SRC}", "-o", quant, os.path.join(REF_SRC, "CentrifugerQuant.cpp"), "-lpthread", "-lz"])
    reports = {}
    for key, p in tsvs.items():
        for tag, extra in (("n", []), ("f", FILTER)):
            for fmt in range(4):
                name = f"{key}.{tag}{fmt}.txt"
                with open(os.path.join(OUT, "report", name), "wb") as fo:
                    run([quant, "-x", os.path.join(tmp, "q8"), "-c", p, "--output-format", str(fmt)] + extra, stdout=fo)
                reports[name] = {"tsv": key, "format": fmt, "args": extra}
    manifest = {"seed": SEED, "index": "q8", "runs": runs, "filter": FILTER, "reports": reports,
                "md5": {os.path.relpath(os.path.join(d, f), OUT): md5(os.path.join(d, f)) for d, _s, fs in os.walk(OUT) for f in fs}}
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    shutil.rmtree(tmp)
    print("wrote", OUT, file=sys.stderr)


if __name__ == "__main__":
    main()
