#!/usr/bin/env python3
"""Regenerate tests/golden/quant_wide/*: a taxonomy wide enough that the E-step of the quantifier runs more than one block of nodes
(811 nodes; tests/golden/quant has 14), synthetic classification rows over it, and what the REAL reference quantifier prints for
them.  Dev container only:  make -C oracle ref && python tests/golden/make_golden_quant_wide.py      (tests/golden/quant is not touched)

  qw.2.cfr, qw.3.cfr     written by the reference's centrifuger-build (oracle/_ref): 1 root / 100..109 genus / 1000..1199 species (20 per
                         genus) / 10000..10599 strain (3 per species), one random sequence of 300..900 bases per strain.  The
                         quantifiers of both projects open nothing else, so .1.cfr and .4.cfr are not kept, and there are no reads.
  wide.tsv.gz            20000 synthetic reads, lists of 1..6 targets drawn from a skewed abundance (mostly within one species or genus),
                         hit lengths that give the weights 4^-0 .. 4^-11, 300 reads whose target is a species or a genus, 60 reads with
                         tax ids the tree does not hold (one of them twice in a list), 400 reads that only the filter removes
                         (score 299 / hitLength 39)
  report/wide.<f|n><format>.txt   the reference centrifuger-quant's stdout: format 0..3, n = no filter, f = --min-score 300 --min-length 40
  manifest.json          arguments and md5 of every file
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
OUT = os.path.join(HERE, "quant_wide")
REF = os.path.join(ROOT, "oracle", "_ref")
REF_SRC = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
SEED = 20261118
N_GENUS, SPECIES_PER_GENUS, STRAINS_PER_SPECIES, N_READS = 10, 20, 3, 20000
FILTER = ["--min-score", "300", "--min-length", "40"]
HEADER = "readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\n"
FOREIGN = (99999, 88888)


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
    tmp = tempfile.mkdtemp(prefix="cfr_golden_quant_wide_")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(os.path.join(OUT, "report"))

    genera = [100 + g for g in range(N_GENUS)]
    species = [1000 + s for s in range(N_GENUS * SPECIES_PER_GENUS)]
    strains = [10000 + t for t in range(len(species) * STRAINS_PER_SPECIES)]
    nodes = [(1, 1, "no rank")] + [(g, 1, "genus") for g in genera]
    nodes += [(s, genera[i // SPECIES_PER_GENUS], "species") for i, s in enumerate(species)]
    nodes += [(t, species[i // STRAINS_PER_SPECIES], "strain") for i, t in enumerate(strains)]
    assert len(nodes) == 811
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(os.path.join(tmp, "ref.fa"), "w") as fa, open(os.path.join(tmp, "seqid.map"), "w") as mp:
        for i, t in enumerate(strains):
            name = f"NC_{2 * i + 1:06d}.1"            # odd numbers: no two accessions are consecutive, every sequence is a genome
            s = acgt[rng.integers(0, 4, size=int(rng.integers(300, 901)))].tobytes().decode()
            fa.write(f">{name}\n" + "\n".join(s[k:k + 80] for k in range(0, len(s), 80)) + "\n")
            mp.write(f"{name}\t{t}\n")
    with open(os.path.join(tmp, "nodes.dmp"), "w") as f:
        for tid, par, rank in nodes:
            f.write(f"{tid}\t|\t{par}\t|\t{rank}\t|\n")
    with open(os.path.join(tmp, "names.dmp"), "w") as f:
        for tid, _par, _rank in nodes:
            f.write(f"{tid}\t|\tname{tid}\t|\t\t|\tscientific name\t|\n")
    run([os.path.join(REF, "centrifuger-build"), "-t", "2", "-r", os.path.join(tmp, "ref.fa"), "--taxonomy-tree", os.path.join(tmp, "nodes.dmp"),
         "--name-table", os.path.join(tmp, "names.dmp"), "--conversion-table", os.path.join(tmp, "seqid.map"), "--ftabchars", "6",
         "-o", os.path.join(tmp, "qw")])
    for k in (2, 3):
        shutil.copy(os.path.join(tmp, f"qw.{k}.cfr"), OUT)

    # rows.  Strain abundances fall off like 1 / rank over a shuffled order, so the EM has something to move.
    order = rng.permutation(len(strains))
    p = np.empty(len(strains))
    p[order] = 1.0 / np.arange(1, len(strains) + 1)
    p /= p.sum()
    first = rng.choice(len(strains), size=N_READS, p=p)
    n_targets = rng.choice([1, 2, 3, 4, 5, 6], size=N_READS, p=[0.18, 0.27, 0.25, 0.15, 0.1, 0.05])
    hit_cut = rng.choice([0, 0, 0, 1, 2, 3, 4, 5, 7, 9, 11, 12, 13, 30], size=N_READS)    # queryLength 150: d = cut - 1, clamped to 0..11
    special = rng.permutation(N_READS)
    internal, foreign, low_score, short_hit = special[:300], special[300:360], special[360:560], special[560:760]
    kind = np.zeros(N_READS, dtype=np.int8)
    kind[internal], kind[foreign], kind[low_score], kind[short_hit] = 1, 2, 3, 4
    rows = []
    for i in range(N_READS):
        k, t0 = int(n_targets[i]), int(first[i])
        sp = t0 // STRAINS_PER_SPECIES
        targets = [strains[t0]]
        while len(targets) < k:      # the other targets: a strain of the same species, of the same genus, or any (repeats allowed)
            u = rng.random()
            if u < 0.5:
                t = sp * STRAINS_PER_SPECIES + int(rng.integers(0, STRAINS_PER_SPECIES))
            elif u < 0.85:
                g = sp // SPECIES_PER_GENUS
                t = (g * SPECIES_PER_GENUS + int(rng.integers(0, SPECIES_PER_GENUS))) * STRAINS_PER_SPECIES + int(rng.integers(0, STRAINS_PER_SPECIES))
            else:
                t = int(rng.integers(0, len(strains)))
            targets.append(strains[t])
        score, hit, length = 5000, 150 - int(hit_cut[i]), 150
        if kind[i] == 1:             # a species or a genus among the targets, sometimes alone
            node = species[sp] if i % 2 else genera[sp // SPECIES_PER_GENUS]
            targets = [node] if i % 3 == 0 else targets[:-1] + [node] if k > 1 else [node]
        elif kind[i] == 2:           # tax ids the tree does not hold; every fifth such read has one of them twice
            targets = [FOREIGN[0], FOREIGN[0]] + targets[:1] if i % 5 == 0 else [FOREIGN[i % 2]] + targets[1:]
        elif kind[i] == 3:
            score = 299
        elif kind[i] == 4:
            hit = 39
        second = score if len(targets) > 1 else (0 if i % 7 else score)
        for t in targets:
            rows.append(f"r{i}\tx\t{t}\t{score}\t{second}\t{hit}\t{length}\t{len(targets)}\n")
    text = (HEADER + "".join(rows)).encode()
    tsv = os.path.join(tmp, "wide.tsv")
    open(tsv, "wb").write(text)
    gz_write(os.path.join(OUT, "wide.tsv.gz"), text)

    quant = os.path.join(tmp, "centrifuger-quant")
    run(["g++", "-O3", "-msse4.2", "-w", f"-I{REF_SRC}", "-o", quant, os.path.join(REF_SRC, "CentrifugerQuant.cpp"), "-lpthread", "-lz"])
    reports = {}
    for tag, extra in (("n", []), ("f", FILTER)):
        for fmt in range(4):
            name = f"wide.{tag}{fmt}.txt"
            with open(os.path.join(OUT, "report", name), "wb") as fo:
                run([quant, "-x", os.path.join(tmp, "qw"), "-c", tsv, "--output-format", str(fmt)] + extra, stdout=fo)
            reports[name] = {"tsv": "wide", "format": fmt, "args": extra}
    manifest = {"seed": SEED, "index": "qw", "reads": N_READS, "rows": len(rows), "filter": FILTER, "reports": reports,
                "md5": {os.path.relpath(os.path.join(d, f), OUT): md5(os.path.join(d, f)) for d, _s, fs in os.walk(OUT) for f in fs}}
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    for d, _s, fs in os.walk(OUT):
        for f in fs:
            assert os.path.getsize(os.path.join(d, f)) < 300 * 1024, f
    shutil.rmtree(tmp)
    print("wrote", OUT, file=sys.stderr)


if __name__ == "__main__":
    main()
