#!/usr/bin/env python3
"""Regenerate tests/golden/merge/*: read pairs for `--merge-readpair`, what the REAL reference prints for them, and the merged
reads themselves.  Dev container only:  make -C oracle ref && python tests/golden/make_golden_merge.py

  pairs_1.fq.gz / pairs_2.fq.gz    ~1400 pairs over the genomes of the f6 index (make_golden.py), qualities random in 33..73
  pairs_1.fa.gz / pairs_2.fa.gz    the first 500 of them without qualities
  tsv/*.tsv.gz                     `centrifuger --merge-readpair` of the reference on them (manifest.json: the arguments)
  un_*.gz / cl_*.gz                its --un / --cl dumps for the FASTA set
  merged_fq.tsv.gz / merged_fa.tsv.gz   per pair: kind, overlapSize, offset, why, merged read, merged qualities - written by a
                                   throw-away driver (text below, compiled into a temporary directory) around the reference's own
                                   ReadPairMerger.hpp.  why: for kind 0, 'T' = exactly one offset passed the plain-overlap test and the
                                   tandem check rejected it, 'M' = more than one offset passed it, '-' = anything else.
Committed: data only."""
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
sys.path.insert(0, ROOT)
from centrifuger_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "merge")
REF = os.path.join(ROOT, "oracle", "_ref")
REF_SRC = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
GENOME_SEED = 20260928          # make_golden.py's: the genomes of the f6 index
SEED = 20261017
READ_LEN = 150
ACGT = synth.ACGT

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define private public
#include "ReadPairMerger.hpp"
#undef private
// stdin: r1 TAB q1 TAB r2 TAB q2 per line (q1 / q2 empty and argv[1] = "fa": no qualities)
int main(int argc, char **argv) {
  const bool fa = argc > 1 && !strcmp(argv[1], "fa");
  ReadPairMerger merger;
  std::string line;
  int c;
  for (;;) {
    line.clear();
    while ((c = getchar()) != EOF && c != '\n') line.push_back((char)c);
    if (c == EOF && line.empty()) break;
    std::vector<std::string> f(1);
    for (char ch : line) { if (ch == '\t') f.emplace_back(); else f.back().push_back(ch); }
    f.resize(4);
    char *r1 = &f[0][0], *q1 = fa ? NULL : &f[1][0], *r2 = &f[2][0], *q2 = fa ? NULL : &f[3][0];
    char *rm = NULL, *qm = NULL;
    int overlapSize = 0, offset = 0, best = 0;
    const int kind = merger.Merge(r1, q1, r2, q2, &rm, &qm, overlapSize, offset, best);
    char why = '-';
    if (kind == 0) {
      const int len1 = (int)strlen(r1), len2 = (int)strlen(r2);
      std::string rc(r2);
      merger.ReverseBuffer(&rc[0], len2);
      merger.ComplementBuffer(&rc[0], len2);
      int mo = (len1 + len2) / 10;
      if (mo > 31) mo = 31;
      int off = -1, b = 0;
      const int plain = merger.IsMateOverlap(r1, len1, &rc[0], len2, mo, off, b, false);
      if (plain >= 0) why = 'T';
      else if (off >= 0) why = 'M';
    }
    printf("%d\t%d\t%d\t%c\t%s\t%s\n", kind, overlapSize, offset, why, rm ? rm : "", qm ? qm : "");
    free(rm); free(qm);
  }
  return 0;
}
"""


def run(cmd, **kw):
    print("+", " ".join(cmd), file=sys.stderr)
    return subprocess.run(cmd, check=True, **kw)


def make_pairs(rng, g):
    cat = np.concatenate(g.seqs)
    starts = np.zeros(len(g.seqs) + 1, dtype=np.int64)
    starts[1:] = np.cumsum([len(s) for s in g.seqs])

    def rnd(L):
        return ACGT[rng.integers(0, 4, size=L)]

    def frag(L):
        s = int(rng.integers(0, len(g.seqs)))
        p = int(rng.integers(0, len(g.seqs[s]) - L))
        f = cat[starts[s] + p:starts[s] + p + L].copy()
        return synth.revcomp(f) if rng.random() < 0.5 else f

    def mutate(r, rate=0.01):
        r = r.copy()
        for i in np.nonzero(rng.random(len(r)) < rate)[0]:
            r[i] = ACGT[(int(np.nonzero(ACGT == r[i])[0][0]) + int(rng.integers(1, 4))) & 3] if r[i] in ACGT else r[i]
        return r

    def mates(f, L1=READ_LEN, L2=READ_LEN, mut=True):
        """the two reads of fragment f; a fragment shorter than the read is followed by a random tail (adapter read-through)"""
        a = np.concatenate([f, rnd(max(0, L1 - len(f)))])[:L1]
        b = np.concatenate([synth.revcomp(f), rnd(max(0, L2 - len(f)))])[:L2]
        return (mutate(a), mutate(b)) if mut else (a, b)

    pairs = []
    for k in range(1400):
        cls = k % 14
        if cls < 8:                                     # plain library: fragments 30..400
            r1, r2 = mates(frag(int(rng.integers(30, 401))))
        elif cls == 8:                                  # N runs and lower-case stretches inside the overlap
            r1, r2 = mates(frag(int(rng.integers(60, 280))))
            for r in (r1, r2):
                a = int(rng.integers(0, READ_LEN - 20)); n = int(rng.integers(1, 20))
                if rng.random() < 0.5:
                    r[a:a + n] = ord("N")
                else:
                    r[a:a + n] = np.frombuffer(bytes(r[a:a + n]).lower(), dtype=np.uint8)
        elif cls in (9, 10):                            # the overlap is a 2-bp / 3-bp tandem repeat of about minOverlap (30) bases
            ov = int(rng.integers(28, 66))
            f = frag(2 * READ_LEN - ov)
            unit = rnd(2 if cls == 9 else 3)
            while len(set(unit.tolist())) == 1:
                unit = rnd(len(unit))
            lo = READ_LEN - ov - int(rng.integers(0, 12))
            hi = READ_LEN + int(rng.integers(0, 12))
            f[lo:hi] = np.resize(unit, hi - lo)
            r1, r2 = mates(f, mut=bool(k & 16))
        elif cls == 11:                                 # r2 inside r1
            f = frag(READ_LEN)
            L2 = int(rng.integers(35, 110)); a = int(rng.integers(0, READ_LEN - L2 + 1))
            r1 = mutate(f); r2 = mutate(synth.revcomp(f[a:a + L2]))
        elif cls == 12:                                 # mates of 0, 1, 9, 10, 11 bases (minOverlap = (len1 + len2) / 10 changes at 10)
            lens = (0, 1, 9, 10, 11)
            j = k // 14
            L1, L2 = lens[j % 5], lens[(j // 5) % 5]
            f = frag(max(L1, L2, 1) + int(rng.integers(0, 4)))
            r1, r2 = mates(f, L1, L2, mut=False)
            if (j // 25) % 2:
                r2 = rnd(L2)
        else:                                           # short fragments with long and short reads mixed
            L1, L2 = int(rng.integers(12, 151)), int(rng.integers(12, 151))
            r1, r2 = mates(frag(int(rng.integers(12, 200))), L1, L2)
        pairs.append((np.ascontiguousarray(r1, dtype=np.uint8), np.ascontiguousarray(r2, dtype=np.uint8)))
    pairs[12 + 14] = (np.zeros(0, dtype=np.uint8), np.frombuffer(b"A", dtype=np.uint8))      # r1 = "", len2 = 1: merges to the empty read (kind 2)
    quals = [(rng.integers(33, 74, size=len(a)).astype(np.uint8), rng.integers(33, 74, size=len(b)).astype(np.uint8)) for a, b in pairs]
    for k in range(0, len(pairs), 7):                   # ties: the mate's quality exactly 14 above, and equal
        a, b = quals[k]
        n = min(len(a), len(b))
        if n:
            if k % 2:
                b[::-1][:n] = np.minimum(a[:n] + 14, 126)
            else:
                b[::-1][:n] = a[:n]
    return pairs, quals


def write_fastx(path, recs, quals, suffix):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        for i, r in enumerate(recs):
            if quals is None:
                f.write(b">p%d%s\n%s\n" % (i, suffix, bytes(r)))
            else:
                f.write(b"@p%d%s\n%s\n+\n%s\n" % (i, suffix, bytes(r), bytes(quals[i])))


def gz_write(path, data):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)


def main():
    assert os.path.exists(os.path.join(REF, "centrifuger")), "make -C oracle ref first"
    rng = np.random.default_rng(SEED)
    g = synth.make_genomes(n_species=5, n_strains=3, genome_len=20000, seed=GENOME_SEED)
    pairs, quals = make_pairs(rng, g)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(os.path.join(OUT, "tsv"))
    tmp = tempfile.mkdtemp(prefix="cfr_golden_merge_")
    n_fa = 500
    write_fastx(os.path.join(OUT, "pairs_1.fq.gz"), [p[0] for p in pairs], [q[0] for q in quals], b"/1")
    write_fastx(os.path.join(OUT, "pairs_2.fq.gz"), [p[1] for p in pairs], [q[1] for q in quals], b"/2")
    write_fastx(os.path.join(OUT, "pairs_1.fa.gz"), [p[0] for p in pairs[:n_fa]], None, b"/1")
    write_fastx(os.path.join(OUT, "pairs_2.fa.gz"), [p[1] for p in pairs[:n_fa]], None, b"/2")

    # ---- the merged reads, by the reference's own ReadPairMerger.hpp
    drv = os.path.join(tmp, "merge_dump")
    with open(drv + ".cpp", "w") as f:
        f.write(DRIVER)
    run(["g++", "-O2", "-w", "-I", REF_SRC, "-o", drv, drv + ".cpp"])
    manifest = {"seed": SEED, "n_fq": len(pairs), "n_fa": n_fa, "cases": {}, "counts": {}}
    for name, n, fa in (("merged_fq", len(pairs), False), ("merged_fa", n_fa, True)):
        text = b"".join(b"\t".join((bytes(pairs[i][0]), b"" if fa else bytes(quals[i][0]), bytes(pairs[i][1]), b"" if fa else bytes(quals[i][1]))) + b"\n"
                        for i in range(n))
        dump = run([drv, "fa" if fa else "fq"], input=text, stdout=subprocess.PIPE).stdout
        rows = [ln.split(b"\t") for ln in dump.split(b"\n")[:-1]]
        assert len(rows) == n
        kinds = [int(r[0]) for r in rows]
        cnt = {k: kinds.count(k) for k in (0, 1, 2)}
        amb = sum(1 for r in rows if r[3] in (b"T", b"M"))
        print(name, "kinds", cnt, "rejected by the tandem check / more than one offset:", amb, file=sys.stderr)
        need = 30 if fa else 100
        assert all(cnt[k] >= need for k in (0, 1, 2)), (name, cnt)
        if not fa:
            assert amb >= 20, amb
            assert rows[12 + 14][:3] == [b"2", b"0", b"0"], rows[12 + 14]
        manifest["counts"][name] = {"kinds": cnt, "tandem_or_multiple": amb}
        gz_write(os.path.join(OUT, name + ".tsv.gz"), dump)

    # ---- the reference's TSVs
    idx = os.path.join(tmp, "f6")
    for k in (1, 2, 4):
        shutil.copy(os.path.join(HERE, f"f6.{k}.cfr"), f"{idx}.{k}.cfr")
    for nm in ("pairs_1.fq", "pairs_2.fq", "pairs_1.fa", "pairs_2.fa"):
        with gzip.open(os.path.join(OUT, nm + ".gz"), "rb") as fi, open(os.path.join(tmp, nm), "wb") as fo:
            shutil.copyfileobj(fi, fo)
    cases = {
        "fq_k1": ["-1", "pairs_1.fq", "-2", "pairs_2.fq"],
        "fq_k5": ["-1", "pairs_1.fq", "-2", "pairs_2.fq", "-k", "5"],
        "fq_nodust": ["-1", "pairs_1.fq", "-2", "pairs_2.fq", "--no-dust"],
        "fa_k1": ["-1", "pairs_1.fa", "-2", "pairs_2.fa"],
        "fa_dump": ["-1", "pairs_1.fa", "-2", "pairs_2.fa", "--un", "un", "--cl", "cl"],
    }
    cf = os.path.join(REF, "centrifuger")
    for cname, args in cases.items():
        out = run([cf, "-x", idx, "-t", "1", "--merge-readpair"] + args, stdout=subprocess.PIPE, cwd=tmp).stdout
        gz_write(os.path.join(OUT, "tsv", cname + ".tsv.gz"), out)
        manifest["cases"][cname] = {"args": args, "md5": hashlib.md5(out).hexdigest()}
    dumps = sorted(f for f in os.listdir(tmp) if f.startswith(("un", "cl")))
    assert dumps, "the reference wrote no --un / --cl files"
    manifest["dumps"] = {}
    for f in dumps:
        raw = open(os.path.join(tmp, f), "rb").read()
        if f.endswith(".gz"):
            raw = gzip.decompress(raw)
        name = f[:-3] if f.endswith(".gz") else f
        gz_write(os.path.join(OUT, name + ".gz"), raw)
        manifest["dumps"][name] = hashlib.md5(raw).hexdigest()
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    shutil.rmtree(tmp)
    total = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(OUT) for f in fs)
    print("tests/golden/merge:", total, "bytes", file=sys.stderr)
    assert total < 1000000


if __name__ == "__main__":
    main()
