#!/usr/bin/env python3
"""Regenerate tests/golden/merge/* and tests/golden/merge_long/*: read pairs for `--merge-readpair`, what the REAL reference prints for them, and the merged
reads themselves.  Dev container only:  make -C oracle ref && python tests/golden/make_golden_merge.py

  pairs_1.fq.gz / pairs_2.fq.gz    ~1400 pairs over the genomes of the f6 index (make_golden.py), qualities random in 33..73
  pairs_1.fa.gz / pairs_2.fa.gz    the first 500 of them without qualities
  tsv/*.tsv.gz                     `centrifuger --merge-readpair` of the reference on them (manifest.json: the arguments)
  un_*.gz / cl_*.gz                its --un / --cl dumps for the FASTA set
  merged_fq.tsv.gz / merged_fa.tsv.gz   per pair: kind, overlapSize, offset, why, merged read, merged qualities - written by a
                                   throw-away driver (text below, compiled into a temporary directory) around the reference's own
                                   ReadPairMerger.hpp.  why: for kind 0, 'T' = exactly one offset passed the plain-overlap test and the
                                   tandem check rejected it, 'M' = more than one offset passed it, '-' = anything else.

tests/golden/merge_long (its own seed and generator; tests/golden/merge comes out byte for byte as before): about 400 pairs with mates
of up to 1100 bases, the same files (the FASTA set holds every pair), qualities from five levels.  manifest.json "classes":
  L1  both mates 151..512, overlaps and read-throughs with K spread over 1..512
  L2  every len1 of WORD_EDGES with four len2 of the list
  L3  one mate at most 512 and the other 513..1100, both orders; both above 512
  L4  pairs exactly on the similarity threshold T(L) (merge_fixtures.threshold: Python floats) and partners with one substitution
      more, plain and read-through pass, substitutions spread over every word of the overlap or packed into its end; "l4": what each
      must do, asserted here on the reference's dump
  L5  true offsets and overlaps at multiples of 64 and next to them; "l5_two_offsets": pairs where two offsets at least 64 apart pass
  L6  N runs, lower case and quality ties inside long overlaps
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from centrifuger_amd import synth  # noqa: E402
import merge_fixtures as mf  # noqa: E402

OUT = os.path.join(HERE, "merge")
REF = os.path.join(ROOT, "oracle", "_ref")
REF_SRC = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
GENOME_SEED = 20260928          # make_golden.py's: the genomes of the f6 index
SEED = 20261017
READ_LEN = 150
OUT_LONG = os.path.join(HERE, "merge_long")
SEED_LONG = 20261019
WORD_EDGES = (63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 447, 448, 449, 511, 512, 513, 514)
L4_LENGTHS = (32, 49, 50, 51, 64, 99, 100, 101, 127, 128, 129, 192, 256, 320, 384, 448, 511, 512)
L5_OFFSETS = (0, 1, 63, 64, 65, 128, 191, 192, 448)
L5_OVERLAPS = tuple(k + d for k in (64, 128, 192, 256, 320, 384, 448, 512) for d in (-1, 0, 1))
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


def make_pairs_long(rng, g):
    """-> pairs, quals, classes {name: [pair numbers]}, l4 [what every threshold pair must do], two [pairs with two passing offsets]"""
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
            r[i] = ACGT[(int(np.nonzero(ACGT == r[i])[0][0]) + int(rng.integers(1, 4))) & 3]
        return r

    pairs, classes, l4, two, ties = [], {c: [] for c in ("L1", "L2", "L3", "L4", "L5", "L6")}, [], [], []

    def add(c, r1, r2):
        classes[c].append(len(pairs))
        pairs.append((np.ascontiguousarray(r1, dtype=np.uint8), np.ascontiguousarray(r2, dtype=np.uint8)))
        return len(pairs) - 1

    def overlap(c, L1, L2, K, mut=True):
        """the mates of a fragment of L1 + L2 - K bases: true offset L1 - K in the plain pass (K <= 0: the mates do not meet)"""
        f = frag(L1 + L2 - K)
        r1, r2 = f[:L1], synth.revcomp(f)[:L2]
        i = add(c, mutate(r1) if mut else r1, mutate(r2) if mut else r2)
        if K > 0 and i % 5 == 0:
            ties.append((i, False, L1 - K, min(K, L2)))
        return i

    def through(c, L1, L2, F, mut=True):
        """a fragment of F <= min(L1, L2) bases and adapters behind it: true offset L2 - F in the read-through pass"""
        f = frag(F)
        r1, r2 = np.concatenate([f, rnd(L1 - F)]), np.concatenate([synth.revcomp(f), rnd(L2 - F)])
        i = add(c, mutate(r1) if mut else r1, mutate(r2) if mut else r2)
        if i % 5 == 0:
            ties.append((i, True, L2 - F, F))
        return i

    # ---- L1: both mates 151..512, K over 1..512
    for i in range(66):
        L1, L2 = int(rng.integers(151, 513)), int(rng.integers(151, 513))
        if i < 24:
            if i % 2:
                L1 = int(rng.integers(449, 513))
            else:
                L2 = int(rng.integers(449, 513))
        K = 1 + (i // 3) * 23 + int(rng.integers(0, 23))                 # 1 .. 507 over the 22 pairs of every mode
        if i % 3 == 0:
            overlap("L1", max(L1, K), max(L2, K), K)
        elif i % 3 == 1:
            through("L1", max(L1, min(512, K + int(rng.integers(0, 40)))), max(L2, min(512, K + int(rng.integers(1, 40)))), K)
        else:
            overlap("L1", L1, L2, -int(rng.integers(0, 200)))
    # ---- L2: lengths at the word edges
    for ai, a in enumerate(WORD_EDGES):
        for t in range(4):
            b = WORD_EDGES[(ai * 3 + t * 5 + 1) % len(WORD_EDGES)]
            m = min(a, b)
            if (ai + t) % 3 == 0:
                overlap("L2", a, b, int(rng.integers(33, m + 1)))
            elif (ai + t) % 3 == 1:
                through("L2", a, b, int(rng.integers(33, m + 1)))
            else:
                overlap("L2", a, b, -int(rng.integers(0, 100)))
    # ---- L3: across and above the 512 bases of the bit planes
    for i in range(42):
        short, long_, long2 = int(rng.integers(100, 513)), int(rng.integers(513, 1101)), int(rng.integers(513, 1101))
        L1, L2 = ((short, long_), (long_, short), (long_, long2))[i % 3]
        m = min(L1, L2)
        if (i // 3) % 3 == 0:
            overlap("L3", L1, L2, int(rng.integers(33, min(m, 700) + 1)))
        elif (i // 3) % 3 == 1:
            through("L3", L1, L2, int(rng.integers(40, m + 1)))
        else:
            overlap("L3", L1, L2, -int(rng.integers(0, 300)))
    # ---- L4: on the threshold, and one substitution past it
    def l4_pairs(L, rt, packed, j, e):
        n = L - mf.threshold(L)
        for extra in (0, 1):
            r1, r2 = mf.threshold_pair(frag(j + L + e), L, rt, j, e, n + extra, packed, rnd(j + e))
            i = add("L4", r1, r2)
            l4.append({"pair": i, "L": L, "pass": "through" if rt else "plain", "packed": packed, "substitutions": n + extra,
                       "kind": 0 if extra else (2 if rt else 1), "offset": j})
    for L in L4_LENGTHS:
        jb, eb = (min(64, 512 - L), min(60, 512 - L)) if L < 512 else (64, 0)       # both mates within the planes where L allows it
        for rt in (False, True):
            l4_pairs(L, rt, False, 40, 60)             # substitutions over every word of the overlap; from L = 453 on the byte path
            l4_pairs(L, rt, True, jb, eb)              # substitutions packed into the end of the overlap
            if L >= 448:
                l4_pairs(L, rt, False, jb, eb)
        if L == 512:                                   # the planes' full length: only the read-through pass can see it (offset 0)
            l4_pairs(L, True, False, 0, 0)
            l4_pairs(L, True, True, 0, 0)
    # ---- L5: offsets and overlaps at multiples of 64
    def fit(j, K):
        return j if j + K <= 512 else max([o for o in L5_OFFSETS if o + K <= 512] or [1])
    for n, K in enumerate(L5_OVERLAPS):
        e = (0, 17, 80)[n % 3]
        j = fit(L5_OFFSETS[1 + n % 8], K)              # (an overlap at offset 0 is the read-through pass's)
        overlap("L5", j + K, K + e, K)
        j = fit(L5_OFFSETS[(n + 4) % 9], K)
        through("L5", K + e, K + j, K)
    for n, j in enumerate(L5_OFFSETS):
        overlap("L5", j + 64, 64 + (0, 17, 80)[n % 3], 64)
        through("L5", 64 + (17, 80, 100)[n % 3], 64 + j, 64)       # (a bare 64-base r1 would pass at many offsets of a 512-base mate)
    for n, (x, p, q, e) in enumerate(((64, 1, 0, 0), (100, 10, 0, 0), (128, 64, 1, 0), (150, 30, 70, 0), (192, 63, 64, 0), (200, 5, 100, 2),
                                      (65, 127, 62, 0), (127, 2, 129, 3), (90, 1, 10, 0), (160, 33, 64, 0), (250, 7, 5, 0))):
        X = frag(x)
        twice = np.concatenate([rnd(p), X, rnd(q), X])
        if n < 8:                                      # r1 holds the overlap twice: two offsets pass the plain test
            i = add("L5", twice, synth.revcomp(np.concatenate([X, rnd(e)])))      # (e bases past it: a few more mismatches at the first copy)
            two.append({"pair": i, "offset": p + x + q, "why": "M"})
        else:                                          # rc(r2) holds it twice: two offsets pass the read-through test, none the plain one
            i = add("L5", X, synth.revcomp(twice))
            two.append({"pair": i, "offset": p + x + q, "why": "-"})
    # ---- L6: N runs and lower case inside long overlaps; every one of them gets quality ties
    for i in range(24):
        L1, L2 = int(rng.integers(250, 513)), int(rng.integers(250, 513))
        K = int(rng.integers(200, min(L1, L2) + 1))   # 30 mismatches allowed: the two runs below (each a mismatch per base) stay under that
        if i % 2:
            k = through("L6", L1, L2, K)
            lo1, lo2 = 0, 0                            # where the overlap starts in r1 / in r2
        else:
            k = overlap("L6", L1, L2, K)
            lo1, lo2 = L1 - K, L2 - K
        for r, lo in zip(pairs[k], (lo1, lo2)):
            n = int(rng.integers(1, 12))
            a = lo + int(rng.integers(0, K - n))
            if rng.random() < 0.5:
                r[a:a + n] = ord("N")
            else:
                r[a:a + n] = np.frombuffer(bytes(r[a:a + n]).lower(), dtype=np.uint8)
        if not ties or ties[-1][0] != k:
            ties.append((k, True, L2 - K, K) if i % 2 else (k, False, L1 - K, K))

    levels = np.array([35, 45, 55, 65, 73], dtype=np.uint8)
    quals = [(levels[rng.integers(0, 5, size=len(a))], levels[rng.integers(0, 5, size=len(b))]) for a, b in pairs]
    for n, (i, rt, off, K) in enumerate(ties):         # exact ties of both rules, and one either side of them, on the true overlap
        q1, rcq2 = quals[i][0], quals[i][1][::-1]      # (rcq2 is a view: quals[i][1] changes)
        d = np.arange(K) % 3 - 1 + (14 if n % 2 else 0)
        if rt:
            rcq2[off:off + K] = q1[:K] + d             # read through: the mate wins iff rcq2[i + offset] > q1[i]
        else:
            rcq2[:K] = q1[off:off + K] + d             # overlap: r1 wins iff q1[i] >= rcq2[i - offset] - 14
    return pairs, quals, classes, l4, two


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


def emit(out, drv, pairs, quals, n_fa, manifest, cases, check, limit):
    """one set: the pairs, the dump of the reference's ReadPairMerger on them (check(name, fa, rows) asserts on it), its TSVs"""
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(os.path.join(out, "tsv"))
    tmp = tempfile.mkdtemp(prefix="cfr_golden_merge_")
    write_fastx(os.path.join(out, "pairs_1.fq.gz"), [p[0] for p in pairs], [q[0] for q in quals], b"/1")
    write_fastx(os.path.join(out, "pairs_2.fq.gz"), [p[1] for p in pairs], [q[1] for q in quals], b"/2")
    write_fastx(os.path.join(out, "pairs_1.fa.gz"), [p[0] for p in pairs[:n_fa]], None, b"/1")
    write_fastx(os.path.join(out, "pairs_2.fa.gz"), [p[1] for p in pairs[:n_fa]], None, b"/2")

    # ---- the merged reads, by the reference's own ReadPairMerger.hpp
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
        check(name, fa, rows)
        manifest["counts"][name] = {"kinds": cnt, "tandem_or_multiple": amb}
        gz_write(os.path.join(out, name + ".tsv.gz"), dump)

    # ---- the reference's TSVs
    idx = os.path.join(tmp, "f6")
    for k in (1, 2, 4):
        shutil.copy(os.path.join(HERE, f"f6.{k}.cfr"), f"{idx}.{k}.cfr")
    for nm in ("pairs_1.fq", "pairs_2.fq", "pairs_1.fa", "pairs_2.fa"):
        with gzip.open(os.path.join(out, nm + ".gz"), "rb") as fi, open(os.path.join(tmp, nm), "wb") as fo:
            shutil.copyfileobj(fi, fo)
    cf = os.path.join(REF, "centrifuger")
    for cname, args in cases.items():
        res = run([cf, "-x", idx, "-t", "1", "--merge-readpair"] + args, stdout=subprocess.PIPE, cwd=tmp).stdout
        gz_write(os.path.join(out, "tsv", cname + ".tsv.gz"), res)
        manifest["cases"][cname] = {"args": args, "md5": hashlib.md5(res).hexdigest()}
    if any("--un" in a for a in cases.values()):
        dumps = sorted(f for f in os.listdir(tmp) if f.startswith(("un", "cl")))
        assert dumps, "the reference wrote no --un / --cl files"
        manifest["dumps"] = {}
        for f in dumps:
            raw = open(os.path.join(tmp, f), "rb").read()
            if f.endswith(".gz"):
                raw = gzip.decompress(raw)
            name = f[:-3] if f.endswith(".gz") else f
            gz_write(os.path.join(out, name + ".gz"), raw)
            manifest["dumps"][name] = hashlib.md5(raw).hexdigest()
    with open(os.path.join(out, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    shutil.rmtree(tmp)
    total = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(out) for f in fs)
    print(os.path.relpath(out, ROOT) + ":", total, "bytes", file=sys.stderr)
    assert total < limit


def check_long(rows, classes, l4, two):
    """what the reference's dump must show for the set to be worth committing (rows: kind, overlapSize, offset, why, ...)"""
    for c in ("L1", "L2", "L3"):
        kinds = [int(rows[i][0]) for i in classes[c]]
        assert all(kinds.count(k) >= 10 for k in (0, 1, 2)), (c, [kinds.count(k) for k in (0, 1, 2)])
    for t in l4:
        r = rows[t["pair"]]
        got = (int(r[0]), int(r[1]), int(r[2]), r[3])
        want = (t["kind"], t["L"], t["offset"], b"-") if t["kind"] else (0, -1, -1, b"-")
        assert got == want, (t, got)
    for t in two:
        r = rows[t["pair"]]
        assert (int(r[0]), int(r[1]), int(r[2]), r[3]) == (0, -1, t["offset"], t["why"].encode()), (t, r[:4])
    assert sum(1 for i in classes["L5"] if rows[i][3] == b"M") >= 5
    assert all(int(rows[i][0]) for i in classes["L6"])          # the N runs and lower-case stretches stay below the threshold


def main():
    assert os.path.exists(os.path.join(REF, "centrifuger")), "make -C oracle ref first"
    g = synth.make_genomes(n_species=5, n_strains=3, genome_len=20000, seed=GENOME_SEED)
    tmp = tempfile.mkdtemp(prefix="cfr_golden_merge_drv_")
    drv = os.path.join(tmp, "merge_dump")
    with open(drv + ".cpp", "w") as f:
        f.write(DRIVER)
    run(["g++", "-O2", "-w", "-I", REF_SRC, "-o", drv, drv + ".cpp"])
    fq = ["-1", "pairs_1.fq", "-2", "pairs_2.fq"]
    fa = ["-1", "pairs_1.fa", "-2", "pairs_2.fa"]

    # ---- tests/golden/merge
    pairs, quals = make_pairs(np.random.default_rng(SEED), g)
    n_fa = 500

    def check(name, fa_set, rows):
        kinds = [int(r[0]) for r in rows]
        need = 30 if fa_set else 100
        assert all(kinds.count(k) >= need for k in (0, 1, 2)), (name, kinds)
        if not fa_set:
            assert sum(1 for r in rows if r[3] in (b"T", b"M")) >= 20
            assert rows[12 + 14][:3] == [b"2", b"0", b"0"], rows[12 + 14]
    emit(OUT, drv, pairs, quals, n_fa, {"seed": SEED, "n_fq": len(pairs), "n_fa": n_fa, "cases": {}, "counts": {}},
         {"fq_k1": fq, "fq_k5": fq + ["-k", "5"], "fq_nodust": fq + ["--no-dust"], "fa_k1": fa, "fa_dump": fa + ["--un", "un", "--cl", "cl"]},
         check, 1000000)

    # ---- tests/golden/merge_long
    pairs, quals, classes, l4, two = make_pairs_long(np.random.default_rng(SEED_LONG), g)
    print("merge_long:", len(pairs), "pairs,", sum(len(a) + len(b) for a, b in pairs), "bases;", {c: len(v) for c, v in classes.items()}, file=sys.stderr)
    assert sum(1 for a, b in (pairs[i] for i in classes["L1"]) if max(len(a), len(b)) >= 449) >= 20
    emit(OUT_LONG, drv, pairs, quals, len(pairs),
         {"seed": SEED_LONG, "n_fq": len(pairs), "n_fa": len(pairs), "cases": {}, "counts": {}, "classes": classes, "l4": l4, "l5_two_offsets": two},
         {"fq_k1": fq, "fq_nodust": fq + ["--no-dust"], "fa_k1": fa}, lambda name, fa_set, rows: check_long(rows, classes, l4, two), 600000)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
