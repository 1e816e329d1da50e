#!/usr/bin/env python3
"""Regenerate tests/golden/barcode/*: whitelists, barcodes, read-format cases and translation tables, and what the REAL reference's
BarcodeCorrector.hpp, ReadFormatter.hpp and BarcodeTranslator.hpp do with them.  Dev container only:
    python tests/golden/make_golden_barcode.py

  wl5.txt / wl16.txt.gz / wlmix.txt      whitelists: 3 entries of L = 5; ~2000 of L = 16 (clusters around common centres, repeated lines,
                                         one line with an N); ~300 of 14..16 bases (some entries are prefixes of others)
  <wl>.background.tsv.gz                 barcodes of the background pass (a FASTA file for the reference's ReadFiles); the cap is in
                                         manifest.json and is smaller than the number of records
  <wl>.counts.tsv.gz                     entry TAB count of every trie node with end = true after CollectBackgroundDistribution
  <wl>.barcodes.tsv.gz                   class TAB barcode TAB qualities
  <wl>.corrected.tsv.gz                  per barcode: Correct's return value and the barcode afterwards, with qualities and without
  formats.json, format_records.tsv.gz,   format strings, records (sequence, qualities, comment; fields separated by 0x1f) and per
  format_<k>.tsv.gz                      format and category: Extract into a buffer and InplaceExtractSeqAndQual, bases and qualities
  translate.txt, translate.tsv.gz        a translation table, barcodes and BarcodeTranslator::Translate of them; manifest.json holds
                                         the message and exit status for a piece that is not in the table
  cli/                                   barcode / UMI inputs for the reads of tests/golden/se.fq (400) and tests/golden/merge/pairs_*.fq.gz
                                         (1400 pairs), and what the REAL reference (oracle/_ref/centrifuger, `make -C oracle ref`) prints
                                         for them on the f6 index: cli/tsv/*.tsv.gz, the --un / --cl dumps of one run, cli/manifest.json
                                         (arguments with {G} = tests/golden, {M} = its merge/, {B} = its barcode/, {C} = barcode/cli; md5s)
The three drivers below are compiled into a temporary directory around the reference's own headers.  Committed: data only."""
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
OUT = os.path.join(HERE, "barcode")
REF_SRC = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
SEED = 20261018
SEP = "\x1f"

CORRECT_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define private public
#include "BarcodeCorrector.hpp"
#undef private
char nucToNum[26], numToNuc[26];   // (defs.h declares them extern for other headers)
static void dump(struct _trie *p, std::string &cur, FILE *fp) {
  if (p->end) fprintf(fp, "%s\t%d\n", cur.c_str(), p->count);
  for (int t = 0; t < 4; ++t)
    if (p->next[t]) { cur.push_back("ACGT"[t]); dump(p->next[t], cur, fp); cur.pop_back(); }
}
// argv: whitelist background.fa cap counts.out ; stdin: barcode TAB qual per line -> stdout
int main(int argc, char **argv) {
  BarcodeCorrector bc;
  bc.SetWhitelist(argv[1]);
  ReadFiles bg;
  bg.AddReadFile(argv[2], false);
  ReadFormatter fmt;
  bc.CollectBackgroundDistribution(bg, fmt, atoi(argv[3]));
  FILE *fp = fopen(argv[4], "w");
  std::string cur;
  dump(&bc.barcodeFreq.head, cur, fp);
  fclose(fp);
  std::string line;
  int c;
  for (;;) {
    line.clear();
    while ((c = getchar()) != EOF && c != '\n') line.push_back((char)c);
    if (c == EOF && line.empty()) break;
    size_t tab = line.find('\t');
    std::string b = line.substr(0, tab), q = line.substr(tab + 1);
    std::string b1 = b, b2 = b;
    int r1 = bc.Correct(&b1[0], &q[0]);
    int r2 = bc.Correct(&b2[0], NULL);
    printf("%d\t%s\t%d\t%s\n", r1, b1.c_str(), r2, b2.c_str());
  }
  return 0;
}
"""

FORMAT_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "ReadFormatter.hpp"
// argv[1]: format string; stdin: seq 0x1f qual 0x1f comment per line -> per record and category with segments:
// category 0x1f Extract(seq) 0x1f Extract(qual) 0x1f in-place seq 0x1f in-place qual   (hd categories: Extract(comment) only)
int main(int argc, char **argv) {
  ReadFormatter fmt;
  fmt.Init(argv[1]);
  std::string line;
  int c;
  for (;;) {
    line.clear();
    while ((c = getchar()) != EOF && c != '\n') line.push_back((char)c);
    if (c == EOF && line.empty()) break;
    std::vector<std::string> f(1);
    for (char ch : line) { if (ch == 0x1f) f.emplace_back(); else f.back().push_back(ch); }
    f.resize(3);
    for (int cat = 0; cat < FORMAT_CATEGORY_COUNT; ++cat) {
      if (fmt.GetSegmentCount(cat) == 0) continue;
      if (fmt.IsInComment(cat)) {
        std::string cm = f[2]; cm.reserve(cm.size() + 8);
        std::string e = fmt.Extract(&cm[0], cat, true, true, 0);
        printf("%d\x1f%s\x1f\x1f\x1f\n", cat, e.c_str());
        continue;
      }
      std::string s = f[0], q = f[1];
      std::string es = fmt.Extract(&s[0], cat, true, true, 0);
      std::string eq = fmt.Extract(&q[0], cat, false, true, 1);
      std::vector<char> is(s.size() + 64, 0), iq(q.size() + 64, 0);
      memcpy(is.data(), s.c_str(), s.size());
      memcpy(iq.data(), q.c_str(), q.size());
      fmt.InplaceExtractSeqAndQual(is.data(), iq.data(), cat);
      printf("%d\x1f%s\x1f%s\x1f%s\x1f%s\n", cat, es.c_str(), eq.c_str(), is.data(), iq.data());
    }
  }
  return 0;
}
"""

TRANSLATE_DRIVER = r"""
#include <stdio.h>
#include <string>
#include "BarcodeTranslator.hpp"
int main(int argc, char **argv) {
  BarcodeTranslator t;
  t.SetTranslateTable(argv[1]);
  std::string line;
  int c;
  for (;;) {
    line.clear();
    while ((c = getchar()) != EOF && c != '\n') line.push_back((char)c);
    if (c == EOF && line.empty()) break;
    printf("%s\n", t.Translate(&line[0], line.size()).c_str());
  }
  return 0;
}
"""

GOOD_FORMATS = [
    "r1:0:-1", "bc:0:15", "um:16:-1", "bc:-10:-1", "bc:0:15,um:16:-1", "r1:26:-1,bc:0:15,um:16:25", "bc:0:200", "bc:0:7,bc:12:19",
    "bc:16:25,bc:0:9", "bc:0:15:-", "bc:0:7:+,bc:12:19:-", "um:4:11:-;r1:0:-1:-", "bc:hd:1:0:-1", "bc:hd:2:0:15", "bc:hd:CB:5:-1",
    "um:hd:UB:5:12,bc:hd:0:0:3", "bc:hd:7:0:-1", "bc:hd:XY:0:-1", "r2:3:-4", "bc:0:15:-,um:16:-1", "r1:0:-1:+", "bc:2:2", "bc:hd:2:5:-1:-",
]
BAD_FORMATS = ["bc", "xx:0:15", "bc:0", "bc:0:15:+:1", "bc-0:15", "bc:0:15,um", "bc:hd:2", "r3:0:-1"]


def run(cmd, **kw):
    print("+", " ".join(cmd[:6]), file=sys.stderr)
    return subprocess.run(cmd, check=True, **kw)


def gz_write(path, data):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)


def rnd(rng, L):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=L))


def sub(rng, s, p, avoid=None):
    c = "ACGT"[int(rng.integers(0, 4))]
    while c == s[p] or c == avoid:
        c = "ACGT"[int(rng.integers(0, 4))]
    return s[:p] + c + s[p + 1:]


def make_whitelist(rng, name):
    """-> (lines of the file, entries, centres: (centre, [(pos, entry), ...]))"""
    if name == "wl5":
        return ["ACGTA", "ACGTC", "TTGCA"], ["ACGTA", "ACGTC", "TTGCA"], [("ACGTG", [(4, "ACGTA"), (4, "ACGTC")])]
    entries, centres = [], []
    lens = (16,) if name == "wl16" else (14, 15, 16)
    n_plain, n_centres = (1200, 300) if name == "wl16" else (200, 30)
    for _ in range(n_plain):
        entries.append(rnd(rng, int(rng.choice(lens))))
    for k in range(n_centres):
        c = rnd(rng, int(rng.choice(lens)))
        cand = []
        while len(cand) < 2 + (k % 3 == 0):
            p = int(rng.integers(0, len(c)))
            e = sub(rng, c, p)
            if e not in [x[1] for x in cand]:
                cand.append((p, e))
        centres.append((c, cand))
        entries += [e for _, e in cand]
    if name == "wlmix":                                # entries that are proper prefixes of other entries
        entries += [e[:14] for e in entries[:10] if len(e) == 16]
    lines = list(entries)
    lines += entries[:25]                               # repeated lines add weight
    lines.insert(7, entries[3][:5] + "N" + entries[3][6:])   # skipped by Insert
    return lines, sorted(set(entries)), centres


def make_barcodes(rng, entries, centres):
    out = []

    def q(n):
        return "".join(chr(int(x)) for x in rng.integers(35, 74, size=n))

    def add(label, b, qual=None):
        out.append((label, b, q(len(b)) if qual is None else qual))

    E = entries
    pick = lambda: E[int(rng.integers(0, len(E)))]   # noqa: E731
    for _ in range(150):
        add("exact", pick())
    for k in range(400):
        e = pick()
        p = k % len(e)
        add("sub_first" if p == 0 else "sub_last" if p == len(e) - 1 else "sub", sub(rng, e, p))
    for _ in range(60):
        e = pick(); p = int(rng.integers(0, len(e)))
        add("one_n", e[:p] + "N" + e[p + 1:])
    for _ in range(40):
        e = pick()
        if len(e) < 2:
            continue
        p1, p2 = sorted(rng.choice(len(e), size=2, replace=False))
        add("two_n", e[:p1] + "N" + e[p1 + 1:p2] + "N" + e[p2 + 1:])
        p = int(rng.integers(0, len(e)))
        s = sub(rng, e, p)
        p2 = (p + 1 + int(rng.integers(0, len(e) - 1))) % len(e)
        add("n_plus_sub", s[:p2] + "N" + s[p2 + 1:])
    for k, (c, cand) in enumerate(centres * (6 if len(centres) < 50 else 1)):
        for mode in ("lower", "equal", "higher"):
            qual = list(q(len(c)))
            base = 50
            for j, (p, _) in enumerate(cand):
                qual[p] = chr(base)
            if mode != "equal" and len({p for p, _ in cand}) > 1:
                p_last = cand[-1][0]
                qual[p_last] = chr(base - 7 if mode == "lower" else base + 7)
            add(f"cand{len(cand)}_{mode}", c, "".join(qual))
    for _ in range(60):
        e = pick()
        if len(e) > 1:
            add("prefix", e[:int(rng.integers(1, len(e)))])
    for _ in range(25):
        add("empty", "")
    for _ in range(40):
        add("longer", pick() + rnd(rng, int(rng.integers(1, 4))))
    for _ in range(200):
        add("hopeless", rnd(rng, len(pick())))
    for _ in range(20):
        e = pick(); p = int(rng.integers(0, len(e)))
        add("other_letter", e[:p] + "R" + e[p + 1:])
    return out


def make_background(rng, entries, centres, n):
    recs = []
    hot = [e for _, cand in centres for _, e in cand[:1]]          # the first candidate of a centre is seen more often: different counts
    for k in range(n):
        r = rng.random()
        if r < 0.45:
            recs.append(entries[int(rng.integers(0, len(entries)))])
        elif r < 0.75 and hot:
            recs.append(hot[int(rng.integers(0, len(hot)))] if k % 3 else hot[k % len(hot)])
        elif r < 0.82:
            e = entries[int(rng.integers(0, len(entries)))]
            recs.append(e[:max(1, len(e) - int(rng.integers(1, 4)))])    # a proper prefix: an inner node is counted
        elif r < 0.9:
            e = entries[int(rng.integers(0, len(entries)))]
            recs.append(e[:2] + "N" + e[3:])
        else:
            recs.append(rnd(rng, len(entries[0])))
    return recs


def make_cli_runs(rng, tmp):
    """the reference's command line on single-cell input"""
    root = os.path.dirname(os.path.dirname(HERE))
    ref = os.path.join(root, "oracle", "_ref", "centrifuger")
    assert os.path.exists(ref), "make -C oracle ref first"
    C = os.path.join(OUT, "cli")
    os.makedirs(os.path.join(C, "tsv"))
    entries = sorted(set(ln for ln in gzip.open(os.path.join(OUT, "wl16.txt.gz"), "rt").read().split("\n") if ln and "N" not in ln))

    def q(n):
        return "".join(chr(int(x)) for x in rng.integers(35, 74, size=n))

    def barcode(k):
        e = entries[int(rng.integers(0, 60))] if k % 3 else entries[int(rng.integers(0, len(entries)))]
        r = k % 10
        if r == 7:
            e = sub(rng, e, int(rng.integers(0, 16)))
        elif r == 8:
            p = int(rng.integers(0, 16)); e = e[:p] + "N" + e[p + 1:]
        elif r == 9:
            e = rnd(rng, 16) if k % 20 == 9 else e[:12]
        return e

    def write(name, recs):           # recs: (header, seq, qual or None)
        gz_write(os.path.join(C, name), "".join(f">{h}\n{s}\n" if ql is None else f"@{h}\n{s}\n+\n{ql}\n" for h, s, ql in recs).encode())

    se = open(os.path.join(HERE, "se.fq")).read().split("\n")
    se = [(se[i][1:], se[i + 1], se[i + 3]) for i in range(0, len(se) - 1, 4)]
    n_se, n_pe = len(se), 1400
    bcs = [barcode(k) for k in range(n_se)]
    ums = [rnd(rng, 10) for _ in range(n_se)]
    write("bc.fq.gz", [(f"r{i}", b, q(len(b))) for i, b in enumerate(bcs)])
    write("bc.fa.gz", [(f"r{i}", b, None) for i, b in enumerate(bcs)])
    write("um.fq.gz", [(f"r{i}", u, q(10)) for i, u in enumerate(ums)])
    write("bc_hd.fq.gz", [(f"r{i} 1:N:0:{rnd(rng, 6)} CB:Z:{b}" + (f" UB:Z:{u}" if i % 7 else ""), "ACGT", "IIII") for i, (b, u) in enumerate(zip(bcs, ums))])
    write("se_cut.fq.gz", [(h, bcs[i][:16].ljust(16, "A") + ums[i] + s, q(26) + ql) for i, (h, s, ql) in enumerate(se)])
    pbc = [barcode(k + 5) for k in range(n_pe)]
    write("bcum_pe.fq.gz", [(f"p{i}", (b.ljust(16, "C")) + rnd(rng, 10), q(26)) for i, b in enumerate(pbc)])
    write("bc_short.fq.gz", [(f"r{i}", b, q(len(b))) for i, b in enumerate(bcs[:-3])])
    # a translation table that knows every whitelist entry (16-mers)
    gz_write(os.path.join(C, "translate.txt.gz"), "".join(f"cell{i:04d}\t{e}\n" for i, e in enumerate(entries)).encode())
    runs = {
        "se_bc_um": ["-u", "{G}/se.fq", "--barcode", "{C}/bc.fq.gz", "--UMI", "{C}/um.fq.gz"],
        "pe_one_file": ["-1", "{M}/pairs_1.fq.gz", "-2", "{M}/pairs_2.fq.gz", "--barcode", "{C}/bcum_pe.fq.gz", "--UMI", "{C}/bcum_pe.fq.gz", "--read-format", "bc:0:15,um:16:-1"],
        "se_cut_from_read1": ["-u", "{C}/se_cut.fq.gz", "--read-format", "bc:0:15,um:16:25,r1:26:-1"],
        "whitelist_fq": ["-u", "{G}/se.fq", "--barcode", "{C}/bc.fq.gz", "--barcode-whitelist", "{B}/wl16.txt.gz"],
        "whitelist_fa": ["-u", "{G}/se.fq", "--barcode", "{C}/bc.fa.gz", "--barcode-whitelist", "{B}/wl16.txt.gz"],
        "whitelist_translate": ["-u", "{G}/se.fq", "--barcode", "{C}/bc.fq.gz", "--barcode-whitelist", "{B}/wl16.txt.gz", "--barcode-translate", "{C}/translate.txt.gz"],
        "hd": ["-u", "{G}/se.fq", "--barcode", "{C}/bc_hd.fq.gz", "--UMI", "{C}/bc_hd.fq.gz", "--read-format", "bc:hd:CB:5:-1,um:hd:UB:5:-1"],
        "pe_merge_k5": ["-1", "{M}/pairs_1.fq.gz", "-2", "{M}/pairs_2.fq.gz", "--merge-readpair", "-k", "5", "--barcode", "{C}/bcum_pe.fq.gz", "--read-format", "bc:0:15",
                        "--barcode-whitelist", "{B}/wl16.txt.gz"],
        "expand": ["-u", "{G}/se.fq", "--barcode", "{C}/bc.fq.gz", "--UMI", "{C}/um.fq.gz", "--expand-taxid", "--barcode-whitelist", "{B}/wl16.txt.gz"],
        "dump": ["-u", "{C}/se_cut.fq.gz", "--read-format", "bc:0:15,um:16:25,r1:26:-1", "--un", "un", "--cl", "cl"],
    }
    idx = os.path.join(tmp, "f6")
    for k in (1, 2, 4):
        shutil.copy(os.path.join(HERE, f"f6.{k}.cfr"), f"{idx}.{k}.cfr")
    where = {"G": HERE, "M": os.path.join(HERE, "merge"), "B": OUT, "C": C}
    man = {"cases": {}, "dumps": {}, "refusals": {}}
    for name, args in runs.items():
        out = run([ref, "-x", idx, "-t", "1"] + [a.format(**where) for a in args], stdout=subprocess.PIPE, cwd=tmp).stdout
        assert out.count(b"\n") > 300, name
        gz_write(os.path.join(C, "tsv", name + ".tsv.gz"), out)
        man["cases"][name] = {"args": args, "md5": hashlib.md5(out).hexdigest()}
    for f in sorted(f for f in os.listdir(tmp) if f.startswith(("un", "cl"))):
        raw = gzip.decompress(open(os.path.join(tmp, f), "rb").read())
        gz_write(os.path.join(C, f), raw)
        man["dumps"][f] = hashlib.md5(raw).hexdigest()
    assert set(man["dumps"]) == {x + y for x in ("un", "cl") for y in (".fq.gz", "_bc.fa.gz", "_um.fa.gz")}, man["dumps"]
    # what the reference says when it refuses
    for name, args in {"whitelist_without_barcode": ["-u", "{C}/se_cut.fq.gz", "--read-format", "bc:0:15,r1:26:-1", "--barcode-whitelist", "{B}/wl16.txt.gz"],
                       "bad_format": ["-u", "{G}/se.fq", "--read-format", "bc:0"],
                       "unequal_counts": ["-u", "{G}/se.fq", "--barcode", "{C}/bc_short.fq.gz"]}.items():
        r = subprocess.run([ref, "-x", idx, "-t", "1"] + [a.format(**where) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp)
        assert r.returncode != 0, name
        last = r.stderr.decode().strip().split("\n")[-1]
        man["refusals"][name] = {"args": args, "returncode": r.returncode, "message": last.split("] ", 1)[-1]}
    json.dump(man, open(os.path.join(C, "manifest.json"), "w"), indent=1, sort_keys=True)


def main():
    rng = np.random.default_rng(SEED)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    tmp = tempfile.mkdtemp(prefix="cfr_golden_barcode_")
    exe = {}
    for nm, text in (("correct", CORRECT_DRIVER), ("format", FORMAT_DRIVER), ("translate", TRANSLATE_DRIVER)):
        exe[nm] = os.path.join(tmp, nm + "_dump")
        with open(exe[nm] + ".cpp", "w") as f:
            f.write(text)
        run(["g++", "-O1", "-w", "-I", REF_SRC, "-o", exe[nm], exe[nm] + ".cpp", "-lz", "-lpthread"])
    manifest = {"seed": SEED, "whitelists": {}, "bad_formats": {}, "translate": {}}

    # ---- whitelists
    ret_total = {-1: 0, 0: 0, 1: 0}
    class_total = {}
    for name, fname in (("wl5", "wl5.txt"), ("wl16", "wl16.txt.gz"), ("wlmix", "wlmix.txt")):
        lines, entries, centres = make_whitelist(rng, name)
        data = ("\n".join(lines) + "\n").encode()
        path = os.path.join(OUT, fname)
        if fname.endswith(".gz"):
            gz_write(path, data)
        else:
            open(path, "wb").write(data)
        n_bg, cap = (40, 25) if name == "wl5" else (1500, 1000)
        bg = make_background(rng, entries, centres, n_bg)
        bg_fa = os.path.join(tmp, name + ".bg.fa")
        open(bg_fa, "w").write("".join(f">b{i}\n{b}\n" for i, b in enumerate(bg)))
        bcs = make_barcodes(rng, entries, centres)
        counts_path = os.path.join(tmp, name + ".counts")
        dump = run([exe["correct"], path, bg_fa, str(cap), counts_path], input="".join(f"{b}\t{q}\n" for _, b, q in bcs).encode(),
                   stdout=subprocess.PIPE).stdout
        rows = [ln.split(b"\t") for ln in dump.split(b"\n")[:-1]]
        assert len(rows) == len(bcs), (len(rows), len(bcs))
        for (label, _, _), r in zip(bcs, rows):
            ret_total[int(r[0])] += 1
            class_total[label] = class_total.get(label, 0) + 1
        differ = sum(1 for r in rows if r[1] != r[3])
        gz_write(os.path.join(OUT, name + ".background.tsv.gz"), ("\n".join(bg) + "\n").encode())
        gz_write(os.path.join(OUT, name + ".counts.tsv.gz"), open(counts_path, "rb").read())
        gz_write(os.path.join(OUT, name + ".barcodes.tsv.gz"), "".join(f"{lb}\t{b}\t{q}\n" for lb, b, q in bcs).encode())
        gz_write(os.path.join(OUT, name + ".corrected.tsv.gz"), dump)
        manifest["whitelists"][name] = {"file": fname, "background_cap": cap, "n_background": n_bg, "n_barcodes": len(bcs),
                                        "n_entries": len(entries), "quality_changes_the_choice": differ}
        print(name, "entries", len(entries), "barcodes", len(bcs), "choice differs with qualities:", differ, file=sys.stderr)
    print("returns", ret_total, "classes", class_total, file=sys.stderr)
    assert all(v >= 100 for v in ret_total.values()), ret_total
    assert all(v >= 20 for v in class_total.values()), class_total
    for need in ("exact", "sub_first", "sub_last", "one_n", "two_n", "n_plus_sub", "cand2_lower", "cand2_equal", "cand2_higher", "cand3_lower",
                 "cand3_equal", "cand3_higher", "prefix", "empty", "longer"):
        assert need in class_total, need
    assert sum(w["quality_changes_the_choice"] for w in manifest["whitelists"].values()) >= 20
    manifest["returns"] = {str(k): v for k, v in ret_total.items()}
    manifest["classes"] = class_total

    # ---- read formats
    recs = []
    for k in range(200):
        L = 0 if k % 20 == 0 else int(rng.integers(1, 70)) if k % 3 else int(rng.integers(26, 70))
        s = "".join("ACGTN"[i] for i in rng.choice(5, size=L, p=[.24, .24, .24, .24, .04]))
        if k % 17 == 5:
            s = s[:L // 2] + s[L // 2:].lower()
        qual = "".join(chr(int(x)) for x in rng.integers(33, 74, size=L))
        cb, ub = rnd(rng, 16), rnd(rng, 10)
        sepc = "\t" if k % 4 == 1 else " "
        cm = [f"1:N:0:{rnd(rng, 8)}", f"CB:Z:{cb}", f"UB:Z:{ub}"]
        if k % 5 == 2:
            cm = cm[:1]
        if k % 11 == 3:
            cm = []
        recs.append((s, qual, sepc.join(cm)))
    gz_write(os.path.join(OUT, "format_records.tsv.gz"), "".join(SEP.join(r) + "\n" for r in recs).encode())
    formats = []
    for k, spec in enumerate(GOOD_FORMATS):
        min_len = 0
        for seg in spec.replace(";", ",").split(","):
            parts = seg.split(":")
            if parts[1] != "hd" and int(parts[1]) < 0:
                min_len = max(min_len, -int(parts[1]))
        use = [i for i, r in enumerate(recs) if len(r[0]) >= min_len]      # a negative start on a shorter read is out of bounds in the reference
        dump = run([exe["format"], spec], input="".join(SEP.join(recs[i]) + "\n" for i in use).encode(), stdout=subprocess.PIPE).stdout
        gz_write(os.path.join(OUT, f"format_{k}.tsv.gz"), dump)
        formats.append({"spec": spec, "records": use if len(use) != len(recs) else None, "file": f"format_{k}.tsv.gz"})
    for spec in BAD_FORMATS:
        r = subprocess.run([exe["format"], spec], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1, (spec, r.returncode)
        manifest["bad_formats"][spec] = r.stderr.decode()
    json.dump(formats, open(os.path.join(OUT, "formats.json"), "w"), indent=1)

    # ---- translation
    froms = sorted({rnd(rng, 8) for _ in range(60)})
    table = "".join(f"cell{i:03d}{',' if i % 3 == 0 else chr(9) if i % 3 == 1 else ' '}{f}\n" for i, f in enumerate(froms))
    table += f"again,{froms[5]}\n"                                       # a repeated `from`: the last `to` stays
    open(os.path.join(OUT, "translate.txt"), "w").write(table)
    bcs = []
    for k in range(120):
        pieces = [froms[int(rng.integers(0, len(froms)))] for _ in range(k % 4)]
        bcs.append("".join(pieces) + rnd(rng, int(rng.integers(0, 8))) if k % 2 else "".join(pieces))
    bcs.append(froms[5])
    dump = run([exe["translate"], os.path.join(OUT, "translate.txt")], input=("\n".join(bcs) + "\n").encode(), stdout=subprocess.PIPE).stdout
    got = dump.decode().split("\n")[:-1]
    assert len(got) == len(bcs)
    gz_write(os.path.join(OUT, "translate.tsv.gz"), "".join(f"{b}\t{t}\n" for b, t in zip(bcs, got)).encode())
    missing = "A" * 8 if "A" * 8 not in froms else "C" * 8
    r = subprocess.run([exe["translate"], os.path.join(OUT, "translate.txt")], input=(froms[0] + missing + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    manifest["translate"] = {"missing_barcode": froms[0] + missing, "stderr": r.stderr.decode(), "returncode": r.returncode}
    assert r.returncode == 255

    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    make_cli_runs(rng, tmp)
    shutil.rmtree(tmp)
    total = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(OUT) for f in fs)
    print("tests/golden/barcode:", total, "bytes", file=sys.stderr)
    assert total < 1000000


if __name__ == "__main__":
    main()
