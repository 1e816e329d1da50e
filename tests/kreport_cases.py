"""Shared by tests/test_kreport_host_cpu.py and tests/test_gpu_kreport.py: the fixtures of tests/golden/kreport (make_golden_kreport.py),
a direct Python restatement of the reference's Perl script (centrifuger-kreport) on original tax ids - dictionaries as in the script,
none of the library's tables - and generators of random reads over the 14-node and the 811-node tree."""
import gzip
import json
import os
import subprocess

import numpy as np

import promote_cases as pc
import quant_fixtures as qf
from conftest import GOLDEN

KDIR = os.path.join(GOLDEN, "kreport")
KREPORT = os.path.join(pc.BIN, "centrifuger-kreport")
PREFIXES = pc.PREFIXES
MANIFEST = json.load(open(os.path.join(KDIR, "manifest.json")))
UNKNOWN = [88888, 99999]                   # tax ids no tree holds
RANK_CODE = {"species": "S", "genus": "G", "family": "F", "order": "O", "class": "C", "phylum": "P", "kingdom": "K", "superkingdom": "D",
             "domain": "D", "acellular root": "D"}


def golden(name):
    return gzip.open(os.path.join(KDIR, name), "rb").read()


def outputs(key=None):
    """[(file name, manifest entry)]"""
    return [(name, o) for name, o in sorted(MANIFEST["outputs"].items()) if key is None or name.startswith(key + ".")]


def run_kreport(args, **kw):
    return subprocess.run([KREPORT] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


def warning_ids(stderr):
    pre, post = "Couldn't find parent of taxID ", " - directly assigned to root."
    return [int(l[len(pre):-len(post)]) for l in stderr.decode().splitlines() if l.startswith(pre) and l.endswith(post)]


def read_rows(path):
    """header columns and rows of a classification file, as lists of strings"""
    raw = (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")).read().decode().split("\n")
    return raw[0].split("\t"), [l.split("\t") for l in raw[1:] if l]


class Script:
    """the script, on a pc.Tree plus the golden name table"""

    def __init__(self, idx):
        self.tree = pc.Tree(idx)
        self.parent = dict(self.tree.parent)
        self.rank = dict(self.tree.level)
        self.name = {}
        for line in open(os.path.join(pc.IDIR, f"{idx}.name-table.txt")):
            c = line.rstrip("\n").rstrip("|").rstrip("\t").split("\t|\t")
            self.name[int(c[0])] = c[1]
        self.children = {}
        for node in self.tree.orig:                       # compact order, as inspect prints the tree
            if node == 1:
                self.parent[node] = 0
            self.children.setdefault(self.parent[node], []).append(node)
        self.lca_tree = pc.Tree(idx)
        self.lca_tree.parent = self.parent                # lca() walks %parent_map, in which node 1's parent is 0

    def in_tree(self, a, warn):                           # isTaxIDInTree
        while a > 1:
            if a not in self.parent:
                warn.append(a)
                return False
            if a == self.parent[a]:
                break
            a = self.parent[a]
        return True

    def count_reads(self, reads, min_score=None, min_length=None):
        """reads: (tax ids, score, hit length); a read without tax ids is the one row with tax id 0 -> counts, scores, seq_count, warnings"""
        counts, scores, seq, warn = {0: 0}, {0: 0}, 0, []
        for taxids, score, hitlen in reads:
            if min_length is not None and hitlen < min_length:
                continue
            if min_score is not None and score < min_score:
                continue
            ids = list(taxids) or [0]
            t = ids[0]
            if not self.in_tree(t, warn):
                t = 1
            for b in ids[1:]:
                t = self.lca_tree.lca(t, b, warn)
            counts[t] = counts.get(t, 0) + 1
            if t not in scores or score > scores[t]:
                scores[t] = score
            seq += 1
        return counts, scores, seq, warn

    def count_rows(self, header, rows, min_score=None, min_length=None, no_lca=False):
        """the script's main loop over the rows of a file"""
        h = {name: k for k, name in enumerate(header)}
        counts, scores, seq, warn = {0: 0}, {0: 0}, 0, []
        k = 0
        while k < len(rows):
            c = rows[k]
            k += 1
            t, score, hitlen, num = int(c[h["taxID"]]), int(c[h["score"]]), int(c[h["hitLength"]]), int(c[h["numMatches"]])
            if min_length is not None and hitlen < min_length:
                continue
            if min_score is not None and score < min_score:
                continue
            if not self.in_tree(t, warn):
                t = 1
            if no_lca:
                counts[t] = counts.get(t, 0) + 1 / num
                seq += 1 / num
                continue
            for _ in range(1, num):
                t = self.lca_tree.lca(t, int(rows[k][h["taxID"]]), warn)
                k += 1
            counts[t] = counts.get(t, 0) + 1
            if t not in scores or score > scores[t]:
                scores[t] = score
            seq += 1
        return counts, scores, seq, warn

    def clades(self, counts, scores):                     # dfs_summation(1)
        clade, cscore = dict(counts), dict(scores)

        def dfs(node):
            for ch in self.children.get(node, []):
                dfs(ch)
                clade[node] = clade.get(node, 0) + clade.get(ch, 0)
                if ch in cscore and (node not in cscore or cscore[ch] > cscore[node]):
                    cscore[node] = cscore[ch]
        dfs(1)
        return clade, cscore

    def report(self, counts, scores, seq, show_zeros=False, score_data=False):
        """the script's stdout; None where it dies"""
        clade, cscore = self.clades(counts, scores if score_data else {0: 0})
        if not seq > 0:
            return None
        out = ["%6.2f\t%d\t%d\t%s\t%d\t%s%s%s\n" % (clade[0] * 100 / seq, int(clade[0]), int(counts[0]), "U", 0, "", "unclassified", "\t0" if score_data else "")]

        def dfs(node, depth):
            if not clade.get(node, 0) and not show_zeros:
                return
            out.append("%6.2f\t%d\t%d\t%s\t%d\t%s%s%s\n" % (clade.get(node, 0) * 100 / seq, int(clade.get(node, 0)), int(counts.get(node, 0)),
                                                         RANK_CODE.get(self.rank[node], "-"), node, "  " * depth, self.name[node],
                                                         "\t%d" % cscore.get(node, 0) if score_data else ""))
            for ch in sorted(self.children.get(node, []), key=lambda c: -clade.get(c, 0)):        # (sorted() is stable, like Perl's merge sort)
                dfs(ch, depth + 1)
        dfs(1, 0)
        return "".join(out).encode()

    def bins(self, counts, node_cnt):
        """a dictionary of the script by tax id -> the library's node_cnt + 1 bins (unclassified last)"""
        out = np.zeros(node_cnt + 1, dtype=np.uint64)
        for t, v in counts.items():
            assert t == 0 or t in self.tree.compact, t            # (the generators below never end a fold on an id the tree lacks)
            out[node_cnt if t == 0 else self.tree.compact[t]] = int(v)
        return out


def options_of(args):
    """script arguments -> keyword arguments of Script.count_rows / report"""
    kw, rep = {}, {}
    it = iter(args)
    for a in it:
        if a == "--min-score":
            kw["min_score"] = int(next(it))
        elif a == "--min-length":
            kw["min_length"] = int(next(it))
        elif a == "--no-lca":
            kw["no_lca"] = True
        elif a == "--show-zeros":
            rep["show_zeros"] = True
        elif a == "--report-score-data":
            rep["score_data"] = True
        else:
            raise AssertionError(a)
    return kw, rep


def random_reads(tree, rng, n, max_list=6, unknown_share=0.1, scores=(0, 1 << 20), lengths=(0, 300)):
    """n reads: (tax ids, score, hit length).  Lists of 0..max_list ids; a share of the draws is in no tree.  No list starts with tax id 0
    (the classifier writes none; cfr_kreport_core.hpp says what would differ)."""
    ids = np.array(tree.orig + UNKNOWN * max(1, int(len(tree.orig) * unknown_share / 2)), dtype=np.uint64)
    out = []
    for _ in range(n):
        t = ids[rng.integers(0, len(ids), size=int(rng.integers(0, max_list + 1)))].tolist()
        out.append((t, int(rng.integers(scores[0], scores[1])), int(rng.integers(lengths[0], lengths[1]))))
    return out


def arrays(tree, reads, node_cnt, **kw):
    """pc.make_arrays with every read's score and hit length"""
    res, mat = pc.make_arrays(tree, [t for t, _s, _l in reads], node_cnt, **kw)
    res["score"] = np.array([s for _t, s, _l in reads], dtype=np.uint64)
    res["hit_length"] = np.array([l for _t, _s, l in reads], dtype=np.int32)
    return res, mat
