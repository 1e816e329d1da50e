"""Shared by tests/test_promote_host_cpu.py and tests/test_gpu_promote.py: the fixtures of tests/golden/promote and tests/golden/inspect
(make_golden_promote.py), result / match arrays made from lists of tax ids, and a direct Python restatement of the reference's Perl
script (centrifuger-promote:44-149) on original tax ids - dictionaries as in the script, none of the library's tables."""
import gzip
import json
import os
import subprocess

import numpy as np

import quant_fixtures as qf
from centrifuger_amd import capi
from conftest import GOLDEN, ROOT

PDIR = os.path.join(GOLDEN, "promote")
IDIR = os.path.join(GOLDEN, "inspect")
BIN = os.path.join(ROOT, "centrifuger_amd", "bin")
PROMOTE = os.path.join(BIN, "centrifuger-promote")
INSPECT = os.path.join(BIN, "centrifuger-inspect")
PREFIXES = {"q8": qf.PREFIX, "qw": qf.WIDE_PREFIX}
MANIFEST = json.load(open(os.path.join(PDIR, "manifest.json")))
LEVELS = MANIFEST["levels"]
assert set(LEVELS) == {"genus", "species", "strain", "subspecies", "no rank", "lca", "bogus"}


def golden(name):
    return gzip.open(os.path.join(PDIR, name), "rb").read()


def outputs(key=None):
    """[(file name, index key, input path, level, warnings)]"""
    return [(name, o["index"], os.path.join(GOLDEN, o["input"]), o["level"], o["warnings"]) for name, o in sorted(MANIFEST["outputs"].items())
            if key is None or name.startswith(key + ".")]


def run_promote(args):
    return subprocess.run([PROMOTE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


class Tree:
    """the script's %taxParent and %taxLevel, read from the golden centrifuger-inspect --taxonomy-tree output"""

    def __init__(self, idx):
        self.parent, self.level = {}, {}
        for line in open(os.path.join(IDIR, f"{idx}.taxonomy-tree.txt")):
            c = line.rstrip("\n").rstrip("|").rstrip("\t").split("\t|\t")
            self.parent[int(c[0])], self.level[int(c[0])] = int(c[1]), c[2]
        self.orig = list(self.level)                       # compact id -> original id (the tree is printed in compact order)
        self.compact = {t: i for i, t in enumerate(self.orig)}

    def promote_taxid(self, tid, level):                   # PromoteTaxId
        while True:
            if tid <= 0 or tid not in self.level:
                return 0
            if self.level[tid] == level:
                return tid
            if tid <= 1 or self.parent[tid] == tid:        # (the second test: the library's stop at a self-parent; the script would not return)
                return 0
            tid = self.parent[tid]

    def lca(self, a, b, warn):                             # lca
        if a == 0:
            return b
        if b == 0 or a == b:
            return a
        path = set()
        while a >= 1:
            path.add(a)
            if a not in self.parent:
                warn.append(a)
                break
            if a == self.parent[a]:
                break
            a = self.parent[a]
        while b > 1:
            if b in path:
                return b
            if b not in self.parent:
                warn.append(b)
                break
            if b == self.parent[b]:
                break
            b = self.parent[b]
        return 1

    def promote_read(self, taxids, level, warn=None):
        """OutputPromotedLines on the tax ids of one read -> [(source row, new tax id, whether column 2 becomes the rank of the new id)]"""
        warn = [] if warn is None else warn
        if not taxids:
            return []
        if level != "lca":
            out, seen = [], set()
            for j, t in enumerate(taxids):
                new = self.promote_taxid(t, level)
                if new <= 1:
                    new = t
                if new in seen:
                    continue
                seen.add(new)
                out.append((j, new, new >= 1 and new in self.level))
            return out
        l = taxids[0]
        for t in taxids[1:]:
            l = self.lca(l, t, warn)
        return [(0, l, l != taxids[0])]


def make_arrays(tree, reads, node_cnt, seq_to_tax=None, rng=None, gap=0):
    """reads: lists of original tax ids.  Every match is kind 1 with its compact id (node_cnt when the tree does not hold it), or - with
    seq_to_tax and rng, for half of the ids that some sequence carries - kind 0 with such a sequence's id.  gap: unused slots behind every read"""
    by_node = {}
    if seq_to_tax is not None:
        for s, c in enumerate(seq_to_tax):
            by_node.setdefault(int(c), []).append(s)
    n = len(reads)
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    total = sum(len(t) + gap for t in reads)
    mat = np.zeros(max(total, 1), dtype=capi.MATCH_DTYPE)
    mat["id"], mat["taxid"], mat["kind"] = 0xdead, 0xdead, 7      # unused slots: never read, never written
    at = 0
    for i, t in enumerate(reads):
        res[i] = (1000 + i, i, 100, 150, len(t), 0, at)
        for j, tid in enumerate(t):
            c = tree.compact.get(tid, node_cnt)
            if rng is not None and c in by_node and rng.random() < 0.5:
                mat[at + j] = (by_node[c][int(rng.integers(0, len(by_node[c])))], tid, 0, 0)
            else:
                mat[at + j] = (c, tid, 1, 0)
        at += len(t) + gap
    return res, mat


def check_against_script(tree, reads, level, res0, mat0, res, mat, src, node_cnt):
    """res / mat / src after cfr_promote_apply on copies of res0 / mat0 against the restatement, read by read"""
    for i, t in enumerate(reads):
        want = tree.promote_read(t, level)
        b = int(res0["match_begin"][i])
        assert int(res["n_match"][i]) == len(want), (i, t, level, res[i], want)
        for f in ("score", "secondary_score", "hit_length", "query_length", "match_begin"):
            assert res[f][i] == res0[f][i]
        for k, (j, new, renamed) in enumerate(want):
            m = mat[b + k]
            assert int(m["taxid"]) == new, (i, t, level, k, m, want)
            assert int(src[b + k]) == b + j, (i, t, level, k, src[b + k], want)
            if level == "lca" and not renamed:
                assert m == mat0[b + j], (i, t, level, m, mat0[b + j])          # untouched, kind and id included
            elif new in tree.compact and (level == "lca" or t[j] in tree.compact):
                assert int(m["kind"]) == 1 and int(m["id"]) == tree.compact[new], (i, t, level, k, m, want)
            elif level == "lca":
                assert int(m["kind"]) == 1 and int(m["id"]) == node_cnt                # the literal 1 of a tree without it
            else:
                assert m == mat0[b + j], (i, t, level, m, mat0[b + j])          # not a node: left as it is
