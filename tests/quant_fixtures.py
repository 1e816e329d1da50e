"""Shared by tests/test_quant_host_cpu.py and tests/test_gpu_quant.py: the fixtures of tests/golden/quant (make_golden_quant.py) and of
tests/golden/quant_wide (make_golden_quant_wide.py; every helper takes the fixture's directory and index prefix, the default is the
first), and a direct Python restatement of how the reference turns TSV rows into coalesced assignments (Quantifier::LoadReadAssignments and
CoalesceAssignments, Quantifier.hpp:490-622)."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT

QDIR = os.path.join(GOLDEN, "quant")
PREFIX = os.path.join(QDIR, "q8")
QUANT = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger-quant")
MANIFEST = json.load(open(os.path.join(QDIR, "manifest.json")))
TSV_KEYS = ("se_k1", "pe_k5", "edge", "header_only")
WIDE_DIR = os.path.join(GOLDEN, "quant_wide")          # 811 nodes: root, 10 genera, 200 species, 600 strains
WIDE_PREFIX = os.path.join(WIDE_DIR, "qw")


def manifest(qdir=QDIR):
    return MANIFEST if qdir == QDIR else json.load(open(os.path.join(qdir, "manifest.json")))


def tsv_path(key, qdir=QDIR):
    p = os.path.join(qdir, key + ".tsv")
    return p if os.path.exists(p) else p + ".gz"


def reports(key=None, qdir=QDIR):
    """[(file name, tsv key, format, extra arguments)]"""
    return [(name, r["tsv"], r["format"], r["args"]) for name, r in sorted(manifest(qdir)["reports"].items()) if key is None or r["tsv"] == key]


def expected(name, qdir=QDIR):
    return open(os.path.join(qdir, "report", name), "rb").read()


def run_quant(args, stdin=None):
    return subprocess.run([QUANT] + args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def orig_taxids(prefix=PREFIX):
    """compact tax id -> original tax id, from <prefix>.2.cfr (Taxonomy::Save, Taxonomy.hpp:1238-1257)"""
    raw = open(prefix + ".2.cfr", "rb").read()
    node_cnt = struct.unpack_from("<Q", raw, 0)[0]
    off = 24 + 16 * node_cnt
    n = struct.unpack_from("<Q", raw, off)[0]
    return list(struct.unpack_from(f"<{n}Q", raw, off + 8))[:node_cnt]


def read_rows(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rt") as f:
        lines = f.read().split("\n")
    rows = []
    for line in lines[1:]:
        if line:
            c = line.split("\t")
            rows.append((c[0], int(c[2]), int(c[3]), int(c[4]), int(c[5]), int(c[6])))
    return rows


def weight(hit_length, read_length):
    diff = read_length - hit_length
    if diff < int(read_length * 0.01):
        return 1.0
    diff -= int(read_length * 0.01)
    return 1.0 / float(1 << (2 * min(diff, 11) if diff <= 10 else 22))


def restate(rows, min_score=0, min_length=0, prefix=PREFIX):
    """rows (read id, taxid, score, second, hit length, read length) -> sorted [(targets, weight, count, uniq)]"""
    compact = {t: i for i, t in enumerate(orig_taxids(prefix))}
    node_cnt = len(compact)
    groups, prev = [], None
    for rid, taxid, score, second, hit, length in rows:
        if hit < min_length or score < min_score or taxid == 0:
            continue
        if rid != prev:
            groups.append([[], weight(hit, length), 1 if score > second else 0])
            prev = rid
        groups[-1][0].append(compact.get(taxid, node_cnt))
    merged = {}
    for targets, w, u in groups:
        m = merged.setdefault(tuple(targets), [0.0, 0, 0])
        m[0] += w; m[1] += 1; m[2] += u
    return [(k, v[0], v[1], v[2]) for k, v in sorted(merged.items(), key=lambda kv: (len(kv[0]), kv[0]))]


def as_tuples(assignments):
    lists, w, c, u = assignments
    return [(lists[i], float(w[i]), int(c[i]), int(u[i])) for i in range(len(lists))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
