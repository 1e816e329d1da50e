"""Reads for the tests of the batch formatter (cfr_tsv_*): results, matches and ids that cover what csrc/cfr_tsv_core.hpp states, and
the reference they are compared with - cfr_format_tsv read after read.  Shared by tests/test_tsv_host_cpu.py, tests/test_gpu_tsv.py
and (through a corpus file) tools/tsv_sanitize.cpp."""
import os
import struct

import numpy as np

import quant_fixtures as qf
from centrifuger_amd import capi
from conftest import GOLDEN

F6 = os.path.join(GOLDEN, "f6")
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# 0, 9, 10, every 10^k - 1 and 10^k up to 10^19, and 2^64 - 1
U64_EDGES = sorted({0, 9, 10, (1 << 64) - 1} | {10 ** k - 1 for k in range(1, 20)} | {10 ** k for k in range(1, 20)})
I32_EDGES = [0, -1, INT32_MIN, INT32_MAX]
ID_LENGTHS = [0, 1, 15, 16, 17, 300]
N_MATCHES = [0, 1, 5, 64]


def hybrid_prefix(tmp):
    """the FM index of f6 under the 811-node taxonomy of quant_wide (cfr_tsv_open reads names and rank codes only)"""
    for ext in ("1", "4"):
        os.symlink(F6 + f".{ext}.cfr", os.path.join(tmp, f"hy.{ext}.cfr"))
    os.symlink(qf.WIDE_PREFIX + ".2.cfr", os.path.join(tmp, "hy.2.cfr"))
    return os.path.join(tmp, "hy")


def read_id(rng, length):
    return bytes(rng.integers(33, 127, size=length, dtype=np.uint8)).replace(b"\t", b"_")


class Batch:
    def __init__(self):
        self.res, self.mat, self.ids = [], [], []

    def add(self, rid, matches, score=0, second=0, hit=0, qlen=0, n_match=None, begin=None):
        """matches: (id, taxid, kind) tuples, appended to the match array (begin = where they start)"""
        begin = len(self.mat) if begin is None else begin
        self.mat.extend(matches)
        self.res.append((score, second, hit, qlen, len(matches) if n_match is None else n_match, 0, begin))
        self.ids.append(rid)

    def arrays(self):
        res = np.array(self.res, dtype=capi.RESULT_DTYPE) if self.res else np.zeros(0, dtype=capi.RESULT_DTYPE)
        mat = np.zeros(len(self.mat), dtype=capi.MATCH_DTYPE)
        for k, (i, t, kind) in enumerate(self.mat):
            mat[k] = (i, t, kind, 0)
        return res, mat, list(self.ids)


def edge_batch(seq_cnt, node_cnt, seed=5):
    """every case the host test lists, one read each (and a few hundred random ones around them)"""
    rng = np.random.default_rng(seed)
    b = Batch()
    k = 0
    for nm in N_MATCHES:
        for kind in (0, 1):
            for L in ID_LENGTHS:
                top = seq_cnt if kind == 0 else node_cnt
                ms = [(int(rng.integers(0, top)), int(rng.integers(0, 1 << 40)), kind) for _ in range(nm)]
                b.add(read_id(rng, L), ms, score=int(rng.integers(0, 1 << 33)), second=int(rng.integers(0, 1000)), hit=int(rng.integers(0, 300)),
                      qlen=int(rng.integers(0, 302)))
                k += 1
    # an id outside the tables: the empty name, rank string 0
    b.add(b"out_seq", [(seq_cnt, 7, 0), (seq_cnt + 12345, 8, 0), ((1 << 64) - 1, 9, 0)], score=1)
    b.add(b"out_node", [(node_cnt, 7, 1), (node_cnt + 1, 8, 1), ((1 << 64) - 1, 9, 1)], score=1)
    b.add(b"other_kind", [(0, 1, 2), (1, 1, -1)], score=1)            # (any kind but 0 prints a rank string)
    for v in U64_EDGES:
        b.add(b"u", [(0, v, 0)], score=v, second=v, hit=1, qlen=2)
        b.add(b"u3", [(1, (1 << 64) - 1 - v, 1)], score=0, second=v)
    for h in I32_EDGES:
        for q in I32_EDGES:
            b.add(b"i32", [(0, 1, 1)], hit=h, qlen=q)
            b.add(b"i32u", [], hit=h, qlen=q, n_match=0)
    for nm in (-1, INT32_MIN):                                        # n_match <= 0 is unclassified, whatever match_begin says
        b.add(b"neg", [], qlen=77, n_match=nm, begin=(1 << 64) - 1)
    b.add(b"big_n", [(0, 1, 0)], n_match=1, hit=INT32_MAX)
    for _ in range(300):
        nm = int(rng.integers(0, 6))
        kind = int(rng.integers(0, 2))
        top = (seq_cnt if kind == 0 else node_cnt) + 1
        b.add(read_id(rng, int(rng.integers(0, 40))), [(int(rng.integers(0, top)), int(rng.integers(0, 1 << 63)) * 2 + 1, kind) for _ in range(nm)],
              score=int(rng.integers(0, 1 << 62)), second=int(rng.integers(0, 1 << 20)), hit=int(rng.integers(-5, 300)), qlen=int(rng.integers(0, 400)))
    return b.arrays()


def random_batch(n, seq_cnt, node_cnt, seed, id_len=(0, 24), max_matches=5, stride=None):
    """n reads as the classifier leaves them; stride: match_begin = i * stride (slots a read does not use stay zero)"""
    rng = np.random.default_rng(seed)
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    nm = rng.integers(0, max_matches + 1, size=n)
    if stride is None:
        begin = np.concatenate([[0], np.cumsum(nm)])[:n]
        slots = int(nm.sum())
    else:
        begin = np.arange(n, dtype=np.uint64) * stride
        slots = n * stride
    res["n_match"] = nm
    res["match_begin"] = begin
    res["score"] = rng.integers(0, 1 << 20, size=n)
    res["secondary_score"] = rng.integers(0, 1 << 12, size=n)
    res["hit_length"] = rng.integers(0, 301, size=n)
    res["query_length"] = rng.integers(30, 302, size=n)
    mat = np.zeros(slots, dtype=capi.MATCH_DTYPE)
    kind = rng.integers(0, 2, size=slots)
    mat["kind"] = kind
    mat["id"] = np.where(kind == 0, rng.integers(0, seq_cnt + 1, size=slots), rng.integers(0, node_cnt + 1, size=slots))
    mat["taxid"] = rng.integers(0, 3000000, size=slots)
    lens = rng.integers(id_len[0], id_len[1] + 1, size=n)
    ids = [read_id(rng, int(L)) for L in lens]
    return res, mat, ids


def reference(index, res, mat, ids):
    """cfr_format_tsv per read -> (text, row_offsets)"""
    rows = [index.format_tsv(ids[i].decode("latin-1"), res[i], mat) for i in range(len(res))]
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    return b"".join(rows), off


def write_corpus(path, tables, batches):
    """what tools/tsv_sanitize.cpp reads: the tables (sequence names, rank codes), then batches of results, matches, ids and the
    text the host twin must make.  Little-endian throughout."""
    names, ranks = tables
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(names), len(ranks)))
        for s in names:
            f.write(struct.pack("<I", len(s)) + s)
        f.write(bytes(ranks))
        for res, mat, ids, want in batches:
            idb, ido = capi.pack_ids(ids)
            f.write(struct.pack("<QQQQ", len(res), len(mat), int(ido[-1]), len(want)))
            f.write(res.tobytes() + mat.tobytes() + ido.tobytes() + idb.tobytes()[:int(ido[-1])] + want)
