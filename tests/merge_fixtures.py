"""Loading of tests/golden/merge (make_golden_merge.py): the pairs, the reference's dump of the merged reads and its TSVs.
Everything is read once per process and handed out as it is (callers copy what they change)."""
import functools
import gzip
import json
import os

import numpy as np

MERGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge")


def _flat(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offs


def _read(path):
    lines = gzip.open(path, "rb").read().split(b"\n")
    ids, seqs, quals = [], [], []
    if lines[0].startswith(b"@"):
        for i in range(0, len(lines) - 1, 4):
            ids.append(lines[i][1:]); seqs.append(lines[i + 1]); quals.append(lines[i + 3])
    else:
        for i in range(0, len(lines) - 1, 2):
            ids.append(lines[i][1:]); seqs.append(lines[i + 1])
    ids = [x[:-2] if x.endswith((b"/1", b"/2")) else x for x in ids]
    b, o = _flat(seqs)
    return ids, b, o, (_flat(quals)[0] if quals else None)


@functools.lru_cache(maxsize=None)
def pairs(fmt):
    """fmt 'fq' / 'fa' -> dict ids, b1, o1, q1, b2, o2, q2 (q* None for 'fa')"""
    ids, b1, o1, q1 = _read(os.path.join(MERGE, f"pairs_1.{fmt}.gz"))
    _, b2, o2, q2 = _read(os.path.join(MERGE, f"pairs_2.{fmt}.gz"))
    return {"ids": ids, "b1": b1, "o1": o1, "q1": q1, "b2": b2, "o2": o2, "q2": q2}


@functools.lru_cache(maxsize=None)
def dump(fmt):
    """the reference's ReadPairMerger on the set: list of (kind, overlap, offset, why, rm, qm)"""
    rows = [ln.split(b"\t") for ln in gzip.open(os.path.join(MERGE, f"merged_{fmt}.tsv.gz"), "rb").read().split(b"\n")[:-1]]
    return [(int(r[0]), int(r[1]), int(r[2]), r[3], r[4], r[5]) for r in rows]


@functools.lru_cache(maxsize=None)
def manifest():
    return json.load(open(os.path.join(MERGE, "manifest.json")))


def golden(name):
    return gzip.open(os.path.join(MERGE, name + ".gz"), "rb").read()


def tsv(case):
    return golden(os.path.join("tsv", case + ".tsv"))


def expected_reads(fmt):
    """what a merge must hand on, from the reference's dump: (b1, o1, q1, b2, o2, q2) with read 1 = merged read, read 2 = empty for
    every merged pair and the pair as it is otherwise"""
    p, d = pairs(fmt), dump(fmt)
    s1, s2, t1, t2 = [], [], [], []
    for i, (kind, _, _, _, rm, qm) in enumerate(d):
        a1, e1, a2, e2 = int(p["o1"][i]), int(p["o1"][i + 1]), int(p["o2"][i]), int(p["o2"][i + 1])
        if kind:
            s1.append(rm); s2.append(b"")
            t1.append(qm); t2.append(b"")
        else:
            s1.append(bytes(p["b1"][a1:e1])); s2.append(bytes(p["b2"][a2:e2]))
            if p["q1"] is not None:
                t1.append(bytes(p["q1"][a1:e1])); t2.append(bytes(p["q2"][a2:e2]))
    b1, o1 = _flat(s1)
    b2, o2 = _flat(s2)
    fq = p["q1"] is not None
    return b1, o1, (_flat(t1)[0] if fq else None), b2, o2, (_flat(t2)[0] if fq else None)


def check_against_dump(fmt, got):
    """got: the dict capi.merge_pairs / DeviceIndex.merge_pairs return"""
    d = dump(fmt)
    assert got["kind"].tolist() == [r[0] for r in d]
    assert got["overlap"].tolist() == [r[1] for r in d]
    assert got["offset"].tolist() == [r[2] for r in d]
    b1, o1, q1, b2, o2, q2 = expected_reads(fmt)
    assert np.array_equal(got["offsets1"], o1) and np.array_equal(got["offsets2"], o2)
    assert np.array_equal(got["bases1"], b1) and np.array_equal(got["bases2"], b2)
    if q1 is not None:
        assert np.array_equal(got["qual1"], q1) and np.array_equal(got["qual2"], q2)
