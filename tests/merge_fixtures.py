"""Loading of tests/golden/merge and tests/golden/merge_long (make_golden_merge.py): the pairs, the reference's dump of the merged
reads and its TSVs; `which` picks the set ("merge" where it is left out).  Everything is read once per process and handed out as it
is (callers copy what they change).  Also the pairs that sit exactly on IsMateOverlap's similarity threshold (threshold_pair),
shared by the generator of merge_long and the device sweep."""
import functools
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MERGE = os.path.join(GOLDEN, "merge")
MERGE_LONG = os.path.join(GOLDEN, "merge_long")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.full(256, ord("N"), dtype=np.uint8)
_COMP[_ACGT] = _ACGT[::-1]


def _dir(which):
    return os.path.join(GOLDEN, which)


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
def pairs(fmt, which="merge"):
    """fmt 'fq' / 'fa' -> dict ids, b1, o1, q1, b2, o2, q2 (q* None for 'fa')"""
    ids, b1, o1, q1 = _read(os.path.join(_dir(which), f"pairs_1.{fmt}.gz"))
    _, b2, o2, q2 = _read(os.path.join(_dir(which), f"pairs_2.{fmt}.gz"))
    return {"ids": ids, "b1": b1, "o1": o1, "q1": q1, "b2": b2, "o2": o2, "q2": q2}


@functools.lru_cache(maxsize=None)
def dump(fmt, which="merge"):
    """the reference's ReadPairMerger on the set: list of (kind, overlap, offset, why, rm, qm)"""
    rows = [ln.split(b"\t") for ln in gzip.open(os.path.join(_dir(which), f"merged_{fmt}.tsv.gz"), "rb").read().split(b"\n")[:-1]]
    return [(int(r[0]), int(r[1]), int(r[2]), r[3], r[4], r[5]) for r in rows]


@functools.lru_cache(maxsize=None)
def manifest(which="merge"):
    return json.load(open(os.path.join(_dir(which), "manifest.json")))


def golden(name, which="merge"):
    return gzip.open(os.path.join(_dir(which), name + ".gz"), "rb").read()


def tsv(case, which="merge"):
    return golden(os.path.join("tsv", case + ".tsv"), which)


@functools.lru_cache(maxsize=None)
def expected_reads(fmt, which="merge"):
    """what a merge must hand on, from the reference's dump: (b1, o1, q1, b2, o2, q2) with read 1 = merged read, read 2 = empty for
    every merged pair and the pair as it is otherwise"""
    p, d = pairs(fmt, which), dump(fmt, which)
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


def check_against_dump(fmt, got, which="merge"):
    """got: the dict capi.merge_pairs / DeviceIndex.merge_pairs return"""
    d = dump(fmt, which)
    assert got["kind"].tolist() == [r[0] for r in d]
    assert got["overlap"].tolist() == [r[1] for r in d]
    assert got["offset"].tolist() == [r[2] for r in d]
    b1, o1, q1, b2, o2, q2 = expected_reads(fmt, which)
    assert np.array_equal(got["offsets1"], o1) and np.array_equal(got["offsets2"], o2)
    assert np.array_equal(got["bases1"], b1) and np.array_equal(got["bases2"], b2)
    if q1 is not None:
        assert np.array_equal(got["qual1"], q1) and np.array_equal(got["qual2"], q2)


def threshold(L):
    """T(L) = int(L * similarityThreshold) of IsMateOverlap (ReadPairMerger.hpp:26-36) for L = flen - j, in Python floats (IEEE
    double, the reference's type and order of operations); on purpose not taken from the library's merge_threshold_table"""
    t = 0.95
    if L >= 100:
        t = 0.85
    elif L >= 50:
        t = 0.85 + (L - 50) / 50.0 * 0.1
    return int(L * t)


def threshold_pair(frag, L, read_through, j, e, nsub, packed, tails):
    """A pair whose only candidate is an overlap of exactly L compared bases (L = flen - j = K) with exactly nsub substitutions on
    it: nsub = L - threshold(L) is the last count that passes, one more the first that does not.
      plain pass (first sequence r1):          r1 = frag[:j + L], rc(r2) = frag[j:j + L + e]; j >= 1 (at j = 0 the read-through
                                               pass would see the same overlap first)
      read-through pass (first sequence rc(r2)): r1 = frag[:L] + e adapter bases, rc(r2) = j adapter bases + frag[:L]; j >= 1, or
                                               j = e = 0 (else the plain pass takes a failed pair at its own, longer L)
    frag: upper-case ACGT, at least j + L + e bases; tails: at least j + e more bases for the adapters.  Substitutions alternate
    between the mates; spread evenly over the overlap (every 64-position word of it gets some), or packed into its last positions."""
    assert nsub <= L and len(frag) >= j + L + e and len(tails) >= j + e
    if read_through:
        r1 = np.concatenate([frag[:L], tails[:e]]).astype(np.uint8)
        rc = np.concatenate([tails[e:e + j], frag[:L]]).astype(np.uint8)
        a1, a2 = 0, j                                   # overlap position k is r1[a1 + k] and rc[a2 + k]
    else:
        r1 = frag[:j + L].astype(np.uint8).copy()
        rc = frag[j:j + L + e].astype(np.uint8).copy()
        a1, a2 = j, 0
    pos = np.arange(L - nsub, L) if packed else ((2 * np.arange(nsub) + 1) * L) // (2 * max(nsub, 1))
    assert len(set(pos.tolist())) == nsub
    for i, k in enumerate(pos.tolist()):
        r, a = (r1, a1) if i % 2 == 0 else (rc, a2)
        r[a + k] = _ACGT[(int(np.nonzero(_ACGT == r[a + k])[0][0]) + 1 + i % 3) & 3]
    return r1, _COMP[rc[::-1]].copy()
