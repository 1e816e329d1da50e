"""Loading of tests/golden/barcode (make_golden_barcode.py) and the random barcode sets of the GPU tests.  Everything is read or made
once per process and handed out as it is (callers copy what they change)."""
import functools
import gzip
import json
import os

import numpy as np

BARCODE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "barcode")
SEP = b"\x1f"


def flat(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:-1].copy(), offs


def unflat(bases, offs):
    raw = bytes(bases)
    return [raw[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def _lines(name):
    return gzip.open(os.path.join(BARCODE, name), "rb").read().split(b"\n")[:-1]


@functools.lru_cache(maxsize=None)
def manifest():
    return json.load(open(os.path.join(BARCODE, "manifest.json")))


def whitelist_path(name):
    return os.path.join(BARCODE, manifest()["whitelists"][name]["file"])


@functools.lru_cache(maxsize=None)
def background(name):
    return flat(_lines(name + ".background.tsv.gz"))


@functools.lru_cache(maxsize=None)
def counts(name):
    rows = [ln.split(b"\t") for ln in _lines(name + ".counts.tsv.gz")]
    return [r[0] for r in rows], [int(r[1]) for r in rows]


@functools.lru_cache(maxsize=None)
def barcodes(name):
    """(labels, bases, offsets, qualities)"""
    rows = [ln.split(b"\t") for ln in _lines(name + ".barcodes.tsv.gz")]
    b, o = flat([r[1] for r in rows])
    return [r[0].decode() for r in rows], b, o, flat([r[2] for r in rows])[0]


@functools.lru_cache(maxsize=None)
def corrected(name):
    """the reference's Correct: (status with qualities, barcodes after, status without, barcodes after)"""
    rows = [ln.split(b"\t") for ln in _lines(name + ".corrected.tsv.gz")]
    return [int(r[0]) for r in rows], [r[1] for r in rows], [int(r[2]) for r in rows], [r[3] for r in rows]


@functools.lru_cache(maxsize=None)
def formats():
    return json.load(open(os.path.join(BARCODE, "formats.json")))


@functools.lru_cache(maxsize=None)
def format_records():
    return [tuple(ln.split(SEP)) for ln in _lines("format_records.tsv.gz")]


def format_dump(entry):
    return [tuple(ln.split(SEP)) for ln in _lines(entry["file"])]


@functools.lru_cache(maxsize=None)
def translations():
    return [tuple(ln.split(b"\t")) for ln in _lines("translate.tsv.gz")]


# ---- random sets for the device tests: a whitelist with clusters at Hamming distance 1 and 2, barcodes of every class of the fixture
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def random_whitelist(L, n, seed=7):
    """n distinct entries of L bases (fewer when 4^L is smaller); every fourth is a neighbour of an earlier one at distance 1 or 2"""
    rng = np.random.default_rng(seed + 1000 * L + n)
    n = min(n, 4 ** L)
    seen, out = set(), []
    while len(out) < n:
        if out and len(out) % 4 == 3:
            e = bytearray(out[int(rng.integers(0, len(out)))])
            for _ in range(1 + int(rng.integers(0, 2))):
                e[int(rng.integers(0, L))] = ACGT[int(rng.integers(0, 4))]
            e = bytes(e)
        else:
            e = bytes(ACGT[rng.integers(0, 4, size=L)])
        if e not in seen:
            seen.add(e)
            out.append(e)
    return out


@functools.lru_cache(maxsize=None)
def random_barcodes(L, n_entries, n, seed=11):
    """(bases, offsets, qualities, number of barcodes whose length is not L)"""
    wl = random_whitelist(L, n_entries)
    rng = np.random.default_rng(seed + L + n_entries)
    cls = rng.integers(0, 16, size=n)
    pick = rng.integers(0, len(wl), size=n)
    out = []
    for k in range(n):
        e = bytearray(wl[pick[k]])
        c = cls[k]
        if c < 6:
            pass                                                    # exact
        elif c < 10:
            e[int(rng.integers(0, L))] = ACGT[int(rng.integers(0, 4))]       # one substitution (may fall back on the entry)
        elif c == 10:
            e[0 if k & 1 else L - 1] = ACGT[int(rng.integers(0, 4))]         # first / last position
        elif c == 11:
            e[int(rng.integers(0, L))] = ord("N")
        elif c == 12:
            e[int(rng.integers(0, L))] = ord("N"); e[int(rng.integers(0, L))] = ord("N" if k & 1 else "R")
        elif c == 13:
            e[int(rng.integers(0, L))] = ord("N"); e[int(rng.integers(0, L))] = ACGT[int(rng.integers(0, 4))]
        elif c == 14:
            e = bytearray(ACGT[rng.integers(0, 4, size=L)])                  # hopeless, mostly
        else:
            j = k % 4
            e = e[:int(rng.integers(0, L))] if j == 0 else bytearray() if j == 1 else e + bytes(ACGT[rng.integers(0, 4, size=1 + k % 3)]) if j == 2 else e
        out.append(bytes(e))
    b, o = flat(out)
    q = rng.integers(33, 43, size=len(b)).astype(np.uint8)          # ten values: ties at the changed positions are common
    return b, o, q, sum(1 for s in out if len(s) != L)


def write_whitelist(path, entries, repeats=0):
    with open(path, "wb") as f:
        f.write(b"\n".join(list(entries) + list(entries[:repeats])) + b"\n")
