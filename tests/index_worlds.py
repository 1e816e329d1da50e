"""Four small seeded index worlds whose text is NOT i.i.d. random DNA over a regular strain tree (what synth.make_genomes gives every
other test): `shared` (one block in 2 .. 60 sequences of different species and genera), `strands` (reverse-complemented blocks, an
inverted repeat, palindromes), `repeats` (tandem repeats, homopolymers) and `ragged` (sequences of 7 .. 30 000 bases under an irregular
taxonomy).  A helper module, not a conftest: tests/test_worlds_oracle_cpu.py and tests/test_gpu_worlds.py import it.

Each generator returns a World = (synth.Genomes, single-end ReadSet, (mate 1 ReadSet, mate 2 ReadSet), info dict).  Every text is below
150 kbp, a world has at most 1 500 single reads and 500 pairs, reads are 30 .. 300 bases long, every second read carries about 1 %
substitutions and a few carry an N or lower case.  No read is drawn within 300 bases of the two ends of the concatenated text (the
first 400 and the last 400 bases of every text are plain random bases that hold no planted feature).

guards(world, oracle, k) computes, from the C oracle alone, what the world claims to provoke and asserts it: a world that does not
provoke it fails instead of passing quietly."""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

from centrifuger_amd import synth

ACGT = synth.ACGT
EDGE = 300                        # no read starts or ends within this many bases of the text's two ends
MAX_TEXT, MAX_READS, MAX_PAIRS = 150_000, 1500, 500
QUERY_HITS_CAP = 4096             # the buffer of oracle_lib.OracleIndex.query_hits
HITK_FACTOR = 40                  # --hitk-factor default: a range above HITK_FACTOR x k rows is sampled by k_enum_rows
SHARED_COUNTS = (2, 3, 4, 5, 6, 23, 24, 25, 26, 60)
RAGGED_LENGTHS = (7, 8, 31, 32, 33, 63, 64, 65, 150, 151, 1000, 30000)
NAMES = ("shared", "strands", "repeats", "ragged")


class World(NamedTuple):
    genomes: synth.Genomes
    reads: synth.ReadSet
    pairs: tuple
    info: dict


# ------------------------------------------------------------------------------------------------ pieces
def _rand(rng, n):
    return ACGT[rng.integers(0, 4, size=int(n))]


def _regular_tree(n_genera, species_per_genus, strains_per_species):
    """genus 10, 20, .. -> species 11, 12, .. -> strain 1101, 1102, ..; returns nodes, names and the strain ids as [genus][species][strain]"""
    nodes = [(1, 1, "no rank"), (2, 1, "superkingdom")]
    names = [(1, "root"), (2, "Bacteria")]
    leaves = []
    for gi in range(n_genera):
        gt = 10 * (gi + 1)
        nodes.append((gt, 2, "genus")); names.append((gt, f"Genus{gi}"))
        leaves.append([])
        for si in range(species_per_genus):
            st = gt + si + 1
            nodes.append((st, gt, "species")); names.append((st, f"Genus{gi} species{si}"))
            leaves[-1].append([])
            for ti in range(strains_per_species):
                tt = st * 100 + ti + 1
                nodes.append((tt, st, "strain")); names.append((tt, f"species{st} strain{ti}"))
                leaves[-1][-1].append(tt)
    return nodes, names, leaves


class _Reads:
    """Collects reads; finish() mutates every second one, adds N / lower case to a few and returns a ReadSet."""

    def __init__(self, rng):
        self.rng, self.seqs, self.kind, self.exact = rng, [], [], []

    def add(self, s, kind, exact=False):
        s = np.ascontiguousarray(s, dtype=np.uint8)
        assert 30 <= len(s) <= 300, (kind, len(s))
        self.seqs.append(s.copy()); self.kind.append(kind); self.exact.append(exact)
        return len(self.seqs) - 1

    def finish(self, limit):
        rng = self.rng
        assert len(self.seqs) <= limit, len(self.seqs)
        for i, s in enumerate(self.seqs):
            if self.exact[i]:
                continue
            if i % 2 == 1:                                   # about 1 % substitutions
                m = rng.random(len(s)) < 0.01
                s[m] = ACGT[(np.searchsorted(ACGT, s[m]) + rng.integers(1, 4, size=int(m.sum()))) & 3]
            if i % 37 == 5:
                s[int(rng.integers(0, len(s)))] = ord("N")
            if i % 41 == 7:
                a = int(rng.integers(0, len(s) - 10))
                s[a:a + 10] |= 0x20                          # lower case
        offs = np.zeros(len(self.seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in self.seqs])
        return synth.ReadSet(np.concatenate(self.seqs), offs)


class _Text:
    """The concatenated text and the checked way to draw from it."""

    def __init__(self, seqs):
        self.cat = np.concatenate(seqs)
        self.n = len(self.cat)
        self.starts = np.zeros(len(seqs) + 1, dtype=np.int64)
        self.starts[1:] = np.cumsum([len(s) for s in seqs])
        assert self.n < MAX_TEXT, self.n

    def take(self, p, L, rc=False):
        p, L = int(p), int(L)
        assert EDGE <= p and p + L <= self.n - EDGE, (p, L, self.n)
        s = self.cat[p:p + L]
        return synth.revcomp(s) if rc else s.copy()

    def crossings(self, p, L):
        """sequence boundaries strictly inside the window [p, p + L)"""
        return int(np.searchsorted(self.starts, p + L - 1, side="right") - np.searchsorted(self.starts, p, side="right"))


def _background(t, reads, pairs, rng, n_reads, n_pairs, n_alien=24):
    """Windows of the text anywhere (both strands), reads that are in no index, and FR pairs of windows of the text."""
    for _ in range(n_reads):
        L = int(rng.integers(30, 301))
        reads.add(t.take(rng.integers(EDGE, t.n - EDGE - L + 1), L, rc=rng.random() < 0.5), "anywhere")
    for _ in range(n_alien):
        reads.add(_rand(rng, rng.integers(30, 301)), "alien")
    for j in range(n_pairs):
        L = int(rng.integers(30, 151))
        ins = int(rng.integers(L, 2 * L + 200))
        p = int(rng.integers(EDGE, t.n - EDGE - ins + 1))
        _add_pair(t, pairs, p, ins, L, flip=rng.random() < 0.5, kind="anywhere")
    for _ in range(8):
        pairs[0].add(_rand(rng, 100), "alien"); pairs[1].add(_rand(rng, 80), "alien")


def _add_pair(t, pairs, p, ins, L, flip, kind, L2=None):
    L2 = L if L2 is None else L2
    left, right = t.take(p, L), t.take(p + ins - L2, L2, rc=True)
    a, b = (right, left) if flip else (left, right)
    pairs[0].add(a, kind); pairs[1].add(b, kind)


def _finish(g, reads, pairs, info):
    r1, r2 = pairs
    info["read_kinds"] = list(reads.kind)
    info["pair_kinds"] = list(r1.kind)
    w = World(g, reads.finish(MAX_READS), (r1.finish(MAX_PAIRS), r2.finish(MAX_PAIRS)), info)
    assert w.pairs[0].n == w.pairs[1].n
    return w


# ------------------------------------------------------------------------------------------------ shared
def shared(seed=9101):
    """72 random sequences of 1.5 .. 3 kbp over 3 genera x 4 species x 6 strains; identical 400-base blocks planted in exactly c
    sequences for c in SHARED_COUNTS (for c <= 6: one block inside one species, one inside one genus, one across genera; the block of 23
    inside genus 0, the one of 24 is all of genus 1, the others span genera)."""
    rng = np.random.default_rng(seed)
    nodes, names, leaves = _regular_tree(3, 4, 6)
    where = [(gi, si) for gi in range(3) for si in range(4) for _ in range(6)]      # (genus, species) of sequence i
    taxids = [t for gen in leaves for sp in gen for t in sp]
    nseq = len(taxids)
    load = np.zeros(nseq, dtype=np.int64)
    load[0] = load[-1] = 2                                                           # the two sequences that get 400 more plain bases hold fewer blocks
    blocks = []                                                                    # (c, scope, [sequence numbers])

    def choose(c, allowed):
        allowed = np.array(allowed)
        order = allowed[np.lexsort((rng.random(len(allowed)), load[allowed]))]       # least loaded first, ties at random
        pick = sorted(int(x) for x in order[:c])
        assert len(pick) == c
        load[pick] += 1
        return pick
    k = 0
    for c in SHARED_COUNTS:
        if c <= 6:
            gi, si = k % 3, k % 4
            k += 1
            blocks.append((c, "species", choose(c, [i for i in range(nseq) if where[i] == (gi, si)])))
            blocks.append((c, "genus", choose(c, [i for i in range(nseq) if where[i][0] == (gi + 1) % 3])))
            pick = choose(c - 1, [i for i in range(nseq) if where[i][0] != gi]) + choose(1, [i for i in range(nseq) if where[i][0] == gi])
            blocks.append((c, "genera", sorted(pick)))
        elif c == 23:
            blocks.append((c, "genus", choose(c, [i for i in range(nseq) if where[i][0] == 0])))
        elif c == 24:
            blocks.append((c, "genus", choose(c, [i for i in range(nseq) if where[i][0] == 1])))
        else:
            blocks.append((c, "genera", choose(c, list(range(nseq)))))
    assert load.max() <= 5
    for c, scope, pick in blocks:
        assert len(set(pick)) == c
        assert (len({where[i][0] for i in pick}) > 1) == (scope == "genera")
    content = [_rand(rng, 400) for _ in blocks]
    seqs, at = [], {}                                                                # at[(block, sequence)] = offset in the sequence
    for i in range(nseq):
        mine = [b for b, (_, _, pick) in enumerate(blocks) if i in pick]
        rng.shuffle(mine)
        gaps = [int(rng.integers(100, 161)) for _ in range(len(mine) + 1)]
        if i == 0: gaps[0] += 400
        if i == nseq - 1: gaps[-1] += 400
        short = 1500 - (sum(gaps) + 400 * len(mine))
        if short > 0:
            gaps[int(rng.integers(0, len(gaps)))] += short + int(rng.integers(0, 200))
        parts, pos = [], 0
        for j, b in enumerate(mine):
            parts.append(_rand(rng, gaps[j])); pos += gaps[j]
            at[(b, i)] = pos
            parts.append(content[b]); pos += 400
        parts.append(_rand(rng, gaps[-1]))
        seqs.append(np.concatenate(parts))
        assert 1500 <= len(seqs[-1]) <= 3000, len(seqs[-1])
    g = synth.Genomes([f"SH_{i:03d}.1" for i in range(nseq)], taxids, seqs, nodes, names)
    t = _Text(seqs)
    reads, pairs = _Reads(rng), (_Reads(rng), _Reads(rng))
    for b, (c, scope, pick) in enumerate(blocks):
        occ = [int(t.starts[i]) + at[(b, i)] for i in pick]                          # text positions of the block
        for j in range(10):                                                          # fully inside, both orientations
            L = int(rng.integers(30, 301))
            reads.add(t.take(occ[j % c] + rng.integers(0, 400 - L + 1), L, rc=j % 2 == 1), "inside")
        for j in range(8):                                                           # >= 40 bases of a unique flank, then into the block
            o = occ[int(rng.integers(0, c))]
            a, inb = int(rng.integers(40, 91)), int(rng.integers(30, 201))
            reads.add(t.take(o - a, a + inb, rc=j % 4 >= 2), "flank_into_block")
            reads.add(t.take(o + 400 - inb, inb + a, rc=j % 4 >= 2), "block_into_flank")
        for j in range(6):                                                           # inside, one substitution
            L = int(rng.integers(60, 301))
            s = t.take(occ[j % c] + rng.integers(0, 400 - L + 1), L, rc=j % 2 == 1)
            q = int(rng.integers(10, L - 10))
            s[q] = ACGT[(int(np.searchsorted(ACGT, s[q])) + 1 + int(rng.integers(0, 3))) & 3]
            reads.add(s, "inside_one_substitution", exact=True)
        o = occ[0]
        _add_pair(t, pairs, o - 60, 460, 100, flip=b % 2 == 1, kind="block_and_flank")
        _add_pair(t, pairs, o + 20, 360, 120, flip=b % 2 == 0, kind="inside")
    _background(t, reads, pairs, rng, n_reads=300, n_pairs=300)
    return _finish(g, reads, pairs, {"name": "shared", "ftab_chars": 10, "blocks": [(c, scope, list(pick)) for c, scope, pick in blocks]})


# ------------------------------------------------------------------------------------------------ strands
def strands(seed=9102):
    """20 sequences of 3 .. 6 kbp (2 genera x 2 species x 5 strains).  The reverse complement of a 2 kbp block of sequence 1 is planted
    in sequence 2 (same species) and in sequence 12 (other genus); sequence 4 holds an inverted repeat (300 bases, and their reverse
    complement 900 bases on); palindromes s + revcomp(s) of 40, 100, 150 and 300 bases sit in sequences 5 .. 8."""
    rng = np.random.default_rng(seed)
    nodes, names, leaves = _regular_tree(2, 2, 5)
    taxids = [t for gen in leaves for sp in gen for t in sp]
    seqs = [_rand(rng, rng.integers(3000, 6001)) for _ in taxids]
    block = seqs[1][600:2600].copy()
    seqs[2][400:2400] = synth.revcomp(block)
    seqs[12][700:2700] = synth.revcomp(block)
    seqs[4][1400:1700] = synth.revcomp(seqs[4][500:800])
    pal_at = {}
    for i, plen in zip((5, 6, 7, 8), (40, 100, 150, 300)):
        half = _rand(rng, plen // 2)
        seqs[i][1000:1000 + plen] = np.concatenate([half, synth.revcomp(half)])
        pal_at[plen] = i
    g = synth.Genomes([f"ST_{i:02d}.1" for i in range(len(seqs))], taxids, seqs, nodes, names)
    t = _Text(seqs)
    reads, pairs = _Reads(rng), (_Reads(rng), _Reads(rng))
    rc_pairs = []
    b0 = int(t.starts[1]) + 600
    for j in range(300):                                                             # reads of the block, both orientations
        L = int(rng.integers(30, 301))
        reads.add(t.take(b0 + rng.integers(0, 2000 - L + 1), L, rc=j % 2 == 1), "block")
    for j in range(40):                                                              # a read and its reverse complement, unchanged
        L = int(rng.integers(40, 301))
        p = b0 + int(rng.integers(0, 2000 - L + 1))
        rc_pairs.append((reads.add(t.take(p, L), "block_twin", exact=True), reads.add(t.take(p, L, rc=True), "block_twin", exact=True)))
    for j in range(40):                                                              # across the block's edges in the three sequences
        for si, off in ((1, 600), (2, 400), (12, 700)):
            e = int(t.starts[si]) + off + (2000 if j % 2 else 0)
            L = int(rng.integers(60, 301))
            reads.add(t.take(e - rng.integers(20, L - 19), L, rc=j % 4 >= 2), "block_edge")
    ir = int(t.starts[4])
    for j in range(80):                                                              # the inverted repeat: inside an arm, and across an arm's edge
        L = int(rng.integers(30, 281))
        arm = ir + (500 if j % 2 else 1400)
        p = arm + int(rng.integers(0, 300 - L + 1)) if j % 4 < 2 and L <= 300 else arm - int(rng.integers(10, 60))
        reads.add(t.take(p, L, rc=j % 8 >= 4), "inverted_repeat")
    for plen, si in pal_at.items():
        p0 = int(t.starts[si]) + 1000
        if plen >= 30:
            for _ in range(3):
                reads.add(t.take(p0, plen), "palindrome_exact", exact=True)          # equal to its own reverse complement
        for j in range(30):                                                          # with flanks on either or both sides
            a = int(rng.integers(0, 80)) if j % 3 != 1 else 0
            b = int(rng.integers(0, 80)) if j % 3 != 2 else 0
            if plen + a + b < 30: a += 30
            L = min(300, plen + a + b)
            reads.add(t.take(p0 - a, L, rc=j % 2 == 1), "palindrome_flanked")
        for j in range(10):                                                          # a window that holds the centre but not the whole palindrome
            L = int(rng.integers(30, max(31, plen)))
            c0 = p0 + plen // 2 - int(rng.integers(5, L - 4))
            reads.add(t.take(c0, L, rc=j % 2 == 1), "palindrome_centre")
    for j in range(100):                                                             # mates that overlap
        L = int(rng.integers(50, 151))
        ins = int(rng.integers(L, 2 * L))
        p = int(rng.integers(EDGE, t.n - EDGE - ins + 1)) if j % 2 else b0 + int(rng.integers(0, 2000 - ins + 1))
        _add_pair(t, pairs, p, ins, L, flip=j % 4 >= 2, kind="overlapping_mates")
    for j in range(120):                                                             # both mates inside the reverse-complemented block
        L = int(rng.integers(30, 151))
        ins = int(rng.integers(2 * L, 2 * L + 300))
        base = (b0, int(t.starts[2]) + 400, int(t.starts[12]) + 700)[j % 3]
        _add_pair(t, pairs, base + int(rng.integers(0, 2000 - ins + 1)), ins, L, flip=j % 2 == 1, kind="both_mates_in_block")
    for plen, si in pal_at.items():
        p0 = int(t.starts[si]) + 1000
        for j in range(5):
            _add_pair(t, pairs, p0 - 40 - 10 * j, plen + 120, max(30, min(150, plen // 2 + 50)), flip=j % 2 == 1, kind="palindrome")
    _background(t, reads, pairs, rng, n_reads=300, n_pairs=200)
    return _finish(g, reads, pairs, {"name": "strands", "ftab_chars": 10, "rc_pairs": rc_pairs})


# ------------------------------------------------------------------------------------------------ repeats
REPEATS = ((1, 400), (2, 600), (3, 1200), (4, 600), (7, 1400), (50, 2000))           # (period, length)


def repeats(seed=9103):
    """16 sequences of 4 .. 8 kbp (2 genera x 2 species x 4 strains): tandem repeats of period 1, 2, 3, 4, 7 and 50 (REPEATS) in
    sequences 0 .. 5, a 1 kbp poly-A in sequence 6 (species 11) and a 1 kbp poly-T in sequence 13 (species 22, the other genus),
    all between random flanks."""
    rng = np.random.default_rng(seed)
    nodes, names, leaves = _regular_tree(2, 2, 4)
    taxids = [t for gen in leaves for sp in gen for t in sp]
    seqs = [_rand(rng, rng.integers(4000, 8001)) for _ in taxids]
    spans = []                                                                       # (label, sequence, offset, length, period)
    for i, (period, length) in enumerate(REPEATS):
        unit = np.frombuffer(b"G", dtype=np.uint8) if period == 1 else _rand(rng, period)
        while period > 1 and any((unit == np.roll(unit, s)).all() for s in range(1, period)):
            unit = _rand(rng, period)                                                # a unit with a shorter period is not this period
        seqs[i][1500:1500 + length] = np.tile(unit, length // period + 1)[:length]
        spans.append((f"period{period}", i, 1500, length, period))
    seqs[6][1500:2500] = ord("A"); spans.append(("poly_a", 6, 1500, 1000, 1))
    seqs[13][1500:2500] = ord("T"); spans.append(("poly_t", 13, 1500, 1000, 1))
    g = synth.Genomes([f"RP_{i:02d}.1" for i in range(len(seqs))], taxids, seqs, nodes, names)
    t = _Text(seqs)
    reads, pairs = _Reads(rng), (_Reads(rng), _Reads(rng))
    for label, si, off, length, period in spans:
        p0 = int(t.starts[si]) + off
        for j in range(60):                                                          # inside the repeat
            L = int(rng.integers(30, min(300, length - 40) + 1))
            reads.add(t.take(p0 + rng.integers(0, length - L + 1), L, rc=j % 2 == 1), "inside_" + label)
        for j in range(40):                                                          # across an edge into the flank
            L = int(rng.integers(60, 301))
            inside = int(rng.integers(20, L - 19))
            p = p0 - (L - inside) if j % 2 else p0 + length - inside
            reads.add(t.take(p, L, rc=j % 4 >= 2), "edge_" + label)
        for j in range(12):
            L = int(rng.integers(40, 121))
            _add_pair(t, pairs, p0 - 150 + 40 * j, L + int(rng.integers(60, 300)), L, flip=j % 2 == 1, kind="around_" + label)
    _background(t, reads, pairs, rng, n_reads=300, n_pairs=200)
    return _finish(g, reads, pairs, {"name": "repeats", "ftab_chars": 10, "spans": spans})


# ------------------------------------------------------------------------------------------------ ragged
def ragged(seed=9104):
    """Sequences of RAGGED_LENGTHS bases plus 60 of 340 .. 700 bases that share one 300-base block, written with ftab_chars = 6 (so that
    a 7-base sequence is kept), under an irregular taxonomy: sequences attached to a genus, a species, a strain, a "no rank" node below
    a strain, the superkingdom and the root.  Text order: the 1 000-base sequence, 30 of the sixty, 150, 151, the other 30, then 7, 8,
    31, 32, 33, 63, 64, 65 right in front of the 30 000-base one."""
    rng = np.random.default_rng(seed)
    nodes = [(1, 1, "no rank"), (2, 1, "superkingdom"), (10, 2, "genus"), (11, 10, "species"), (111, 11, "strain"), (1111, 111, "no rank"),
             (20, 2, "genus"), (21, 20, "species"), (211, 21, "strain")]
    names = [(1, "root"), (2, "Bacteria"), (10, "Alpha"), (11, "Alpha one"), (111, "Alpha one str"), (1111, "Alpha one str isolate"),
             (20, "Beta"), (21, "Beta one"), (211, "Beta one str")]
    tax_of_len = {7: 111, 8: 1111, 31: 2, 32: 1, 33: 211, 63: 10, 64: 1111, 65: 21, 150: 111, 151: 2, 1000: 1, 30000: 211}
    block = _rand(rng, 300)
    mids = []
    for j in range(60):
        L = int(rng.integers(340, 701))
        s = _rand(rng, L)
        off = int(rng.integers(20, L - 300 - 19))
        s[off:off + 300] = block
        mids.append((s, (10, 11, 20, 21)[j % 4], off))
    order = ([("len", 1000)] + [("mid", j) for j in range(30)] + [("len", 150), ("len", 151)] + [("mid", j) for j in range(30, 60)]
             + [("len", L) for L in (7, 8, 31, 32, 33, 63, 64, 65, 30000)])
    seqs, taxids, seq_names, block_at = [], [], [], []
    for what, v in order:
        if what == "len":
            seqs.append(_rand(rng, v)); taxids.append(tax_of_len[v]); seq_names.append(f"RG_len{v}.1")
        else:
            s, tid, off = mids[v]
            block_at.append((len(seqs), off))
            seqs.append(s); taxids.append(tid); seq_names.append(f"RG_mid{v:02d}.1")
    assert sorted(len(s) for s in seqs if len(s) < 340 or len(s) > 700) == sorted(RAGGED_LENGTHS) and len(block_at) == 60
    g = synth.Genomes(seq_names, taxids, seqs, nodes, names)
    t = _Text(seqs)
    reads, pairs = _Reads(rng), (_Reads(rng), _Reads(rng))
    crossed = []

    def window(p, L, rc, kind, to=reads):
        crossed.append(t.crossings(p, L))
        to.add(t.take(p, L, rc=rc), kind)
    tiny0 = int(t.starts[len(seqs) - 9])                                            # start of the run 7, 8, 31, .. in front of the 30 kbp sequence
    tiny1 = int(t.starts[len(seqs) - 1])
    for j in range(200):                                                             # windows over the run of short sequences: 1 .. 8 boundaries
        L = int(rng.integers(30, 301))
        window(int(rng.integers(tiny0 - L + 2, tiny1 - 1)), L, j % 2 == 1, "short_run")
    for j in range(500):                                                             # windows over the boundaries of the sixty and of 150 / 151
        b = int(t.starts[int(rng.integers(2, len(seqs) - 9))])
        L = int(rng.integers(30, 301))
        window(b - int(rng.integers(1, L)), L, j % 2 == 1, "boundary")
    for si, s in enumerate(seqs):                                                    # whole short sequences (30 bases and more: a read's shortest)
        if 30 <= len(s) <= 300:
            for rc in (False, True):
                window(int(t.starts[si]), len(s), rc, "whole_sequence")
    for j in range(150):                                                             # the shared block
        si, off = block_at[j % 60]
        L = int(rng.integers(30, 301))
        window(int(t.starts[si]) + off + int(rng.integers(0, 300 - L + 1)), L, j % 2 == 1, "shared_block")
    for j in range(150):                                                             # the 30 kbp sequence
        L = int(rng.integers(30, 301))
        window(int(rng.integers(tiny1, t.n - EDGE - L + 1)), L, j % 2 == 1, "long_sequence")
    for j in range(150):                                                             # pairs over the short run and over boundaries
        L = int(rng.integers(30, 121))
        ins = int(rng.integers(L, 2 * L + 150))
        p = int(rng.integers(tiny0 - ins + 2, tiny1 - 1)) if j % 2 else int(t.starts[int(rng.integers(2, len(seqs) - 9))]) - int(rng.integers(1, ins))
        _add_pair(t, pairs, p, ins, L, flip=j % 4 >= 2, kind="boundary")
    n_before = len(reads.seqs)
    _background(t, reads, pairs, rng, n_reads=200, n_pairs=250)
    crossed += [0] * (len(reads.seqs) - n_before)                                    # (not counted: the guard needs a lower bound only)
    return _finish(g, reads, pairs, {"name": "ragged", "ftab_chars": 6, "crossings": crossed})


GENERATORS = {"shared": shared, "strands": strands, "repeats": repeats, "ragged": ragged}


def make(name) -> World:
    w = GENERATORS[name]()
    assert w.genomes.total_len < MAX_TEXT and w.reads.n <= MAX_READS and w.pairs[0].n <= MAX_PAIRS
    lens = np.concatenate([np.diff(r.offsets.astype(np.int64)) for r in (w.reads,) + tuple(w.pairs)])
    assert lens.min() >= 30 and lens.max() <= 300
    return w


def build_kwargs(world):
    return {"ftab_chars": world.info["ftab_chars"]}


def write_reads(world, d):
    """se.fq, p_1.fq, p_2.fq under d (ids r0, r1, ..)"""
    synth.write_fastq(world.reads, os.path.join(d, "se.fq"))
    synth.write_fastq(world.pairs[0], os.path.join(d, "p_1.fq"), suffix="/1")
    synth.write_fastq(world.pairs[1], os.path.join(d, "p_2.fq"), suffix="/2")


# ------------------------------------------------------------------------------------------------ guards
def hit_lists(world, oracle):
    """the oracle's hit list of every single read and of every pair (they do not depend on -k)"""
    out = {"se": [], "pe": []}
    rs = world.reads
    for i in range(rs.n):
        out["se"].append(oracle.query_hits(rs.get(i), None, cap=QUERY_HITS_CAP))
    r1, r2 = world.pairs
    for i in range(r1.n):
        out["pe"].append(oracle.query_hits(r1.get(i), r2.get(i), cap=QUERY_HITS_CAP))
    return out


def _matches(r):
    return [(int(r.kind[q]), int(r.id[q]), int(r.taxid[q])) for q in range(r.nmatch)]


def guards(world, oracle, k, hits=None):
    """Asserts what the world must provoke, from the oracle's answers alone (oracle: oracle_lib.OracleIndex opened with max_result = k
    on an index of this world; hits: hit_lists(world, oracle) if the caller holds them already).  Returns the values reached."""
    info = world.info
    name = info["name"]
    assert 1 <= k <= 64 and oracle.param.maxResult == k                              # ORA_MAX_MATCH: the oracle's result holds 64 matches
    assert oracle.param.maxResultPerHitFactor == HITK_FACTOR
    rank_of = {tid: rank for tid, _, rank in world.genomes.nodes}
    hits = hit_lists(world, oracle) if hits is None else hits
    reached = {"most_hits_of_one_read": max(len(h) for hs in hits.values() for h in hs)}
    assert reached["most_hits_of_one_read"] <= QUERY_HITS_CAP                        # (query_hits itself asserts that the list fitted)
    rs, (r1, r2) = world.reads, world.pairs
    se = oracle.classify(rs.bases, rs.offsets, threads=4)
    pe = oracle.classify(r1.bases, r1.offsets, r2.bases, r2.offsets, threads=4)
    for tag, res, n in (("se", se, rs.n), ("pe", pe, r1.n)):
        classified = sum(1 for i in range(n) if res[i].nmatch > 0)
        reached[f"classified_{tag}"] = (classified, n)
        assert classified < n, f"{name} {tag}: no read is unclassified"
        assert 2 * classified > n, f"{name} {tag}: only {classified} of {n} classified"
    sizes = {}
    for h in hits["se"]:
        for x in (h["ep"] - h["sp"] + 1).tolist():
            sizes[x] = sizes.get(x, 0) + 1
    if name == "shared":
        reached["range_sizes"] = {c: sizes.get(c, 0) for c in SHARED_COUNTS}
        assert all(sizes.get(c, 0) > 0 for c in SHARED_COUNTS), reached["range_sizes"]
        if k == 1:
            levels = {}
            for i in range(rs.n):
                for _, _, tid in _matches(se[i]):
                    levels[rank_of[tid]] = levels.get(rank_of[tid], 0) + 1
            reached["levels_k1"] = levels
            assert levels.get("strain", 0) + levels.get("species", 0) > 0 and levels.get("genus", 0) > 0 and levels.get("superkingdom", 0) > 0, levels
        if k == 5:
            reached["reads_with_2_matches_or_more"] = sum(1 for i in range(rs.n) if se[i].nmatch >= 2)
            assert reached["reads_with_2_matches_or_more"] >= 1
    if name == "strands":
        def tied(h):                                                                 # hits on both strands, of equal summed length
            one = h["strand"] == h["strand"][0]
            return not one.all() and int(h["l"][one].sum()) == int(h["l"][~one].sum())
        reached["reads_tied_between_strands"] = sum(1 for h in hits["se"] if len(h) and tied(h))
        assert reached["reads_tied_between_strands"] >= 50
        if k == 5:
            flipped = [(i, j) for i, j in info["rc_pairs"] if _matches(se[i]) != _matches(se[j]) and sorted(_matches(se[i])) == sorted(_matches(se[j]))]
            reached["twins_with_other_match_order"] = len(flipped)
            assert flipped, "no read whose -k 5 match order differs from that of its reverse complement"
    if name == "repeats":
        big = sum(1 for h in hits["se"] if len(h) and int((h["ep"] - h["sp"] + 1).max()) > HITK_FACTOR * 5)
        mid = sum(1 for h in hits["se"] if len(h) and bool(((h["ep"] - h["sp"] + 1 > HITK_FACTOR) & (h["ep"] - h["sp"] + 1 <= HITK_FACTOR * 5)).any()))
        reached["reads_with_range_above_200"], reached["reads_with_range_41_to_200"] = big, mid
        reached["largest_range"] = max(sizes)
        if k == 5:
            assert big >= 20 and mid >= 20, (big, mid)
    if name == "ragged":
        cr = np.array(info["crossings"])
        reached["reads_crossing_boundaries"] = {b: int((cr == b).sum()) for b in range(1, 9) if (cr == b).any()}
        assert int((cr == 1).sum()) >= 100 and int((cr == 3).sum()) >= 10, reached["reads_crossing_boundaries"]
        if k == 5:
            mixed = sum(1 for i in range(rs.n) if len({rank_of[tid] for _, _, tid in _matches(se[i])}) > 1)
            reached["results_with_matches_of_different_ranks"] = mixed
            assert mixed >= 1
    return reached
