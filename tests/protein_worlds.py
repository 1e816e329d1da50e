"""Four small seeded protein worlds for the translated search (k_translate_prot, k_search_prot_sm / k_search_prot, k_select_prot and the
protein branch of the post stage), whose proteomes are NOT i.i.d. random residues under a regular tree (what tests/golden/prot is):
`shared` (one 120-residue block in exactly 2 .. 40 proteins, copies of the 5- and 6-copy blocks differing in single residues), `repeats`
(homopolymers, tandem repeats), `ragged` (proteins of 3 .. 5 000 residues under an irregular taxonomy) and `frames` (DNA reads that hold
indexed segments in two frames or on two strands, with scores at the edges of the frame and strand rules).  A helper module, not a
conftest: tests/test_protein_worlds_oracle_cpu.py, tests/test_gpu_protein_worlds.py and tests/test_gpu_protein_chains.py import it.

A world = (synth.Genomes whose seqs are amino-acid letters, single-end DNA ReadSet, (mate 1, mate 2), info dict).  Every proteome is
below 60 000 residues; its first and last protein are 400 random residues from which no read is drawn, so no read comes from within
300 residues of the text's two ends.  Planted segments are written into a read between two stop codons (TAA): the search of a chain can
neither run past a stop codon nor start inside a segment, so a planted segment of m residues gives a hit of exactly m.

guards(world, oracle, k) asserts from the C oracle's hit lists alone what the world claims to provoke: a category that no read reaches
fails the world."""
from __future__ import annotations

import itertools
import os
from typing import NamedTuple

import numpy as np

from centrifuger_amd import synth

AA = np.frombuffer(b"ARNDCEQGHILKMFPSTWYV", dtype=np.uint8)
# the standard genetic code, codons in the order AAA, AAC, AAG, AAT, ACA, ..  ('_' = stop)
_CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV_Y_YSSSS_CWCLFLF"
CODONS = {}
for _i, (_a, _b, _c) in enumerate(itertools.product("ACGT", repeat=3)):
    CODONS.setdefault(_CODE[_i], []).append((_a + _b + _c).encode())
STOP = b"TAA"
MAX_RESIDUES = 60_000
PAD = 400                         # the first and the last protein: random residues, no read is drawn from them
QUERY_HITS_CAP = 4096
HITK_FACTOR = 40                  # --hitk-factor default: a range above HITK_FACTOR x k rows is sampled
MIN_HIT_LEN = 11                  # what InferMinHitLen gives a protein index of this size
SIGMA = 21                        # '$' and the twenty amino acids
SHARED_COUNTS = (2, 3, 4, 5, 6, 12, 40)
VARIANT_DISTANCES = (6, 7, 8, 9, 16, 1)      # one per 5- and 6-copy block: residues between the 5 -> 4 and the 4 -> 1 narrowing
RAGGED_LENGTHS = (3, 5, 8, 11, 12, 13, 52, 53, 63, 64, 65, 150, 1000, 5000)      # 3 = ftab_chars + 1
CHAIN_CODES = (52, 53, 63, 64, 65, 76)
SHORT_READS = (32, 33, 35, 36)    # chains of 10, 11, 11 and 12 codes: below and at MIN_HIT_LEN
LONG_READS = (600, 3000)
NAMES = ("shared", "repeats", "ragged", "frames")


class World(NamedTuple):
    genomes: synth.Genomes
    reads: synth.ReadSet
    pairs: tuple
    info: dict


def text_min_l(n):
    """after how many matched residues the device's search may continue on the text: log_sigma(n) rounded down, + 2"""
    ls, x = 0, float(n)
    while x >= SIGMA:
        x /= SIGMA
        ls += 1
    return ls + 2


# ------------------------------------------------------------------------------------------------ pieces
def _rand(rng, n):
    return AA[rng.integers(0, 20, size=int(n))]


def _other(rng, a):
    """a residue that is not a"""
    return AA[(int(np.nonzero(AA == a)[0][0]) + 1 + int(rng.integers(0, 19))) % 20]


def revtrans(rng, seg):
    return b"".join(CODONS[chr(a)][int(rng.integers(len(CODONS[chr(a)])))] for a in bytes(seg))


def revcomp(d: bytes) -> bytes:
    return synth.revcomp(np.frombuffer(d, dtype=np.uint8)).tobytes()


def wrapped(rng, seg):
    """the segment between two stop codons: a hit of exactly len(seg) residues"""
    return STOP + revtrans(rng, seg) + STOP


def _bases(rng, n):
    return bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=int(n)))


def _regular_tree(n_genera, species_per_genus, strains_per_species):
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
            leaves[-1].append([st * 100 + ti + 1 for ti in range(strains_per_species)])
            for ti, tt in enumerate(leaves[-1][-1]):
                nodes.append((tt, st, "strain")); names.append((tt, f"species{st} strain{ti}"))
    return nodes, names, leaves


class _Reads:
    """Collects DNA reads; finish() gives every second one that is not `exact` about 1 % substitutions, a few an N or lower case."""

    def __init__(self, rng):
        self.rng, self.seqs, self.kind, self.exact = rng, [], [], []

    def add(self, d: bytes, kind, exact=False):
        self.seqs.append(np.frombuffer(bytes(d), dtype=np.uint8).copy()); self.kind.append(kind); self.exact.append(exact)
        return len(self.seqs) - 1

    def finish(self):
        rng = self.rng
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        for i, s in enumerate(self.seqs):
            if self.exact[i] or len(s) < 12:
                continue
            if i % 2 == 1:
                m = rng.random(len(s)) < 0.01
                s[m] = acgt[rng.integers(0, 4, size=int(m.sum()))]
            if i % 37 == 5:
                s[int(rng.integers(0, len(s)))] = ord("N")
            if i % 41 == 7:
                a = int(rng.integers(0, len(s) - 10))
                s[a:a + 10] |= 0x20
        offs = np.zeros(len(self.seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in self.seqs])
        return synth.ReadSet(np.concatenate(self.seqs) if self.seqs else np.zeros(0, dtype=np.uint8), offs)


class _Pool:
    """the proteins reads may be drawn from (never the two padding proteins)"""

    def __init__(self, prots, rng):
        self.prots, self.rng = prots, rng
        self.usable = [i for i in range(1, len(prots) - 1)]

    def window(self, naa):
        rng = self.rng
        ok = [i for i in self.usable if len(self.prots[i]) >= naa]
        i = ok[int(rng.integers(len(ok)))]
        a = int(rng.integers(0, len(self.prots[i]) - naa + 1))
        return self.prots[i][a:a + naa]

    def composite(self, naa):
        """naa residues: windows of 25 .. 60 residues of any usable proteins, one after the other"""
        parts, left = [], naa
        while left > 0:
            L = min(left, int(self.rng.integers(25, 61)))
            if left - L < 12: L = left
            longest = max(len(self.prots[i]) for i in self.usable)
            parts.append(self.window(min(L, longest)))
            left -= len(parts[-1])
        return parts


def dna_of(rng, seg, frame=0, tail=0, rc=False):
    d = _bases(rng, frame) + revtrans(rng, seg) + _bases(rng, tail)
    return revcomp(d) if rc else d


def long_read(rng, pool, nbases, first_len):
    """A read of nbases bases, a run of wrapped segments: counted from the read's end its chain is stop, `first_len` residues, stop, .. -
    the second search starts at code first_len + 2 and, where its segment is unique, enters text mode text_min_l codes further on."""
    segs = [pool.window(first_len)]
    total = 3 + 3 * first_len + 3
    while nbases - total >= 3 * 12 + 3:
        L = min(int(rng.integers(20, 61)), (nbases - total - 3) // 3)
        segs.append(pool.window(L))
        total += 3 * L + 3
    d = STOP + b"".join(revtrans(rng, s) + STOP for s in reversed(segs))
    d = _bases(rng, nbases - len(d)) + d
    assert len(d) == nbases
    return d


def _standard_reads(rng, pool, reads, pairs):
    """what every world's read set holds: the listed read lengths and chain lengths, background windows, aliens, pairs"""
    for L in SHORT_READS:
        for rc in (False, True):
            reads.add(dna_of(rng, pool.window(L // 3), tail=L % 3, rc=rc), f"len{L}", exact=True)
    for k in CHAIN_CODES:
        for j in range(3):
            segs = pool.composite(k) if j else [pool.window(k)]
            d = b"".join(revtrans(rng, s) for s in segs)
            assert len(d) == 3 * k
            reads.add(revcomp(d) if j == 2 else d, f"chain{k}", exact=j == 0)
    for first in range(43, 55):                                 # the second search starts at window offsets 45 .. 56, text mode from 50 on
        reads.add(long_read(rng, pool, 600, first), "long600", exact=True)
    for first in (45, 50, 53):
        reads.add(long_read(rng, pool, 3000, first), "long3000", exact=first != 50)
    for j in range(120):                                        # windows anywhere, every frame, both strands
        naa = int(rng.integers(12, 100))
        reads.add(dna_of(rng, np.concatenate(pool.composite(naa)), frame=j % 3, tail=int(rng.integers(0, 3)), rc=j % 2 == 1), "anywhere")
    for j in range(12):
        reads.add(_bases(rng, rng.integers(30, 301)), "alien")
    for d in (b"", b"A", b"AC", b"ACGTA", b"N" * 70):
        reads.add(d, "degenerate", exact=True)
    r1, r2 = pairs
    for j in range(60):                                         # mates of different lengths
        a, b = pool.composite(int(rng.integers(15, 50))), pool.composite(int(rng.integers(15, 90)))
        m1 = dna_of(rng, np.concatenate(a), frame=j % 3, tail=(j // 3) % 3)
        m2 = dna_of(rng, np.concatenate(b), frame=(j // 2) % 3, tail=j % 2, rc=True)
        if j % 4 >= 2: m1, m2 = m2, m1
        r1.add(m1, "two_windows"); r2.add(m2, "two_windows")
    for j in range(6):
        r1.add(_bases(rng, 100), "alien"); r2.add(_bases(rng, 70), "alien")
    for j in range(6):                                          # an empty mate; only mate 2 matches
        m = dna_of(rng, pool.window(40), frame=j % 3)
        if j % 3 == 0: r1.add(m, "empty_mate_2", exact=True); r2.add(b"", "empty_mate_2", exact=True)
        elif j % 3 == 1: r1.add(b"", "empty_mate_1", exact=True); r2.add(m, "empty_mate_1", exact=True)
        else: r1.add(_bases(rng, 90), "only_mate_2_matches", exact=True); r2.add(m, "only_mate_2_matches", exact=True)
    r1.add(long_read(rng, pool, 600, 48), "long_and_short", exact=True); r2.add(dna_of(rng, pool.window(11)), "long_and_short", exact=True)


def _finish(names, taxids, prots, nodes, tax_names, reads, pairs, info):
    g = synth.Genomes(names, taxids, [np.ascontiguousarray(p, dtype=np.uint8) for p in prots], nodes, tax_names)
    info["read_kinds"], info["pair_kinds"] = list(reads.kind), list(pairs[0].kind)
    info["n_text"] = g.total_len + len(prots)                  # every protein is followed by its '$'
    w = World(g, reads.finish(), (pairs[0].finish(), pairs[1].finish()), info)
    assert w.pairs[0].n == w.pairs[1].n
    return w


def _padded(rng, prots, names, taxids, pad_taxid):
    """the two padding proteins around the world's own"""
    return ([_rand(rng, PAD)] + prots + [_rand(rng, PAD)], ["PAD_first"] + names + ["PAD_last"], [pad_taxid] + taxids + [pad_taxid])


# ------------------------------------------------------------------------------------------------ shared
def shared(seed=9201):
    """3 genera x 4 species x 4 strains.  For every c of SHARED_COUNTS a 120-residue block of its own in exactly c proteins (c <= 6: one
    block inside a species, one inside a genus, one across genera; 12: inside a genus; 40: everywhere), each copy in a protein of its own
    between random flanks of 40 .. 80 residues.  In the 5- and 6-copy blocks the copies are not equal: copy 0 is what the reads are drawn
    from, copy 1 differs at block position 80 (5 -> 4 rows), copies 2 .. 4 differ - each in its own way - d residues further left
    (4 -> 1 rows; d of VARIANT_DISTANCES: inside a text round, at its 8th character, at the next round's first and 8th), and the sixth
    copy differs at position 84 (6 -> 5 rows)."""
    rng = np.random.default_rng(seed)
    nodes, names, leaves = _regular_tree(3, 4, 4)
    prots, pnames, ptax, blocks, variant = [], [], [], [], 0
    for c in SHARED_COUNTS:
        for scope in (("species", "genus", "genera") if c <= 6 else ("genus",) if c == 12 else ("genera",)):
            gi, si = len(blocks) % 3, len(blocks) % 4
            if scope == "species": where = [(gi, si)] * c
            elif scope == "genus": where = [(gi, j % 4) for j in range(c)]
            else: where = [(j % 3, (j // 3) % 4) for j in range(c)]
            content = _rand(rng, 120)
            d = None
            if c in (5, 6):
                d = VARIANT_DISTANCES[variant]; variant += 1
            mine = []
            for j, (g_, s_) in enumerate(where):
                copy = content.copy()
                if d is not None and j == 1: copy[80] = _other(rng, content[80])
                if d is not None and 2 <= j <= 4: copy[80 - d] = AA[(int(np.nonzero(AA == content[80 - d])[0][0]) + j) % 20]
                if d is not None and j == 5: copy[84] = _other(rng, content[84])
                left, right = _rand(rng, rng.integers(40, 81)), _rand(rng, rng.integers(40, 81))
                mine.append((len(prots) + 1, len(left)))                           # (protein number after padding, offset of the block)
                prots.append(np.concatenate([left, copy, right]))
                pnames.append(f"SH_c{c}_{scope}_{j}")
                ptax.append(leaves[g_][s_][int(rng.integers(0, 4))])
            blocks.append({"c": c, "scope": scope, "copies": mine, "d": d})
    prots, pnames, ptax = _padded(rng, prots, pnames, ptax, leaves[0][0][0])
    pool = _Pool(prots, rng)
    reads, pairs = _Reads(rng), (_Reads(rng), _Reads(rng))
    for b in blocks:
        pi, off = b["copies"][0]
        src = prots[pi]
        for j in range(12):                                                        # inside the block: every frame, both strands
            naa = int(rng.integers(12, 60))
            a = off + int(rng.integers(0, 120 - naa + 1))
            reads.add(dna_of(rng, src[a:a + naa], frame=j % 3, tail=(j // 3) % 3, rc=j % 2 == 1), "inside", exact=j < 6)
        for j in range(4):                                                         # from a flank of the first copy into the block and out of it
            reads.add(dna_of(rng, src[off - 15:off + 25 + j], frame=j % 3, rc=j % 2 == 1), "flank_into_block", exact=True)
            reads.add(dna_of(rng, src[off + 95 - j:off + 135], frame=j % 3, rc=j % 2 == 1), "block_into_flank", exact=True)
        if b["d"] is not None:
            d = b["d"]
            for e in (85, 88, 90, 97, 110, 119):                                   # the read's last residue: c rows right of 84, then 5, 4 and 1
                for s in (0, 80 - d - 10, 80 - d + 1, 81):
                    if e - s + 1 >= 12:
                        reads.add(dna_of(rng, src[off + s:off + e + 1], frame=(e + s) % 3, rc=s % 2 == 1), "across_variants", exact=True)
            pj, oj = b["copies"][2]                                                # and reads of a copy that leaves the others at the second variant
            reads.add(dna_of(rng, prots[pj][oj + 40:oj + 100]), "across_variants_other_copy", exact=True)
        p2, o2 = b["copies"][-1]
        m1 = dna_of(rng, src[off + 5:off + 45], frame=1)
        m2 = dna_of(rng, prots[p2][o2 + 70:o2 + 115], tail=1, rc=True)
        pairs[0].add(m1, "both_in_block"); pairs[1].add(m2, "both_in_block")
    _standard_reads(rng, pool, reads, pairs)
    return _finish(pnames, ptax, prots, nodes, names, reads, pairs,
                   {"name": "shared", "ftab_chars": 3, "rbbwt_b": 4, "offrate": 4, "blocks": blocks})


# ------------------------------------------------------------------------------------------------ repeats
HOMOPOLYMERS = (40, 100, 300)
TANDEM = ((2, 300), (3, 100), (5, 40), (8, 25), (12, 20))       # (period, units)


def repeats(seed=9202):
    """2 genera x 2 species x 3 strains, 30 random proteins of 200 .. 400 residues; homopolymers of HOMOPOLYMERS residues and tandem
    repeats (TANDEM) between random flanks, every one of them in a protein of species 11 and again in one of species 21 (the other
    genus): ranges of hundreds of rows that never get below four, and above hitk_factor x k."""
    rng = np.random.default_rng(seed)
    nodes, names, leaves = _regular_tree(2, 2, 3)
    strains = [t for gen in leaves for sp in gen for t in sp]
    prots = [_rand(rng, rng.integers(200, 401)) for _ in range(30)]
    pnames = [f"RP_{i:02d}" for i in range(30)]
    ptax = [strains[i % len(strains)] for i in range(30)]
    spans = []
    for hi, L in enumerate(HOMOPOLYMERS):
        spans.append((f"homo{L}", np.full(L, AA[(6, 10, 15)[hi]], dtype=np.uint8)))
    for period, units in TANDEM:
        unit = _rand(rng, period)
        while any((unit == np.roll(unit, s)).all() for s in range(1, period)):
            unit = _rand(rng, period)
        spans.append((f"period{period}", np.tile(unit, units)))
    where = []
    for label, body in spans:
        for sp_leaves in (leaves[0][0], leaves[1][0]):
            left, right = _rand(rng, 60), _rand(rng, 60)
            where.append((label, len(prots) + 1, 60, len(body)))
            prots.append(np.concatenate([left, body, right])); pnames.append(f"RP_{label}_{sp_leaves[0]}"); ptax.append(sp_leaves[int(rng.integers(0, 3))])
    prots, pnames, ptax = _padded(rng, prots, pnames, ptax, strains[0])
    pool = _Pool(prots, rng)
    reads, pairs = _Reads(rng), (_Reads(rng), _Reads(rng))
    for label, pi, off, L in where:
        p = prots[pi]
        for j in range(10):                                                        # inside the repeat
            naa = int(rng.integers(12, min(L, 90) + 1))
            a = off + int(rng.integers(0, L - naa + 1))
            reads.add(dna_of(rng, p[a:a + naa], frame=j % 3, tail=(j // 3) % 3, rc=j % 2 == 1), "inside_" + label, exact=j < 5)
        for j in range(6):                                                         # across an edge into the flank
            inside = int(rng.integers(6, min(L, 50) + 1))
            out = int(rng.integers(6, 40))
            seg = p[off - out:off + inside] if j % 2 else p[off + L - inside:off + L + out]
            reads.add(dna_of(rng, seg, frame=j % 3, rc=j % 4 >= 2), "edge_" + label, exact=j < 3)
        pairs[0].add(dna_of(rng, p[off - 20:off + min(L, 30)], frame=1), "around_" + label)
        pairs[1].add(dna_of(rng, p[off + L - min(L, 25):off + L + 30], tail=2, rc=True), "around_" + label)
    _standard_reads(rng, pool, reads, pairs)
    return _finish(pnames, ptax, prots, nodes, names, reads, pairs,
                   {"name": "repeats", "ftab_chars": 2, "rbbwt_b": 0, "offrate": 2, "spans": where})


# ------------------------------------------------------------------------------------------------ ragged
def ragged(seed=9203):
    """Proteins of RAGGED_LENGTHS residues next to forty of 120 .. 300, attached to a genus, a species, a strain, a "no rank" node below
    a strain and the root; one protein's tax id is in no tree.  Text order: the 1 000-residue protein, twenty of the forty, then the short
    ones 3, 5, 8, 11, 12, 13, 52, 53, 63, 64, 65, 150 in a row, the other twenty, the 5 000-residue one."""
    rng = np.random.default_rng(seed)
    nodes = [(1, 1, "no rank"), (2, 1, "superkingdom"), (10, 2, "genus"), (11, 10, "species"), (111, 11, "strain"), (1111, 111, "no rank"),
             (20, 2, "genus"), (21, 20, "species"), (211, 21, "strain")]
    names = [(1, "root"), (2, "Bacteria"), (10, "Alpha"), (11, "Alpha one"), (111, "Alpha one str"), (1111, "Alpha one str isolate"),
             (20, "Beta"), (21, "Beta one"), (211, "Beta one str")]
    tax_of_len = {3: 111, 5: 1111, 8: 2, 11: 1, 12: 211, 13: 10, 52: 1111, 53: 21, 63: 111, 64: 777777, 65: 1, 150: 11, 1000: 1, 5000: 211}
    mids = [(_rand(rng, rng.integers(120, 301)), (10, 11, 111, 1111, 20, 21, 211, 1)[j % 8]) for j in range(40)]
    order = [("len", 1000)] + [("mid", j) for j in range(20)] + [("len", L) for L in RAGGED_LENGTHS[:12]] + [("mid", j) for j in range(20, 40)] + [("len", 5000)]
    prots, pnames, ptax = [], [], []
    for what, v in order:
        if what == "len":
            prots.append(_rand(rng, v)); pnames.append(f"RG_len{v}"); ptax.append(tax_of_len[v])
        else:
            prots.append(mids[v][0]); pnames.append(f"RG_mid{v:02d}"); ptax.append(mids[v][1])
    prots, pnames, ptax = _padded(rng, prots, pnames, ptax, 211)
    num = {n: i for i, n in enumerate(pnames)}
    pool = _Pool(prots, rng)
    reads, pairs = _Reads(rng), (_Reads(rng), _Reads(rng))
    first_residue = []                                                             # (read, residues matched)
    for m in range(MIN_HIT_LEN, MIN_HIT_LEN + 20):                                 # the match ends on a protein's first residue
        for j in range(2):
            p = prots[num[f"RG_mid{(m + 7 * j) % 40:02d}"]]
            d = (STOP if j == 0 else revtrans(rng, _rand(rng, 4))) + revtrans(rng, p[:m]) + STOP
            first_residue.append((reads.add(_bases(rng, m % 3) + d, "ends_on_first_residue", exact=True), m))
    short0 = num["RG_len3"]
    for a in range(short0, short0 + 11):                                           # across two and three adjacent short proteins
        for span in (2, 3):
            seg = np.concatenate([prots[a][-min(len(prots[a]), 20):]] + list(prots[a + 1:a + span - 1]) + [prots[a + span - 1][:min(len(prots[a + span - 1]), 20)]])
            if len(seg) >= 12:
                reads.add(dna_of(rng, seg, frame=a % 3, rc=span == 3), f"across_{span}_proteins", exact=True)
    for L in (11, 12, 13):                                                         # a whole short protein, with and without stop codons around it
        p = prots[num[f"RG_len{L}"]]
        reads.add(wrapped(rng, p), "whole_protein", exact=True)
        reads.add(revcomp(wrapped(rng, p)), "whole_protein", exact=True)
        reads.add(dna_of(rng, np.concatenate([_rand(rng, 5), p, _rand(rng, 5)]), frame=1), "whole_protein", exact=True)
    for L in (52, 53, 63, 64, 65, 150):
        reads.add(dna_of(rng, prots[num[f"RG_len{L}"]], frame=L % 3, rc=L % 2 == 1), "whole_protein", exact=True)
    for j in range(40):                                                            # windows over the ends of the forty
        i = num[f"RG_mid{j:02d}"]
        tail, head = prots[i][-int(rng.integers(8, 40)):], prots[i + 1][:int(rng.integers(8, 40))]
        reads.add(dna_of(rng, np.concatenate([tail, head]), frame=j % 3, rc=j % 2 == 1), "boundary")
    for j in range(20):
        a = int(rng.integers(0, 5000 - 90))
        reads.add(dna_of(rng, prots[num["RG_len5000"]][a:a + int(rng.integers(12, 90))], frame=j % 3, rc=j % 2 == 1), "long_protein")
        pairs[0].add(dna_of(rng, prots[num["RG_len1000"]][10 * j:10 * j + 30], frame=j % 3), "long_protein")
        pairs[1].add(dna_of(rng, prots[num["RG_len1000"]][10 * j + 60:10 * j + 60 + 20 + j], rc=True), "long_protein")
    _standard_reads(rng, pool, reads, pairs)
    return _finish(pnames, ptax, prots, nodes, names, reads, pairs,
                   {"name": "ragged", "ftab_chars": 2, "rbbwt_b": 0, "offrate": 4, "first_residue": first_residue})


# ------------------------------------------------------------------------------------------------ frames
def _score(l):
    return (l - 5) ** 2 if l >= MIN_HIT_LEN else 0              # Classifier::CalculateHitScore with the protein index's adjustment (15 / 3)


def _strand_cases():
    """hit lengths (plus strand, minus strand) whose summed scores are equal, differ by exactly 1 % (the sum of one strand = the other's
    + its hundredth, in integers: both strands are still kept), by one less and by one more (then only the larger strand is kept)"""
    lens = range(MIN_HIT_LEN, 31)
    sums = {}
    for n in (1, 2, 3):
        for combo in itertools.combinations_with_replacement(lens, n):
            sums.setdefault(sum(_score(l) for l in combo), combo)
    out = {}
    for lo in sorted(sums):
        if lo // 100 < 2:
            continue
        for label, hi in (("exactly_1_percent", lo + lo // 100), ("just_below_1_percent", lo + lo // 100 - 1), ("just_above_1_percent", lo + lo // 100 + 1)):
            if label not in out and hi in sums:
                out[label] = (sums[hi], sums[lo])
    out["equal"] = ((20, 14), (20, 14))
    assert len(out) == 4, out
    return out


def frames(seed=9204):
    """60 random proteins of 200 .. 400 residues (2 genera x 2 species x 3 strains) and reads built from wrapped segments of them: two
    frames of one strand that both hold segments (one long hit against two shorter ones: (hits x sum) decides), two strands whose scores
    are equal or 1 % apart, a stop codon / N / IUPAC letter at each of the first 12 codes of a search, pairs of unequal mates."""
    rng = np.random.default_rng(seed)
    nodes, names, leaves = _regular_tree(2, 2, 3)
    strains = [t for gen in leaves for sp in gen for t in sp]
    prots = [_rand(rng, rng.integers(200, 401)) for _ in range(60)]
    pnames, ptax = [f"FR_{i:02d}" for i in range(60)], [strains[i % len(strains)] for i in range(60)]
    prots, pnames, ptax = _padded(rng, prots, pnames, ptax, strains[0])
    pool = _Pool(prots, rng)
    reads, pairs = _Reads(rng), (_Reads(rng), _Reads(rng))
    two_frames, strand_rule = [], []
    for j, (la, lb) in enumerate([(30, 20), (40, 20), (30, 21), (25, 17), (36, 18), (28, 19), (50, 30), (45, 20)] * 2):
        # frame 0: one hit of la; one or two bases on: two hits of lb each.  (2 x 2 x score(lb) against score(la))
        a_part = wrapped(rng, pool.window(la))
        b_part = STOP + revtrans(rng, pool.window(lb)) + STOP + revtrans(rng, pool.window(lb)) + STOP
        spacer = _bases(rng, 1 + j % 2)
        d = a_part + spacer + b_part if j % 4 < 2 else b_part + spacer + a_part
        d = revcomp(d) if j >= 8 else d
        two_frames.append((reads.add(d, "two_frames", exact=True), la, lb, 4 * _score(lb) > _score(la)))
    for label, (plus, minus) in _strand_cases().items():
        for flip in (False, True):
            p_part = b"".join(wrapped(rng, pool.window(l)) for l in plus)
            m_part = revcomp(b"".join(wrapped(rng, pool.window(l)) for l in minus))
            d = p_part + _bases(rng, 1) + m_part
            i = reads.add(revcomp(d) if flip else d, "strands_" + label, exact=True)
            strand_rule.append((i, label, sum(_score(l) for l in plus), sum(_score(l) for l in minus), flip))
            pairs[0].add(p_part, "strands_" + label, exact=True); pairs[1].add(m_part if not flip else revcomp(m_part), "strands_" + label, exact=True)
    for pos in range(12):                                                          # an odd codon at each of the key's codes (counted from the read's end)
        for what in (b"TAA", b"ANT", b"RCT"):
            seg = pool.window(40)
            codons = [revtrans(rng, seg[q:q + 1]) for q in range(40)]
            codons[39 - pos] = what
            reads.add(b"".join(codons), "odd_codon_in_key", exact=True)
            reads.add(revcomp(_bases(rng, pos % 3) + b"".join(codons)), "odd_codon_in_key", exact=True)
    for j in range(20):                                                            # mates of very different lengths: the second mate's lists start at 6 x cap(len1)
        l1, l2 = (12, 90) if j % 2 else (95, 11 + j)
        pairs[0].add(dna_of(rng, np.concatenate(pool.composite(l1)), frame=j % 3), "unequal_mates", exact=j < 10)
        pairs[1].add(dna_of(rng, np.concatenate(pool.composite(l2)), tail=j % 3, rc=True), "unequal_mates", exact=j < 10)
    _standard_reads(rng, pool, reads, pairs)
    return _finish(pnames, ptax, prots, nodes, names, reads, pairs,
                   {"name": "frames", "ftab_chars": 3, "rbbwt_b": 0, "offrate": 4, "two_frames": two_frames, "strand_rule": strand_rule})


GENERATORS = {"shared": shared, "repeats": repeats, "ragged": ragged, "frames": frames}
_made = {}


def make(name) -> World:
    if name not in _made:
        w = GENERATORS[name]()
        assert w.genomes.total_len < MAX_RESIDUES
        assert SIGMA ** 3 <= w.info["n_text"] < SIGMA ** 4 and text_min_l(w.info["n_text"]) == 5   # the read sets are laid out for this
        assert len(w.genomes.seqs[0]) == PAD and len(w.genomes.seqs[-1]) == PAD
        lens = set(np.diff(w.reads.offsets.astype(np.int64)).tolist())
        assert lens >= set(SHORT_READS) | set(LONG_READS) | {3 * k for k in CHAIN_CODES}
        _made[name] = w
    return _made[name]


def build_kwargs(world):
    return {"ftab_chars": world.info["ftab_chars"], "rbbwt_b": world.info["rbbwt_b"], "offrate": world.info["offrate"], "protein": True}


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


def guards(world, oracle, k, hits=None):
    """Asserts what the world must provoke, from the oracle's hit lists alone (oracle: oracle_lib.OracleIndex opened with max_result = k
    on an index of this world).  Returns the values reached."""
    info = world.info
    name = info["name"]
    assert oracle.param.maxResult == k and oracle.param.maxResultPerHitFactor == HITK_FACTOR and oracle.param.minHitLen == 0   # (0: inferred, 11)
    hits = hit_lists(world, oracle) if hits is None else hits
    se = hits["se"]
    rs = world.reads
    lens = np.diff(rs.offsets.astype(np.int64))
    reached = {"most_hits_of_one_read": max(len(h) for hs in hits.values() for h in hs)}
    for tag in ("se", "pe"):
        with_hits = sum(1 for h in hits[tag] if len(h))
        reached[f"reads_with_hits_{tag}"] = (with_hits, len(hits[tag]))
        assert 2 * with_hits > len(hits[tag]) and with_hits < len(hits[tag]), reached
    # chains of each listed length, and a hit in at least one read of each (a read of 3 k bases has a chain of k codes)
    chains = {c: sum(1 for i in range(rs.n) if lens[i] == 3 * c and len(se[i])) for c in CHAIN_CODES + (200, 1000)}
    reached["reads_with_hits_by_chain_codes"] = chains
    assert all(v > 0 for v in chains.values()), chains
    short = {L: sum(1 for i in range(rs.n) if lens[i] == L and len(se[i])) for L in SHORT_READS}
    reached["short_reads_with_hits"] = short
    assert short[32] == 0 and all(short[L] > 0 for L in (33, 35, 36)), short        # 10 codes are below min_hit_len, 11 are at it
    most = max((len(se[i]) for i in range(rs.n) if lens[i] == 3000), default=0)
    reached["most_hits_of_a_3000_base_read"] = most
    assert most >= 10
    # the 600-base reads: a hit's offset is the code its search started at; the second search of each starts at codes 45 .. 56 of the
    # chain's first 64-code window (52 is the last start whose twelve key codes lie inside it), text mode at the earliest 5 codes on
    starts = {int(x) for i, h in enumerate(se) if info["read_kinds"][i] == "long600" for x in h["offset"].tolist()}
    reached["search_starts_45_to_56"] = sorted(starts & set(range(45, 57)))
    assert starts >= set(range(45, 57)), sorted(starts)
    both = sum(1 for h in se if len(h) and len(set(h["strand"].tolist())) == 2)
    reached["reads_with_both_strands_kept"] = both
    sizes = {}
    for h in se:
        for x in (h["ep"] - h["sp"] + 1).tolist():
            sizes[x] = sizes.get(x, 0) + 1
    if name == "shared":
        reached["range_sizes"] = {c: sizes.get(c, 0) for c in SHARED_COUNTS}
        assert all(sizes.get(c, 0) > 0 for c in SHARED_COUNTS), reached["range_sizes"]
        # the reads over the variant residues: from the first copy they end in one row after 5 (6) and 4 rows
        kinds = info["read_kinds"]
        one_row = sum(1 for i, h in enumerate(se) if kinds[i] == "across_variants" and len(h) == 1 and int(h["ep"][0] - h["sp"][0]) == 0)
        reached["variant_reads_ending_in_one_row"] = one_row
        assert one_row >= 30
    if name == "repeats":
        big = sum(1 for h in se if len(h) and int((h["ep"] - h["sp"] + 1).max()) > HITK_FACTOR * k)
        reached["reads_with_range_above_hitk_factor_x_k"], reached["largest_range"] = big, max(sizes)
        assert big >= 10 and max(sizes) > HITK_FACTOR * 5, (big, max(sizes))
    if name == "ragged":
        rem = {}
        for i, m in info["first_residue"]:
            if len(se[i]) == 1 and int(se[i]["l"][0]) == m and int(se[i]["ep"][0] - se[i]["sp"][0]) == 0 and m > text_min_l(info["n_text"]):
                r = (m - text_min_l(info["n_text"]) - 1) % 8 + 1                     # residues left to match in the last text round
                rem[r] = rem.get(r, 0) + 1
        reached["first_residue_hits_by_remainder"] = rem
        assert set(rem) == set(range(1, 9)), rem
        whole = sum(1 for i, h in enumerate(se) if info["read_kinds"][i] == "whole_protein" and len(h) and int(h["l"].max()) in (11, 12, 13))
        reached["whole_short_proteins_hit"] = whole
        assert whole >= 6
    if name == "frames":
        assert both >= 4, both
        short_wins = long_wins = 0
        for i, la, lb, two_short in info["two_frames"]:
            ls = sorted(se[i]["l"].tolist())
            if two_short:
                assert ls == [lb, lb], (i, la, lb, ls)                              # not the frame with the longest hit
                short_wins += 1
            else:
                assert ls == [la], (i, la, lb, ls)
                long_wins += 1
        reached["frame_choice"] = {"two_shorter_hits": short_wins, "one_longer_hit": long_wins}
        assert short_wins >= 2 and long_wins >= 2
        rule = {}
        for i, label, s_plus, s_minus, flip in info["strand_rule"]:
            got = {s: sum(_score(int(l)) for l, t in zip(se[i]["l"], se[i]["strand"]) if t == s) for s in (1, -1)}
            hi, lo = (1, -1) if not flip else (-1, 1)
            if label == "just_above_1_percent":
                assert got[hi] == s_plus and got[lo] == 0, (label, got)
            else:
                assert got[hi] == s_plus and got[lo] == s_minus, (label, got, s_plus, s_minus)
            rule[label] = rule.get(label, 0) + 1
        reached["strand_rule"] = rule
        assert set(rule) == {"equal", "exactly_1_percent", "just_below_1_percent", "just_above_1_percent"}
    return reached
