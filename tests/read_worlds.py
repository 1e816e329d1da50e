"""Read worlds: one small index of near-identical strains and eleven seeded families of reads that walk the read-shape boundaries of the
nucleotide search and of the post stage - every length 0 .. 130, every buffer alignment mod 16 and mod 32, a non-symbol or a
substitution at every position, chimeras of the two strands, reads of 4 095 .. 100 000 bases, reads of 4 094 .. 70 000 hits, the
length thresholds 32 768 and 2^20, ragged pairs.  Every other test varies the index and keeps its reads at 30 .. 300 bases (12 reads of
2 .. 6 kbase and one exact 70 kbase copy aside).  A helper module, not a conftest: tests/test_read_worlds_oracle_cpu.py and
tests/test_gpu_read_worlds.py import it.

genomes() gives the text; the caller writes the index and passes what the INDEX says (min_hit_len, the ftab width w) to make(), which
returns a World of four batches: small_se, small_pe (families 1 - 7 and 11: a few thousand reads), giant_se, giant_pe (families 8 - 10:
two dozen reads).  "Window" = an exact copy of the text; no read is drawn within 300 bases of the text's two ends.

guards(world, oracle, k) asserts, from the C oracle alone, what the families claim and returns the values reached: no family passes
quietly."""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

from centrifuger_amd import synth

ACGT = synth.ACGT
EDGE = 300
MAX_TEXT, MAX_SEQS = 500_000, 64              # the oracle's result holds 64 matches (ORA_MAX_MATCH)
FTAB_CHARS = 6
N_SPECIES, N_STRAINS, GENOME_LEN, DIVERGENCE = 4, 10, 9000, 0.004
NONSYMBOLS = b"NnRacgt-.*"
LENGTHS_MAX = 130
LONG_LENGTHS = (1000, 4095, 4096, 4097, 32767, 32768, 100000)
MANY_HITS = (4094, 4095, 4096, 65535, 65536, 70000)
LATE_FEW, LATE_MANY = 65600, 400              # the `late_hand_over` read: windows of 1 .. 4 rows that are searched first, windows of 5 .. 24 rows behind them
THRESHOLD_LENGTHS = (32767, 32768, (1 << 20) - 1, 1 << 20)
RAGGED = ("0", "1", "mhl-1", "mhl", "150", "5000")
HITS_CAP = 1 << 17                            # buffer of oracle_lib.OracleIndex.query_hits for these reads
SHAPES_ONE_NONSYMBOL, SHAPES_ONE_SUBSTITUTION = 140, 190
BATCHES = ("small_se", "small_pe", "giant_se", "giant_pe")


class Batch(NamedTuple):
    reads: synth.ReadSet
    mates: synth.ReadSet | None               # None: single-end
    family: list                              # family name of every read
    tag: list                                 # what the read is within its family

    @property
    def n(self):
        return self.reads.n

    def of(self, family):
        return [i for i, f in enumerate(self.family) if f == family]

    def subset(self, keep):
        """the reads `keep` (indexes) as a batch of their own"""
        def cut(rs):
            seqs = [rs.bases[int(rs.offsets[i]):int(rs.offsets[i + 1])] for i in keep]
            return _readset(seqs)
        return Batch(cut(self.reads), None if self.mates is None else cut(self.mates), [self.family[i] for i in keep], [self.tag[i] for i in keep])


class World(NamedTuple):
    genomes: synth.Genomes
    min_hit_len: int
    w: int
    batches: dict


def genomes(seed=9301):
    g = synth.make_genomes(N_SPECIES, N_STRAINS, GENOME_LEN, seed=seed, divergence_step=DIVERGENCE)
    assert g.total_len < MAX_TEXT and len(g.seqs) <= MAX_SEQS
    return g


def build_kwargs():
    return {"ftab_chars": FTAB_CHARS}


def _readset(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    bases = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)
    return synth.ReadSet(np.ascontiguousarray(bases, dtype=np.uint8), offs)


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, size=int(n))]


def text_min_l(n):
    """the number of matched characters from which the device's search looks at the size of its range (1 .. 4 rows: on to the text,
    5 .. 24 rows: wide text mode, or the hand-over of the two-launch search): floor(log4(n)) + 2"""
    log4n = 0
    while 4 ** (log4n + 1) <= n:
        log4n += 1
    return log4n + 2


def _kmers(codes, L):
    """codes: (.., >= L) array of 0 .. 3; the value of the L-mer at every position of the last axis"""
    n = codes.shape[-1] - L + 1
    v = np.zeros(codes.shape[:-1] + (n,), dtype=np.int64)
    for j in range(L):
        v = v * 4 + codes[..., j:n + j]
    return v


def rows_of_kmers(cat, L, of=None):
    """in how many places of the text `cat` L bases stand (the rows of their range): those at every text position, or the L-mers `of`
    (an array of bases whose last axis has length L)"""
    uniq, inverse, counts = np.unique(_kmers(np.searchsorted(ACGT, cat).astype(np.int64), L), return_inverse=True, return_counts=True)
    if of is None:
        return counts[inverse.reshape(-1)]
    v = _kmers(np.searchsorted(ACGT, of).astype(np.int64), L)[..., 0]
    at = np.minimum(np.searchsorted(uniq, v), len(uniq) - 1)
    return np.where(uniq[at] == v, counts[at], 0)


def _substitute(s, pos, rng):
    pos = np.atleast_1d(pos)
    s[pos] = ACGT[(np.searchsorted(ACGT, s[pos]) + rng.integers(1, 4, size=len(pos))) & 3]


class _Maker:
    def __init__(self, g, mhl, w, seed):
        self.rng = np.random.default_rng(seed)
        self.cat = np.concatenate(g.seqs)
        self.n = len(self.cat)
        self.mhl, self.w = int(mhl), int(w)
        self.se = {"small": ([], [], []), "giant": ([], [], [])}                  # reads, family, tag
        self.pe = {"small": ([], [], [], []), "giant": ([], [], [], [])}          # mate 1, mate 2, family, tag

    def take(self, p, L, rc=False):
        p, L = int(p), int(L)
        assert EDGE <= p and p + L <= self.n - EDGE, (p, L, self.n)
        s = self.cat[p:p + L]
        return synth.revcomp(s) if rc else s.copy()

    def where(self, L):
        return int(self.rng.integers(EDGE, self.n - EDGE - L + 1))

    def single(self, which, s, family, tag):
        seqs, fam, tags = self.se[which]
        seqs.append(np.ascontiguousarray(s, dtype=np.uint8)); fam.append(family); tags.append(tag)

    def pair(self, which, a, b, family, tag):
        m1, m2, fam, tags = self.pe[which]
        m1.append(np.ascontiguousarray(a, dtype=np.uint8)); m2.append(np.ascontiguousarray(b, dtype=np.uint8)); fam.append(family); tags.append(tag)

    def offset(self, which, mate=None):
        """where the next read of the batch starts in its flat buffer"""
        seqs = self.se[which][0] if mate is None else self.pe[which][mate]
        return sum(len(s) for s in seqs)

    # ---- 1
    def lengths(self):
        for p in (self.where(LENGTHS_MAX) for _ in range(3)):
            for rc in (False, True):
                for L in range(LENGTHS_MAX + 1):
                    self.single("small", self.take(p, L, rc), "lengths", (L, rc))

    # ---- 2
    def residues(self):
        """48 residues mod 32, every one at least once, in an order that makes the fillers' lengths differ"""
        return self.rng.permutation(32).tolist() + self.rng.permutation(32)[:16].tolist()

    def alignment(self):
        p = self.where(400)
        for rc in (False, True):
            copy = self.take(p, 150, rc)
            cur = self.offset("small")
            for j, target in enumerate(self.residues()):                          # the copy's first byte at residue `target` mod 32
                f = (target - cur) % 32
                if j % 2 and f < 16:
                    f += 32
                self.single("small", self.take(self.where(f), f, j % 2 == 1), "alignment", ("filler", f))
                cur += f
                self.single("small", copy, "alignment", ("copy", rc))
                cur += 150
            mate1 = self.take(p + 200, 100, not rc)                               # FR with the copy (rc: RF - the pair is flipped)
            cur = self.offset("small", 1)
            for j, target in enumerate(self.residues()):
                f = (target - cur) % 32
                if j % 2 and f < 16:
                    f += 32
                self.pair("small", self.take(self.where(40), 40), self.take(self.where(f), f, j % 2 == 0), "alignment", ("filler", f))
                cur += f
                self.pair("small", mate1, copy, "alignment", ("copy", rc))
                cur += 150

    # ---- 3
    def one_nonsymbol(self):
        p = self.where(150)
        for rc in (False, True):
            for q in range(150):
                s = self.take(p, 150, rc)
                s[q] = NONSYMBOLS[q % len(NONSYMBOLS)]
                self.single("small", s, "one_nonsymbol", (q, rc))

    # ---- 4
    def two_nonsymbols(self):
        for a in (0, 1, 5, 40, 100):
            p = self.where(200)
            for d in range(1, 61):                                                # the segment between them holds d - 1 symbols
                s = self.take(p, 200, rc=d % 2 == 0)
                s[a] = ord("N"); s[a + d] = b"NR-.*"[d % 5]
                self.single("small", s, "two_nonsymbols", (a, d))

    # ---- 5
    def periods(self):
        m = self.mhl
        return sorted({8, 16, m - 1, m, m + 1, m + 2, m + 3, 32, 33, 48, 49, 64})

    def periodic_nonsymbols(self):
        for d in self.periods():
            p = self.where(300)
            for rc in (False, True):
                s = self.take(p, 300, rc)
                s[d - 1::d] = ord("N")                                            # segments of d - 1 symbols
                self.single("small", s, "periodic_nonsymbols", (d, rc))
                s = self.take(p, 300, rc)
                s[d::d + 1] = ord("N")                                            # segments of d symbols
                self.single("small", s, "periodic_nonsymbols", (d + 1, rc))

    # ---- 6
    def one_substitution(self):
        p = self.where(200)
        for rc in (False, True):
            for q in range(200):
                s = self.take(p, 200, rc)
                _substitute(s, q, self.rng)
                self.single("small", s, "one_substitution", (q, rc))

    # ---- 7
    def chimeras(self):
        for i in range(200):
            # a search that starts in the other half ends a few bases inside this one and cuts its hit short by up to ~10 bases on either
            # strand: the two scores (l - 15)^2 stay within 1 % of each other only where a base weighs little - halves of 1 500 bases
            # (140 reads); the 60 reads with halves of 100 mostly keep one strand
            base = 100 if i < 60 else 1500
            h = base + (i - self.offset("small") - base) % 16                     # the junction at residue i mod 16
            a, b = self.take(self.where(h), h), self.take(self.where(h), h, rc=True)
            self.single("small", np.concatenate([a, b]), "chimeras", (self.offset("small") + h) % 16)

    # ---- 8
    def long(self):
        for L in LONG_LENGTHS:
            p = self.where(L)
            s = self.take(p, L, rc=L % 2 == 1)
            self.single("giant", s, "long", (L, "exact"))
            s = self.take(self.where(L), L, rc=L % 2 == 0)
            _substitute(s, np.nonzero(self.rng.random(L) < 0.02)[0], self.rng)
            self.single("giant", s, "long", (L, "substitutions"))

    # ---- 9
    def many_hits_read(self, windows, alternate=False, p=None):
        m = self.mhl
        p = self.rng.integers(EDGE, self.n - EDGE - m + 1, size=windows) if p is None else p
        body = np.full((windows, m + 1), ord("N"), dtype=np.uint8)
        body[:, :m] = self.cat[p[:, None] + np.arange(m)[None, :]]
        if alternate:
            body[1::2, :m] = synth.revcomp(body[1::2, :m])
        return body.reshape(-1)[:-1].copy()

    def late_hand_over_read(self):
        """The two-launch search hands a chain over at its first search that holds 5 .. 24 rows after text_min_l characters, with the
        number of hits it has written so far in the record.  A search walks a read from its END and a window from its last base: this
        read ends in LATE_FEW windows whose last text_min_l - 1 bases (and whose first, for the other walking direction) stand in 1 .. 4
        places of the text, because they cover a substitution that one strain has alone - those searches stay in the first stage - and
        starts with LATE_MANY windows that stand in 5 .. 24 places, the first of which hands the chain over with LATE_FEW hits."""
        m, L = self.mhl, text_min_l(self.n) - 1
        at = np.arange(EDGE, self.n - EDGE - m + 1)
        ends, whole = rows_of_kmers(self.cat, L), rows_of_kmers(self.cat, m)
        few = at[(ends[at] <= 4) & (ends[at + m - L] <= 4)]
        many = at[(whole[at] >= 5) & (whole[at] <= 24)]
        assert len(few) >= 1000 and len(many) >= 1000, (len(few), len(many))
        return self.many_hits_read(LATE_MANY + LATE_FEW, p=np.concatenate([self.rng.choice(many, LATE_MANY), self.rng.choice(few, LATE_FEW)]))

    def many_hits(self):
        for c in MANY_HITS:
            self.single("giant", self.many_hits_read(c), "many_hits", c)
        self.single("giant", self.many_hits_read(4096, alternate=True), "many_hits", "alternating")
        self.single("giant", self.late_hand_over_read(), "many_hits", "late_hand_over")

    # ---- 10
    def length_thresholds(self):
        for L in THRESHOLD_LENGTHS:
            s = _rand(self.rng, L)
            slot = L // 40
            for j in range(40):
                at = j * slot + int(self.rng.integers(0, slot - 150))
                s[at:at + 150] = self.take(self.where(150), 150, rc=j % 2 == 1)
            self.single("giant", s, "length_thresholds", L)

    # ---- 11
    def ragged_pairs(self):
        m = self.mhl
        lens = (0, 1, m - 1, m, 150, 5000)
        p = self.where(12000)
        for a, L1 in zip(RAGGED, lens):
            for b, L2 in zip(RAGGED, lens):
                self.pair("small", self.take(p, L1), self.take(p + 12000 - L2, L2, rc=True), "ragged_pairs", (a, b))
        p = self.where(40000)
        for L1, L2 in ((16383, 16384), (16384, 16384), (32000, 767), (768, 32000)):
            self.pair("small", self.take(p, L1), self.take(p + 40000 - L2, L2, rc=True), "ragged_pairs", ("sum", L1 + L2))
        self.pair("small", self.many_hits_read(4095), self.take(self.where(150), 150, rc=True), "ragged_pairs", ("many_hits", 4095))

    def giant_pairs(self):
        """every giant read cut in two at an odd place: mate 1 its head, mate 2 the reverse complement of the rest (len1 + len2 is the
        read's length and the two mates' hits add up to the read's, so the pair sits on the same side of every threshold).  Two reads
        stay single: that of 70 000 windows, which sits on no threshold, and `late_hand_over`, whose subject is one chain's count."""
        seqs, fam, tags = self.se["giant"]
        for s, f, t in zip(seqs, fam, tags):
            if f == "many_hits" and t in (70000, "late_hand_over"):
                continue
            c = len(s) // 3 + 1
            self.pair("giant", s[:c].copy(), synth.revcomp(s[c:]), f, t)

    def batches(self):
        out = {}
        for which in ("small", "giant"):
            seqs, fam, tags = self.se[which]
            out[which + "_se"] = Batch(_readset(seqs), None, fam, tags)
            m1, m2, fam, tags = self.pe[which]
            out[which + "_pe"] = Batch(_readset(m1), _readset(m2), fam, tags)
        return out


def make(g, min_hit_len, w, seed=9302) -> World:
    """g: genomes(); min_hit_len, w: what the index written from g says (info().min_hit_len, info().precompute_width)"""
    assert FTAB_CHARS == w < min_hit_len <= 32, (w, min_hit_len)
    m = _Maker(g, min_hit_len, w, seed)
    m.alignment()                                    # first: its fillers steer the offsets of the flat buffers from their start
    m.lengths(); m.one_nonsymbol(); m.two_nonsymbols(); m.periodic_nonsymbols(); m.one_substitution(); m.chimeras()
    m.ragged_pairs()
    m.long(); m.many_hits(); m.length_thresholds(); m.giant_pairs()
    world = World(g, int(min_hit_len), int(w), m.batches())
    assert 2000 <= world.batches["small_se"].n <= 5000 and world.batches["small_se"].reads.offsets[-1] < 1_500_000 and world.batches["giant_se"].n <= 30
    return world


def ids(batch):
    return [f"r{i}" for i in range(batch.n)]


def write_fasta(batch, d, stem):
    """stem.fa, or stem_1.fa and stem_2.fa, under d (ids r0, r1, ..; one line per read); returns the command line's input options"""
    if batch.mates is None:
        synth.write_fasta(batch.reads, os.path.join(d, stem + ".fa"))
        return ["-u", os.path.join(d, stem + ".fa")]
    synth.write_fasta(batch.reads, os.path.join(d, stem + "_1.fa"))
    synth.write_fasta(batch.mates, os.path.join(d, stem + "_2.fa"))
    return ["-1", os.path.join(d, stem + "_1.fa"), "-2", os.path.join(d, stem + "_2.fa")]


# ------------------------------------------------------------------------------------------------ guards
def hit_lists(world, oracle):
    """the oracle's hit list of every read and pair of the four batches (they do not depend on -k)"""
    out = {}
    for name in BATCHES:
        b = world.batches[name]
        out[name] = [oracle.query_hits(b.reads.get(i), None if b.mates is None else b.mates.get(i), cap=HITS_CAP) for i in range(b.n)]
    return out


def _shape(h):
    return tuple(zip(h["l"].tolist(), h["offset"].tolist(), h["strand"].tolist(), (h["ep"] - h["sp"] + 1).tolist()))


def _length(rs, i):
    return int(rs.offsets[i + 1]) - int(rs.offsets[i])


def guards(world, oracle, k, hits=None):
    """oracle: oracle_lib.OracleIndex opened with max_result = k on an index of world.genomes.  Returns the values reached."""
    assert oracle.param.maxResult == k
    mhl, w = world.min_hit_len, world.w
    hits = hit_lists(world, oracle) if hits is None else hits
    res = {}
    for name in BATCHES:
        b = world.batches[name]
        if b.mates is None:
            res[name] = oracle.classify(b.reads.bases, b.reads.offsets, threads=8)
        else:
            res[name] = oracle.classify(b.reads.bases, b.reads.offsets, b.mates.bases, b.mates.offsets, threads=8)
    reached = {"min_hit_len": mhl, "w": w}
    se, pe, gs = world.batches["small_se"], world.batches["small_pe"], world.batches["giant_se"]

    # lengths
    for i in se.of("lengths"):
        L = se.tag[i][0]
        assert _length(se.reads, i) == L and (res["small_se"][i].nmatch > 0) == (L >= mhl), ("lengths", se.tag[i], res["small_se"][i].nmatch)
    assert {se.tag[i][0] for i in se.of("lengths")} == set(range(LENGTHS_MAX + 1)) and mhl + 40 < LENGTHS_MAX

    # alignment
    for name, b, rs in (("small_se", se, se.reads), ("small_pe", pe, pe.mates)):
        for rc in (False, True):
            copies = [i for i in b.of("alignment") if b.tag[i] == ("copy", rc)]
            at = [int(rs.offsets[i]) for i in copies]
            assert len(copies) == 48 and {a % 16 for a in at} == set(range(16)) and {a % 32 for a in at} == set(range(32)), (name, rc, at)
            rows = {oracle.format("r", res[name][i]) for i in copies}
            assert len(rows) == 1 and res[name][copies[0]].nmatch > 0, (name, rc, rows)
            assert len({_shape(hits[name][i]) for i in copies}) == 1
        fillers = sorted({b.tag[i][1] for i in b.of("alignment") if b.tag[i][0] == "filler"})
        assert len(fillers) >= 20 and fillers[0] <= 3 and fillers[-1] >= 44, fillers
    reached["alignment_residues"] = (16, 32)

    # one non-symbol, one substitution: the hit lists differ from position to position
    for family, floor in (("one_nonsymbol", SHAPES_ONE_NONSYMBOL), ("one_substitution", SHAPES_ONE_SUBSTITUTION)):
        shapes = {_shape(hits["small_se"][i]) for i in se.of(family)}
        reached["shapes_" + family] = len(shapes)
        assert len(shapes) >= floor, (family, len(shapes))

    # two non-symbols: the segment between them below w, between w and the derived table's K (up to 17), at min_hit_len - 1 and at min_hit_len
    seg = {se.tag[i][1] - 1 for i in se.of("two_nonsymbols")}
    assert set(range(0, 60)) <= seg and {w - 1, w, mhl - 1, mhl} <= seg
    hit_of_segment = {}
    for i in se.of("two_nonsymbols"):
        a, d = se.tag[i]
        if a >= 40:                                                               # [0, a) holds a hit of its own only from a = 40 on; count hits of length d - 1
            hit_of_segment.setdefault(d - 1, []).append(int((hits["small_se"][i]["l"] == d - 1).sum()))
    assert all(sum(v) == 0 for s, v in hit_of_segment.items() if s < mhl), hit_of_segment
    assert all(min(v) >= 1 for s, v in hit_of_segment.items() if s >= mhl), hit_of_segment
    reached["two_nonsymbols_segments_with_hit"] = sorted(s for s, v in hit_of_segment.items() if min(v) >= 1)[:3]

    # periodic non-symbols: segments of min_hit_len - 1 symbols give nothing, of min_hit_len symbols a hit each
    per = {}
    for i in se.of("periodic_nonsymbols"):
        per.setdefault(se.tag[i][0] - 1, []).append(len(hits["small_se"][i]))
    reached["periodic_hits_by_segment"] = {s: max(v) for s, v in sorted(per.items())}
    assert all(max(v) == 0 for s, v in per.items() if s < mhl) and all(min(v) >= 300 // (s + 1) - 1 for s, v in per.items() if s >= mhl), per
    assert {mhl - 1, mhl, 31, 32, 47, 48} <= set(per)

    # chimeras
    both = sum(1 for i in se.of("chimeras") if len(set(hits["small_se"][i]["strand"].tolist())) == 2)
    reached["chimeras_with_both_strands"] = both
    assert both >= 100 and {se.tag[i] for i in se.of("chimeras")} == set(range(16)), both

    # long
    for i in gs.of("long"):
        assert res["giant_se"][i].nmatch > 0 and res["giant_se"][i].queryLength == gs.tag[i][0]
    reached["long_hits"] = {gs.tag[i]: len(hits["giant_se"][i]) for i in gs.of("long") if gs.tag[i][0] >= 32767}

    # many hits
    counts = {}
    for i in gs.of("many_hits"):
        h = hits["giant_se"][i]
        strands = set(h["strand"].tolist())
        counts[gs.tag[i]] = len(h)
        if gs.tag[i] == "alternating":
            assert len(h) == 4096 and len(strands) == 2
        elif gs.tag[i] == "late_hand_over":
            # in the order of the search (from the read's end, as the offsets count): LATE_FEW hits of 1 .. 4 rows, then hits of 5 .. 24 rows; and the few rows
            # are reached before the device looks at the range for the first time (one character of margin), from the text itself
            rows = h["ep"] - h["sp"] + 1
            assert (np.diff(h["offset"].astype(np.int64)) == mhl + 1).all() and h["offset"][0] == 0                  # the list is in the order of the search
            assert len(h) == LATE_FEW + LATE_MANY and len(strands) == 1 and (h["l"] == mhl).all(), (len(h), strands)
            assert LATE_FEW > 65535 and rows[:LATE_FEW].min() >= 1 and rows[:LATE_FEW].max() <= 4, (rows[:LATE_FEW].min(), rows[:LATE_FEW].max())
            assert rows[LATE_FEW:].min() >= 5 and rows[LATE_FEW:].max() <= 24, (rows[LATE_FEW:].min(), rows[LATE_FEW:].max())
            m = mhl
            windows = np.frombuffer(gs.reads.get(i) + b"N", dtype=np.uint8).reshape(-1, m + 1)[LATE_MANY:, :m]
            L = text_min_l(world.genomes.total_len) - 1
            ends = rows_of_kmers(np.concatenate(world.genomes.seqs), L, of=windows[:, m - L:])
            assert len(windows) == LATE_FEW and ends.min() >= 1 and ends.max() <= 4, (L, ends.min(), ends.max())
            reached["late_hand_over"] = (int(rows[:LATE_FEW].max()), int(rows[LATE_FEW:].min()), int(rows[LATE_FEW:].max()))
        else:
            assert len(h) == gs.tag[i] and len(strands) == 1 and (h["l"] == mhl).all(), (gs.tag[i], len(h), strands)
        assert res["giant_se"][i].nmatch > 0
    reached["many_hits"] = counts
    assert set(MANY_HITS) <= set(counts)

    # length thresholds
    for i in gs.of("length_thresholds"):
        assert _length(gs.reads, i) == gs.tag[i] and res["giant_se"][i].nmatch > 0 and len(hits["giant_se"][i]) >= 20, gs.tag[i]      # (20 of the 40 windows per strand)
    gp = world.batches["giant_pe"]
    for i in range(gp.n):
        assert res["giant_pe"][i].queryLength == _length(gp.reads, i) + _length(gp.mates, i) and res["giant_pe"][i].nmatch > 0

    # range sizes
    sizes = np.concatenate([(h["ep"] - h["sp"] + 1).astype(np.int64) for name in ("small_se", "small_pe") for h in hits[name]])
    reached["hits_with_2_to_4_rows"], reached["hits_with_5_to_24_rows"] = int(((sizes >= 2) & (sizes <= 4)).sum()), int(((sizes >= 5) & (sizes <= 24)).sum())
    assert reached["hits_with_2_to_4_rows"] >= 50 and reached["hits_with_5_to_24_rows"] >= 50, reached

    # ragged pairs
    short = {"0", "1", "mhl-1"}
    for i in pe.of("ragged_pairs"):
        r = res["small_pe"][i]
        assert r.queryLength == _length(pe.reads, i) + _length(pe.mates, i), pe.tag[i]
        if pe.tag[i][0] in RAGGED:
            assert (r.nmatch == 0) == (pe.tag[i][0] in short and pe.tag[i][1] in short), (pe.tag[i], r.nmatch)
        else:
            assert r.nmatch > 0
    assert len(pe.of("ragged_pairs")) == 36 + 4 + 1
    reached["ragged_pair_hits_of_many_hits_mate"] = len(hits["small_pe"][pe.of("ragged_pairs")[-1]])
    assert reached["ragged_pair_hits_of_many_hits_mate"] >= 4095
    return reached
