"""Nine index worlds that differ ONLY in the taxonomy: one text, one set of reads, nine ways of hanging the 64 sequences into a tree - or
into a forest.  Every other tree of the suite is regular, single-rooted at tax id 1 and at most six levels deep; the shapes here are
what pruned NCBI dumps and converted GTDB trees give.  A helper module, not a conftest: tests/test_tax_worlds_oracle_cpu.py,
tests/test_gpu_tax_worlds.py, tests/test_gpu_build.py and tests/golden/make_golden_taxworlds.py import it.

The text: NSEQ = 64 sequences of 1 200 .. 3 400 random bases (below 100 kb in all; ORA_MAX_MATCH = 64 is what the oracle's result
holds).  A *cassette* is an exact 120-base segment copied into a chosen subset of the sequences; a read is a cassette, a window of
one, the reverse complement of either, or a pair of mates out of one cassette or out of two cassettes of the same subset.  So every
such read hits exactly its subset with one score, and the tail has to reduce a KNOWN id set: the taxonomy alone decides the answer.
Subset sizes are SIZES (the eight-entry register fold, the team fold, the single-lane general form); a subset lies in the low half
(sequences 1 .. 31), in the high half (32 .. 62), or spans both and holds sequence 0 ("with_first") or sequence 63 ("with_last") -
the sequences a world puts on a second root, so that the second root comes first or last in the hit list (ascending sequence id).
Two more subsets ("ends") hold only the sequences 0, 63 and 0, 1, 62, 63, which seq_on_roots puts on its two roots: lists of tops only.

A world = (synth.Genomes, single-end ReadSet, (mate 1, mate 2), info).  guards(world, oracle) asserts from the oracle alone that every
cassette read's hit list is exactly its subset, and that the world reaches what info["claims"] says: no family passes quietly."""
from __future__ import annotations

import functools
import os
from typing import NamedTuple

import numpy as np

from centrifuger_amd import synth

ACGT = synth.ACGT
NSEQ, CASSETTE = 64, 120
SIZES = (2, 3, 8, 9, 16, 17, 40, 64)
PAIR_SIZES = (2, 9, 17, 64)           # subsets that hold a second cassette, for the pairs of two cassettes
MAX_TEXT = 100_000
NAMES = ("regular", "orphan_subtree", "two_self_roots", "no_tax_id_1", "seq_on_roots", "deep_chain", "ranks", "outside", "big_ids")
FOREST = ("orphan_subtree", "two_self_roots", "no_tax_id_1", "seq_on_roots")
COMMITTED = ("orphan_subtree", "two_self_roots", "no_tax_id_1")      # tests/golden/taxworlds holds the reference's files for these
FTAB_CHARS = 6                        # as the f6 golden files: a small .1.cfr
RANKS = ["no rank", "strain", "species", "genus", "family", "order", "class", "phylum", "kingdom", "domain", "forma",
         "infraclass", "infraorder", "parvorder", "subclass", "subfamily", "subgenus", "subkingdom", "suborder",
         "subphylum", "subspecies", "subtribe", "superclass", "superfamily", "superkingdom", "superorder", "superphylum",
         "tribe", "varietas", "life", "acellular root"]


class World(NamedTuple):
    genomes: synth.Genomes
    reads: synth.ReadSet
    pairs: tuple
    info: dict


class Cassette(NamedTuple):
    size: int
    pattern: str          # low, high, with_first, with_last, all, ends, twins
    subset: tuple         # ascending sequence numbers
    second: bool          # the subset holds a second cassette as well
    copies: int = 1       # how often every sequence of the subset holds the cassette (more rows than sequences)


# ------------------------------------------------------------------------------------------------ the text and the reads
def _rand(rng, n):
    return ACGT[rng.integers(0, 4, size=int(n))]


def _readset(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return synth.ReadSet(np.concatenate(seqs), offs)


@functools.lru_cache(maxsize=None)
def _text(seed=9301):
    """-> (sequences, cassettes, single reads, (mates 1, mates 2), cassette of every single read, of every pair; -1: none)"""
    rng = np.random.default_rng(seed)
    load = np.zeros(NSEQ, dtype=np.int64)

    def choose(c, allowed):
        allowed = np.array(allowed)
        order = allowed[np.lexsort((rng.random(len(allowed)), load[allowed]))]       # least loaded first, ties at random
        pick = [int(x) for x in order[:c]]
        assert len(pick) == c
        load[pick] += 1
        return pick
    low, high = list(range(1, 32)), list(range(32, 63))
    cassettes = []
    for c in SIZES:
        if c == NSEQ:
            cassettes.append(Cassette(c, "all", tuple(range(NSEQ)), True))
            continue
        if c <= 17:
            cassettes.append(Cassette(c, "low", tuple(sorted(choose(c, low))), False))
            cassettes.append(Cassette(c, "high", tuple(sorted(choose(c, high))), False))
        for pattern, end in (("with_first", 0), ("with_last", NSEQ - 1)):
            n_high = c // 2 if end == 0 else (c - 1) // 2                             # the subset spans both halves, the end counted in
            pick = [end] + choose(n_high, high) + choose(c - 1 - n_high, low)
            cassettes.append(Cassette(c, pattern, tuple(sorted(pick)), pattern == "with_first" and c in PAIR_SIZES))
    # the four sequences that seq_on_roots puts ON its two roots, and no other: a list of tops only.  Two sequences in the register
    # fold; four with the cassette three times each - twelve rows, more than the register fold takes, so a team folds four ids
    cassettes.append(Cassette(2, "ends", (0, NSEQ - 1), False))
    cassettes.append(Cassette(4, "ends", (0, 1, NSEQ - 2, NSEQ - 1), False, copies=3))
    cassettes.append(Cassette(2, "twins", (4, 12), False))             # two sequences of one strain (_half): the answer is a leaf's id
    for cs in cassettes:
        assert len(set(cs.subset)) == cs.size
        assert cs.pattern not in ("with_first", "with_last") or (min(cs.subset) < 32 <= max(cs.subset))
        assert (0 in cs.subset) == (cs.pattern in ("with_first", "all", "ends")) and (NSEQ - 1 in cs.subset) == (cs.pattern in ("with_last", "all", "ends"))
    content = [(_rand(rng, CASSETTE), _rand(rng, CASSETTE) if cs.second else None) for cs in cassettes]
    seqs = []
    for i in range(NSEQ):
        mine = [j for j, cs in enumerate(cassettes) if i in cs.subset]
        rng.shuffle(mine)
        parts = [_rand(rng, 400 if i == 0 else rng.integers(40, 81))]                # (no read lies within 300 bases of the text's ends)
        for j in mine:
            for _ in range(cassettes[j].copies - 1):
                parts.append(content[j][0])
                parts.append(_rand(rng, rng.integers(40, 81)))
            parts.append(content[j][0])
            if content[j][1] is not None:                                             # the second cassette 30 .. 80 bases on, another gap in every sequence
                parts.append(_rand(rng, rng.integers(30, 81)))
                parts.append(content[j][1])
            parts.append(_rand(rng, rng.integers(40, 81)))
        have = sum(len(p) for p in parts)
        parts.append(_rand(rng, max(0, 1200 - have) + (400 if i == NSEQ - 1 else 0)))
        seqs.append(np.concatenate(parts))
        assert 1200 <= len(seqs[-1]) <= 3400, len(seqs[-1])
    assert sum(len(s) for s in seqs) < MAX_TEXT
    cat = np.concatenate(seqs)
    se, se_of, p1, p2, pe_of = [], [], [], [], []
    for j, cs in enumerate(cassettes):
        a, b = content[j]
        se += [a.copy(), synth.revcomp(a)]; se_of += [j, j]
        for q in range(4):                                                           # windows of the cassette, both strands
            L = int(rng.integers(60, 111))
            o = int(rng.integers(0, CASSETTE - L + 1))
            se.append(synth.revcomp(a[o:o + L]) if q % 2 else a[o:o + L].copy()); se_of.append(j)
        m1, m2 = a[:70].copy(), synth.revcomp(a[50:])                                # mates out of one cassette
        if j % 2:
            m1, m2 = m2, m1
        p1.append(m1); p2.append(m2); pe_of.append(j)
        if b is not None:
            se += [b.copy(), synth.revcomp(b)]; se_of += [j, j]
            p1 += [a.copy(), synth.revcomp(b)]; p2 += [synth.revcomp(b), a.copy()]; pe_of += [j, j]      # a pair of two cassettes, both orders
    for _ in range(40):                                                              # windows of the text anywhere, and reads that are in no index
        L = int(rng.integers(40, 151))
        p = int(rng.integers(300, len(cat) - 300 - L))
        se.append(synth.revcomp(cat[p:p + L]) if rng.random() < 0.5 else cat[p:p + L].copy()); se_of.append(-1)
    for _ in range(10):
        se.append(_rand(rng, rng.integers(40, 151))); se_of.append(-1)
    for _ in range(20):
        L, ins = int(rng.integers(40, 121)), int(rng.integers(150, 400))
        p = int(rng.integers(300, len(cat) - 300 - ins))
        p1.append(cat[p:p + L].copy()); p2.append(synth.revcomp(cat[p + ins - L:p + ins])); pe_of.append(-1)
    for _ in range(4):
        p1.append(_rand(rng, 100)); p2.append(_rand(rng, 80)); pe_of.append(-1)
    return seqs, tuple(cassettes), _readset(se), (_readset(p1), _readset(p2)), tuple(se_of), tuple(pe_of)


# ------------------------------------------------------------------------------------------------ the taxonomies
def _half(nodes, names, top_parent, base, tag, strain_of=lambda sp, t: sp * 100 + t):
    """genus `base` below top_parent, four species base + 1 .. base + 4, two strains each; -> the tax ids of 32 sequences: every
    fourth sits on a species, the others on strains (so a subset mixes depths)"""
    nodes.append((base, top_parent, "genus")); names.append((base, f"Genus {tag}"))
    out = []
    for s in range(4):
        sp = base + 1 + s
        nodes.append((sp, base, "species")); names.append((sp, f"Genus {tag} species{s}"))
        for t in (1, 2):
            nodes.append((strain_of(sp, t), sp, "strain")); names.append((strain_of(sp, t), f"{tag} species{s} strain{t}"))
    for j in range(32):
        sp = base + 1 + j % 4
        out.append(sp if j // 4 == 0 else strain_of(sp, 1 + (j // 4) % 2))
    return out


def _regular():
    nodes, names = [(1, 1, "no rank"), (2, 1, "superkingdom")], [(1, "root"), (2, "Bacteria")]
    return nodes, names, _half(nodes, names, 2, 10, "A") + _half(nodes, names, 2, 50, "B")


def _taxonomy(name):
    """-> nodes, tax names, the tax id of every sequence, the ORIGINAL tax id of the root the index must have, claims"""
    if name == "regular":
        return _regular() + (1, ("tree_lca",))
    if name == "orphan_subtree":                    # 50 | 999 | genus with no node 999: the reference adds the phantom nodes 999 and 0
        nodes, names = [(1, 1, "no rank"), (2, 1, "superkingdom")], [(1, "root"), (2, "Bacteria")]
        return nodes, names, _half(nodes, names, 2, 10, "A") + _half(nodes, names, 999, 50, "B"), 0, ("root", "cross_tree")
    if name in ("two_self_roots", "seq_on_roots"):
        nodes, names = [(1, 1, "no rank"), (500, 500, "no rank")], [(1, "root"), (500, "second root")]
        taxids = _half(nodes, names, 1, 10, "A") + _half(nodes, names, 500, 510, "B")
        if name == "two_self_roots":
            return nodes, names, taxids, 1, ("root", "cross_tree")
        taxids[0] = taxids[NSEQ - 1] = 500          # the second root first and last in a hit list
        taxids[1] = taxids[NSEQ - 2] = 1
        return nodes, names, taxids, 1, ("root", "cross_tree", "second_root_first", "second_root_last", "tops_only")
    if name == "no_tax_id_1":
        nodes, names = [(50, 50, "no rank"), (70, 70, "no rank")], [(50, "fifty"), (70, "seventy")]
        return nodes, names, _half(nodes, names, 50, 5000, "A") + _half(nodes, names, 70, 7000, "B"), 50, ("root", "cross_tree")
    if name == "deep_chain":                        # 300 "no rank" nodes below species 11, beside the depth-2 leaves 12 and 13
        nodes = [(1, 1, "no rank"), (2, 1, "superkingdom"), (11, 2, "species"), (12, 2, "species"), (13, 2, "species")]
        names = [(1, "root"), (2, "Bacteria"), (11, "eleven"), (12, "twelve"), (13, "thirteen")]
        for q in range(1, 301):
            nodes.append((30000 + q, 11 if q == 1 else 30000 + q - 1, "no rank")); names.append((30000 + q, f"link {q}"))
        return nodes, names, [(30300, 30299, 12, 13)[i % 4] for i in range(NSEQ)], 1, ("tree_lca", "depth_difference_299", "depth_difference_1")
    if name == "ranks":
        nodes, names = [(1, 1, "no rank")], [(1, "root")]
        taxids = []
        for r, rank in enumerate(RANKS):            # all 31 rank codes, in paths of two
            nodes.append((2000 + r, 2000 + r - 1 if r % 2 else 1, rank)); names.append((2000 + r, f"rank {rank}"))
            taxids.append(2000 + r)
        for base, ranks in ((3000, ("species", "genus", "strain")),                  # a genus below a species
                            (3100, ("species", "species", "species")),               # a rank repeated on one path
                            (3200, ("clade", "serotype", "species")),                # rank strings the table does not know
                            (3300, ("no rank", "no rank", "no rank")),               # a path with no ranked node
                            (3400, ("genus", "species", "strain"))):
            for q, rank in enumerate(ranks):
                nodes.append((base + q, base + q - 1 if q else 1, rank)); names.append((base + q, f"node {base + q}"))
            n = 6 if base < 3400 else NSEQ - len(taxids)
            taxids += [base + 1 + q % 2 for q in range(n)]
        return nodes, names, taxids, 1, ("root", "tree_lca")
    if name == "outside":                           # one sequence whose tax id the tree lacks: compact id 0
        nodes, names, taxids = _regular()
        taxids[5] = 777777
        return nodes, names, taxids, 1, ("tree_lca", "outside_id")
    if name == "big_ids":                           # tax ids above 2^32 and near 2^63
        nodes, names = [(1, 1, "no rank"), (2, 1, "superkingdom")], [(1, "root"), (2, "Bacteria")]
        big = lambda sp, t: (1 << 63) - 100000 + (sp & 0xffff) * 100 + t
        return nodes, names, _half(nodes, names, 2, (1 << 32) + 10, "A", big) + _half(nodes, names, 2, (1 << 33) + 50, "B", big), 1, ("tree_lca", "id_above_2_32", "id_near_2_63")
    raise KeyError(name)


def tops(nodes):
    """tax id -> the tax id its walk ends on, the reference's way: an id no line names has parent 0, and 0 is its own parent"""
    par = {t: p for t, p, _ in reversed(nodes)}     # (the first line of an id wins)
    out = {}
    for t in list(par):
        x, seen = t, set()
        while par.get(x, 0) != x and x not in seen:
            seen.add(x)
            x = par.get(x, 0)
        out[t] = x
    return out


@functools.lru_cache(maxsize=None)
def make(name) -> World:
    seqs, cassettes, reads, pairs, se_of, pe_of = _text()
    nodes, names, taxids, root_taxid, claims = _taxonomy(name)
    assert len(taxids) == NSEQ and len({t for t, _, _ in nodes}) == len(nodes)
    g = synth.Genomes([f"TW_{i:02d}.1" for i in range(NSEQ)], list(taxids), seqs, nodes, names)
    info = {"name": name, "ftab_chars": FTAB_CHARS, "cassettes": cassettes, "read_cassette": se_of, "pair_cassette": pe_of,
            "root_taxid": root_taxid, "claims": claims}
    return World(g, reads, pairs, info)


def build_kwargs(world):
    return {"ftab_chars": world.info["ftab_chars"]}


def write_reads(world, d):
    """se.fq, p_1.fq, p_2.fq under d (ids r0, r1, ..)"""
    synth.write_fastq(world.reads, os.path.join(d, "se.fq"))
    synth.write_fastq(world.pairs[0], os.path.join(d, "p_1.fq"), suffix="/1")
    synth.write_fastq(world.pairs[1], os.path.join(d, "p_2.fq"), suffix="/2")


# ------------------------------------------------------------------------------------------------ guards
def subset_kinds(world):
    """per cassette: (spans two trees, the second root first, the second root last) - from the world's own nodes"""
    g, info = world.genomes, world.info
    top = tops(g.nodes)
    self_parented = {t for t, p, _ in g.nodes if t == p}
    out = []
    for cs in info["cassettes"]:
        tids = [g.taxids[i] for i in cs.subset]
        in_tree = [t for t in tids if t in top]
        second = lambda t: t in self_parented and t != info["root_taxid"]
        plain = any(t not in self_parented for t in in_tree)
        out.append((len({top[t] for t in in_tree}) > 1, second(tids[0]) and plain, second(tids[-1]) and not second(tids[0]) and plain))
    return out


def tree_lca(nodes, root, ids):
    """the lowest common ancestor in a single-rooted tree, from the lines of nodes.dmp alone: ids the tree lacks count as the root,
    and the root takes no part (Taxonomy::LCA)"""
    par = {t: p for t, p, _ in reversed(nodes)}
    ids = [t for t in ids if t in par and t != root]
    if not ids:
        return root

    def path(t):
        out = [t]
        while par[out[-1]] != out[-1]:
            out.append(par[out[-1]])
        return out
    others = [set(path(t)) for t in ids[1:]]
    return next(x for x in path(ids[0]) if all(x in o for o in others))


def guards(world, oracle):
    """oracle: oracle_lib.OracleIndex with max_result = 1 on an index of this world.  Returns the values reached."""
    info, g = world.info, world.genomes
    assert oracle.param.maxResult == 1
    cassettes = info["cassettes"]
    located = {}

    def seq_ids(h):
        key = (int(h["sp"]), int(h["ep"]))
        if key not in located:
            located[key] = tuple(sorted({oracle.locate(r)[0] for r in range(key[0], key[1] + 1)}))
        return located[key]
    rs, (r1, r2) = world.reads, world.pairs
    for i, j in enumerate(info["read_cassette"]):
        if j < 0:
            continue
        hits = oracle.query_hits(rs.get(i), None)
        assert len(hits) == 1 and seq_ids(hits[0]) == cassettes[j].subset, (info["name"], "read", i, cassettes[j])
    for i, j in enumerate(info["pair_cassette"]):
        if j < 0:
            continue
        hits = oracle.query_hits(r1.get(i), r2.get(i))
        assert len(hits) == 2 and all(seq_ids(h) == cassettes[j].subset for h in hits), (info["name"], "pair", i, cassettes[j])
    se = oracle.classify(rs.bases, rs.offsets, threads=4)
    kinds = subset_kinds(world)
    reached = {"root": 0, "cross_tree": 0, "second_root_first": 0, "second_root_last": 0, "classified": 0, "tree_lca": 0, "tops_only": 0,
               "depth_difference_299": 0, "depth_difference_1": 0, "outside_id": 0, "id_above_2_32": 0, "id_near_2_63": 0}
    par = {t: p for t, p, _ in reversed(g.nodes)}
    tops_of_world = {t for t, p in par.items() if t == p}

    def depth(t):
        d = 0
        while par[t] != t:
            t = par[t]; d += 1
        return d
    for i, j in enumerate(info["read_cassette"]):
        if j < 0:
            continue
        assert se[i].nmatch == 1, (info["name"], i)
        reached["classified"] += 1
        cross, first, last = kinds[j]
        is_root = se[i].kind[0] == 1 and int(se[i].taxid[0]) == info["root_taxid"]
        reached["root"] += is_root
        reached["cross_tree"] += cross
        reached["second_root_first"] += first
        reached["second_root_last"] += last
        if first:
            assert is_root, (info["name"], i, "a second root in front of a plain id gives the root (Taxonomy.hpp:746-762)")
        if cross and not first and not last and not any(t == p for t, p, _ in g.nodes if t in {g.taxids[q] for q in cassettes[j].subset}):
            assert is_root, (info["name"], i, "ids of two trees meet in the root")
        tids = [g.taxids[q] for q in cassettes[j].subset]
        got = int(se[i].taxid[0])
        if "tree_lca" in info["claims"] and cassettes[j].size <= 40:          # (64 rows are sampled at -k 1: 40 of them are located)
            want = tree_lca(g.nodes, info["root_taxid"], tids)
            assert se[i].kind[0] == 1 and got == want, (info["name"], i, cassettes[j], got, want)
            reached["tree_lca"] += 1
            known = [depth(t) for t in tids if t in par]
            spread = max(known) - min(known)
            reached["depth_difference_299"] += spread >= 299
            reached["depth_difference_1"] += spread == 1 and got == min((t for t in tids if t in par), key=depth)
            reached["outside_id"] += any(t not in par for t in tids)
            reached["id_above_2_32"] += (1 << 32) < got < (1 << 62)
            reached["id_near_2_63"] += got >= (1 << 62)
        if all(t in tops_of_world for t in tids) and any(t != info["root_taxid"] for t in tids):
            assert got == next(t for t in tids if t != info["root_taxid"]), (info["name"], i, "tops only: the first that is not the root")
            reached["tops_only"] += 1
    for claim in info["claims"]:
        assert reached[claim] > 0, (info["name"], claim, reached)
    return reached
