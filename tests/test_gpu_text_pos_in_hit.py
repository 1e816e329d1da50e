"""Text-space hits that carry their rows' text positions (kVirtInline, csrc/cfr_kernels.hip.inc): a search of k_search_chains_v2 that ends
on the text with one row, or with two rows of a 32-bit image, writes the positions it holds in registers into the hit, and virt_text_pos
answers from them without a suffix-array entry.  Hits of 3 and more rows, two-row hits of a 36-bit image and the lookup stage of the
two-launch search keep the form with the entry range and the mask, so one read's list can hold both.

Two small indexes written once per module by the native writer: `unique` (six unrelated random sequences: every kept hit is one row) and
`strains` (three species of twelve strains, strain k 0.4 k % from its base: searches end with 1 .. 12 rows, and a read of twelve rows
has more (strand, sequence) entries than the post stage folds in registers: it needs the scratch pool).  Their reads are windows of the text with
substitutions and N's, plus the producer's edges: a match that ends at an N, at a mismatch and with the read used up, and windows of
the first and the last 48 bases of the text and of sequences on both strands (a row at text position 0, rows closer to 0 than a step).
Single-end reads run with -k 1, pairs with -k 5.

Every expected row is the C oracle's (tests/oracle_lib.py), computed once.  The library runs in this process with its defaults and in
one child process per set of switches (they are read once per process); the child started with CFR_SEARCH_PROF=1 also reports how many
text hits were written and how many of them inline: all of them on `unique`, some but not all on `strains` - a dead path fails here.
Integer work: everything is bit-exact.  -m gpu."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT          # (first: it puts the repository on sys.path, which the child process needs too)

import oracle_lib as ora
from centrifuger_amd import capi, synth

pytestmark = pytest.mark.gpu

WORLDS = ("unique", "strains")
ENDS = (("se", 1), ("pe", 5))           # single-end reads with -k 1, pairs with -k 5
EDGE = 48
SWITCHES = {
    "prof": {"CFR_SEARCH_PROF": "1"},                                                # the defaults, counted
    "wide_36_bit": {"CFR_FORCE_WIDE": "1"},                                         # two-row hits keep the mask, one-row hits go inline
    "search_split": {"CFR_SEARCH_SPLIT": "1"},                                      # stage 1 writes the mask form, stage 2 the inline one
    "two_kernel_post_stage": {"CFR_FUSED_POST": "0"},                              # rows leave through k_enum_rows
    "post_fast": {"CFR_POST_FAST": "1"},
    # the multi-kernel form after the pool ran dry (CFR_POST_STATS: the library says on stderr when that happened)
    # (CFR_TEAM_TAIL=0: reads with more than eight entries take their table from the pool instead of a team's LDS)
    "post_pool_overflow_redo": {"CFR_POOL_CAP": "3", "CFR_TEAM_TAIL": "0", "CFR_SUBBATCH": "50", "CFR_TAPER_FLOOR": "0", "CFR_POST_STATS": "1"},
}


# ------------------------------------------------------------------------------------------------ the two worlds
def _genomes(name):
    if name == "unique":
        return synth.make_genomes(n_species=6, n_strains=1, genome_len=20000, seed=7301)
    return synth.make_genomes(n_species=3, n_strains=12, genome_len=5000, seed=7302, divergence_step=0.004)


def _edge_reads(g, rng):
    """the producer's edges, as a list of uint8 arrays"""
    cat = np.concatenate(g.seqs)
    n = len(cat)
    starts = np.cumsum([0] + [len(s) for s in g.seqs])
    out = []

    def both(s):
        out.append(np.ascontiguousarray(s))
        out.append(synth.revcomp(np.ascontiguousarray(s)))

    def junk(k):
        return synth.ACGT[rng.integers(0, 4, size=k)]
    for b in [int(x) for x in starts]:                   # the text's two ends and every sequence boundary
        for L in (30, 40, EDGE):
            if b + L <= n:
                w = cat[b:b + L]                         # the first L bases of the text / of a sequence
                both(w)
                both(np.concatenate([junk(25), w]))      # ... reached by a search that cannot go on to the left
                both(np.concatenate([w, junk(25)]))
            if b - L >= 0:
                w = cat[b - L:b]                         # the last L bases of the text / of a sequence
                both(w)
                both(np.concatenate([junk(25), w]))
                both(np.concatenate([w, junk(25)]))
        if b - EDGE >= 0 and b + EDGE <= n:
            both(cat[b - EDGE:b + EDGE])                 # across the boundary
            both(cat[b - 3:b + 60])                      # rows that come closer to the boundary than one text step
            both(cat[b - 60:b + 3])
    for j in range(60):
        p = int(rng.integers(0, n - 150))
        w = cat[p:p + 150].copy()
        kind = j % 3
        if kind == 0:                                    # the match ends at an N (both halves long enough to be kept)
            w[int(rng.integers(40, 110))] = ord("N")
        elif kind == 1:                                  # ... at a mismatch
            q = int(rng.integers(40, 110))
            w[q] = synth.ACGT[(int(np.searchsorted(synth.ACGT, w[q])) + 1 + int(rng.integers(0, 3))) & 3]
        both(w)                                          # kind 2: the read is used up
        both(w[:int(rng.integers(30, 150))])
    return out


def _readset(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return synth.ReadSet(np.ascontiguousarray(np.concatenate(seqs), dtype=np.uint8), offs)


def _split(rs):
    return [rs.bases[int(rs.offsets[i]):int(rs.offsets[i + 1])] for i in range(rs.n)]


def _reads(name, g):
    """{"se": (bases, offsets, None, None), "pe": (bases 1, offsets 1, bases 2, offsets 2)}"""
    rng = np.random.default_rng(7400 + len(name))
    edges = _edge_reads(g, rng)
    se = _split(synth.make_reads(g, 2000, 100, seed=7311)) + _split(synth.make_reads(g, 500, 37, seed=7312)) + edges
    p1, p2 = synth.make_pairs(g, 1000, 100, seed=7313)
    m1, m2 = _split(p1), _split(p2)
    order = rng.permutation(len(edges))
    for i, j in enumerate(order):                        # the edges as mates: once with each other, once beside a window of the text
        m1.append(edges[i]); m2.append(edges[int(j)])
    for i in range(0, len(edges), 2):
        m1.append(m1[i % p1.n]); m2.append(edges[i])
    a, b, c = _readset(se), _readset(m1), _readset(m2)
    return {"se": (a.bases, a.offsets, None, None), "pe": (b.bases, b.offsets, c.bases, c.offsets)}


class _Setup:
    def __init__(self, root):
        self.root, self.prefix, self.reads, self.want, self.hits = str(root), {}, {}, {}, {}
        for name in WORLDS:
            g = _genomes(name)
            self.prefix[name] = os.path.join(self.root, name)
            rep = capi.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, self.prefix[name])
            assert rep["n"] == g.total_len
            self.reads[name] = _reads(name, g)
            for ends, k in ENDS:
                b1, o1, b2, o2 = self.reads[name][ends]
                np.savez(os.path.join(self.root, f"{name}_{ends}.npz"), b1=b1, o1=o1, **({} if b2 is None else {"b2": b2, "o2": o2}))
                o = ora.OracleIndex(self.prefix[name], max_result=k)
                res = o.classify(b1, o1, b2, o2, threads=8)
                self.want[(name, ends)] = tuple(o.format(f"r{i}", res[i]) for i in range(len(o1) - 1))
                self.hits[(name, ends)] = [o.query_hits(b1[int(o1[i]):int(o1[i + 1])].tobytes(),
                                                        None if b2 is None else b2[int(o2[i]):int(o2[i + 1])].tobytes()) for i in range(len(o1) - 1)]
                o.close()
        self.children = {}

    def child(self, switches):
        """{(world, ends): (rows, prof)} of a fresh process under SWITCHES[switches]; run once"""
        if switches not in self.children:
            env = dict(os.environ, CFR_DEBUG_ENV="1")
            env.update(SWITCHES[switches])
            out = os.path.join(self.root, f"out_{switches}.json")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), self.root, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT)
            assert r.returncode == 0, f"{switches}: exit {r.returncode}\n{r.stderr.decode()[-2000:]}"
            with open(out) as f:
                rows = json.load(f)
            prof = _parse_prof(r.stderr.decode())
            self.children[switches] = {(n, e): (tuple(x.encode("latin-1") for x in rows[f"{n} {e}"]), prof.get(f"{n} {e}")) for n in WORLDS for e, _ in ENDS}
        return self.children[switches]


def _parse_prof(err):
    """{"world ends": {"text_hits": count, "text_hits_inline": count, "pool_ran_dry": sub-batches}} from the [search prof] lines and the
    post stage's overflow lines behind each [case ...] marker (a key is there only if its line was)"""
    out, case = {}, None
    for line in err.splitlines():
        m = re.match(r"\[case (\w+ \w+)\]", line)
        if m:
            case = m.group(1)
            continue
        m = re.match(r"\[search prof\] reads (\d+) [^:]*:(.*)\(per read\)", line)
        if m and case:
            tok = m.group(2).split()
            per_read = {tok[i]: float(tok[i + 1]) for i in range(0, len(tok) - 1, 2)}
            acc = out.setdefault(case, {})
            for key in ("text_hits", "text_hits_inline"):
                acc[key] = acc.get(key, 0) + int(round(per_read[key] * int(m.group(1))))      # (four decimals: exact below 10 000 reads per launch)
        m = re.match(r"\[cfr\] scratch pool ran dry in (\d+) of \d+ sub-batches", line)
        if m and case:
            acc = out.setdefault(case, {})
            acc["pool_ran_dry"] = acc.get("pool_ran_dry", 0) + int(m.group(1))
    return out


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    return _Setup(tmp_path_factory.mktemp("text_pos_in_hit"))


def _device_rows(prefix, k, b1, o1, b2, o2):
    idx = capi.Index(prefix, capi.default_params(max_result=k))
    dev = capi.DeviceIndex(idx)
    try:
        results, matches = dev.classify(b1.copy(), o1, None if b2 is None else b2.copy(), o2)
        return tuple(idx.format_tsv(f"r{i}", results[i], matches) for i in range(len(o1) - 1))
    finally:
        dev.close()


def _assert_rows(got, want, what):
    assert len(got) == len(want), what
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{what}: {len(bad)} rows differ, first r{bad[0]}: got {got[bad[0]]!r} want {want[bad[0]]!r}"


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("ends", [e for e, _ in ENDS])
def test_the_worlds_hold_what_they_claim(ends, setup):
    """from the oracle alone: every kept hit of `unique` is one row; `strains` ends searches with 1, 2 and 3 or more rows, has reads
    whose list holds a hit of at most two rows beside one of three or more (both forms in one list), and hits of nine rows and more
    (more than the eight entries of the register fold: the pool overflow case needs them)"""
    sizes = [(h["ep"] - h["sp"] + 1) for h in setup.hits[("unique", ends)]]
    assert sum(len(s) for s in sizes) > 1000 and all((s == 1).all() for s in sizes)
    sizes = [(h["ep"] - h["sp"] + 1) for h in setup.hits[("strains", ends)]]
    allsz = np.concatenate(sizes)
    assert all(int((allsz == c).sum()) >= 20 for c in (1, 2, 3, 4, 5)) and int((allsz >= 9).sum()) >= 20, np.bincount(allsz.astype(np.int64))[:14]
    assert sum(1 for s in sizes if len(s) and s.min() <= 2 and s.max() >= 3) >= 20


@pytest.mark.parametrize("ends,k", ENDS)
@pytest.mark.parametrize("name", WORLDS)
def test_rows_equal_oracle(name, ends, k, setup):
    """the defaults, in this process"""
    _assert_rows(_device_rows(setup.prefix[name], k, *setup.reads[name][ends]), setup.want[(name, ends)], f"{name} {ends}")


@pytest.mark.parametrize("ends", [e for e, _ in ENDS])
def test_every_text_hit_of_unique_sequence_is_inline(ends, setup):
    rows, prof = setup.child("prof")[("unique", ends)]
    _assert_rows(rows, setup.want[("unique", ends)], f"unique {ends} under CFR_SEARCH_PROF")
    print("unique", ends, prof)
    assert prof is not None, "no [search prof] line"
    assert prof["text_hits_inline"] == prof["text_hits"] > 0, prof


@pytest.mark.parametrize("ends", [e for e, _ in ENDS])
def test_strains_write_both_forms(ends, setup):
    rows, prof = setup.child("prof")[("strains", ends)]
    _assert_rows(rows, setup.want[("strains", ends)], f"strains {ends} under CFR_SEARCH_PROF")
    print("strains", ends, prof)
    assert prof is not None, "no [search prof] line"
    assert 0 < prof["text_hits_inline"] < prof["text_hits"], prof


@pytest.mark.parametrize("ends", [e for e, _ in ENDS])
@pytest.mark.parametrize("name", WORLDS)
@pytest.mark.parametrize("switches", [s for s in SWITCHES if s != "prof"])
def test_rows_equal_oracle_under_switches(switches, name, ends, setup):
    rows, _ = setup.child(switches)[(name, ends)]
    _assert_rows(rows, setup.want[(name, ends)], f"{name} {ends} under {SWITCHES[switches]}")


@pytest.mark.parametrize("ends", [e for e, _ in ENDS])
def test_the_pool_overflow_case_takes_the_fallback(ends, setup):
    """with three pool entries the twelve-row reads cannot be folded in the one-launch form: the library reports the sub-batches it
    repeated in the multi-kernel form (their rows are compared in test_rows_equal_oracle_under_switches)"""
    _, diag = setup.child("post_pool_overflow_redo")[("strains", ends)]
    print("strains", ends, diag)
    assert diag is not None and diag.get("pool_ran_dry", 0) > 0, diag


# ------------------------------------------------------------------------------------------------ the child process
def _child(root, out):
    rows = {}
    for name in WORLDS:
        for ends, k in ENDS:
            z = np.load(os.path.join(root, f"{name}_{ends}.npz"))
            sys.stderr.write(f"[case {name} {ends}]\n")
            sys.stderr.flush()
            got = _device_rows(os.path.join(root, name), k, z["b1"], z["o1"], z["b2"] if "b2" in z else None, z["o2"] if "o2" in z else None)
            rows[f"{name} {ends}"] = [r.decode("latin-1") for r in got]
    with open(out, "w") as f:
        json.dump(rows, f)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
