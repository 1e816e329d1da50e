"""The translated search and its post stage on proteomes that are not random residues: the four worlds of tests/protein_worlds.py
(a block in 2 .. 40 proteins whose copies differ in single residues around the hand-over to text mode; homopolymers and tandem repeats;
proteins of 3 .. 5 000 residues under an irregular taxonomy; reads with segments in two frames and on two strands), written by the native
writer once per module.  For every world, -k 1 and -k 5, single-end and paired: hit lists and TSV rows of every read against the C
oracle, the command line, and (where oracle/_ref is present) the reference binary on the same index files.  Bit-exact.  -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ora
import protein_worlds as pw
from centrifuger_amd import capi
from conftest import REF_DIR, ROOT, have_ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
KS = [1, 5]
ENDS = ["se", "pe"]


class Worlds:
    """Worlds, their index files, device images and oracle handles: each made on first use, once per module."""

    def __init__(self, factory):
        self.factory, self.built, self.devs, self.oracles, self.expected, self.hit_lists = factory, {}, {}, {}, {}, {}

    def world(self, name):
        if name not in self.built:
            w = pw.make(name)
            d = str(self.factory.mktemp(name))
            g = w.genomes
            prefix = os.path.join(d, "idx")
            rep = capi.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, prefix, **pw.build_kwargs(w))
            assert rep["n"] == w.info["n_text"]
            pw.write_reads(w, d)
            self.built[name] = (w, d, prefix)
        return self.built[name]

    def dev(self, name, k):
        if (name, k) not in self.devs:
            idx = capi.Index(self.world(name)[2], capi.default_params(max_result=k))
            assert idx.info().is_protein == 1 and idx.info().min_hit_len == pw.MIN_HIT_LEN
            self.devs[(name, k)] = capi.DeviceIndex(idx)
        return self.devs[(name, k)]

    def oracle(self, name, k):
        if (name, k) not in self.oracles:
            self.oracles[(name, k)] = ora.OracleIndex(self.world(name)[2], max_result=k)
        return self.oracles[(name, k)]

    def reads(self, name, ends):
        w = self.world(name)[0]
        if ends == "se":
            return [f"r{i}" for i in range(w.reads.n)], w.reads.bases, w.reads.offsets, None, None
        r1, r2 = w.pairs
        return [f"r{i}" for i in range(r1.n)], r1.bases, r1.offsets, r2.bases, r2.offsets

    def rows(self, name, k, ends):
        """the oracle's TSV rows, computed once and left unchanged"""
        key = (name, k, ends)
        if key not in self.expected:
            o = self.oracle(name, k)
            ids, b1, o1, b2, o2 = self.reads(name, ends)
            res = o.classify(b1, o1, b2, o2, threads=8)
            self.expected[key] = tuple(o.format(ids[i], res[i]) for i in range(len(ids)))
        return self.expected[key]

    def hits(self, name):
        if name not in self.hit_lists:
            self.hit_lists[name] = pw.hit_lists(self.world(name)[0], self.oracle(name, KS[0]))
        return self.hit_lists[name]

    def close(self):
        for d in self.devs.values():
            d.close()
        for o in self.oracles.values():
            o.close()


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    ws = Worlds(tmp_path_factory)
    yield ws
    ws.close()


def device_rows(dev, ids, b1, o1, b2, o2):
    results, matches = dev.classify(b1, o1, b2, o2)
    return tuple(dev.index.format_tsv(ids[i], results[i], matches) for i in range(len(ids)))


def by_read(stdout, ids):
    """a TSV (header, then one row per match, a read's rows back to back in input order) cut into one entry per read"""
    assert stdout.startswith(capi.tsv_header())
    out, lines, q = [], stdout[len(capi.tsv_header()):].split(b"\n")[:-1], 0
    for rid in ids:
        a = q
        while q < len(lines) and lines[q].split(b"\t")[0] == rid.encode():
            q += 1
        out.append(b"".join(r + b"\n" for r in lines[a:q]))
    assert q == len(lines), lines[q]
    return tuple(out)


def assert_rows(got, want, what):
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{what}: {len(bad)} rows differ, first r{bad[0]}: got {got[bad[0]]!r} want {want[bad[0]]!r}"


@pytest.mark.parametrize("name", pw.NAMES)
def test_world_guards_on_the_native_writers_index(name, worlds):
    """the world provokes what it claims on the index the device runs on too (the CPU test checks the host writer's index)"""
    for k in KS:
        print(name, "k", k, pw.guards(worlds.world(name)[0], worlds.oracle(name, k), k, hits=worlds.hits(name)))


@pytest.mark.parametrize("name", pw.NAMES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ends", ENDS)
def test_hit_lists_equal_oracle(name, k, ends, worlds):
    """TranslatedSearch + the strand choice: every _BWTHit field, read by read."""
    ids, b1, o1, b2, o2 = worlds.reads(name, ends)
    hits, hb = worlds.dev(name, k).search(b1, o1, b2, o2)
    wants = worlds.hits(name)[ends]
    assert len(wants) == len(ids)
    for i, want in enumerate(wants):
        got = hits[int(hb[i]):int(hb[i + 1])]
        same = len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in ("sp", "ep", "l", "strand", "offset"))
        if not same:
            r1 = b1[int(o1[i]):int(o1[i + 1])].tobytes()
            r2 = None if b2 is None else b2[int(o2[i]):int(o2[i + 1])].tobytes()
            assert False, (ids[i], r1, r2, got, want)


@pytest.mark.parametrize("name", pw.NAMES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ends", ENDS)
def test_tsv_rows_equal_oracle(name, k, ends, worlds):
    """Full Query on the device (text mode, hits in text-position space), formatted like ResultWriter: every read's row."""
    got = device_rows(worlds.dev(name, k), *worlds.reads(name, ends))
    assert_rows(got, worlds.rows(name, k, ends), f"{name} -k {k} {ends}")


def _cli_args(d, ends):
    return ["-u", os.path.join(d, "se.fq")] if ends == "se" else ["-1", os.path.join(d, "p_1.fq"), "-2", os.path.join(d, "p_2.fq")]


@pytest.mark.parametrize("name,k,ends", [("shared", 5, "se"), ("repeats", 1, "se"), ("ragged", 5, "pe"), ("frames", 1, "pe")])
def test_command_line_equals_oracle(name, k, ends, worlds):
    """bin/centrifuger on the world's FASTQ files."""
    _, d, prefix = worlds.world(name)
    want = worlds.rows(name, k, ends)
    out = subprocess.run([CLI, "-x", prefix, "-t", "3", "-k", str(k)] + _cli_args(d, ends), check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                         timeout=120).stdout
    assert_rows(by_read(out, [f"r{i}" for i in range(len(want))]), want, f"{name} -k {k} {ends} command line")


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
@pytest.mark.parametrize("name", pw.NAMES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ends", ENDS)
def test_reference_binary_equals_device(name, k, ends, worlds):
    """The reference binary on the native writer's index files and the same reads against the device's TSV."""
    _, d, prefix = worlds.world(name)
    want = subprocess.run([os.path.join(REF_DIR, "centrifuger"), "-x", prefix, "-t", "4", "-k", str(k)] + _cli_args(d, ends),
                          check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120).stdout
    got = device_rows(worlds.dev(name, k), *worlds.reads(name, ends))
    assert_rows(got, by_read(want, [f"r{i}" for i in range(len(got))]), f"{name} -k {k} {ends} reference")
