"""The search and post kernels on indexes whose text is not random DNA: the four worlds of tests/index_worlds.py (a block shared by
2 .. 60 sequences across species and genera; reverse-complemented blocks, an inverted repeat and palindromes; tandem repeats and
homopolymers; sequences of 7 .. 30 000 bases under an irregular taxonomy), written by the native writer once per module.  For every
world, -k 1 and -k 5, single-end and paired: hit lists and TSV rows against the C oracle, the device's dust pre-step, the command line,
and (where oracle/_ref is present) the reference binary on the same index files.  Integer work: everything is bit-exact.  -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import index_worlds as iw
import oracle_lib as ora
from centrifuger_amd import capi
from conftest import REF_DIR, ROOT, have_ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
KS = [1, 5]
ENDS = ["se", "pe"]


class _Worlds:
    """Worlds, their index files, device images and oracle handles: each made on first use, once per module."""

    def __init__(self, factory):
        self.factory, self.built, self.devs, self.oracles, self.expected, self.hit_lists = factory, {}, {}, {}, {}, {}

    def world(self, name):
        if name not in self.built:
            w = iw.make(name)
            d = str(self.factory.mktemp(name))
            g = w.genomes
            prefix = os.path.join(d, "idx")
            rep = capi.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, prefix, **iw.build_kwargs(w))
            assert rep["n"] == g.total_len
            iw.write_reads(w, d)
            self.built[name] = (w, d, prefix)
        return self.built[name]

    def dev(self, name, k):
        if (name, k) not in self.devs:
            idx = capi.Index(self.world(name)[2], capi.default_params(max_result=k))
            self.devs[(name, k)] = capi.DeviceIndex(idx)
        return self.devs[(name, k)]

    def oracle(self, name, k):
        if (name, k) not in self.oracles:
            self.oracles[(name, k)] = ora.OracleIndex(self.world(name)[2], max_result=k)
        return self.oracles[(name, k)]

    def reads(self, name, ends):
        """(ids, bases 1, offsets 1, bases 2, offsets 2) - fresh copies of the bases: the dust pre-step masks in place"""
        w = self.world(name)[0]
        if ends == "se":
            return [f"r{i}" for i in range(w.reads.n)], w.reads.bases.copy(), w.reads.offsets, None, None
        r1, r2 = w.pairs
        return [f"r{i}" for i in range(r1.n)], r1.bases.copy(), r1.offsets, r2.bases.copy(), r2.offsets

    def rows(self, name, k, ends, dust):
        """the oracle's TSV rows, computed once and left unchanged"""
        key = (name, k, ends, dust)
        if key not in self.expected:
            o = self.oracle(name, k)
            ids, b1, o1, b2, o2 = self.reads(name, ends)
            res = o.classify(b1, o1, b2, o2, dust=dust, threads=8)
            self.expected[key] = tuple(o.format(ids[i], res[i]) for i in range(len(ids)))
        return self.expected[key]

    def hits(self, name):
        """the oracle's hit lists {"se": [...], "pe": [...]} (they do not depend on -k), computed once and left unchanged"""
        if name not in self.hit_lists:
            self.hit_lists[name] = iw.hit_lists(self.world(name)[0], self.oracle(name, KS[0]))
        return self.hit_lists[name]

    def close(self):
        for d in self.devs.values():
            d.close()
        for o in self.oracles.values():
            o.close()


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    ws = _Worlds(tmp_path_factory)
    yield ws
    ws.close()


def _device_rows(dev, ids, b1, o1, b2, o2):
    results, matches = dev.classify(b1, o1, b2, o2)
    return tuple(dev.index.format_tsv(ids[i], results[i], matches) for i in range(len(ids)))


def _by_read(stdout, ids):
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


def _assert_rows(got, want, what):
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{what}: {len(bad)} rows differ, first r{bad[0]}: got {got[bad[0]]!r} want {want[bad[0]]!r}"


@pytest.mark.parametrize("name", iw.NAMES)
def test_world_guards_on_the_native_writers_index(name, worlds):
    """the world provokes what it claims on the index the device runs on too (the CPU test checks the Python writer's index)"""
    for k in KS:
        print(name, "k", k, iw.guards(worlds.world(name)[0], worlds.oracle(name, k), k, hits=worlds.hits(name)))


@pytest.mark.parametrize("name", iw.NAMES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ends", ENDS)
def test_hit_lists_equal_oracle(name, k, ends, worlds):
    """A. SearchForwardAndReverse output (after AdjustHitBoundary + strand choice): every _BWTHit field, read by read."""
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


@pytest.mark.parametrize("name", iw.NAMES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ends", ENDS)
def test_tsv_rows_equal_oracle(name, k, ends, worlds):
    """B. Full Query on the device, formatted like ResultWriter: every read's row."""
    got = _device_rows(worlds.dev(name, k), *worlds.reads(name, ends))
    _assert_rows(got, worlds.rows(name, k, ends, False), f"{name} -k {k} {ends}")


@pytest.mark.parametrize("name", ["repeats", "strands"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ends", ENDS)
def test_device_dust_equals_oracle(name, k, ends, worlds):
    """C. SDUST on the device in front of the search: repeats and palindromes are what it masks."""
    dev = worlds.dev(name, k)
    dev.set_dust(True)
    try:
        got = _device_rows(dev, *worlds.reads(name, ends))
    finally:
        dev.set_dust(False)
    want = worlds.rows(name, k, ends, True)
    _assert_rows(got, want, f"{name} -k {k} {ends} dust")
    if ends == "se":
        assert want != worlds.rows(name, k, ends, False), "dust changed no row of this world"


def _cli_args(d, ends):
    return ["-u", os.path.join(d, "se.fq")] if ends == "se" else ["-1", os.path.join(d, "p_1.fq"), "-2", os.path.join(d, "p_2.fq")]


@pytest.mark.parametrize("name,options", [(n, "default") for n in iw.NAMES] + [("shared", "nodust_k5_pe"), ("strands", "nodust_k5_pe")])
def test_command_line_equals_oracle(name, options, worlds):
    """D. bin/centrifuger on the world's FASTQ files."""
    _, d, prefix = worlds.world(name)
    if options == "default":
        args, want = _cli_args(d, "se"), worlds.rows(name, 1, "se", True)
    else:
        args, want = ["--no-dust", "-k", "5"] + _cli_args(d, "pe"), worlds.rows(name, 5, "pe", False)
    out = subprocess.run([CLI, "-x", prefix, "-t", "3"] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    _assert_rows(_by_read(out, [f"r{i}" for i in range(len(want))]), want, f"{name} {options}")


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
@pytest.mark.parametrize("name", iw.NAMES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ends", ENDS)
def test_reference_binary_equals_device(name, k, ends, worlds):
    """E. The reference binary on the same index files and reads (dust on, as it runs by default) against the device's TSV."""
    _, d, prefix = worlds.world(name)
    want = subprocess.run([os.path.join(REF_DIR, "centrifuger"), "-x", prefix, "-t", "4", "-k", str(k)] + _cli_args(d, ends),
                          check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    dev = worlds.dev(name, k)
    dev.set_dust(True)
    try:
        got = _device_rows(dev, *worlds.reads(name, ends))
    finally:
        dev.set_dust(False)
    _assert_rows(got, _by_read(want, [f"r{i}" for i in range(len(got))]), f"{name} -k {k} {ends} reference")
