"""The search and post kernels at the read-shape edges: the read world of tests/read_worlds.py (every length 0 .. 130, every buffer
alignment, a non-symbol or a substitution at every position, chimeras, reads of up to 2^20 bases and up to 70 000 hits, ragged pairs) on
an index written by the native writer once per module.  -k 1 and -k 5, single-end and paired: hit lists and TSV rows against the C
oracle for every read, the device's dust pre-step, the packed / resident / compact entries at four pointer alignments, and the
command line with and without the device's parser and formatter.  Integer work: everything is bit-exact.  -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ora
import read_worlds as rw
from centrifuger_amd import capi
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
KS = [1, 5]
# the four batches, and the single reads of 4 094 | 4 095 | 4 096 windows as a batch of their own (for the switch sets of the search in
# tests/test_gpu_variants.py, which run the small set and these)
SEARCHED = rw.BATCHES + ("giant_4095",)
FIELDS = ("sp", "ep", "l", "strand", "offset")


class _ReadWorld:
    """The world, its index files, device images, oracle handles and the oracle's answers: each made on first use, once per module."""

    def __init__(self, d):
        self.d = d
        g = rw.genomes()
        self.prefix = os.path.join(d, "idx")
        rep = capi.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, self.prefix, **rw.build_kwargs())
        assert rep["n"] == g.total_len
        info = capi.Index(self.prefix).info()
        self.world = rw.make(g, info.min_hit_len, info.precompute_width)
        self.devs, self.oracles, self.expected, self.hit_lists, self.files, self.subsets = {}, {}, {}, None, {}, {}

    def batch(self, name):
        return self.subset(name)[0]

    def subset(self, name):
        """(batch, the indexes of its reads in the batch it was cut from - None for a whole batch)"""
        if name not in self.subsets:
            if name in rw.BATCHES:
                self.subsets[name] = (self.world.batches[name], None)
            else:
                b = self.world.batches["giant_se"]
                keep = {"giant_long": b.of("long"), "giant_thresholds": b.of("length_thresholds"),                      # one family alone
                        "giant_4095": [i for i in b.of("many_hits") if b.tag[i] in (4094, 4095, 4096, "alternating")]}[name]
                self.subsets[name] = (b.subset(keep), keep)
        return self.subsets[name]

    def dev(self, k):
        if k not in self.devs:
            self.devs[k] = capi.DeviceIndex(capi.Index(self.prefix, capi.default_params(max_result=k)))
        return self.devs[k]

    def oracle(self, k):
        if k not in self.oracles:
            self.oracles[k] = ora.OracleIndex(self.prefix, max_result=k)
        return self.oracles[k]

    def reads(self, name):
        """(ids, bases 1, offsets 1, bases 2, offsets 2) - fresh copies of the bases: the dust pre-step masks in place"""
        b = self.batch(name)
        if b.mates is None:
            return rw.ids(b), b.reads.bases.copy(), b.reads.offsets, None, None
        return rw.ids(b), b.reads.bases.copy(), b.reads.offsets, b.mates.bases.copy(), b.mates.offsets

    def rows(self, name, k, dust):
        """the oracle's TSV rows, computed once and left unchanged"""
        key = (name, k, dust)
        if key not in self.expected:
            o = self.oracle(k)
            ids, b1, o1, b2, o2 = self.reads(name)
            res = o.classify(b1, o1, b2, o2, dust=dust, threads=8)
            self.expected[key] = tuple(o.format(ids[i], res[i]) for i in range(len(ids)))
        return self.expected[key]

    def hits(self):
        """the oracle's hit lists of the four batches (they do not depend on -k), computed once and left unchanged"""
        if self.hit_lists is None:
            self.hit_lists = rw.hit_lists(self.world, self.oracle(KS[0]))
        return self.hit_lists

    def hits_of(self, name):
        keep = self.subset(name)[1]
        return self.hits()[name] if keep is None else [self.hits()["giant_se"][i] for i in keep]

    def fasta(self, name):
        if name not in self.files:
            self.files[name] = rw.write_fasta(self.batch(name), self.d, name)
        return self.files[name]

    def close(self):
        for d in self.devs.values():
            d.close()
        for o in self.oracles.values():
            o.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = _ReadWorld(str(tmp_path_factory.mktemp("read_world")))
    yield w
    w.close()


def _rows_of(dev, ids, results, matches):
    return tuple(dev.index.format_tsv(ids[i], results[i], matches) for i in range(len(ids)))


def _assert_rows(got, want, what, batch):
    assert len(got) == len(want), (what, len(got), len(want))
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (f"{what}: {len(bad)} of {len(want)} reads differ, first r{bad[0]} ({batch.family[bad[0]]} {batch.tag[bad[0]]}): "
                     f"got {got[bad[0]][:300]!r} want {want[bad[0]][:300]!r}")


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


def test_guards_on_the_native_writers_index(world):
    """the families provoke what they claim on the index the device runs on too (the CPU test checks the Python writer's index)"""
    for k in KS:
        print("read world k", k, rw.guards(world.world, world.oracle(k), k, hits=world.hits()))


@pytest.mark.parametrize("name", SEARCHED)
@pytest.mark.parametrize("k", KS)
def test_hit_lists_equal_oracle(name, k, world):
    """A. SearchForwardAndReverse output (after AdjustHitBoundary + strand choice): every _BWTHit field, read by read - the reads of
    65 535 hits and more included."""
    ids, b1, o1, b2, o2 = world.reads(name)
    hits, hb = world.dev(k).search(b1, o1, b2, o2)
    wants = world.hits_of(name)
    batch = world.batch(name)
    assert len(wants) == len(ids) == len(hb) - 1
    for i, want in enumerate(wants):
        got = hits[int(hb[i]):int(hb[i + 1])]
        same = len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in FIELDS)
        if not same:
            first = next((j for j in range(min(len(got), len(want))) if any(got[f][j] != want[f][j] for f in FIELDS)), min(len(got), len(want)))
            assert False, (ids[i], batch.family[i], batch.tag[i], len(got), len(want), "first difference at hit", first, got[first:first + 3], want[first:first + 3])


@pytest.mark.parametrize("name", SEARCHED)
@pytest.mark.parametrize("k", KS)
def test_tsv_rows_equal_oracle(name, k, world):
    """B. Full Query on the device, formatted like ResultWriter: every read of every family."""
    ids, b1, o1, b2, o2 = world.reads(name)
    dev = world.dev(k)
    got = _rows_of(dev, ids, *dev.classify(b1, o1, b2, o2))
    _assert_rows(got, world.rows(name, k, False), f"{name} -k {k}", world.batch(name))


@pytest.mark.parametrize("name", ["small_se", "small_pe", "giant_long"])
@pytest.mark.parametrize("k", KS)
def test_device_dust_equals_oracle(name, k, world):
    """C. SDUST on the device in front of the search (reads of 0 .. 100 000 bases; the reads of 1 Mbase and more run with dust off only)."""
    dev = world.dev(k)
    ids, b1, o1, b2, o2 = world.reads(name)
    dev.set_dust(True)
    try:
        got = _rows_of(dev, ids, *dev.classify(b1, o1, b2, o2))
    finally:
        dev.set_dust(False)
    _assert_rows(got, world.rows(name, k, True), f"{name} -k {k} dust", world.batch(name))


def _up(a, shift=0):
    """a on the device, `shift` bytes behind a 256-byte boundary, with 64 spare bytes behind it"""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8)
    t = torch.zeros(len(raw) + shift + 64, dtype=torch.uint8, device="cuda")
    t[shift:shift + len(raw)] = torch.from_numpy(raw.copy())
    return t, t.data_ptr() + shift


@pytest.mark.parametrize("entry", ["packed", "resident_0", "resident_1", "resident_2", "resident_3"])
@pytest.mark.parametrize("name", rw.BATCHES)
@pytest.mark.parametrize("k", KS)
def test_packed_and_resident_entries_equal_oracle(name, k, entry, world):
    """D. The same reads as packed blocks (cfr_classify_batch_packed) and from device memory (cfr_classify_batch_resident) with the
    bases 0, 1, 2 and 3 bytes off a 256-byte boundary (mate 2: two bytes further)."""
    import torch
    ids, b1, o1, b2, o2 = world.reads(name)
    dev, want, batch = world.dev(k), world.rows(name, k, False), world.batch(name)
    if entry == "packed":
        if b2 is None:
            res, mat = dev.classify_packed(capi.pack_reads(b1, threads=3), o1)
        else:
            res, mat = dev.classify_packed(capi.pack_reads(b1, threads=3), o1, capi.pack_reads(b2), o2)
    else:
        shift = int(entry[-1])
        keep_o1, p_o1 = _up(o1.astype(np.int64))
        keep_o2, p_o2 = (None, 0) if b2 is None else _up(o2.astype(np.int64))
        keep1, p1 = _up(b1, shift)
        keep2, p2 = (None, 0) if b2 is None else _up(b2, (shift + 2) & 3)
        torch.cuda.synchronize()
        res, mat = dev.classify_resident(p1, p_o1, len(ids), int(o1[-1]), p2, p_o2, 0 if b2 is None else int(o2[-1]))
        del keep1, keep2, keep_o1, keep_o2
    _assert_rows(_rows_of(dev, ids, res, mat), want, f"{name} -k {k} {entry}", batch)


@pytest.mark.parametrize("name", ["small_se", "small_pe", "giant_thresholds", "giant_long"])
@pytest.mark.parametrize("k", KS)
def test_compact_entry_equals_oracle(name, k, world):
    """E. cfr_classify_batch_resident_compact + expand_compact (a read whose values do not fit the narrow layout comes back through the
    wide side list): the small set, the reads of 32 767 .. 2^20 bases of the `length_thresholds` family, and the `long` family, whose
    exact window of 100 000 bases scores (100 000 - 15)^2 > 2^32 and has to come back through that list."""
    import torch
    batch = world.batch(name)
    ids, b1, o1, b2, o2 = world.reads(name)
    dev, want = world.dev(k), world.rows(name, k, False)
    keep_o1, p_o1 = _up(o1.astype(np.int64))
    keep_o2, p_o2 = (None, 0) if b2 is None else _up(o2.astype(np.int64))
    keep1, p1 = _up(b1)
    keep2, p2 = (None, 0) if b2 is None else _up(b2)
    torch.cuda.synchronize()
    cres, cmat = dev.classify_resident_compact(p1, p_o1, len(ids), int(o1[-1]), p2, p_o2, 0 if b2 is None else int(o2[-1]))
    wide = dev.compact_wide()
    if name == "giant_long":
        exact = [i for i in range(batch.n) if batch.tag[i] == (100000, "exact")]
        assert len(exact) == 1 and exact[0] in np.asarray(wide[0]).tolist(), ("not flagged CFR_COMPACT_WIDE", exact, wide[0])
    res, mat = capi.expand_compact(cres, cmat, k, wide=wide)
    _assert_rows(_rows_of(dev, ids, res, mat), want, f"{name} -k {k} compact", batch)
    del keep1, keep2, keep_o1, keep_o2


@pytest.mark.parametrize("options", ["default", "gpu_parse_gpu_format"])
@pytest.mark.parametrize("name", rw.BATCHES)
def test_command_line_equals_oracle(name, options, world):
    """F. bin/centrifuger on FASTA files (one line per read, up to 2^20 bases): the small set with the default dust pre-step, the giant
    set with --no-dust (the default would mask reads of 1 Mbase and more on the device)."""
    dust = name.startswith("small")
    args = [CLI, "-x", world.prefix, "-t", "3"] + world.fasta(name) + ([] if dust else ["--no-dust"])
    if options == "gpu_parse_gpu_format":
        args += ["--gpu-parse", "--gpu-format"]
    out = subprocess.run(args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    want = world.rows(name, 1, dust)
    _assert_rows(_by_read(out, rw.ids(world.batch(name))), want, f"{name} {options}", world.batch(name))
