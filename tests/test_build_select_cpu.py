"""The selection (select_genomes in csrc/cfr_build.cpp: two-column file lists, --subset-tax, --concat-tax-genome) and the taxonomy files
without a GPU: tools/dbg/select_writer_host.cpp compiles cfr_build.cpp and the front end's host twin with g++ and puts a naive suffix
sort in the device's place; its files for the runs of tests/buildsel_world.py against what the reference builder wrote for them
(tests/golden/buildsel): .2.cfr and .3.cfr byte for byte, .1.cfr field by field.  Every run at two chunk sizes: whole files, and 1 KiB
chunks that cut every record into pieces."""
import gzip
import os
import shutil
import subprocess

import pytest

import buildsel_world as bw
from centrifuger_amd import capi
from cfr_fields import parse_1cfr
from conftest import GOLDEN, ROOT

GOLD = os.path.join(GOLDEN, "buildsel")
NAMES = ["concat", "subset", "filelist", "filelist_concat", "concat_uncat"]


@pytest.fixture(scope="module")
def writer(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("selw") / "select_writer_host")
    csrc = os.path.join(ROOT, "centrifuger_amd", "csrc")
    subprocess.run([gxx, "-O2", "-std=c++17", "-I", csrc, "-o", exe, os.path.join(ROOT, "tools", "dbg", "select_writer_host.cpp"),
                    os.path.join(csrc, "cfr_build.cpp"), os.path.join(csrc, "cfr_refseq.cpp"), "-lpthread"], check=True)
    return exe


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return bw.write_inputs(str(tmp_path_factory.mktemp("selworld")))


def same_as_golden(prefix, name, tmp_path):
    ref1 = str(tmp_path / (name + ".ref.1.cfr"))
    with gzip.open(os.path.join(GOLD, name + ".1.cfr.gz"), "rb") as fi, open(ref1, "wb") as fo:
        fo.write(fi.read())
    for k in (2, 3):
        assert open(f"{prefix}.{k}.cfr", "rb").read() == open(os.path.join(GOLD, f"{name}.{k}.cfr"), "rb").read(), f".{k}.cfr differs"
    mine, ref = parse_1cfr(prefix + ".1.cfr"), parse_1cfr(ref1)
    assert len(mine) == len(ref)
    for (na, va), (nb, vb) in zip(mine, ref):
        assert na == nb and va == vb, f"field {na} differs"


@pytest.mark.parametrize("chunk_log2", [24, 10])
@pytest.mark.parametrize("name", NAMES)
def test_host_writer_equals_the_reference_builder(name, chunk_log2, writer, world, tmp_path):
    table, files = bw.host_runs(world)[name]
    prefix = str(tmp_path / name)
    r = subprocess.run([writer, prefix, str(bw.FTAB), world["nodes"], world["names"]] + table + [str(chunk_log2)] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    same_as_golden(prefix, name, tmp_path)
    if name == "concat_uncat":
        assert b"taxonomy id doesn't exist for uncategorized_contig" in r.stderr


def test_subset_outside_the_tree_and_under_a_leafless_node_find_no_genomes(writer, world, tmp_path):
    for tax in ("999999", "2000000"):
        r = subprocess.run([writer, str(tmp_path / "none"), str(bw.FTAB), world["nodes"], world["names"], world["map"], "0", "0", tax, "0", "24", world["ref"]],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and b"found 0 genomes in the input or after filtering." in r.stderr


def records_of(world, key="ref"):
    h = capi.Refseq(None)
    recs = [(rid, world[key], pcs) for rid, pcs in h.feed_file(open(world[key], "rb").read(), 1 << 24)]
    h.close()
    return recs


def table_of(world):
    g = bw.genomes()
    rows = [ln.split("\t") for ln in open(world["map"]).read().splitlines()]
    return [r[0] for r in rows], [int(r[1]) for r in rows], g.nodes, g.tax_names


def test_selection_rules_through_the_c_abi(world):
    names, taxids, nodes, tax_names = table_of(world)
    recs = records_of(world)
    plain = capi.BuildSelection(names, taxids, nodes, tax_names, recs, ftab_chars=bw.FTAB)
    assert (plain.n_genomes, plain.n_extra, plain.n) == (12, 0, 18000)
    assert len(plain.segments) == 1                                         # every record in order: one run of U
    # subset: Genus0 holds species0 and species1 = 8 of the 12 contigs; the check runs before the unknown-id rule (no extra name)
    sub = capi.BuildSelection(names, taxids, nodes, tax_names, recs + [("stranger", world["ref"], [(0, 500)])], ftab_chars=bw.FTAB, subset_tax=bw.GENUS0)
    assert (sub.n_genomes, sub.n_extra, sub.n) == (8, 0, 12000)
    # a strain node: its two contigs
    one = capi.BuildSelection(names, taxids, nodes, tax_names, recs, ftab_chars=bw.FTAB, subset_tax=taxids[2])
    assert (one.n_genomes, one.n) == (2, 3000)
    # concat: one genome per strain tax id, the stranger under "uncategorized"; a record too short is dropped from its group
    cat = capi.BuildSelection(names, taxids, nodes, tax_names, recs + [("stranger", world["ref"], [(0, 500)]), (names[0] + "x", world["ref"], [(0, 3)])],
                              ftab_chars=bw.FTAB, concat=True)
    assert (cat.n_genomes, cat.n) == (7, 18500)
    # a repeated id is taken once; ignore_uncategorized drops the stranger
    rep = capi.BuildSelection(names, taxids, nodes, tax_names, recs + [recs[0], ("stranger", world["ref"], [(0, 500)])], ftab_chars=bw.FTAB, ignore_uncategorized=True)
    assert (rep.n_genomes, rep.n_extra, rep.n) == (12, 0, 18000)
    with pytest.raises(capi.CfrError) as e:
        capi.BuildSelection(names, taxids, nodes, tax_names, recs, ftab_chars=bw.FTAB, subset_tax=424242)
    assert "found 0 genomes in the input or after filtering." in str(e.value)
    with pytest.raises(capi.CfrError):
        capi.BuildSelection(names, taxids, nodes, tax_names, recs, ftab_chars=4, concat=True, protein=True)


@pytest.mark.parametrize("path,base", [("/a/b/GCF_1.2_x.fna.gz", "GCF_1.2_x"), ("x.fa", "x"), ("dir.d/x.fasta.txt", "x"), ("x.faa.bz2", "x"), ("x.txt", "x"),
                                       ("noext", "noext"), ("a.fna.fa.gz", "a.fna"), ("y.fa.fna", "y"), ("z.fasta", "z"), ("w.gb.gz", "w.gb"), (".fa.gz", "")])
def test_file_base_name_is_get_file_base_name(path, base):
    assert capi.file_base_name(path) == base
