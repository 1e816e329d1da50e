"""bin/centrifuger-build with a two-column -l list, --subset-tax and --concat-tax-genome, alone and combined: its files against what the
reference builder wrote for the runs of tests/buildsel_world.py (tests/golden/buildsel), with the front end's default chunks and with
1 KiB chunks (CFR_REFSEQ_CHUNK_LOG2); the refusal of a subset id outside the tree; this project's classifier on the golden indexes
against the reference classifier's TSV; and, with oracle/_ref, a live comparison on one messy input that combines all three.  -m gpu."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import buildsel_world as bw
from cfr_fields import parse_1cfr
from conftest import GOLDEN, REF_DIR, ROOT, have_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(GOLDEN, "buildsel")
BUILD = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger-build")
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
NAMES = ["concat", "subset", "filelist", "filelist_concat", "concat_uncat"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return bw.write_inputs(str(tmp_path_factory.mktemp("selworld")))


def golden_index(name, tmp_path):
    prefix = str(tmp_path / (name + ".ref"))
    with gzip.open(os.path.join(GOLD, name + ".1.cfr.gz"), "rb") as fi, open(prefix + ".1.cfr", "wb") as fo:
        fo.write(fi.read())
    for k in (2, 3):
        with open(os.path.join(GOLD, f"{name}.{k}.cfr"), "rb") as fi, open(f"{prefix}.{k}.cfr", "wb") as fo:
            fo.write(fi.read())
    return prefix


def same_index(prefix, ref):
    for k in (2, 3):
        assert open(f"{prefix}.{k}.cfr", "rb").read() == open(f"{ref}.{k}.cfr", "rb").read(), f".{k}.cfr differs"
    mine, want = parse_1cfr(prefix + ".1.cfr"), parse_1cfr(ref + ".1.cfr")
    assert len(mine) == len(want)
    for (na, va), (nb, vb) in zip(mine, want):
        assert na == nb and va == vb, f"field {na} differs"


@pytest.mark.parametrize("chunk_log2", [None, 10])
@pytest.mark.parametrize("name", NAMES)
def test_command_line_writes_the_reference_builders_files(name, chunk_log2, world, tmp_path):
    prefix = str(tmp_path / name)
    env = dict(os.environ)
    if chunk_log2:
        env.update(CFR_DEBUG_ENV="1", CFR_REFSEQ_CHUNK_LOG2=str(chunk_log2))
    r = subprocess.run([BUILD, "-t", "4"] + bw.runs(world)[name] + bw.common(world, prefix), stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    same_index(prefix, golden_index(name, tmp_path))
    if name == "concat_uncat":
        assert b"taxonomy id doesn't exist for uncategorized_contig" in r.stderr


def test_subset_outside_the_tree_is_refused_in_the_reference_builders_words(world, tmp_path):
    r = subprocess.run([BUILD, "-r", world["ref"], "--conversion-table", world["map"], "--subset-tax", "999999"] + bw.common(world, str(tmp_path / "none")),
                       stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"ERROR: found 0 genomes in the input or after filtering." in r.stderr
    assert not os.path.exists(str(tmp_path / "none.1.cfr"))


def test_list_without_a_second_column_still_needs_a_conversion_table(world, tmp_path):
    one = tmp_path / "one_column.list"
    one.write_text("".join(ln.split("\t")[0] + "\n" for ln in open(world["files"]).read().splitlines()))
    r = subprocess.run([BUILD, "-l", str(one)] + bw.common(world, str(tmp_path / "none")), stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"Should use two-column file" in r.stderr
    # ... and with one it is a plain list of files: the same index as the FASTA of all contigs gives
    a, b = str(tmp_path / "by_list"), str(tmp_path / "by_fasta")
    subprocess.run([BUILD, "-l", str(one), "--conversion-table", world["map"]] + bw.common(world, a), check=True, stderr=subprocess.DEVNULL)
    subprocess.run([BUILD, "-r", world["ref"], "--conversion-table", world["map"]] + bw.common(world, b), check=True, stderr=subprocess.DEVNULL)
    same_index(a, b)


@pytest.mark.parametrize("name", ["concat", "filelist", "filelist_concat"])
def test_classifier_prints_the_reference_tsv_on_the_golden_indexes(name, world, tmp_path):
    out = subprocess.run([CLI, "-x", golden_index(name, tmp_path), "-u", world["reads"], "-t", "2"], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    assert out == open(os.path.join(GOLD, name + ".tsv"), "rb").read()


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
def test_list_subset_and_concat_together_equal_a_live_reference_build(world, tmp_path):
    """A species-level file list with --subset-tax Genus0 and --concat-tax-genome, over files that hold CRLF lines, lower-case and N
    runs, a contig that is too short after filtering (6 kept symbols, --ftabchars 6), a '>' inside a line, and one file of another genus (dropped by the subset)."""
    rng = np.random.default_rng(11)
    rows = [ln.split("\t") for ln in open(world["species"]).read().splitlines()]
    lines = []
    for k, (path, tax) in enumerate(rows):
        data = open(path, "rb").read()
        if k == 0:
            data = data.replace(b"\n", b"\r\n")
        if k == 1:
            data = data[:600] + data[600:900].lower() + b"N" * 5000 + b"\n" + data[900:] + b">tiny\nACGTNNNNNNNNacgt\nA>G\n"
        if k == 2:
            data = data + b">tail of the file without a newline\n" + bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=333)])
        messy = tmp_path / os.path.basename(path)
        messy.write_bytes(data)
        lines.append(f"{messy}\t{tax}\n")
    lst = tmp_path / "messy.list"
    lst.write_text("".join(lines))
    args = ["-l", str(lst), "--subset-tax", str(bw.GENUS0), "--concat-tax-genome"]
    ref, own = str(tmp_path / "ref"), str(tmp_path / "own")
    subprocess.run([os.path.join(REF_DIR, "centrifuger-build"), "-t", "2"] + args + bw.common(world, ref), check=True, stderr=subprocess.DEVNULL)
    env = dict(os.environ, CFR_DEBUG_ENV="1", CFR_REFSEQ_CHUNK_LOG2="9")
    r = subprocess.run([BUILD, "-t", "2"] + args + bw.common(world, own), stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"tiny is filtered due to its short length" in r.stderr
    same_index(own, ref)
