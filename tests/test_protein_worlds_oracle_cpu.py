"""The four protein worlds of tests/protein_worlds.py on the CPU.  The GPU tests trust the C oracle, which had only been compared with
the reference on the random golden proteome: here each world must provoke what it claims (guards, from the oracle's hit lists alone, at
-k 1 and -k 5), and where the compiled reference is present (oracle/_ref) the oracle's TSV must equal the reference classifier's stdout
on this content - shared and near-equal blocks, repeats, proteins of 3 residues, a tax id outside the tree.  The index is written by the
host half of the native protein writer (tools/dbg/prot_writer_host.cpp, as tests/test_protein_writer_host.py builds it); with the
reference present its files must be those of `centrifuger-build --protein`.  CPU only."""
import os
import subprocess

import pytest

import oracle_lib as ora
import protein_worlds as pw
from centrifuger_amd import synth
from cfr_fields import parse_1cfr
from conftest import REF_DIR, ROOT, have_ref


@pytest.fixture(scope="module")
def writer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("protw") / "prot_writer_host")
    csrc = os.path.join(ROOT, "centrifuger_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", csrc, "-o", exe, os.path.join(ROOT, "tools", "dbg", "prot_writer_host.cpp"),
                    os.path.join(csrc, "cfr_build.cpp"), "-lpthread"], check=True)
    return exe


@pytest.fixture(scope="module", params=pw.NAMES)
def built(request, writer, tmp_path_factory):
    d = str(tmp_path_factory.mktemp(request.param))
    w = pw.make(request.param)
    synth.write_reference_inputs(w.genomes, d, line_width=60)
    prefix = os.path.join(d, "own")
    kw = pw.build_kwargs(w)
    subprocess.run([writer, os.path.join(d, "ref.fa"), os.path.join(d, "nodes.dmp"), os.path.join(d, "names.dmp"), os.path.join(d, "seqid.map"),
                    prefix, str(kw["ftab_chars"]), str(kw["offrate"]), str(kw["rbbwt_b"]), "4"], check=True, stderr=subprocess.DEVNULL)
    pw.write_reads(w, d)
    return w, d, prefix


@pytest.fixture(scope="module")
def lists(built):
    """the oracle's hit lists at -k 1 and -k 5, computed once and left unchanged"""
    w, _, prefix = built
    out = {}
    for k in (1, 5):
        o = ora.OracleIndex(prefix, max_result=k)
        out[k] = pw.hit_lists(w, o)
        o.close()
    return out


@pytest.fixture(scope="module")
def ref_built(built):
    w, d, _ = built
    prefix = os.path.join(d, "ref")
    kw = pw.build_kwargs(w)
    subprocess.run([os.path.join(REF_DIR, "centrifuger-build"), "--protein", "-t", "2", "-r", os.path.join(d, "ref.fa"), "--taxonomy-tree", os.path.join(d, "nodes.dmp"),
                    "--name-table", os.path.join(d, "names.dmp"), "--conversion-table", os.path.join(d, "seqid.map"), "-o", prefix,
                    "--ftabchars", str(kw["ftab_chars"]), "--offrate", str(kw["offrate"])] + (["--rbbwt-b", str(kw["rbbwt_b"])] if kw["rbbwt_b"] else []),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return w, d, prefix


@pytest.mark.parametrize("k", [1, 5])
def test_world_provokes_what_it_claims(built, lists, k):
    w, _, prefix = built
    o = ora.OracleIndex(prefix, max_result=k)
    print(w.info["name"], "k", k, pw.guards(w, o, k, hits=lists[k]))
    o.close()


def test_oracle_hit_lists_do_not_depend_on_k(built, lists):
    """tests/test_gpu_protein_worlds.py compares the device's lists at -k 1 and -k 5 with one set of oracle lists"""
    for ends in ("se", "pe"):
        assert len(lists[1][ends]) == len(lists[5][ends])
        for x, y in zip(lists[1][ends], lists[5][ends]):
            assert len(x) == len(y) and all((x[f] == y[f]).all() for f in ("sp", "ep", "l", "strand", "offset"))


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
def test_host_writer_equals_reference_builder(built, ref_built):
    _, _, own = built
    _, _, ref = ref_built
    mine, want = parse_1cfr(own + ".1.cfr", protein=True), parse_1cfr(ref + ".1.cfr", protein=True)
    assert len(mine) == len(want)
    for (na, va), (nb, vb) in zip(mine, want):
        assert na == nb and va == vb, f"field {na} differs"
    assert open(own + ".2.cfr", "rb").read() == open(ref + ".2.cfr", "rb").read()
    assert open(own + ".4.cfr").read().split("\n")[:3] == open(ref + ".4.cfr").read().split("\n")[:3]


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
@pytest.mark.parametrize("paired", ["se", "pe"])
@pytest.mark.parametrize("k", [1, 5])
def test_oracle_tsv_equals_reference_binary(ref_built, k, paired):
    w, d, prefix = ref_built
    files = ["-u", os.path.join(d, "se.fq")] if paired == "se" else ["-1", os.path.join(d, "p_1.fq"), "-2", os.path.join(d, "p_2.fq")]
    ref = subprocess.run([os.path.join(REF_DIR, "centrifuger"), "-x", prefix, "-t", "2", "-k", str(k)] + files,
                         check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    o = ora.OracleIndex(prefix, max_result=k)
    if paired == "se":
        n, res = w.reads.n, o.classify(w.reads.bases, w.reads.offsets, threads=8)
    else:
        r1, r2 = w.pairs
        n, res = r1.n, o.classify(r1.bases, r1.offsets, r2.bases, r2.offsets, threads=8)
    own = o.tsv([f"r{i}" for i in range(n)], res)
    o.close()
    assert ref.count(b"\n") > n
    if own != ref:
        a, b = own.split(b"\n"), ref.split(b"\n")
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        assert False, f"{len(a)} / {len(b)} lines, {len(diff)} rows differ (oracle, reference), first: {diff[:3]}"
