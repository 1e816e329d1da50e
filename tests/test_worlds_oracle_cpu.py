"""The four index worlds of tests/index_worlds.py on the CPU: each must provoke what it claims (guards, from the C oracle alone), and
where the compiled reference is present (oracle/_ref) the oracle's TSV must equal the reference classifier's stdout on this content
too - text that is not random DNA, sequences of 7 bases, an irregular taxonomy - on which the oracle had never been compared.  The
index writers are compared on the way: the Python writer's files must be the reference builder's.  CPU only."""
import os
import subprocess

import pytest
import torch

import index_worlds as iw
import oracle_lib as ora
from centrifuger_amd import indexbuild, synth
from cfr_fields import parse_1cfr
from conftest import REF_DIR, have_ref


@pytest.fixture(scope="module", params=iw.NAMES)
def built(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp(request.param))
    w = iw.make(request.param)
    g = w.genomes
    prefix = os.path.join(d, "own")
    indexbuild.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, prefix, device=torch.device("cpu"), **iw.build_kwargs(w))
    return w, d, prefix


@pytest.fixture(scope="module")
def ref_built(built):
    """the same world written by the reference's centrifuger-build, and the reads as FASTQ files"""
    w, d, _ = built
    synth.write_reference_inputs(w.genomes, d)
    prefix = os.path.join(d, "ref")
    subprocess.run([os.path.join(REF_DIR, "centrifuger-build"), "-t", "2", "-r", os.path.join(d, "ref.fa"), "--taxonomy-tree", os.path.join(d, "nodes.dmp"),
                    "--name-table", os.path.join(d, "names.dmp"), "--conversion-table", os.path.join(d, "seqid.map"), "-o", prefix,
                    "--ftabchars", str(w.info["ftab_chars"])], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    iw.write_reads(w, d)
    return w, d, prefix


@pytest.mark.parametrize("k", [1, 5])
def test_world_provokes_what_it_claims(built, k):
    w, _, prefix = built
    o = ora.OracleIndex(prefix, max_result=k)
    reached = iw.guards(w, o, k)
    print(w.info["name"], "k", k, reached)
    o.close()


def test_oracle_hit_lists_do_not_depend_on_k(built):
    """tests/test_gpu_worlds.py compares the device's lists at -k 1 and -k 5 with one set of oracle lists"""
    w, _, prefix = built
    a, b = (iw.hit_lists(w, ora.OracleIndex(prefix, max_result=k)) for k in (1, 5))
    for ends in ("se", "pe"):
        for x, y in zip(a[ends], b[ends]):
            assert len(x) == len(y) and all((x[f] == y[f]).all() for f in ("sp", "ep", "l", "strand", "offset"))


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
def test_python_writer_equals_reference_builder(built, ref_built):
    _, _, own = built
    _, _, ref = ref_built
    mine, want = parse_1cfr(own + ".1.cfr"), parse_1cfr(ref + ".1.cfr")
    assert len(mine) == len(want)
    for (na, va), (nb, vb) in zip(mine, want):
        assert na == nb and va == vb, f"field {na} differs"
    for ext in (".2.cfr", ".3.cfr"):
        assert open(own + ext, "rb").read() == open(ref + ext, "rb").read(), ext


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
@pytest.mark.parametrize("dust", ["dust", "no_dust"])
@pytest.mark.parametrize("paired", ["se", "pe"])
@pytest.mark.parametrize("k", [1, 5])
def test_oracle_tsv_equals_reference_binary(ref_built, oracle_bin, k, paired, dust):
    w, d, prefix = ref_built
    files = ["-u", os.path.join(d, "se.fq")] if paired == "se" else ["-1", os.path.join(d, "p_1.fq"), "-2", os.path.join(d, "p_2.fq")]
    args = ["-x", prefix, "-t", "2", "-k", str(k)] + files + (["--no-dust"] if dust == "no_dust" else [])
    ref = subprocess.run([os.path.join(REF_DIR, "centrifuger")] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    own = subprocess.run([oracle_bin, "classify"] + args, check=True, stdout=subprocess.PIPE).stdout
    assert ref.count(b"\n") > (w.reads.n if paired == "se" else w.pairs[0].n)
    if own != ref:
        a, b = own.split(b"\n"), ref.split(b"\n")
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        assert False, f"{len(diff)} rows differ (oracle, reference), first: {diff[:3]}"
