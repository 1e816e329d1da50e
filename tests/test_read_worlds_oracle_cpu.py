"""The read world of tests/read_worlds.py on the CPU: every family must provoke what it claims (guards, from the C oracle alone), the
oracle's hit lists must not depend on -k, and where the compiled reference is present (oracle/_ref) the oracle's TSV must equal the
reference classifier's stdout on these reads too - reads of 0 .. 1 048 576 bases, up to 70 000 hits, empty mates - on which the oracle
had never been compared.  CPU only."""
import os
import subprocess

import pytest
import torch

import oracle_lib as ora
import read_worlds as rw
from centrifuger_amd import capi, indexbuild
from conftest import REF_DIR, have_ref


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("read_world"))
    g = rw.genomes()
    prefix = os.path.join(d, "own")
    indexbuild.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, prefix, device=torch.device("cpu"), **rw.build_kwargs())
    info = capi.Index(prefix).info()
    w = rw.make(g, info.min_hit_len, info.precompute_width)
    files = {name: rw.write_fasta(w.batches[name], d, name) for name in rw.BATCHES}
    return w, prefix, files


@pytest.fixture(scope="module")
def lists(built):
    w, prefix, _ = built
    out = {}
    for k in (1, 5):
        o = ora.OracleIndex(prefix, max_result=k)
        out[k] = rw.hit_lists(w, o)
        o.close()
    return out


@pytest.mark.parametrize("k", [1, 5])
def test_read_world_provokes_what_it_claims(built, lists, k):
    w, prefix, _ = built
    o = ora.OracleIndex(prefix, max_result=k)
    reached = rw.guards(w, o, k, hits=lists[k])
    print("read world k", k, reached)
    o.close()


def test_oracle_hit_lists_do_not_depend_on_k(lists):
    """tests/test_gpu_read_worlds.py compares the device's lists at -k 1 and -k 5 with one set of oracle lists"""
    for name in rw.BATCHES:
        for x, y in zip(lists[1][name], lists[5][name]):
            assert len(x) == len(y) and all((x[f] == y[f]).all() for f in ("sp", "ep", "l", "strand", "offset"))


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
@pytest.mark.parametrize("name,dust", [("small_se", True), ("small_se", False), ("small_pe", True), ("small_pe", False), ("giant_se", False), ("giant_pe", False)])
@pytest.mark.parametrize("k", [1, 5])
def test_oracle_tsv_equals_reference_binary(built, oracle_bin, k, name, dust):
    w, prefix, files = built
    args = ["-x", prefix, "-t", "4", "-k", str(k)] + files[name] + ([] if dust else ["--no-dust"])
    ref = subprocess.run([os.path.join(REF_DIR, "centrifuger")] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    own = subprocess.run([oracle_bin, "classify"] + args, check=True, stdout=subprocess.PIPE).stdout
    assert ref.count(b"\n") > w.batches[name].n
    if own != ref:
        a, b = own.split(b"\n"), ref.split(b"\n")
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        assert False, f"{len(diff)} rows differ (oracle, reference), first: {diff[:3]}"
