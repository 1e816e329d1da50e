"""--merge-readpair on the host: cfr_merge_pairs (the literal restatement of ReadPairMerger::Merge, csrc/cfr_merge.cpp) against what
the reference itself did with the pairs of tests/golden/merge."""
import os
import subprocess

import numpy as np
import pytest

import merge_fixtures as mf
import oracle_lib as ora
from centrifuger_amd import capi
from conftest import GOLDEN, ROOT


@pytest.mark.parametrize("fmt", ["fq", "fa"])
@pytest.mark.parametrize("threads", [1, 5])
def test_host_merge_equals_reference_dump(fmt, threads):
    p = mf.pairs(fmt)
    got = capi.merge_pairs(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], p["q2"], threads=threads)
    mf.check_against_dump(fmt, got)


def test_fixture_holds_every_kind_and_the_ambiguous_overlaps():
    for fmt, need in (("fq", 100), ("fa", 30)):
        kinds = [r[0] for r in mf.dump(fmt)]
        assert all(kinds.count(k) >= need for k in (0, 1, 2))
    assert sum(1 for r in mf.dump("fq") if r[3] in (b"T", b"M")) >= 20
    assert mf.dump("fq")[26][:3] == (2, 0, 0)            # r1 = "", len2 = 1: merges to the empty read


@pytest.mark.parametrize("case", ["fq_k1", "fq_k5", "fq_nodust", "fa_k1"])
def test_host_merge_then_dust_then_oracle_equals_reference_tsv(case, golden_dir):
    args = mf.manifest()["cases"][case]["args"]
    fmt = "fq" if case.startswith("fq") else "fa"
    p = mf.pairs(fmt)
    m = capi.merge_pairs(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], p["q2"], threads=2)
    b1, b2 = m["bases1"].copy(), m["bases2"].copy()
    if "--no-dust" not in args:
        capi.dust_mask(b1, m["offsets1"])
        capi.dust_mask(b2, m["offsets2"])
    k = int(args[args.index("-k") + 1]) if "-k" in args else 1
    o = ora.OracleIndex(golden_dir + "/f6", max_result=k)
    res = o.classify(b1, m["offsets1"], b2, m["offsets2"])
    assert o.tsv([i.decode() for i in p["ids"]], res) == mf.tsv(case)


def test_mixed_qualities_are_an_argument_error():
    p = mf.pairs("fq")
    with pytest.raises(capi.CfrError) as e:
        capi.merge_pairs(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], None)
    assert e.value.status == capi.CFR_ERR_ARG
    with pytest.raises(capi.CfrError) as e:
        capi.merge_pairs(p["b1"], p["o1"], p["b2"], p["o2"], None, p["q2"])
    assert e.value.status == capi.CFR_ERR_ARG


def test_homopolymer_pair_is_ambiguous():
    """40 + 40 bases: minOverlap 8; every one of the 32 offsets of a homopolymer passes both tests, so nothing is merged and
    `offset` is left at the last one (ReadPairMerger.hpp:43-53)"""
    a = np.frombuffer(b"A" * 40, dtype=np.uint8)
    o = np.array([0, 40], dtype=np.uint64)
    got = capi.merge_pairs(a, o, np.frombuffer(b"T" * 40, dtype=np.uint8), o)
    assert got["kind"].tolist() == [0] and got["overlap"].tolist() == [-1] and got["offset"].tolist() == [31]


def test_cli_refuses_merge_readpair_where_it_cannot_merge(golden_dir):
    """before any device work: a protein index (the translated search of a merged pair's empty mate is not covered) and single-end input"""
    cli = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
    prot = os.path.join(GOLDEN, "prot")
    r = subprocess.run([cli, "-x", os.path.join(prot, "p2"), "-1", os.path.join(prot, "pe_1.fa"), "-2", os.path.join(prot, "pe_2.fa"), "--merge-readpair"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"--merge-readpair is not available with a protein index" in r.stderr and r.stdout == b""
    r = subprocess.run([cli, "-x", os.path.join(golden_dir, "f6"), "-u", os.path.join(golden_dir, "se.fq"), "--merge-readpair"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"--merge-readpair needs paired-end reads" in r.stderr
    r = subprocess.run([cli], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"--merge-readpair: merge overlapped paired-end reads" in r.stderr
