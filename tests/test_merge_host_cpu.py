"""--merge-readpair on the host: cfr_merge_pairs (the literal restatement of ReadPairMerger::Merge, csrc/cfr_merge.cpp) against what
the reference itself did with the pairs of tests/golden/merge and tests/golden/merge_long (mates of up to 1100 bases, pairs on the
similarity threshold, offsets and overlaps at multiples of 64)."""
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


@pytest.mark.parametrize("fmt", ["fq", "fa"])
@pytest.mark.parametrize("threads", [1, 5])
def test_host_merge_equals_reference_dump_long(fmt, threads):
    p = mf.pairs(fmt, "merge_long")
    got = capi.merge_pairs(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], p["q2"], threads=threads)
    mf.check_against_dump(fmt, got, "merge_long")


def test_long_fixture_holds_its_classes():
    """what make_golden_merge.py asserted when it wrote the set, from the committed files: every kind in the three length classes,
    each threshold pair merging with overlapSize = L at exactly L - T(L) substitutions and not at one more (T from Python floats),
    and the pairs with two passing offsets at least 64 apart (kind 0, `offset` the larger, why 'M' when the plain pass saw both)"""
    m = mf.manifest("merge_long")
    p = mf.pairs("fq", "merge_long")
    len1, len2 = np.diff(p["o1"].astype(np.int64)), np.diff(p["o2"].astype(np.int64))
    cls = m["classes"]
    assert sorted(i for c in cls.values() for i in c) == list(range(m["n_fq"])) and m["n_fa"] == m["n_fq"]
    assert all(151 <= len1[i] <= 512 and 151 <= len2[i] <= 512 for i in cls["L1"])
    assert sum(1 for i in cls["L1"] if max(len1[i], len2[i]) >= 449) >= 20
    edges = [63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 447, 448, 449, 511, 512, 513, 514]
    for a in edges:
        assert len({int(len2[i]) for i in cls["L2"] if len1[i] == a}) >= 3, a
    assert all(len1[i] in edges and len2[i] in edges for i in cls["L2"])
    assert all(max(len1[i], len2[i]) > 512 for i in cls["L3"])
    shape = [(len1[i] > 512, len2[i] > 512) for i in cls["L3"]]
    assert min(shape.count(s) for s in ((False, True), (True, False), (True, True))) >= 10
    assert max(len1.max(), len2.max()) <= 1100 and max(len1[i] for i in cls["L3"]) > 1000
    for fmt in ("fq", "fa"):
        d = mf.dump(fmt, "merge_long")
        for c in ("L1", "L2", "L3"):
            kinds = [d[i][0] for i in cls[c]]
            assert all(kinds.count(k) >= 10 for k in (0, 1, 2)), (c, kinds)
        seen = set()
        for t in m["l4"]:
            L, on = t["L"], t["substitutions"] == t["L"] - mf.threshold(t["L"])
            assert on or t["substitutions"] == L - mf.threshold(L) + 1
            want = ((2 if t["pass"] == "through" else 1), L, t["offset"], b"-") if on else (0, -1, -1, b"-")
            assert d[t["pair"]][:4] == want and t["kind"] == want[0], t
            seen.add((L, t["pass"], t["packed"], on))
        assert seen == {(L, ps, pk, on) for L in (32, 49, 50, 51, 64, 99, 100, 101, 127, 128, 129, 192, 256, 320, 384, 448, 511, 512)
                        for ps in ("plain", "through") for pk in (False, True) for on in (False, True)}
        assert sorted(t["pair"] for t in m["l4"]) == cls["L4"]
        for t in m["l5_two_offsets"]:
            assert d[t["pair"]][:4] == (0, -1, t["offset"], t["why"].encode()), t
        assert sum(1 for i in cls["L5"] if d[i][3] == b"M") >= 5
        # true offsets at the word edges, overlaps at multiples of 64 and next to them, both passes, among the merged pairs of L5
        for kind in (1, 2):
            offs = {d[i][2] for i in cls["L5"] if d[i][0] == kind}
            assert offs >= {1, 63, 64, 65, 128, 191, 192, 448} | ({0} if kind == 2 else set()), (kind, sorted(offs))
            ovs = {d[i][1] for i in cls["L5"] if d[i][0] == kind}
            assert ovs >= {k + e for k in (64, 128, 192, 256, 320, 384, 448) for e in (-1, 0, 1)} | {511}, (kind, sorted(ovs))
        assert {512, 513} <= {d[i][1] for i in cls["L5"] if d[i][0]}
        assert all(d[i][0] for i in cls["L6"])
    raw = b"".join(bytes(p["b1"][int(p["o1"][i]):int(p["o1"][i + 1])]) + bytes(p["b2"][int(p["o2"][i]):int(p["o2"][i + 1])]) for i in cls["L6"])
    assert b"NNN" in raw and any(c in raw for c in b"acgt")


@pytest.mark.parametrize("case", ["fq_k1", "fq_nodust", "fa_k1"])
def test_host_merge_then_dust_then_oracle_equals_reference_tsv_long(case, golden_dir):
    args = mf.manifest("merge_long")["cases"][case]["args"]
    fmt = "fq" if case.startswith("fq") else "fa"
    p = mf.pairs(fmt, "merge_long")
    m = capi.merge_pairs(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], p["q2"], threads=2)
    b1, b2 = m["bases1"].copy(), m["bases2"].copy()
    if "--no-dust" not in args:
        capi.dust_mask(b1, m["offsets1"])
        capi.dust_mask(b2, m["offsets2"])
    o = ora.OracleIndex(golden_dir + "/f6", max_result=1)
    res = o.classify(b1, m["offsets1"], b2, m["offsets2"])
    assert o.tsv([i.decode() for i in p["ids"]], res) == mf.tsv(case, "merge_long")


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
