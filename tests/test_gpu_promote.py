"""centrifuger-promote on the device (k_promote_table, k_promote_reads, k_promote_lca) against the host twin (cfr_promote with
device = -1, itself pinned to the Perl script by tests/test_promote_host_cpu.py): cfr_promote_apply on random lists, the offline
command line against the script's output, and promotion inside the classifier - through the C-ABI against classify + host twin,
through bin/centrifuger --promote against the script's output on the reference classifier's TSV.  -m gpu."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ora
import promote_cases as pc
import quant_fixtures as qf
from centrifuger_amd import capi
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")


def _kept_mask(res, size):
    """the slots the reads own after promotion: slots past a read's new n_match are not compared"""
    keep = np.zeros(size, dtype=bool)
    for b, n in zip(res["match_begin"], res["n_match"]):
        keep[int(b):int(b) + max(int(n), 0)] = True
    return keep


def _assert_same(host, dev):
    (hr, hm, hs), (dr, dm, ds) = host, dev
    assert np.array_equal(hr, dr)
    keep = _kept_mask(hr, len(hm))
    assert np.array_equal(hm[keep], dm[keep])
    if hs is not None:
        assert np.array_equal(hs[keep], ds[keep])


@pytest.fixture(scope="module")
def wide():
    tree = pc.Tree("qw")
    t = capi.Taxonomy(qf.WIDE_PREFIX)
    ids = np.array(tree.orig + [88888, 99999] * 45, dtype=np.uint64)       # 811 + 90: a tenth of the draws are in no tree
    return tree, t, ids


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_device_apply_equals_host(n, wide):
    tree, t, ids = wide
    rng = np.random.default_rng(4000 + n)
    reads = [ids[rng.integers(0, len(ids), size=int(rng.integers(0, 7)))].tolist() for _ in range(n)]
    if n > 1:
        reads[n // 2] = ids[rng.integers(0, len(ids), size=40)].tolist()      # one read of 40
    res0, mat0 = pc.make_arrays(tree, reads, int(t.node_cnt), seq_to_tax=t.seq_to_tax, rng=rng, gap=1)
    if n > 1:
        assert set(mat0["kind"].tolist()) == {0, 1, 7} and (mat0["id"][mat0["kind"] == 1] == t.node_cnt).any()
    for level in pc.LEVELS:
        out = []
        for device in (None, 0):
            p = capi.Promote(qf.WIDE_PREFIX, level, device=device)
            res, mat = res0.copy(), mat0.copy()
            src = p.apply(res, mat, want_src=True)
            st = p.stats()
            p.close()
            out.append((res, mat, src))
        _assert_same(out[0], out[1])
        assert st.table_ms >= 0 and st.reads_ms >= 0 and (level != "lca" or st.table_ms == 0)
        if n == 4097:                     # (an event pair around a kernel over one read may resolve to 0.0 ms)
            assert st.reads_ms > 0
        # and both are what the script does (the restatement of tests/promote_cases.py), so the comparison is not of two empty answers
        if n <= 65:
            pc.check_against_script(tree, reads, level, res0, mat0, out[1][0], out[1][1], out[1][2], int(t.node_cnt))
        # slots outside every read's list are as they were
        own = _kept_mask(res0, len(mat0))
        assert np.array_equal(out[1][1][~own], mat0[~own])


def test_no_device_is_an_error_not_a_fallback():
    with pytest.raises(capi.CfrError) as e:
        capi.Promote(qf.PREFIX, "genus", device=capi.device_count() + 7)
    assert e.value.status == capi.CFR_ERR_NO_DEVICE


@pytest.mark.parametrize("key", ["wide", "pe_k5"])
def test_command_line_on_the_device_equals_script(key):
    for name, idx, tsv, level, warnings in pc.outputs(key):
        r = pc.run_promote(["--gpu", "0", pc.PREFIXES[idx], tsv, level])
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == pc.golden(name), name
        assert r.stderr.decode().count("Couldn't find parent of taxID ") == warnings, name


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("promote_reads")
    for f in ("reads_se.fq", "reads_1.fq", "reads_2.fq"):
        (d / f).write_bytes(gzip.open(os.path.join(qf.QDIR, f + ".gz"), "rb").read())
    return d


@pytest.fixture(scope="module")
def pipeline(reads):
    """the q8 index on the device with sub-batches of 64 reads, 200 pairs (four sub-batches), their plain results with -k 5"""
    idx = capi.Index(qf.PREFIX, capi.default_params(max_result=5))
    dev = capi.DeviceIndex(idx, 0, capi.default_device_options(sub_batch=64))
    _, b1, o1 = ora.read_fastx(str(reads / "reads_1.fq"))
    _, b2, o2 = ora.read_fastx(str(reads / "reads_2.fq"))
    n = 200
    o1, o2 = o1[:n + 1].copy(), o2[:n + 1].copy()
    b1, b2 = b1[:int(o1[n])].copy(), b2[:int(o2[n])].copy()
    res, mat = dev.classify(b1, o1, b2, o2)
    res, mat = res.copy(), mat.copy()
    assert (res["n_match"] > 1).sum() >= 5 and (res["n_match"] == 0).sum() >= 5 and len(mat) == 5 * n
    yield dev, (b1, o1, b2, o2), res, mat
    dev.close()
    idx.close()


def _host_promoted(level, res, mat):
    res, mat = res.copy(), mat.copy()
    p = capi.Promote(qf.PREFIX, level, device=None)
    p.apply(res, mat)
    p.close()
    return res, mat, None


@pytest.mark.parametrize("level", ["genus", "species", "lca", "no rank", "bogus"])
def test_promotion_inside_classify_batch(level, pipeline):
    dev, inputs, res0, mat0 = pipeline
    want = _host_promoted(level, res0, mat0)
    dev.set_promote(level)
    try:
        res, mat = dev.classify(*inputs)
        _assert_same(want, (res, mat, None))
        assert dev.last_promote_ms() >= 0
        if level in ("genus", "lca"):
            assert not np.array_equal(res["n_match"], res0["n_match"])          # (something was there to promote)
        # once more through submit / wait
        res2, mat2 = dev.wait(dev.submit(*inputs))
        _assert_same(want, (res2, mat2, None))
    finally:
        dev.set_promote(None)
    res, mat = dev.classify(*inputs)                                            # switched off: the plain results again
    _assert_same((res0, mat0, None), (res, mat, None))
    assert dev.last_promote_ms() == 0


def test_compact_and_expanded_entries_refuse_while_promoting(pipeline):
    import torch
    dev, (b1, o1, _b2, _o2), _res0, _mat0 = pipeline
    tb = torch.from_numpy(b1).cuda()
    to = torch.from_numpy(o1.view(np.int64)).cuda()
    torch.cuda.synchronize()
    n = len(o1) - 1
    dev.set_promote("genus")
    try:
        with pytest.raises(capi.CfrError) as e:
            dev.classify_resident_compact(tb.data_ptr(), to.data_ptr(), n, int(o1[n]))
        assert e.value.status == capi.CFR_ERR_ARG and "promotion" in str(e.value)
    finally:
        dev.set_promote(None)
    cres, cmat = dev.classify_resident_compact(tb.data_ptr(), to.data_ptr(), n, int(o1[n]))      # and works again without
    assert len(cres) == n
    xidx = capi.Index(qf.PREFIX, capi.default_params(max_result=5, output_expanded=1))
    xdev = capi.DeviceIndex(xidx, 0)
    xdev.set_promote("genus")
    with pytest.raises(capi.CfrError) as e:
        xdev.classify_expanded(b1, o1)
    assert e.value.status == capi.CFR_ERR_ARG and "promotion" in str(e.value)
    xdev.set_promote(None)
    assert len(xdev.classify_expanded(b1, o1)[0]) == n
    xdev.close()
    xidx.close()


@pytest.mark.parametrize("key", ["se_k1", "pe_k5"])
def test_classifier_promote_option(key, reads):
    """bin/centrifuger --promote L equals the script's output on the reference classifier's TSV for the same reads"""
    args = ["-u", str(reads / "reads_se.fq"), "-k", "1"] if key == "se_k1" else ["-1", str(reads / "reads_1.fq"), "-2", str(reads / "reads_2.fq"), "-k", "5"]
    for level in ("genus", "species", "lca"):
        r = subprocess.run([CLI, "-x", qf.PREFIX, "-t", "2"] + args + ["--promote", level], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == pc.golden(f"{key}.{level}.tsv.gz"), (key, level)


def test_classifier_promote_is_refused_with_quant_and_expand_taxid(reads, tmp_path):
    base = [CLI, "-x", qf.PREFIX, "-u", str(reads / "reads_se.fq"), "--promote", "genus"]
    for extra, word in ((["--quant", str(tmp_path / "rep.txt")], b"--quant"), (["--expand-taxid"], b"--expand-taxid")):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode != 0 and r.stdout == b""
        assert b"--promote cannot be combined with " + word in r.stderr
    assert not (tmp_path / "rep.txt").exists()
