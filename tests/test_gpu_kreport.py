"""centrifuger-kreport on the device (k_kreport_fold, k_kreport_accumulate) against the host twin (cfr_kreport with device = -1, itself
pinned to the Perl script by tests/test_kreport_host_cpu.py): the bins, the maxima and seq_count must be equal exactly - everything is
an integer and every order of the atomics gives the same sums - at the smallest shapes at which the kernels take another path; then
the offline command line on the device against the script's output, and the report inside the classifier: the image's bins through
the C-ABI against the host twin, bin/centrifuger --kreport against the script's output on the reference classifier's TSV.  -m gpu."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import kreport_cases as kc
import oracle_lib as ora
import promote_cases as pc
import quant_fixtures as qf
from centrifuger_amd import capi
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wide():
    tree = pc.Tree("qw")
    t = capi.Taxonomy(qf.WIDE_PREFIX)
    assert int(t.node_cnt) == 811
    return tree, t


def _both(prefix, res, mat, calls=None, dev_options=None, **options):
    """(own, own_score, seq_count, warnings) of the host twin and of the device; calls: the slices of `res` given to add_results one by one"""
    out = []
    for device, extra in ((None, {}), (0, dev_options or {})):
        k = capi.Kreport(prefix, device=device, **options, **extra)
        for a, b in (calls or [(0, len(res))]):
            k.add_results(res[a:b].copy(), mat)
        own, clade, sc, csc, seq = k.counts()
        out.append((own, clade, sc, csc, seq, k.warnings().tolist()))
        st = k.stats()
        k.close()
    for h, d in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(h, d)
    assert out[0][4] == out[1][4] and out[0][5] == out[1][5]
    return out[1], st


@pytest.mark.parametrize("n,dev_options", [(0, {}), (1, {}), (63, {}), (64, {}), (65, {}), (3000, {"max_blocks": 2})])
def test_device_equals_host(n, dev_options, wide):
    """n around the wave; 3000 reads on two blocks of 256 lanes: the stride loops of both kernels run six times"""
    tree, t = wide
    nc = int(t.node_cnt)
    rng = np.random.default_rng(7000 + n)
    reads = kc.random_reads(tree, rng, n, scores=(0, 1 << 40))
    if n > 1:
        reads[n // 2] = (tree.orig[:64], (1 << 40) + 5, 150)              # a list of 64
        reads[0] = ([], 0, 0)
    res, mat = kc.arrays(tree, reads, nc, seq_to_tax=t.seq_to_tax, rng=rng, gap=1)
    if n > 64:
        assert set(mat["kind"].tolist()) == {0, 1, 7} and {0, 1, 5} <= set(res["n_match"].tolist()) and int(res["score"].max()) > 1 << 32
    (own, clade, sc, csc, seq, warn), _st = _both(qf.WIDE_PREFIX, res, mat, dev_options=dev_options, score_data=True)
    assert seq == n and int(own.sum()) == n
    # ... and both are what the script does, so the comparison is not of two empty answers
    s = kc.Script("qw")
    counts, scores, want_seq, want_warn = s.count_reads(reads)
    assert np.array_equal(own, s.bins(counts, nc)) and np.array_equal(sc, s.bins(scores, nc)) and seq == want_seq and warn == want_warn


def test_one_taxon_and_all_unclassified(wide):
    """100 000 reads in one bin: the wave's leaders take 64 reads each, the block's table one slot, HBM one atomic per block"""
    tree, t = wide
    nc, n = int(t.node_cnt), 100_000
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    res["n_match"], res["match_begin"], res["hit_length"] = 1, 0, 150          # every read points at the same slot
    res["score"] = np.arange(n, dtype=np.uint64) * np.uint64(1 << 20)
    mat = np.zeros(1, dtype=capi.MATCH_DTYPE)
    node = tree.compact[tree.orig[400]]
    mat[0] = (node, tree.orig[400], 1, 0)
    (own, _cl, sc, _cs, seq, _w), st = _both(qf.WIDE_PREFIX, res, mat)
    assert seq == n and int(own[node]) == n and int(sc[node]) == (n - 1) << 20 and np.count_nonzero(own) == 1
    assert st.fold_ms > 0 and st.accumulate_ms > 0
    res["n_match"] = 0
    (own, _cl, sc, _cs, seq, _w), _st = _both(qf.WIDE_PREFIX, res, mat)
    assert seq == n and int(own[nc]) == n and np.count_nonzero(own) == 1


def test_every_read_in_another_node_and_the_overflow_path(wide):
    """811 bins in one block: with 64 slots (8 tries each) most pairs go straight to HBM; with the default 1024 all but a few fit"""
    tree, t = wide
    nc = int(t.node_cnt)
    reads = [([tid], 1000 + k, 150) for k, tid in enumerate(tree.orig)] * 3
    res, mat = kc.arrays(tree, reads, nc)
    for dev_options in ({"max_blocks": 1, "lds_slots": 64}, {"max_blocks": 1}, {}):
        (own, _cl, sc, _cs, seq, _w), _st = _both(qf.WIDE_PREFIX, res, mat, dev_options=dev_options)
        assert seq == 3 * nc and int(own[nc]) == 0 and (own[:nc] == 3).all() and (sc[:nc] == 1000 + np.arange(nc, dtype=np.uint64)).all()


def test_unknown_ids_thresholds_and_uneven_calls(wide):
    tree, t = wide
    nc = int(t.node_cnt)
    a, b, c = tree.orig[100], tree.orig[500], tree.orig[700]
    reads = [([88888, a], 10, 100), ([a, 88888, b], 10, 100), ([88888], 10, 100), ([88888, 88888], 10, 100), ([88888, 99999, c], 10, 100),
             ([a], 10, 100), ([a], 9, 100), ([a], 10, 99), ([b], 1 << 33, 100), ([], 10, 100), ([], 0, 0)]
    rng = np.random.default_rng(99)
    reads = reads + kc.random_reads(tree, rng, 989, scores=(0, 20), lengths=(90, 110))
    res, mat = kc.arrays(tree, reads, nc, gap=3)
    one, _st = _both(qf.WIDE_PREFIX, res, mat, min_score=10, min_length=100, score_data=True)
    three, _st = _both(qf.WIDE_PREFIX, res, mat, calls=[(0, 7), (7, 600), (600, 1000)], min_score=10, min_length=100, score_data=True)
    for x, y in zip(one[:4], three[:4]):
        assert np.array_equal(x, y)
    assert one[4] == three[4] and one[5] == three[5] and 0 < one[4] < 1000
    s = kc.Script("qw")
    counts, scores, seq, warn = s.count_reads(reads, min_score=10, min_length=100)
    assert np.array_equal(one[0], s.bins(counts, nc)) and np.array_equal(one[2], s.bins(scores, nc)) and one[4] == seq and one[5] == warn
    assert int(one[0][tree.compact[a]]) >= 1 and int(one[2][tree.compact[b]]) == 1 << 33 and warn[:4] == [88888] * 4


def test_no_device_is_an_error_not_a_fallback():
    with pytest.raises(capi.CfrError) as e:
        capi.Kreport(qf.PREFIX, device=capi.device_count() + 7)
    assert e.value.status == capi.CFR_ERR_NO_DEVICE


@pytest.mark.parametrize("key", ["se_k1", "pe_k5", "edge", "wide"])
def test_command_line_on_the_device_equals_script(key):
    for name, o in kc.outputs(key):
        if name.split(".")[1] not in ("default", "filter_score_zeros", "drop_all"):      # (every set runs on the host in test_kreport_host_cpu.py)
            continue
        r = kc.run_kreport(["--gpu", "0", "-x", kc.PREFIXES[o["index"]]] + o["args"] + [os.path.join(GOLDEN, o["input"])])
        assert r.stdout == kc.golden(name), name
        assert kc.warning_ids(r.stderr) == o["warnings"], name
        assert (r.returncode != 0) == (o["status"] != 0), (name, r.stderr.decode())


# ---- the report inside the classifier: cfr_device_index_set_kreport and bin/centrifuger --kreport ----
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
RERUN = {"CFR_DEBUG_ENV": "1", "CFR_POOL_INIT": "3", "CFR_SUBBATCH": "50", "CFR_TAPER_FLOOR": "0"}      # tests/test_gpu_variants.py "post_pool_growth": sub-batches computed again


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("kreport_reads")
    for f in ("reads_se.fq", "reads_1.fq", "reads_2.fq"):
        (d / f).write_bytes(gzip.open(os.path.join(qf.QDIR, f + ".gz"), "rb").read())
    return d


def _host_bins(res, mat, **options):
    k = capi.Kreport(qf.PREFIX, device=None, **options)
    k.add_results(res, mat)
    own, _cl, sc, _cs, seq = k.counts()
    k.close()
    return own, sc, seq


def test_report_inside_classify_batch(reads):
    """q8 on the device with sub-batches of 64 reads, 200 pairs (four sub-batches), -k 5: the image's bins against the host twin on the
    call's own results; a second call adds, switching on again zeroes, promotion beside it changes nothing, off launches nothing"""
    idx = capi.Index(qf.PREFIX, capi.default_params(max_result=5))
    dev = capi.DeviceIndex(idx, 0, capi.default_device_options(sub_batch=64))
    _, b1, o1 = ora.read_fastx(str(reads / "reads_1.fq"))
    _, b2, o2 = ora.read_fastx(str(reads / "reads_2.fq"))
    n = 200
    o1, o2 = o1[:n + 1].copy(), o2[:n + 1].copy()
    inputs = (b1[:int(o1[n])].copy(), o1, b2[:int(o2[n])].copy(), o2)
    res0, mat0 = dev.classify(*inputs)
    res0, mat0 = res0.copy(), mat0.copy()
    assert dev.last_kreport_ms() == 0
    bins = 15
    for options in ({}, {"min_score": 10000, "min_length": 100}):
        want_own, want_sc, want_seq = _host_bins(res0, mat0, **options)
        assert 0 < want_seq <= n and (not options or want_seq < n)
        dev.set_kreport(**options)
        res, mat = dev.classify(*inputs)
        keep = np.zeros(len(mat0), dtype=bool)                                       # (slots past a read's n_match are nobody's: not compared)
        for b, k in zip(res0["match_begin"], res0["n_match"]):
            keep[int(b):int(b) + max(int(k), 0)] = True
        assert np.array_equal(res, res0) and np.array_equal(mat[keep], mat0[keep])   # the results are untouched
        own, sc, seq = dev.kreport_counts(bins)
        assert np.array_equal(own, want_own) and np.array_equal(sc, want_sc) and seq == want_seq
        assert dev.last_kreport_ms() > 0
        dev.set_promote("genus")                                                     # the fold runs in front of the promotion
        res, mat = dev.wait(dev.submit(*inputs))
        dev.set_promote(None)
        assert not np.array_equal(res["n_match"], res0["n_match"])
        own, sc, seq = dev.kreport_counts(bins)
        assert np.array_equal(own, 2 * want_own) and np.array_equal(sc, want_sc) and seq == 2 * want_seq
        dev.set_kreport(**options)                                                   # on again: zeroed
        assert dev.kreport_counts(bins)[2] == 0
    dev.set_kreport(False)
    dev.classify(*inputs)
    assert dev.last_kreport_ms() == 0 and dev.kreport_counts(bins)[2] == 0
    with pytest.raises(capi.CfrError) as e:
        dev.set_kreport(no_lca=True)
    assert e.value.status == capi.CFR_ERR_ARG
    with pytest.raises(capi.CfrError) as e:
        dev.kreport_counts(bins - 1)
    assert e.value.status == capi.CFR_ERR_CAPACITY
    # the compact entry refuses while the report is on
    import torch
    tb = torch.from_numpy(inputs[0]).cuda()
    to = torch.from_numpy(o1.view(np.int64)).cuda()
    torch.cuda.synchronize()
    dev.set_kreport()
    with pytest.raises(capi.CfrError) as e:
        dev.classify_resident_compact(tb.data_ptr(), to.data_ptr(), n, int(o1[n]))
    assert e.value.status == capi.CFR_ERR_ARG and "report" in str(e.value)
    dev.set_kreport(False)
    assert len(dev.classify_resident_compact(tb.data_ptr(), to.data_ptr(), n, int(o1[n]))[0]) == n
    dev.close()
    idx.close()
    assert capi.lib().cfr_device_index_set_kreport(None, None) == capi.CFR_ERR_ARG
    assert capi.lib().cfr_last_kreport_ms(None, None) == capi.CFR_ERR_ARG


def _classifier(key, reads, report, extra=(), env=None):
    args = ["-u", str(reads / "reads_se.fq"), "-k", "1"] if key == "se_k1" else ["-1", str(reads / "reads_1.fq"), "-2", str(reads / "reads_2.fq"), "-k", "5"]
    r = subprocess.run([CLI, "-x", qf.PREFIX, "-t", "2"] + args + (["--kreport", str(report)] if report else []) + list(extra), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()
    return r


def _tsv(key):
    return gzip.open(qf.tsv_path(key), "rb").read()


@pytest.mark.parametrize("key", ["se_k1", "pe_k5"])
def test_classifier_kreport_option(key, reads, tmp_path):
    """bin/centrifuger --kreport FILE equals the script's default report on the reference classifier's TSV for the same reads; the TSV
    is the golden one with the switch and without it"""
    want = kc.golden(f"{key}.default.txt.gz")
    r = _classifier(key, reads, tmp_path / "a.txt")
    assert (tmp_path / "a.txt").read_bytes() == want and r.stdout == _tsv(key)
    assert _classifier(key, reads, None).stdout == _tsv(key)                          # never set: the parent's behaviour
    r = _classifier(key, reads, tmp_path / "b.txt", ["--gpu-batch", "300"])           # several batches: the bins persist between calls
    assert (tmp_path / "b.txt").read_bytes() == want and r.stdout == _tsv(key)
    r = _classifier(key, reads, tmp_path / "c.txt", ["--promote", "genus"])           # the report is unchanged, the TSV is the promoted one
    assert (tmp_path / "c.txt").read_bytes() == want and r.stdout == pc.golden(f"{key}.genus.tsv.gz")


@pytest.mark.parametrize("key", ["se_k1", "pe_k5"])
def test_classifier_kreport_counts_recomputed_sub_batches_once(key, reads, tmp_path):
    """a fresh child under the re-run recipe: sub-batches whose scratch pool ran dry are computed again after copy_out has run for them"""
    r = _classifier(key, reads, tmp_path / "r.txt", env=RERUN)
    assert (tmp_path / "r.txt").read_bytes() == kc.golden(f"{key}.default.txt.gz") and r.stdout == _tsv(key)


def test_classifier_kreport_refusals_and_help(reads, tmp_path):
    r = subprocess.run([CLI, "-x", qf.PREFIX, "-u", str(reads / "reads_se.fq"), "--kreport", str(tmp_path / "x.txt"), "--expand-taxid"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and r.stdout == b"" and b"--kreport cannot be combined with --expand-taxid" in r.stderr and not (tmp_path / "x.txt").exists()
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--kreport FILE" in r.stdout + r.stderr
    # the count of the script's warning lines is logged once: the edge fixture's reads are not at hand, so the line is checked on a run without any
    r = _classifier("se_k1", reads, tmp_path / "y.txt")
    assert r.stderr.count(b"--kreport:") == 0


def test_classifier_kreport_on_two_gpus(reads, tmp_path):
    if capi.device_count() < 2:
        pytest.skip("needs two devices")
    r = _classifier("pe_k5", reads, tmp_path / "two.txt", ["--gpu", "0,1", "--gpu-batch", "300"])
    assert (tmp_path / "two.txt").read_bytes() == kc.golden("pe_k5.default.txt.gz") and r.stdout == _tsv("pe_k5")
