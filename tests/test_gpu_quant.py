"""centrifuger-quant on the device (k_quant_coalesce, k_quant_estep_terms / k_quant_estep_sum) against the host twin (cfr_quant with
device = -1, itself pinned to the reference quantifier by tests/test_quant_host_cpu.py): coalesced assignments and EM values bit for
bit, and the two command lines against the reference's reports.  -m gpu."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import quant_fixtures as qf
from centrifuger_amd import capi
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")


def _records(lists, rng=None, metas=None):
    """results / matches for cfr_quant_add_results: read i has the ORIGINAL tax ids lists[i]; score, lengths and second score vary so
    that every weight 4^-d (d = 0..11) and both values of uniq occur"""
    n = len(lists)
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    begin = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.uint64)
    mat = np.zeros(max(int(begin[-1]), 1), dtype=capi.MATCH_DTYPE)
    for i, t in enumerate(lists):
        d, uniq = metas[i] if metas is not None else (int(rng.integers(0, 12)), int(rng.integers(0, 2)))
        res[i] = (1000, 0 if uniq else 1000, 150 - 1 - d if d else 150, 150, len(t), 0, begin[i])
        mat["taxid"][int(begin[i]):int(begin[i + 1])] = t
    return res, mat


def _both(res, mat, table_slots=0):
    out = []
    for device in (None, 0):
        q = capi.Quant(qf.PREFIX, device=device, table_slots=table_slots)
        q.add_results(res, mat)
        out.append(qf.as_tuples(q.assignments()))
        st = q.stats()
        q.close()
    return out[0], out[1], st


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_coalesce_equals_host(n, k):
    rng = np.random.default_rng(n * 10 + k)
    ids = np.array(qf.orig_taxids() + [9999], dtype=np.uint64)          # 9999: not in the tree -> node_cnt
    lists = [ids[rng.integers(0, len(ids), size=int(rng.integers(1, k + 1)))].tolist() for _ in range(n)]
    host, dev, _st = _both(*_records(lists, rng))
    assert dev == host and sum(c for _t, _w, c, _u in dev) == n


def test_coalesce_identical_records():
    """4097 lanes add to one entry: the sums are exact whatever the order"""
    lists = [[61, 62, 9999]] * 4097
    metas = [(i % 12, i % 2) for i in range(4097)]
    host, dev, _st = _both(*_records(lists, metas=metas))
    assert dev == host and len(dev) == 1
    assert dev[0][2] == 4097 and dev[0][3] == 2048 and dev[0][1] == sum(4.0 ** -(i % 12) for i in range(4097))


def test_coalesce_table_growth():
    """all lists distinct, a table of 64 slots: it is grown (and the batch run again) until 4097 entries fit.  The table is kept at most
    half full, so 4097 entries need 16384 slots = 64 * 2^8: at least 8 doublings"""
    ids = qf.orig_taxids() + [9999]
    lists = []
    for i in range(4097):
        x, t = i, []
        for _ in range(4):
            t.append(ids[x % len(ids)]); x //= len(ids)
        lists.append(t)
    rng = np.random.default_rng(7)
    host, dev, st = _both(*_records(lists, rng), table_slots=64)
    assert dev == host and len(dev) == 4097
    assert st.grow_count >= 8 and st.table_slots >= 16384


def test_closed_handles_give_their_device_memory_back():
    """three handles in turn in this process, each opened, fed 100 records, run and closed: after every close the device's free memory is
    back within 64 MB (slack for the runtime's own pools, not a measured figure) of what it was before the first"""
    import torch
    rng = np.random.default_rng(3)
    ids = np.array(qf.orig_taxids() + [9999], dtype=np.uint64)
    res, mat = _records([ids[rng.integers(0, len(ids), size=int(rng.integers(1, 4)))].tolist() for _ in range(100)], rng)
    torch.cuda.synchronize(0)
    before = torch.cuda.mem_get_info(0)[0]
    for k in range(3):
        q = capi.Quant(qf.PREFIX, device=0)
        q.add_results(res, mat)
        assert sum(c for _t, _w, c, _u in qf.as_tuples(q.assignments())) == 100
        q.run()
        q.close()
        after = torch.cuda.mem_get_info(0)[0]
        print(f"handle {k}: free before the first {before}, after this close {after}, held {(before - after) / 2**20:.1f} MB")
        assert before - after <= 64 << 20, (k, before, after)


def test_coalesce_order_prefix_and_unknown():
    node_cnt = len(qf.orig_taxids())
    lists = [[61, 62], [62, 61], [61, 62], [61], [61, 62, 70], [61, 62, 70, 71], [9999], [9999, 8888], [9999, 61], [61, 9999], [61, 62, 70]]
    metas = [(i % 3, 1 if len(t) == 1 else 0) for i, t in enumerate(lists)]
    host, dev, _st = _both(*_records(lists, metas=metas))
    assert dev == host and len(dev) == 9
    got = [t for t, _w, _c, _u in dev]
    c = {o: i for i, o in enumerate(qf.orig_taxids())}
    assert (c[61], c[62]) in got and (c[62], c[61]) in got and (node_cnt, node_cnt) in got and (node_cnt,) in got


def _run_both(feed):
    out = []
    for device in (None, 0):
        q = capi.Quant(qf.PREFIX, device=device)
        feed(q)
        rounds = q.run()
        v = q.values()
        out.append((rounds, {k: qf.bits(v[k]) if k != "taxid_length" else v[k] for k in ("abund", "read_count", "uniq_count", "taxid_length")}))
        q.close()
    return out


def _assert_same_bits(host, dev):
    assert dev[0] == host[0], f"EM rounds: device {dev[0]}, host {host[0]}"
    for k in host[1]:
        assert np.array_equal(dev[1][k], host[1][k]), k


@pytest.mark.parametrize("key", ["se_k1", "pe_k5", "edge"])
def test_em_values_equal_host_bit_for_bit(key):
    host, dev = _run_both(lambda q: q.add_tsv(qf.tsv_path(key)))
    _assert_same_bits(host, dev)
    assert host[0] >= 1 and host[1]["abund"].any()


def test_em_fan_in_and_double_root():
    """strain 62 stands in 1000 distinct lists, subspecies 71 in one, and one list holds the root twice (two foreign tax ids)"""
    ids = [50, 60, 61, 70, 80, 90, 91, 40, 30, 20]
    lists = []
    for i in range(1000):
        lists.append([62, ids[i % 10], ids[(i // 10) % 10], ids[(i // 100) % 10]])
    lists += [[71, 61], [9999, 8888], [61], [90, 91]] + [[61]] * 37 + [[91]] * 11
    rng = np.random.default_rng(11)
    res, mat = _records(lists, rng)
    host, dev = _run_both(lambda q: q.add_results(res, mat))
    _assert_same_bits(host, dev)
    assert host[0] > 1


@pytest.mark.parametrize("key", qf.TSV_KEYS)
def test_quant_cli_device_equals_reference(key):
    for name, _key, fmt, extra in qf.reports(key):
        r = qf.run_quant(["-x", qf.PREFIX, "-c", qf.tsv_path(key), "--output-format", str(fmt)] + extra)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == qf.expected(name), name
        assert b"device" in r.stderr


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("quant_reads")
    for f in ("reads_se.fq", "reads_1.fq", "reads_2.fq"):
        (d / f).write_bytes(gzip.open(os.path.join(qf.QDIR, f + ".gz"), "rb").read())
    return d


@pytest.mark.parametrize("key", ["se_k1", "pe_k5"])
def test_classifier_quant_option(key, reads, tmp_path):
    """bin/centrifuger --quant: the report of the run equals the reference quantifier's on the reference's TSV for the same reads,
    in all four formats, and the TSV on stdout is the one the run prints without the option"""
    args = ["-u", str(reads / "reads_se.fq"), "-k", "1"] if key == "se_k1" else ["-1", str(reads / "reads_1.fq"), "-2", str(reads / "reads_2.fq"), "-k", "5"]
    base = [CLI, "-x", qf.PREFIX, "-t", "2"] + args
    plain = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert plain.returncode == 0, plain.stderr.decode()
    assert plain.stdout == gzip.open(qf.tsv_path(key), "rb").read()
    for fmt in range(4):
        rep = tmp_path / f"r{fmt}.txt"
        r = subprocess.run(base + ["--quant", str(rep), "--quant-format", str(fmt)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == plain.stdout
        assert rep.read_bytes() == qf.expected(f"{key}.n{fmt}.txt"), fmt
