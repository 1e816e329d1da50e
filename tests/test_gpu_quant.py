"""centrifuger-quant on the device (k_quant_coalesce, k_quant_estep_terms / k_quant_estep_sum) against the host twin (cfr_quant with
device = -1, itself pinned to the reference quantifier by tests/test_quant_host_cpu.py): coalesced assignments and EM values bit for
bit, and the two command lines against the reference's reports; the E-step alone (cfr_quant_estep_probe) against the sequential
restatement of tests/quant_estep_cases.py and against the host twin, bit for bit.  -m gpu."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import quant_estep_cases as ec
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


def _both(res, mat, table_slots=0, prefix=qf.PREFIX):
    out = []
    for device in (None, 0):
        q = capi.Quant(prefix, device=device, table_slots=table_slots)
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


def _run_both(feed, prefix=qf.PREFIX):
    out = []
    for device in (None, 0):
        q = capi.Quant(prefix, device=device)
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


# ---- the wide fixture (tests/golden/quant_wide: 811 nodes, so k_quant_estep_sum runs four blocks and node indices go far beyond 13) ----
def test_wide_em_values_equal_host_bit_for_bit():
    host, dev = _run_both(lambda q: q.add_tsv(qf.tsv_path("wide", qf.WIDE_DIR)), prefix=qf.WIDE_PREFIX)
    print(f"EM rounds: host {host[0]}, device {dev[0]}")
    _assert_same_bits(host, dev)
    assert host[0] > 100 and host[1]["abund"].any()


def test_wide_quant_cli_device_equals_reference():
    cases = qf.reports("wide", qf.WIDE_DIR)
    assert len(cases) == 8
    for name, _key, fmt, extra in cases:
        r = qf.run_quant(["-x", qf.WIDE_PREFIX, "-c", qf.tsv_path("wide", qf.WIDE_DIR), "--output-format", str(fmt)] + extra)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == qf.expected(name, qf.WIDE_DIR), name
        assert b"device" in r.stderr


# ---- the E-step alone ----
def _probe_both(case):
    a_begin, a_target, a_weight, n_nodes, abund, init = case
    return [capi.quant_estep_probe(a_begin, a_target, a_weight, n_nodes, abund, init=init, device=d) for d in (None, 0)]


@pytest.mark.parametrize("n_slots", ec.GRID_SLOTS)
@pytest.mark.parametrize("n_nodes", ec.GRID_NODES)
def test_estep_probe_grid(n_nodes, n_slots):
    """the edges of both grids (one lane per slot, one lane per node; blocks of 256); nodes without a term give +0.0"""
    host, dev = _probe_both(ec.grid(n_nodes, n_slots))
    ec.assert_same_bits(dev, ec.want("grid", n_nodes, n_slots), "device against the restatement")
    ec.assert_same_bits(dev, host, "device against the host twin")
    assert not ec.bits(dev[:, ec.grid_silent(n_nodes)]).any()


@pytest.mark.parametrize("name", ["order", "long_lists", "value_range"])
def test_estep_probe(name):
    """order: 100 000 terms of 2^-60 .. 2^20 in one node's segment, slot order far from node-major; long_lists: a list of 5000 targets
    over 40 nodes beside lists of 1, 2, 63, 64, 65; value_range: abund drawn by exponent down to the denormals, weights 2^-22 .. 2^40"""
    host, dev = _probe_both(ec.get(name))
    ec.assert_same_bits(dev, ec.want(name), "device against the restatement")
    ec.assert_same_bits(dev, host, "device against the host twin")


def test_estep_probe_zero_sum():
    """one list whose targets all have abund 0: NaN at exactly its three nodes (as NaN-ness: the sign of a default NaN is the
    platform's), equal bits everywhere else.  What each side returned there is printed."""
    host, dev = _probe_both(ec.get("zero_sum"))
    want = ec.want("zero_sum")
    z = list(ec.ZERO_NODES)
    print("NaN bits at the zero-sum nodes: device", [hex(int(x)) for x in ec.bits(dev[0, z])], "host twin", [hex(int(x)) for x in ec.bits(host[0, z])],
          "numpy", [hex(int(x)) for x in ec.bits(want[0, z])])
    assert np.nonzero(np.isnan(want[0]))[0].tolist() == z
    ec.assert_same_bits(dev, want, "device against the restatement", nan_ok=True)
    ec.assert_same_bits(host, want, "host twin against the restatement", nan_ok=True)


def test_estep_probe_reuse():
    """the init round and three abundance vectors through one E-step object (d_abund_, terms_ and the pinned buffer are used four
    times): every round equals the restatement, and round 3 equals a fresh object that is given vector 3 alone"""
    case = ec.get("reuse")
    a_begin, a_target, a_weight, n_nodes, abund, _init = case
    host, dev = _probe_both(case)
    ec.assert_same_bits(dev, ec.want("reuse"), "device against the restatement")
    ec.assert_same_bits(dev, host, "device against the host twin")
    fresh = capi.quant_estep_probe(a_begin, a_target, a_weight, n_nodes, abund[2:3], init=False, device=0)
    ec.assert_same_bits(dev[3:4], fresh, "round 3 of 4 against a fresh object")


# ---- coalesce: several batches, dead entries, the arena ----
def _records_flat(lengths, taxids, d, uniq):
    """_records without a loop: read i has the original tax ids taxids[begin[i] .. begin[i] + lengths[i]), the weight 4^-d[i] and uniq[i]"""
    n = len(lengths)
    begin = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    res["score"] = 1000
    res["secondary_score"] = np.where(uniq, 0, 1000)
    res["hit_length"] = np.where(d > 0, 150 - 1 - d, 150)
    res["query_length"] = 150
    res["n_match"] = lengths
    res["match_begin"] = begin[:-1]
    mat = np.zeros(int(begin[-1]), dtype=capi.MATCH_DTYPE)
    mat["taxid"] = taxids
    return res, mat


def _wide_ids():
    return np.array(qf.orig_taxids(qf.WIDE_PREFIX) + [99999], dtype=np.uint64)        # 99999: not in the tree -> node_cnt


def test_coalesce_three_batches():
    """2^21 + 5000 records in one add_results call: the records are handed to the coalescer in batches of 2^20, 2^20 and (at finish)
    5000, so both pinned buffers are used, the first one twice.  Batch 1 draws from 5000 lists of 2 targets, batch 2 from 5000 lists
    of 3, batch 3 is 5000 distinct lists of 850 - more words than batch 1, so the first buffer is regrown on its second use.  Every
    batch brings more new lists than the table has room for: a 64-slot table grows while batch 1 is resolved (inside the add of batch 2),
    while batch 2 is resolved (inside the add of batch 3), and at finish"""
    ids = _wide_ids()
    rng = np.random.default_rng(21)
    n1 = 1 << 20
    j1, j2, j3 = rng.integers(0, 5000, size=n1), rng.integers(0, 5000, size=n1), np.arange(5000)
    t1 = np.stack([j1 % 812, j1 // 812], axis=1)
    t2 = np.stack([j2 % 812, j2 // 812, np.full(n1, 5)], axis=1)
    t3 = rng.integers(0, 812, size=(5000, 850))
    t3[:, 0], t3[:, 1] = j3 % 812, j3 // 812
    assert 5000 * (850 + 2) > n1 * (2 + 2)
    lengths = np.concatenate([np.full(n1, 2), np.full(n1, 3), np.full(5000, 850)])
    taxids = ids[np.concatenate([t1.ravel(), t2.ravel(), t3.ravel()])]
    n = len(lengths)
    assert n == (1 << 21) + 5000
    res, mat = _records_flat(lengths, taxids, rng.integers(0, 12, size=n), rng.integers(0, 2, size=n))
    host, dev, st = _both(res, mat, table_slots=64, prefix=qf.WIDE_PREFIX)
    distinct = len(host)
    by_len = {k: sum(1 for t, _w, _c, _u in host if len(t) == k) for k in (2, 3, 850)}
    print(f"distinct {distinct} {by_len}, grow_count {st.grow_count}, table_slots {st.table_slots}")
    assert min(by_len.values()) >= 4097 and sum(by_len.values()) == distinct
    assert dev == host and sum(c for _t, _w, c, _u in dev) == n
    assert st.grow_count >= int(np.ceil(np.log2(2 * distinct / 64))) and st.table_slots >= 2 * distinct


def test_coalesce_dead_entries_then_growth():
    """4097 distinct lists, 40 copies of each in random order, a table of 64 slots: lanes that hold the same list write an entry each
    and all but one lose the slot (dead entries); the growths that follow carry the dead entries along and must skip them"""
    ids = _wide_ids()
    rng = np.random.default_rng(40)
    j = rng.permutation(np.repeat(np.arange(4097), 40))
    t = np.stack([j % 812, j // 812, (7 * j) % 812], axis=1)
    n = len(j)
    res, mat = _records_flat(np.full(n, 3), ids[t.ravel()], rng.integers(0, 12, size=n), rng.integers(0, 2, size=n))
    host, dev, st = _both(res, mat, table_slots=64, prefix=qf.WIDE_PREFIX)
    print(f"grow_count {st.grow_count}, table_slots {st.table_slots}")
    assert dev == host and len(dev) == 4097 and sum(c for _t, _w, c, _u in dev) == n
    assert all(c == 40 for _t, _w, c, _u in dev)
    assert st.grow_count >= 8 and st.table_slots >= 2 * 4097


def test_coalesce_arena_fills_first():
    """18 records, so entries (live and dead) stay below the 32 a 64-slot table holds: every growth is the arena's (256 words at the
    start, doubled until the keys fit; the longest alone needs 65535 = 256 * 2^8).  Lists of 1, 2, 255, 256, 257, 4096 and 65535 targets;
    each of the five long ones has a twin that differs in its last word only and a twin without the last word; the list of 2 is given twice"""
    ids = _wide_ids()
    rng = np.random.default_rng(65535)
    lists = [ids[rng.integers(0, 812, size=k)].tolist() for k in (1, 2)]
    lists.append(list(lists[1]))
    for k in (255, 256, 257, 4096, 65535):
        t = ids[rng.integers(0, 811, size=k)].tolist()
        lists += [t, t[:-1] + [99999], t[:-1]]
    assert len(lists) == 18 <= 30
    order = rng.permutation(len(lists))
    lists = [lists[i] for i in order]
    host, dev, st = _both(*_records(lists, rng), table_slots=64, prefix=qf.WIDE_PREFIX)
    print(f"grow_count {st.grow_count}, table_slots {st.table_slots}")
    assert dev == host and len(dev) == 17 and sum(c for _t, _w, c, _u in dev) == 18
    assert [c for t, _w, c, _u in dev if len(t) == 2] == [2] and sorted(c for t, _w, c, _u in dev if len(t) != 2) == [1] * 16
    assert sorted(len(t) for t, _w, _c, _u in dev) == sorted([1, 2] + [k - e for k in (255, 256, 257, 4096, 65535) for e in (0, 0, 1)])
    assert st.grow_count >= 8
