"""centrifuger-quant on the host (`--gpu none`, cfr_quant with device = -1) against the reference quantifier's own output for the
fixtures of tests/golden/quant and tests/golden/quant_wide: every report byte for byte, the coalesced assignments against a Python
restatement, the reader (gz, stdin, threads), and the E-step alone (cfr_quant_estep_probe) against a sequential restatement.  No GPU."""
import gzip
import os

import numpy as np
import pytest

import quant_estep_cases as ec
import quant_fixtures as qf
from centrifuger_amd import capi


@pytest.mark.parametrize("key", qf.TSV_KEYS)
def test_reports_equal_reference(key):
    cases = qf.reports(key)
    assert len(cases) == 8
    for name, _key, fmt, extra in cases:
        r = qf.run_quant(["--gpu", "none", "-x", qf.PREFIX, "-c", qf.tsv_path(key), "--output-format", str(fmt)] + extra)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == qf.expected(name), name
        assert b"starts" in r.stderr and b"finishes" in r.stderr


def test_gz_plain_and_stdin_give_the_same_bytes(tmp_path):
    raw = gzip.open(qf.tsv_path("pe_k5"), "rb").read()
    plain = tmp_path / "pe_k5.tsv"
    plain.write_bytes(raw)
    want = qf.expected("pe_k5.n2.txt")
    base = ["--gpu", "none", "-x", qf.PREFIX, "--output-format", "2"]
    assert qf.run_quant(base + ["-c", str(plain)]).stdout == want
    assert qf.run_quant(base + ["-c", qf.tsv_path("pe_k5")]).stdout == want
    assert qf.run_quant(base + ["-c", "-"], stdin=raw).stdout == want
    assert qf.run_quant(base + ["-c", "-"], stdin=gzip.compress(raw)).stdout == want


@pytest.mark.parametrize("min_score,min_length", [(0, 0), (300, 40)])
def test_assignments_equal_python_restatement(min_score, min_length):
    for key in ("edge", "pe_k5"):
        q = capi.Quant(qf.PREFIX, device=None, min_score=min_score, min_length=min_length)
        q.add_tsv(qf.tsv_path(key))
        got = qf.as_tuples(q.assignments())
        q.close()
        want = qf.restate(qf.read_rows(qf.tsv_path(key)), min_score, min_length)
        assert got == want
    # the edge file holds what it was made for
    lists = [t for t, _w, _c, _u in qf.restate(qf.read_rows(qf.tsv_path("edge")))]
    node_cnt = len(qf.orig_taxids())
    assert (node_cnt, node_cnt) in lists and any(len(t) == 3 for t in lists)
    a, b = sorted(set(t for t in lists if len(t) == 2 and node_cnt not in t))[:2]
    assert a == b[::-1]


def test_reader_threads_and_chunk_borders(tmp_path):
    """a file of many line-aligned chunks whose borders fall inside groups: 1 and 16 reader threads give the sequential result"""
    rows = open(qf.tsv_path("edge")).read().split("\n")
    header, body = rows[0], [r for r in rows[1:] if r]
    big = tmp_path / "big.tsv"
    with open(big, "w") as f:
        f.write(header + "\n")
        for rep in range(3000):      # the last and the first row of the block share the id r1: one group across the seam
            f.write("\n".join(r if rep % 3 else r.replace("ab\t", f"ab{rep}\t") for r in body) + "\n")
    assert os.path.getsize(big) > 16 * 65536
    out = {}
    for t in (1, 16):
        q = capi.Quant(qf.PREFIX, device=None, threads=t)
        q.add_tsv(str(big))
        out[t] = qf.as_tuples(q.assignments())
        rounds = q.run()
        out[t, "v"] = (rounds, [qf.bits(v).tolist() for k, v in sorted(q.values().items()) if k != "node_cnt"])
        q.close()
    assert out[1] == out[16] and out[1, "v"] == out[16, "v"]
    assert out[1] == qf.restate(qf.read_rows(str(big)))
    r1 = qf.run_quant(["--gpu", "none", "-x", qf.PREFIX, "-c", str(big), "-t", "1"])
    r16 = qf.run_quant(["--gpu", "none", "-x", qf.PREFIX, "-c", str(big), "-t", "16"])
    assert r1.returncode == 0 and r1.stdout == r16.stdout and len(r1.stdout) > 100


def test_add_results_is_one_assignment_per_read():
    """cfr_quant_add_results against the TSV path: the same rows as results, every read its own group"""
    orig = qf.orig_taxids()
    res = np.zeros(5, dtype=capi.RESULT_DTYPE)
    mat = np.zeros(10, dtype=capi.MATCH_DTYPE)
    rows = []
    spec = [(18225, 0, 150, 150, [orig[3]]), (5000, 5000, 130, 150, [orig[7], orig[8]]), (0, 0, 0, 150, []),
            (299, 0, 39, 76, [orig[7]]), (700, 0, 70, 76, [9999, orig[8]])]
    for i, (score, second, hit, length, taxids) in enumerate(spec):
        res[i] = (score, second, hit, length, len(taxids), 0, 2 * i)
        for k, t in enumerate(taxids):
            mat[2 * i + k]["taxid"] = t
            rows.append((f"r{i}", t, score, second, hit, length))
    for ms, ml in ((0, 0), (300, 40)):
        q = capi.Quant(qf.PREFIX, device=None, min_score=ms, min_length=ml)
        q.add_results(res, mat)
        assert qf.as_tuples(q.assignments()) == qf.restate(rows, ms, ml)
        q.close()


@pytest.mark.parametrize("opt", ["--taxonomy-tree", "--name-table", "--size-table"])
def test_unsupported_options_are_rejected(opt):
    r = qf.run_quant(["-c", qf.tsv_path("edge"), opt, "nodes.dmp"])
    assert r.returncode != 0 and r.stdout == b""
    assert b"not supported" in r.stderr and opt.encode() in r.stderr


def test_bad_arguments_fail_with_a_message(tmp_path):
    r = qf.run_quant(["--gpu", "none", "-c", qf.tsv_path("edge")])
    assert r.returncode != 0 and b"-x" in r.stderr
    r = qf.run_quant(["--gpu", "none", "-x", str(tmp_path / "absent"), "-c", qf.tsv_path("edge")])
    assert r.returncode != 0 and r.stdout == b"" and b"absent" in r.stderr
    r = qf.run_quant(["--gpu", "x", "-x", qf.PREFIX, "-c", qf.tsv_path("edge")])
    assert r.returncode != 0 and b"--gpu" in r.stderr


# ---- the wide fixture (tests/golden/quant_wide: 811 nodes) ----
def test_wide_reports_equal_reference():
    cases = qf.reports("wide", qf.WIDE_DIR)
    assert len(cases) == 8
    for name, _key, fmt, extra in cases:
        r = qf.run_quant(["--gpu", "none", "-x", qf.WIDE_PREFIX, "-c", qf.tsv_path("wide", qf.WIDE_DIR), "--output-format", str(fmt)] + extra)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == qf.expected(name, qf.WIDE_DIR), name
    assert qf.expected("wide.n0.txt", qf.WIDE_DIR) != qf.expected("wide.f0.txt", qf.WIDE_DIR)       # the filter leg differs


@pytest.mark.parametrize("min_score,min_length", [(0, 0), (300, 40)])
def test_wide_assignments_equal_python_restatement(min_score, min_length):
    q = capi.Quant(qf.WIDE_PREFIX, device=None, min_score=min_score, min_length=min_length)
    q.add_tsv(qf.tsv_path("wide", qf.WIDE_DIR))
    got = qf.as_tuples(q.assignments())
    q.close()
    want = qf.restate(qf.read_rows(qf.tsv_path("wide", qf.WIDE_DIR)), min_score, min_length, prefix=qf.WIDE_PREFIX)
    assert got == want
    # the file holds what it was made for: 811 nodes, lists of 1..6, several weights, internal nodes, a foreign tax id twice in a list
    orig = qf.orig_taxids(qf.WIDE_PREFIX)
    node_cnt = len(orig)
    assert node_cnt == 811
    lists = [t for t, _w, _c, _u in want]
    assert {len(t) for t in lists} >= {1, 2, 3, 4, 5, 6}
    assert any(t.count(node_cnt) == 2 for t in lists)
    assert sum(1 for t in lists if any(x < node_cnt and orig[x] < 10000 for x in t)) >= 100
    if not min_score:
        assert len({qf.weight(h, n) for _i, _t, _s, _2, h, n in qf.read_rows(qf.tsv_path("wide", qf.WIDE_DIR))}) >= 8


# ---- the E-step alone: cfr_quant_estep_probe with device = -1 (HostEStep behind make_host_estep, after quant_csr_finish) against the
# sequential restatement of tests/quant_estep_cases.py, bit for bit ----
def _probe(case, device=None):
    a_begin, a_target, a_weight, n_nodes, abund, init = case
    return capi.quant_estep_probe(a_begin, a_target, a_weight, n_nodes, abund, init=init, device=device)


@pytest.mark.parametrize("n_slots", ec.GRID_SLOTS)
@pytest.mark.parametrize("n_nodes", ec.GRID_NODES)
def test_estep_probe_host_grid(n_nodes, n_slots):
    got = _probe(ec.grid(n_nodes, n_slots))
    ec.assert_same_bits(got, ec.want("grid", n_nodes, n_slots), "host twin")
    assert not ec.bits(got[:, ec.grid_silent(n_nodes)]).any()          # no term: +0.0


@pytest.mark.parametrize("name", ["order", "long_lists", "value_range", "reuse"])
def test_estep_probe_host(name):
    ec.assert_same_bits(_probe(ec.get(name)), ec.want(name), "host twin")


def test_estep_probe_host_zero_sum():
    want = ec.want("zero_sum")
    assert np.nonzero(np.isnan(want[0]))[0].tolist() == list(ec.ZERO_NODES)
    ec.assert_same_bits(_probe(ec.get("zero_sum")), want, "host twin", nan_ok=True)


def test_estep_cases_hold_what_they_were_made_for():
    a_begin, a_target, _w, n_nodes, _ab, _init = ec.get("order")
    assert int((a_target == 150).sum()) == 100000 and n_nodes == 301
    pos = ec.slot_pos(a_target, n_nodes)
    assert np.mean(pos == np.arange(len(pos))) < 0.01 and np.mean(np.abs(pos - np.arange(len(pos)))) > len(pos) / 10
    a_begin, a_target, _w, n_nodes, _ab, _init = ec.get("long_lists")
    lens = np.diff(a_begin.astype(np.int64)).tolist()
    assert set(lens) == {1, 2, 63, 64, 65, 5000}
    big = a_target[int(a_begin[lens.index(5000)]):int(a_begin[lens.index(5000) + 1])]
    assert len(set(big.tolist())) == 40 and np.bincount(big).max() > 1 and (np.bincount(big)[np.unique(big)] > 1).all()
    a_begin, a_target, _w, n_nodes, ab, _init = ec.get("value_range")
    tiny = np.finfo(np.float64).tiny
    assert (ab[0, :200] < tiny).all() and ab.min() == 2.0 ** -1074 and ab.max() < 2 and (ab > 0).all()
    out = ec.want("value_range")[0]
    assert np.isfinite(out).all()
    assert ((out[100:150] > 0) & (out[100:150] < tiny)).sum() >= 10          # results that are sums of denormal terms
    ab3 = ec.get("reuse")[4]
    assert ab3.shape == (3, 700) and not np.array_equal(ab3[0], ab3[2])


def test_estep_probe_rejects_bad_input():
    ok = (np.array([0, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint32), np.array([1.0]))
    with pytest.raises(capi.CfrError, match="below n_nodes"):
        capi.quant_estep_probe(ok[0], np.array([0, 2], dtype=np.uint32), ok[2], 2, np.ones((1, 2)))
    with pytest.raises(capi.CfrError, match="a_begin"):
        capi.quant_estep_probe(np.array([1, 2], dtype=np.uint64), ok[1], ok[2], 2, np.ones((1, 2)))
    with pytest.raises(capi.CfrError, match="n_nodes"):
        capi.quant_estep_probe(np.array([0, 0], dtype=np.uint64), np.zeros(0, dtype=np.uint32), ok[2], 0)
    assert capi.quant_estep_probe(*ok, 2, np.ones((1, 2))).tolist() == [[0.5, 0.5]]


def test_a_read_of_65536_targets_is_refused():
    """kQuantMaxTargets: 65535 targets are one record, 65536 fail with the library's message - and the handle can still be closed"""
    taxid = qf.orig_taxids()[3]
    for n, fits in ((65535, True), (65536, False)):
        res = np.zeros(1, dtype=capi.RESULT_DTYPE)
        res[0] = (1000, 0, 150, 150, n, 0, 0)
        mat = np.zeros(n, dtype=capi.MATCH_DTYPE)
        mat["taxid"] = taxid
        q = capi.Quant(qf.PREFIX, device=None)
        if fits:
            q.add_results(res, mat)
            (lists, w, c, u) = q.assignments()
            assert len(lists) == 1 and len(lists[0]) == 65535 and set(lists[0]) == {3} and (w[0], c[0], u[0]) == (1.0, 1, 1)
        else:
            with pytest.raises(capi.CfrError, match="more than 65535 targets"):
                q.add_results(res, mat)
        q.close()
        assert not q._q
