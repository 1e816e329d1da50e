"""centrifuger-quant on the host (`--gpu none`, cfr_quant with device = -1) against the reference quantifier's own output for the
fixtures of tests/golden/quant: every report byte for byte, the coalesced assignments against a Python restatement, and the reader
(gz, stdin, threads).  No GPU."""
import gzip
import os

import numpy as np
import pytest

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
