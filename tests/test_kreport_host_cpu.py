"""centrifuger-kreport on the host (`--gpu none`, cfr_kreport with device = -1) against the Perl script's own output for the fixtures of
tests/golden/kreport, the Python restatement of the script (tests/kreport_cases.py) against the same fixtures, and the host twin
through the C-ABI against the restatement on random reads: the semantics stated in csrc/cfr_kreport_core.hpp.  No GPU."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import kreport_cases as kc
import quant_fixtures as qf
from centrifuger_amd import capi
from conftest import GOLDEN

KEYS = ["se_k1", "pe_k5", "edge", "wide"]


def test_manifest_is_what_the_issue_recorded():
    out = kc.MANIFEST["outputs"]
    assert len(out["edge.default.txt.gz"]["warnings"]) == 4 and len(out["wide.default.txt.gz"]["warnings"]) == 73
    assert out["wide.default.txt.gz"]["lines"] == 734
    assert out["pe_k5.filter.txt.gz"]["kept"] == 1117 and out["pe_k5.filter.txt.gz"]["args"] == ["--min-score", "10000", "--min-length", "100"]
    first = kc.golden("se_k1.default.txt.gz").split(b"\n")[0].split(b"\t")
    assert first[1] == b"300" and first[0] == b" 10.00"                                  # 300 unclassified of 3000
    assert all(o["status"] != 0 and o["died"] and o["lines"] == 0 for n, o in out.items() if ".drop_all." in n)
    assert kc.MANIFEST["usage_status"] == 64


@pytest.mark.parametrize("key", KEYS)
def test_restatement_equals_script(key):
    """pins tests/kreport_cases.py: every option set of the manifest, stdout and the warning lines in order"""
    cases = kc.outputs(key)
    assert len(cases) == 8
    s = kc.Script(cases[0][1]["index"])
    header, rows = kc.read_rows(os.path.join(GOLDEN, cases[0][1]["input"]))
    for name, o in cases:
        kw, rep = kc.options_of(o["args"])
        counts, scores, seq, warn = s.count_rows(header, rows, **kw)
        got = s.report(counts, scores, seq, **rep)
        assert warn == o["warnings"], name
        assert (got or b"") == kc.golden(name), name
        assert (got is None) == (o["status"] != 0), name


@pytest.mark.parametrize("key", KEYS + ["count_table"])
def test_command_line_equals_script(key):
    cases = kc.outputs(key)
    assert len(cases) == (2 if key == "count_table" else 8)
    for name, o in cases:
        r = kc.run_kreport(["--gpu", "none", "-x", kc.PREFIXES[o["index"]]] + o["args"] + [os.path.join(GOLDEN, o["input"])])
        assert r.stdout == kc.golden(name), name
        assert kc.warning_ids(r.stderr) == o["warnings"], name
        assert (r.returncode != 0) == (o["status"] != 0), (name, r.stderr.decode())
        if o["died"]:
            assert b"No sequence matches with given settings" in r.stderr and r.returncode == o["status"]


def test_plain_file_stdin_and_option_order(tmp_path):
    raw = gzip.open(qf.tsv_path("pe_k5"), "rb").read()
    plain = tmp_path / "pe_k5.tsv"
    plain.write_bytes(raw)
    want = kc.golden("pe_k5.score.txt.gz")
    assert kc.run_kreport(["--report-score-data", str(plain), "--gpu", "none", "-x", qf.PREFIX, "-t", "1"]).stdout == want
    assert kc.run_kreport(["--gpu", "none", "-x", qf.PREFIX, "--report-score-data"], input=raw).stdout == want                 # stdin
    assert kc.run_kreport(["--gpu", "none", "-x", qf.PREFIX, "--report-score-data", "-"], input=gzip.compress(raw)).stdout == want   # gz on stdin
    # --no-lca runs on the host for every --gpu, with a log line, and touches no device
    r = kc.run_kreport(["-x", qf.PREFIX, "--no-lca", str(plain)], env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert r.returncode == 0 and r.stdout == kc.golden("pe_k5.no_lca.txt.gz") and b"--no-lca" in r.stderr and b"host" in r.stderr


def test_wider_files_and_moved_columns(tmp_path):
    """columns are found by the header's names"""
    header, rows = kc.read_rows(qf.tsv_path("edge"))
    order = [7, 2, 0, 3, 1, 5, 6, 4]
    lines = [header + ["barcode", "UMI"]] + [r + ["ACGT", "TT"] for r in rows]
    p = tmp_path / "moved.tsv"
    p.write_text("\n".join("\t".join([l[k] for k in order] + l[8:]) for l in lines))            # (no newline at the end of the file)
    head = p.read_text().split("\n")[0].split("\t")
    assert head[0] == "numMatches" and head[-2:] == ["barcode", "UMI"] and len(head) == 10
    r = kc.run_kreport(["--gpu", "none", "-x", qf.PREFIX, str(p)])
    assert r.returncode == 0 and r.stdout == kc.golden("edge.default.txt.gz"), r.stderr.decode()


def test_usage_and_refusals(tmp_path):
    r = kc.run_kreport([])
    assert r.returncode == 64 and r.stdout == b"" and b"Usage: centrifuger-kreport -x <index name>" in r.stderr
    r = kc.run_kreport(["--gpu", "none", qf.tsv_path("edge")])
    assert r.returncode == 64 and r.stdout == b""
    r = kc.run_kreport(["--help"])
    assert r.returncode == 0 and b"--gpu" in r.stderr
    r = kc.run_kreport(["--gpu", "none", "-x", qf.PREFIX, qf.tsv_path("edge"), qf.tsv_path("edge")])
    assert r.returncode != 0 and r.stdout == b"" and b"one classification file" in r.stderr
    r = kc.run_kreport(["--gpu", "none", "-x", str(tmp_path / "absent"), qf.tsv_path("edge")])
    assert r.returncode != 0 and r.stdout == b"" and b"absent" in r.stderr
    r = kc.run_kreport(["--gpu", "none", "-x", qf.PREFIX, str(tmp_path / "absent.tsv")])
    assert r.returncode != 0 and r.stdout == b""
    r = kc.run_kreport(["--gpu", "x", "-x", qf.PREFIX, qf.tsv_path("edge")])
    assert r.returncode != 0 and b"--gpu" in r.stderr
    # a file that ends inside a row group, and a header without the columns
    cut = tmp_path / "cut.tsv"
    cut.write_text("readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\na\tx\t61\t9\t9\t99\t100\t3\na\tx\t62\t9\t9\t99\t100\t3\n")
    r = kc.run_kreport(["--gpu", "none", "-x", qf.PREFIX, str(cut)])
    assert r.returncode != 0 and r.stdout == b"" and b"ends inside a row group" in r.stderr
    bad = tmp_path / "bad.tsv"
    bad.write_text("a\tb\tc\n1\t2\t3\n")
    r = kc.run_kreport(["--gpu", "none", "-x", qf.PREFIX, str(bad)])
    assert r.returncode != 0 and r.stdout == b"" and b"header" in r.stderr


def _index_without_node_one(tmp_path):
    """q8 with its root renumbered: <prefix>.2.cfr is all the report reads; the tax id is patched in the golden file's bytes"""
    t = capi.Taxonomy(qf.PREFIX)
    assert int(t.orig_taxid[t.root]) == 1
    t.close()
    raw = open(qf.PREFIX + ".2.cfr", "rb").read()
    one = (1).to_bytes(8, "little")
    at = [k for k in range(0, len(raw) - 7) if raw[k:k + 8] == one]
    return raw, at


def test_index_without_tax_id_one_is_refused(tmp_path):
    raw, at = _index_without_node_one(tmp_path)
    L = capi.lib()
    refused = 0
    for k in at:                                           # whichever 8 bytes hold the root's original id: that patch must be refused
        patched = raw[:k] + (7777).to_bytes(8, "little") + raw[k + 8:]
        (tmp_path / "nr.2.cfr").write_bytes(patched)
        try:
            t = capi.Taxonomy(str(tmp_path / "nr"))
        except capi.CfrError:
            continue
        is_it = 1 not in t.orig_taxid.tolist() and 7777 in t.orig_taxid.tolist()
        t.close()
        if not is_it:
            continue
        h = C.c_void_p()
        o = capi.kreport_options()
        assert L.cfr_kreport_open(str(tmp_path / "nr").encode(), C.byref(o), -1, C.byref(h)) == capi.CFR_ERR_FORMAT and not h
        assert b"tax id 1" in L.cfr_last_error()
        r = kc.run_kreport(["--gpu", "none", "-x", str(tmp_path / "nr"), qf.tsv_path("edge")])
        assert r.returncode != 0 and r.stdout == b"" and b"tax id 1" in r.stderr
        refused += 1
    assert refused >= 1


def _host(prefix, reads, tree, nc, chunks=1, arrays_kw=None, **options):
    k = capi.Kreport(prefix, device=None, **options)
    res, mat = kc.arrays(tree, reads, nc, **(arrays_kw or {}))
    edges = np.linspace(0, len(reads), chunks + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        k.add_results(res[a:b].copy(), mat)
    out = k.counts(), k.warnings().tolist()
    k.close()
    return out


@pytest.mark.parametrize("idx,n", [("q8", 3000), ("qw", 6000)])
def test_host_twin_equals_restatement(idx, n):
    s = kc.Script(idx)
    t = capi.Taxonomy(kc.PREFIXES[idx])
    nc = int(t.node_cnt)
    rng = np.random.default_rng(2718)
    reads = kc.random_reads(s.tree, rng, n) + [(s.tree.orig[:40] * 2, 1 << 40, 150)]
    for options, kw in (({}, {}), ({"min_score": 500000, "min_length": 150, "score_data": True}, {"min_score": 500000, "min_length": 150})):
        counts, scores, seq, warn = s.count_reads(reads, **kw)
        clade, cscore = s.clades(counts, scores)
        (own, cl, sc, csc, seq_count), w = _host(kc.PREFIXES[idx], reads, s.tree, nc, chunks=3, arrays_kw={"seq_to_tax": t.seq_to_tax, "rng": np.random.default_rng(5), "gap": 1},
                                                 **options)
        assert seq_count == seq and 0 < seq < len(reads) + (0 if kw else 1)
        assert np.array_equal(own, s.bins(counts, nc)) and np.array_equal(cl, s.bins({k: v for k, v in clade.items() if k == 0 or k in s.tree.compact}, nc))
        assert np.array_equal(sc, s.bins(scores, nc)) and np.array_equal(csc, s.bins(cscore, nc))
        assert w == warn and len(warn) > 0
        assert int(own.sum()) == seq
    t.close()


def test_named_cases():
    s = kc.Script("q8")
    c, nc = s.tree.compact, 14
    reads = [([61, 62, 61], 10, 100), ([61, 90], 20, 100), ([9999, 61], 30, 100), ([61, 9999], 40, 100), ([9999, 9999], 50, 100), ([9999], 60, 100),
             ([], 0, 0), ([50], 5, 100), ([1], 70, 100), ([61], 100, 99), ([61], 4, 100), ([61], 100, 100)]
    (own, clade, sc, csc, seq), w = _host(qf.PREFIX, reads, s.tree, nc, min_score=5, min_length=100, score_data=True)
    # [] is dropped by min_length (its one row has hit length 0); a score and a length AT the threshold stay, one below goes
    assert seq == 9 and int(own[nc]) == 0
    assert int(own[c[60]]) == 1 and int(own[c[40]]) == 1 and int(own[c[50]]) == 1 and int(own[c[61]]) == 1
    assert int(own[c[1]]) == 5 and int(sc[c[1]]) == 70 and int(sc[c[61]]) == 100 and int(sc[c[50]]) == 5
    assert int(clade[c[1]]) == 9 and int(csc[c[1]]) == 100 and int(clade[c[50]]) == 3
    # [9999, 9999]: isTaxIDInTree, then lca(1, 9999) prints once more - the one place where the fold differs from centrifuger-promote's
    assert w == [9999] * 5
    (own, _c, _s, _cs, seq), w = _host(qf.PREFIX, reads, s.tree, nc)
    assert seq == 12 and int(own[nc]) == 1 and int(own[c[61]]) == 3 and w == [9999] * 5


def test_add_counts_write_and_nothing_counted(tmp_path):
    k = capi.Kreport(qf.PREFIX, device=None)
    with pytest.raises(capi.CfrError) as e:
        k.write(str(tmp_path / "none.txt"))
    assert e.value.status == capi.CFR_ERR_ARG and "No sequence matches with given settings" in str(e.value) and not (tmp_path / "none.txt").exists()
    a = capi.Kreport(qf.PREFIX, device=None)
    a.add_tsv(qf.tsv_path("pe_k5"))
    own, _cl, sc, _cs, seq = a.counts()
    half = own // np.uint64(2)
    k.add_counts(half, sc)
    k.add_counts(own - half)
    k.write(str(tmp_path / "r.txt"))
    assert (tmp_path / "r.txt").read_bytes() == kc.golden("pe_k5.default.txt.gz") and k.counts()[4] == seq == 2000
    with pytest.raises(capi.CfrError):
        k.add_counts(own[:5].copy())
    st = a.stats()
    assert st.parse_ms > 0 and st.accumulate_ms == 0
    a.close()
    k.close()


def test_argument_errors():
    L = capi.lib()
    h = C.c_void_p()
    o = capi.kreport_options()
    p = qf.PREFIX.encode()
    assert L.cfr_kreport_open(None, C.byref(o), -1, C.byref(h)) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_open(p, None, -1, C.byref(h)) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_open(p, C.byref(o), -1, None) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_open(p, C.byref(o), -2, C.byref(h)) == capi.CFR_ERR_ARG
    bad = capi.kreport_options(lds_slots=100)
    assert L.cfr_kreport_open(p, C.byref(bad), -1, C.byref(h)) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_open((qf.PREFIX + "_absent").encode(), C.byref(o), -1, C.byref(h)) == capi.CFR_ERR_IO and not h
    assert L.cfr_kreport_open(p, C.byref(o), -1, C.byref(h)) == capi.CFR_OK and h
    res = np.zeros(1, dtype=capi.RESULT_DTYPE)
    res["n_match"] = 1
    n = C.c_size_t(0)
    seq = C.c_double(0)
    assert L.cfr_kreport_add_results(h, None, None, C.c_size_t(1)) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_add_results(h, capi._p(res), None, C.c_size_t(1)) == capi.CFR_ERR_ARG       # a classified read and no matches
    assert L.cfr_kreport_add_results(h, None, None, C.c_size_t(0)) == capi.CFR_OK
    assert L.cfr_kreport_add_tsv(h, None) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_add_tsv(h, (qf.PREFIX + "_absent.tsv").encode()) == capi.CFR_ERR_IO
    assert L.cfr_kreport_add_count_table(h, None) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_add_counts(h, None, None, C.c_size_t(15)) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_bins(h, None) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_counts(h, None, None, None, None, C.c_size_t(0), None) == capi.CFR_ERR_ARG
    own = np.zeros(15, dtype=np.uint64)
    assert L.cfr_kreport_counts(h, capi._p(own), None, None, None, C.c_size_t(14), C.byref(seq)) == capi.CFR_ERR_CAPACITY
    assert L.cfr_kreport_counts(h, None, None, None, None, C.c_size_t(0), C.byref(seq)) == capi.CFR_OK and seq.value == 0
    assert L.cfr_kreport_warnings(h, None, C.c_size_t(0), None) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_warnings(h, None, C.c_size_t(3), C.byref(n)) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_get_stats(h, None) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_write(h, None) == capi.CFR_ERR_ARG and L.cfr_last_error() == b"No sequence matches with given settings"
    assert L.cfr_kreport_close(h) == capi.CFR_OK
    # a handle that is not open: closed, null, or never one
    assert L.cfr_kreport_close(h) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_add_results(h, None, None, C.c_size_t(0)) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_add_tsv(None, b"x") == capi.CFR_ERR_ARG
    assert L.cfr_kreport_write(h, None) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_close(None) == capi.CFR_ERR_ARG
    assert b"cfr_kreport" in L.cfr_last_error()
    # --no-lca takes a file, not result arrays
    no = capi.kreport_options(no_lca=True)
    assert L.cfr_kreport_open(p, C.byref(no), -1, C.byref(h)) == capi.CFR_OK
    mat = np.zeros(1, dtype=capi.MATCH_DTYPE)
    assert L.cfr_kreport_add_results(h, capi._p(res), capi._p(mat), C.c_size_t(1)) == capi.CFR_ERR_ARG
    assert L.cfr_kreport_close(h) == capi.CFR_OK
