"""centrifuger-promote on the host (`--gpu none`, cfr_promote with device = -1) against the Perl script's own output for the fixtures of
tests/golden/promote, and the host twin through the C-ABI against a Python restatement of the script (tests/promote_cases.py) on
hand-made reads: every branch of the semantics stated in csrc/cfr_promote.hpp.  No GPU."""
import ctypes as C
import gzip

import numpy as np
import pytest

import promote_cases as pc
import quant_fixtures as qf
from centrifuger_amd import capi

NC = 14                        # nodes of q8: 1 root / 10 superkingdom / 20 clade / 30 phylum / 40 no rank / 50, 80 genus / 60, 70, 90, 91 species / 61, 62 strain / 71 subspecies


@pytest.mark.parametrize("key", ["se_k1", "pe_k5", "edge", "wide"])
def test_command_line_equals_script(key):
    cases = pc.outputs(key)
    assert len(cases) == 7
    for name, idx, tsv, level, warnings in cases:
        r = pc.run_promote(["--gpu", "none", pc.PREFIXES[idx], tsv, level])
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == pc.golden(name), name
        lines = r.stderr.decode().splitlines()
        assert len(lines) == warnings and all(l.startswith("Couldn't find parent of taxID ") and l.endswith(" - directly assigned to root.") for l in lines), name
    if key == "wide":
        assert dict((level, w) for _n, _i, _t, level, w in cases)["lca"] == 53


def test_plain_file_options_in_any_place_and_threads(tmp_path):
    plain = tmp_path / "pe_k5.tsv"
    plain.write_bytes(gzip.open(qf.tsv_path("pe_k5"), "rb").read())
    want = pc.golden("pe_k5.genus.tsv.gz")
    assert pc.run_promote([qf.PREFIX, str(plain), "genus", "--gpu", "none", "-t", "1"]).stdout == want
    assert pc.run_promote(["-t", "16", qf.PREFIX, "--gpu", "none", str(plain), "genus"]).stdout == want
    # many blocks of rows for the parallel parser and formatter: the wide file four times over, read ids kept distinct
    raw = gzip.open(qf.tsv_path("wide", qf.WIDE_DIR), "rb").read().split(b"\n")
    header, rows = raw[0], [r for r in raw[1:] if r]
    big = tmp_path / "big.tsv"
    big.write_bytes(header + b"\n" + b"".join(b"c%d" % k + r + b"\n" for k in range(4) for r in rows))
    one = pc.run_promote(["--gpu", "none", "-t", "1", qf.WIDE_PREFIX, str(big), "species"])
    many = pc.run_promote(["--gpu", "none", "-t", "16", qf.WIDE_PREFIX, str(big), "species"])
    gold = pc.golden("wide.species.tsv.gz").split(b"\n")
    assert one.returncode == 0 and one.stdout == many.stdout
    assert one.stdout == gold[0] + b"\n" + b"".join(b"c%d" % k + r + b"\n" for k in range(4) for r in gold[1:] if r)


def test_wider_files_keep_their_further_columns(tmp_path):
    """the script writes the count into the LAST column; this tool rewrites column 8 and copies what follows"""
    rows = ["readID\tseqID\ttaxID\tscore\t2ndBestScore\thitLength\tqueryLength\tnumMatches\tbarcode\tUMI",
            "a\tNC_000001.1\t61\t9\t9\t99\t100\t2\tACGT\tTT", "a\tNC_000003.1\t62\t9\t9\t99\t100\t2\tACGT\tTT", "b\tx\t9999\t9\t0\t99\t100\t1\t\t",
            "short\tx\t61"]
    p = tmp_path / "bc.tsv"
    p.write_text("\n".join(rows))                          # (no newline at the end of the file)
    r = pc.run_promote(["--gpu", "none", qf.PREFIX, str(p), "species"])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().split("\n") == [rows[0], "a\tspecies\t60\t9\t9\t99\t100\t1\tACGT\tTT", rows[3], "short\tspecies\t60", ""]


def test_usage_and_errors(tmp_path):
    r = pc.run_promote([])
    assert r.returncode != 0 and r.stdout == b"" and r.stderr.startswith(b"Usage: centrifuger-promote")
    r = pc.run_promote(["-h"])
    assert r.returncode == 0 and b"column" in r.stdout and b"--gpu" in r.stdout
    r = pc.run_promote(["--gpu", "none", str(tmp_path / "absent"), qf.tsv_path("edge"), "genus"])
    assert r.returncode != 0 and r.stdout == b"" and b"absent" in r.stderr
    r = pc.run_promote(["--gpu", "none", qf.PREFIX, str(tmp_path / "absent.tsv"), "genus"])
    assert r.returncode != 0 and r.stdout == b""
    r = pc.run_promote(["--gpu", "x", qf.PREFIX, qf.tsv_path("edge"), "genus"])
    assert r.returncode != 0 and b"--gpu" in r.stderr


def _apply(prefix, level, res0, mat0, device=None):
    res, mat = res0.copy(), mat0.copy()
    p = capi.Promote(prefix, level, device=device)
    src = p.apply(res, mat, want_src=True)
    p.close()
    return res, mat, src


# hand-made reads over q8, as lists of original tax ids; 9999 and 8888 are in no tree
HAND = [
    [],                                    # unclassified
    [61],                                  # one match
    [61, 62],                              # two strains of one species
    [61, 62, 61],                          # A, B, A
    [61, 62, 70, 71, 60, 50],              # everything below one genus: collapses into one match at genus level
    [61, 90],                              # two genera
    [50], [60], [71], [1], [10], [20], [40],   # a level equal to the match's own rank; nodes above every level; the root
    [9999], [9999, 9999], [9999, 61], [61, 9999], [9999, 8888, 61, 62],
    [0], [0, 61], [61, 0, 62],             # tax id 0 (lca() hands the other argument through)
    [1, 61], [61, 1], [10, 61, 91],
    [61, 62, 70, 71, 90, 91, 60, 50, 80, 40] * 4,      # 40 matches
]


@pytest.mark.parametrize("level", pc.LEVELS)
def test_host_twin_equals_script_restatement(level):
    tree = pc.Tree("q8")
    assert len(tree.orig) == NC
    res0, mat0 = pc.make_arrays(tree, HAND, NC, gap=2)
    res, mat, src = _apply(qf.PREFIX, level, res0, mat0)
    pc.check_against_script(tree, HAND, level, res0, mat0, res, mat, src, NC)
    # slots no read keeps are not written: the gaps behind the reads, and an unclassified read as a whole
    used = np.zeros(len(mat), dtype=bool)
    for i in range(len(HAND)):
        b = int(res0["match_begin"][i])
        used[b:b + len(HAND[i])] = True
    assert np.array_equal(mat[~used], mat0[~used]) and np.all(src[~used] == np.uint64(0xffffffffffffffff))
    assert res[0] == res0[0]


def test_named_cases():
    tree = pc.Tree("q8")
    c = tree.compact
    reads = [[61, 62, 61], [61, 62, 70, 71, 60, 50], [61, 90], [9999, 61], [50], [61, 62]]
    res0, mat0 = pc.make_arrays(tree, reads, NC)

    def kept(level):
        res, mat, src = _apply(qf.PREFIX, level, res0, mat0)
        return [[(int(m["kind"]), int(m["id"]), int(m["taxid"])) for m in mat[int(b):int(b) + int(n)]] for b, n in zip(res["match_begin"], res["n_match"])], src
    sp, src = kept("species")
    assert sp[0] == [(1, c[60], 60)] and int(src[0]) == 0                                    # A, B, A with A and B in one species: one match
    st, src = kept("strain")
    assert st[0] == [(1, c[61], 61), (1, c[62], 62)] and src[:2].tolist() == [0, 1]          # A, B, A collapses to A, B
    assert st[1] == [(1, c[61], 61), (1, c[62], 62), (1, c[70], 70), (1, c[71], 71), (1, c[60], 60), (1, c[50], 50)]   # nothing above a strain is one
    ge, src = kept("genus")
    assert ge[1] == [(1, c[50], 50)] and ge[2] == [(1, c[50], 50), (1, c[80], 80)]           # all into one; two genera
    assert ge[3] == [(1, NC, 9999), (1, c[50], 50)] and src[int(res0["match_begin"][3]) + 1] == res0["match_begin"][3] + 1
    assert ge[4] == [(1, c[50], 50)]                                                         # its own rank
    nr, _ = kept("no rank")
    assert nr[5] == [(1, c[40], 40)]                                                         # first "no rank" above: 40, not the clade (20) or the root
    assert kept("bogus")[0][5] == [(1, c[61], 61), (1, c[62], 62)]
    lc, _ = kept("lca")
    assert [x[0][2] for x in lc] == [60, 50, 40, 1, 50, 60] and all(len(x) == 1 for x in lc)
    assert lc[3] == [(1, c[1], 1)] and lc[4] == [(1, c[50], 50)]
    p = capi.Promote(qf.PREFIX, "lca", device=None)
    assert p.lca_warnings(res0, mat0).tolist() == [9999]
    p.close()
    p = capi.Promote(qf.PREFIX, "genus", device=None)
    assert p.lca_warnings(res0, mat0).tolist() == []
    p.close()


def test_sequence_level_matches():
    """kind 0: the node is the sequence's; a sequence without a node counts as the root, which is what its TSV row says"""
    t = capi.Taxonomy(qf.PREFIX)
    tree = pc.Tree("q8")
    s61 = int(np.nonzero(t.orig_taxid[t.seq_to_tax] == 61)[0][0])
    res = np.zeros(3, dtype=capi.RESULT_DTYPE)
    mat = np.zeros(4, dtype=capi.MATCH_DTYPE)
    res["n_match"], res["match_begin"] = [1, 1, 2], [0, 1, 2]
    mat[0] = (s61, 61, 0, 0)
    mat[1] = (t.seq_cnt + 5, 1, 0, 0)                     # SeqIdToTaxId gives node_cnt, GetOrigTaxId the root's id
    mat[2], mat[3] = (s61, 61, 0, 0), (tree.compact[62], 62, 1, 0)
    r, m, _ = _apply(qf.PREFIX, "species", res, mat)
    assert m[0] == np.array((tree.compact[60], 60, 1, 0), dtype=capi.MATCH_DTYPE) and r["n_match"].tolist() == [1, 1, 1]
    assert m[1] == np.array((int(t.root), 1, 1, 0), dtype=capi.MATCH_DTYPE)
    assert m[2] == m[0]
    r, m, _ = _apply(qf.PREFIX, "lca", res, mat)
    assert m[0] == mat[0] and m[1] == mat[1] and m[2] == np.array((tree.compact[60], 60, 1, 0), dtype=capi.MATCH_DTYPE)
    t.close()


def test_random_lists_over_the_wide_taxonomy():
    tree = pc.Tree("qw")
    t = capi.Taxonomy(qf.WIDE_PREFIX)
    rng = np.random.default_rng(811)
    ids = np.array(tree.orig + [88888, 99999] * 45, dtype=np.uint64)       # a tenth of the draws are in no tree
    reads = [ids[rng.integers(0, len(ids), size=int(rng.integers(0, 7)))].tolist() for _ in range(600)] + [ids[rng.integers(0, len(ids), size=40)].tolist()]
    res0, mat0 = pc.make_arrays(tree, reads, int(t.node_cnt), seq_to_tax=t.seq_to_tax, rng=rng)
    assert set(mat0["kind"][:-1].tolist()) >= {0, 1}
    for level in ("genus", "species", "strain", "lca", "no rank"):
        res, mat, src = _apply(qf.WIDE_PREFIX, level, res0, mat0)
        pc.check_against_script(tree, reads, level, res0, mat0, res, mat, src, int(t.node_cnt))
    t.close()


def test_argument_errors():
    L = capi.lib()
    h = C.c_void_p()
    assert L.cfr_promote_open(None, b"genus", -1, C.byref(h)) == capi.CFR_ERR_ARG
    assert L.cfr_promote_open(qf.PREFIX.encode(), None, -1, C.byref(h)) == capi.CFR_ERR_ARG
    assert L.cfr_promote_open(qf.PREFIX.encode(), b"genus", -1, None) == capi.CFR_ERR_ARG
    assert L.cfr_promote_open(qf.PREFIX.encode(), b"genus", -2, C.byref(h)) == capi.CFR_ERR_ARG
    assert L.cfr_promote_open((qf.PREFIX + "_absent").encode(), b"genus", -1, C.byref(h)) == capi.CFR_ERR_IO and not h
    assert L.cfr_promote_open(qf.PREFIX.encode(), b"genus", -1, C.byref(h)) == capi.CFR_OK and h
    res = np.zeros(1, dtype=capi.RESULT_DTYPE)
    res["n_match"] = 1
    assert L.cfr_promote_apply(h, None, None, C.c_size_t(1), None) == capi.CFR_ERR_ARG
    assert L.cfr_promote_apply(h, capi._p(res), None, C.c_size_t(1), None) == capi.CFR_ERR_ARG      # a classified read and no matches
    assert L.cfr_promote_apply(h, None, None, C.c_size_t(0), None) == capi.CFR_OK
    assert L.cfr_promote_lca_warnings(h, None, None, C.c_size_t(0), None, C.c_size_t(0), None) == capi.CFR_ERR_ARG
    assert L.cfr_promote_get_stats(h, None) == capi.CFR_ERR_ARG
    assert L.cfr_promote_close(h) == capi.CFR_OK
    # a handle that is not open: closed, null, or never one
    assert L.cfr_promote_close(h) == capi.CFR_ERR_ARG
    assert L.cfr_promote_apply(h, None, None, C.c_size_t(0), None) == capi.CFR_ERR_ARG
    assert L.cfr_promote_apply(None, None, None, C.c_size_t(0), None) == capi.CFR_ERR_ARG
    assert L.cfr_promote_close(None) == capi.CFR_ERR_ARG
    assert b"cfr_promote" in L.cfr_last_error()
    assert L.cfr_device_index_set_promote(None, b"genus") == capi.CFR_ERR_ARG
