"""bin/centrifuger-inspect against the reference centrifuger-inspect's own output (tests/golden/inspect, make_golden_promote.py) for
the q8 and qw indexes, its usage and exit codes, and the taxonomy tables through the C-ABI (cfr_taxonomy_*).  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import promote_cases as pc
import quant_fixtures as qf
from centrifuger_amd import capi

MODES = pc.MANIFEST["inspect_modes"]


def run_inspect(args):
    return subprocess.run([pc.INSPECT] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


@pytest.mark.parametrize("idx", ["q8", "qw"])
@pytest.mark.parametrize("mode", ["summary", "conversion-table", "taxonomy-tree", "name-table", "size-table"])
def test_every_mode_equals_reference(idx, mode):
    """qw has no .1.cfr: the FM index is never opened"""
    assert mode in MODES
    if idx == "qw":
        assert not os.path.exists(pc.PREFIXES[idx] + ".1.cfr")
    r = run_inspect(["-x", pc.PREFIXES[idx], "--" + mode])
    assert r.returncode == 0, r.stderr.decode()
    want = open(os.path.join(pc.IDIR, f"{idx}.{mode}.txt"), "rb").read()
    assert len(want) > 0 and r.stdout == want
    assert r.stderr == b""


def test_last_item_counts_and_option_order():
    r = run_inspect(["--summary", "--name-table", "-x", qf.PREFIX])
    assert r.returncode == 0 and r.stdout == open(os.path.join(pc.IDIR, "q8.name-table.txt"), "rb").read()


def test_usage_and_exit_codes():
    r = run_inspect(["-h"])
    assert r.returncode == 0 and r.stdout.startswith(b"./centrifuger-inspect [OPTIONS]:\n") and r.stderr == b""
    for opt in (b"--summary", b"--conversion-table", b"--taxonomy-tree", b"--name-table", b"--size-table", b"-x STRING"):
        assert opt in r.stdout
    assert b"Not supported: --index-size" in r.stdout
    usage = r.stdout
    r = run_inspect(["-x", qf.PREFIX])                      # no item
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"Use inspect options from " + usage
    r = run_inspect(["--summary"])                          # no -x
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"Need -x to specify index.\n" + usage
    r = run_inspect(["-x", qf.PREFIX, "--seq-name"])        # prints nothing, as the reference does
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    r = run_inspect(["-x", qf.PREFIX, "--no-such-option"])
    assert r.returncode != 0 and r.stdout == b"" and usage in r.stderr


def test_index_size_is_refused():
    r = run_inspect(["-x", qf.PREFIX, "--index-size"])
    assert r.returncode != 0 and r.stdout == b""
    assert b"--index-size is not supported" in r.stderr


def test_missing_and_malformed_index(tmp_path):
    r = run_inspect(["-x", str(tmp_path / "nothing"), "--summary"])
    assert r.returncode not in (0, -11, 139) and r.stdout == b"" and b"nothing" in r.stderr
    # .2.cfr without .3.cfr
    shutil.copy(qf.PREFIX + ".2.cfr", tmp_path / "half.2.cfr")
    r = run_inspect(["-x", str(tmp_path / "half"), "--taxonomy-tree"])
    assert r.returncode not in (0, -11, 139) and r.stdout == b"" and b"half.3.cfr" in r.stderr
    # a .2.cfr cut in the middle of its tables
    raw = open(qf.PREFIX + ".2.cfr", "rb").read()
    (tmp_path / "cut.2.cfr").write_bytes(raw[:len(raw) // 2])
    shutil.copy(qf.PREFIX + ".3.cfr", tmp_path / "cut.3.cfr")
    r = run_inspect(["-x", str(tmp_path / "cut"), "--name-table"])
    assert r.returncode not in (0, -11, 139) and r.stdout == b"" and len(r.stderr) > 0


def test_taxonomy_tables_through_the_c_abi():
    t = capi.Taxonomy(qf.PREFIX, with_lengths=True)
    assert t.node_cnt == 14 and t.orig_taxid.tolist() == qf.orig_taxids() and t.orig_taxid[t.root] == 1
    tree = pc.Tree("q8")
    assert [capi.tax_rank_string(int(r)) for r in t.rank] == [tree.level[o] for o in tree.orig]
    assert [int(t.orig_taxid[p]) for p in t.parent] == [tree.parent[o] for o in tree.orig]
    names = [l.split("\t")[0] for l in open(os.path.join(pc.IDIR, "q8.conversion-table.txt"))]
    assert t.seq_names == names and len(t.seq_to_tax) == t.seq_cnt
    # genome lengths: the ones the quantifier works with (shared code)
    q = capi.Quant(qf.PREFIX, device=None)
    q.add_tsv(qf.tsv_path("edge"))
    q.run()
    assert np.array_equal(np.asarray(q.values()["taxid_length"]), t.taxid_length)
    q.close()
    assert t.tax_name(int(t.root)) == "root" and t.tax_name(10 ** 6) == "Unknown"
    assert sorted(t.length_seq_id.tolist()) == t.length_seq_id.tolist() and len(t.length_value) == len(t.length_seq_id) > 0
    bare = capi.Taxonomy(qf.WIDE_PREFIX)
    assert bare.node_cnt == 811 and bare.taxid_length is None
    with pytest.raises(capi.CfrError) as e:
        capi.Taxonomy(qf.PREFIX + "_absent")
    assert e.value.status == capi.CFR_ERR_IO
    t.close(); bare.close()
