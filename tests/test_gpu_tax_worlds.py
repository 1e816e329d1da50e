"""The nine taxonomy worlds of tests/tax_worlds.py on the device: one text, nine taxonomies - forests, a root other than tax id 1,
sequences on the roots, a 300-node chain, irregular ranks, an id outside the tree, 64-bit tax ids.  The FM index is written once per
module by the native writer; every other world links its .1/.3/.4.cfr and gets a .2.cfr of its own (indexbuild.write_taxonomy, which
tests/test_tax_worlds_oracle_cpu.py holds to the reference builder's bytes).

  * every world at -k 1, 2, 5 (CFR_TEST_K: that one), single-end and paired, through classify, submit / wait, classify_resident,
    classify_resident_compact and classify_expanded: results, matches and expanded lists equal the C oracle's, field by field;
  * bin/centrifuger prints the reference classifier's committed TSV (tests/golden/taxworlds);
  * every form of the LCA fold takes reads whose ids lie in two trees, shown by the library's own CFR_POST_STATS line in child
    processes (the switches are read once per process): tail_emit_small, the register form of k_post_fast, the team form of
    k_tail_heavy in both tiers, and d_tax_lca through the pool (CFR_TEAM_TAIL=0) and through --expand-taxid;
  * promote, kreport, quant and the TSV formatter on the device against their host twins on the forest worlds.
Integer work: everything is bit-exact.  -m gpu."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT          # (first: it puts the repository on sys.path, which the child process needs too)

import oracle_lib as ora
import promote_cases as pc
import tax_worlds as tw
from centrifuger_amd import capi, indexbuild

pytestmark = pytest.mark.gpu

KS = (int(os.environ["CFR_TEST_K"]),) if os.environ.get("CFR_TEST_K") else (1, 2, 5)
ENDS = ("se", "pe")
TDIR = os.path.join(GOLDEN, "taxworlds")
CONSUMER_WORLDS = ("orphan_subtree", "no_tax_id_1", "seq_on_roots", "deep_chain")
CENTRIFUGER = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
# the child processes: the switches, and which cassette sizes their reads come from
FOLD_SITES = {
    "tail_emit_small": ({}, (2, 3, 8)),
    "post_fast_registers": ({"CFR_POST_FAST": "1", "CFR_POST_FAST_LAST": "1"}, (2, 3, 8)),
    "small_teams": ({}, (9, 16, 17, 40, 64)),
    "large_teams": ({"CFR_HEAVY_DIRECT_ROWS": "12"}, (16, 17, 40, 64)),
    "single_lane_pool": ({"CFR_TEAM_TAIL": "0"}, (9, 16, 17, 40, 64)),
    # four sequences with the cassette three times each: twelve rows, four ids - on seq_on_roots all four sit on the two roots, so a
    # team folds a list of tops only
    "small_teams_tops_only": ({}, (4,)),
    "large_teams_tops_only": ({"CFR_HEAVY_DIRECT_ROWS": "8"}, (4,)),
}
FOLD_WORLDS = ("orphan_subtree", "seq_on_roots")


def _reads(w, ends):
    if ends == "se":
        return w.reads.bases, w.reads.offsets, None, None
    (r1, r2) = w.pairs
    return r1.bases, r1.offsets, r2.bases, r2.offsets


class _Setup:
    def __init__(self, root):
        self.root, self.prefix, self.devs, self.wants, self.kids = str(root), {}, {}, {}, {}
        w = tw.make("regular")
        g = w.genomes
        first = os.path.join(self.root, "regular")
        rep = capi.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, first, **tw.build_kwargs(w))
        assert rep["n"] == g.total_len
        for name in tw.NAMES:
            self.prefix[name] = os.path.join(self.root, name)
            if name == "regular":
                continue
            g = tw.make(name).genomes
            for ext in ("1", "3", "4"):
                os.symlink(f"{first}.{ext}.cfr", f"{self.prefix[name]}.{ext}.cfr")
            indexbuild.write_taxonomy(self.prefix[name] + ".2.cfr", g.names, g.taxids, g.nodes, g.tax_names)
        for ends in ENDS:
            b1, o1, b2, o2 = _reads(w, ends)
            np.savez(os.path.join(self.root, f"reads_{ends}.npz"), b1=b1, o1=o1, **({} if b2 is None else {"b2": b2, "o2": o2}))

    def dev(self, name, k, expand=False):
        if (name, k, expand) not in self.devs:
            idx = capi.Index(self.prefix[name], capi.default_params(max_result=k, **({"output_expanded": 1} if expand else {})))
            self.devs[(name, k, expand)] = (idx, capi.DeviceIndex(idx))
        return self.devs[(name, k, expand)]

    def want(self, name, k, ends, expand=False):
        """the oracle's results for the world's reads: a list of (score, secondary, hit length, query length, matches, expanded lists)"""
        key = (name, k, ends, expand)
        if key not in self.wants:
            o = ora.OracleIndex(self.prefix[name], max_result=k, expand=expand)
            b1, o1, b2, o2 = _reads(tw.make(name), ends)
            res = o.classify(b1, o1, b2, o2, threads=8)
            self.wants[key] = [(int(r.score), int(r.secondaryScore), int(r.hitLength), int(r.queryLength),
                                [(int(r.kind[q]), int(r.id[q]), int(r.taxid[q])) for q in range(r.nmatch)],
                                [r.expanded_ids(q) for q in range(r.nmatch)] if expand else None) for r in (res[i] for i in range(len(o1) - 1))]
            o.close()
        return self.wants[key]

    def plain(self, name, k, ends):
        """(results, matches) of the device for the world's reads, compared with the oracle once"""
        key = ("plain", name, k, ends)
        if key not in self.wants:
            _, dev = self.dev(name, k)
            res, mat = dev.classify(*_reads(tw.make(name), ends))
            _assert_same(res, mat, self.want(name, k, ends), f"{name} -k {k} {ends}")
            self.wants[key] = (res, mat)
        return self.wants[key]

    def child(self, site):
        """{(world, ends): (rows as (score, matches) lists, the CFR_POST_STATS numbers)} of a fresh process under the site's switches"""
        if site not in self.kids:
            switches, sizes = FOLD_SITES[site]
            env = dict(os.environ, CFR_DEBUG_ENV="1", CFR_POST_STATS="1")
            for key in ("CFR_POST_FAST", "CFR_POST_FAST_LAST", "CFR_HEAVY_DIRECT_ROWS", "CFR_TEAM_TAIL", "CFR_SUBBATCH"):
                env.pop(key, None)
            env.update(switches)
            out = os.path.join(self.root, f"out_{site}.json")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), self.root, out, ",".join(str(s) for s in sizes)], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=300)
            assert r.returncode == 0, f"{site}: exit {r.returncode}\n{r.stderr.decode()[-2000:]}"
            with open(out) as f:
                rows = json.load(f)
            self.kids[site] = (rows, _parse_stats(r.stderr.decode()))
        return self.kids[site]

    def close(self):
        for idx, dev in self.devs.values():
            dev.close()
        self.devs.clear()


def _parse_stats(err):
    """{"world ends": (reads, left to k_adjust_tail, folded by small teams, by large teams)} from the [cfr] post stage lines"""
    out, case = {}, None
    for line in err.splitlines():
        m = re.match(r"\[case (\w+ \w+)\]", line)
        if m:
            case = m.group(1)
            continue
        m = re.match(r"\[cfr\] post stage of (\d+) reads: (\d+) left to k_adjust_tail, (\d+) folded by small teams, (\d+) by large teams", line)
        if m and case:
            old = out.get(case, (0, 0, 0, 0))
            out[case] = tuple(a + int(b) for a, b in zip(old, m.groups()))
    return out


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    s = _Setup(tmp_path_factory.mktemp("tax_worlds"))
    yield s
    s.close()


def _assert_same(res, mat, want, what, spans=None, xids=None):
    assert len(res) == len(want), what
    for i, (score, second, hitlen, qlen, matches, expanded) in enumerate(want):
        r = res[i]
        got = (int(r["score"]), int(r["secondary_score"]), int(r["hit_length"]), int(r["query_length"]), int(r["n_match"]))
        assert got == (score, second, hitlen, qlen, len(matches)), f"{what}: read {i}: got {got}, oracle {(score, second, hitlen, qlen, len(matches))}"
        b = int(r["match_begin"])
        mine = [(int(m["kind"]), int(m["id"]), int(m["taxid"])) for m in mat[b:b + len(matches)]]
        assert mine == matches, f"{what}: read {i}: got {mine}, oracle {matches}"
        if spans is not None:
            lists = [[int(x) for x in xids[int(s["begin"]):int(s["begin"]) + int(s["count"])]] for s in spans[b:b + len(matches)]]
            assert lists == expanded, f"{what}: read {i}: expanded {lists}, oracle {expanded}"


def _up(a):
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8)
    t = torch.zeros(len(raw) + 64, dtype=torch.uint8, device="cuda")
    t[:len(raw)] = torch.from_numpy(raw.copy())
    return t, t.data_ptr()


# ------------------------------------------------------------------------------------------------ classification
@pytest.mark.parametrize("name", tw.NAMES)
def test_worlds_hold_what_they_claim(name, setup):
    o = ora.OracleIndex(setup.prefix[name], max_result=1)
    print(name, tw.guards(tw.make(name), o))
    o.close()


@pytest.mark.parametrize("ends", ENDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", tw.NAMES)
def test_entries_equal_oracle(name, k, ends, setup):
    import torch
    w = tw.make(name)
    b1, o1, b2, o2 = _reads(w, ends)
    n = len(o1) - 1
    want = setup.want(name, k, ends)
    what = f"{name} -k {k} {ends}"
    _, dev = setup.dev(name, k)
    setup.plain(name, k, ends)                                                        # classify
    _assert_same(*dev.wait(dev.submit(b1, o1, b2, o2)), want, what + " submit/wait")
    keep = [_up(o1.astype(np.int64)), _up(b1)] + ([] if b2 is None else [_up(o2.astype(np.int64)), _up(b2)])
    p = [x[1] for x in keep] + [0, 0]
    torch.cuda.synchronize()
    t2 = 0 if b2 is None else int(o2[-1])
    _assert_same(*dev.classify_resident(p[1], p[0], n, int(o1[-1]), p[3], p[2], t2), want, what + " resident")
    cres, cmat = dev.classify_resident_compact(p[1], p[0], n, int(o1[-1]), p[3], p[2], t2)
    _assert_same(*capi.expand_compact(cres, cmat, k, wide=dev.compact_wide()), want, what + " compact")
    del keep
    _, xdev = setup.dev(name, k, expand=True)                                         # (--expand-taxid is a parameter of the index handle)
    res, mat, spans, xids = xdev.classify_expanded(b1, o1, b2, o2)
    _assert_same(res, mat, setup.want(name, k, ends, expand=True), what + " expanded", spans, xids)


@pytest.mark.parametrize("ends,k", [("se", 1), ("se", 5), ("pe", 1), ("pe", 5)])
@pytest.mark.parametrize("name", tw.COMMITTED + ("seq_on_roots",))
def test_command_line_prints_the_reference_tsv(name, ends, k, setup, tmp_path):
    w = tw.make(name)
    tw.write_reads(w, str(tmp_path))
    files = ["-u", str(tmp_path / "se.fq")] if ends == "se" else ["-1", str(tmp_path / "p_1.fq"), "-2", str(tmp_path / "p_2.fq")]
    r = subprocess.run([CENTRIFUGER, "-x", setup.prefix[name], "-t", "2", "-k", str(k)] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    want = gzip.open(os.path.join(TDIR, f"{name}.{ends}_k{k}.tsv.gz"), "rb").read()
    if r.stdout != want:
        diff = [(x, y) for x, y in zip(r.stdout.split(b"\n"), want.split(b"\n")) if x != y]
        assert False, f"{len(diff)} rows differ (own, reference), first: {diff[:3]}"


# ------------------------------------------------------------------------------------------------ every fold is reached
def _fold_reads(name, ends, sizes):
    """the numbers of the reads whose cassette has one of `sizes` and ids in two trees"""
    w = tw.make(name)
    kinds = tw.subset_kinds(w)
    of = w.info["read_cassette"] if ends == "se" else w.info["pair_cassette"]
    cs = w.info["cassettes"]
    return [i for i, j in enumerate(of) if j >= 0 and cs[j].size in sizes and kinds[j][0]]


@pytest.mark.parametrize("ends", ENDS)
@pytest.mark.parametrize("name", FOLD_WORLDS)
@pytest.mark.parametrize("site", sorted(FOLD_SITES))
def test_every_fold_takes_reads_across_two_trees(site, name, ends, setup):
    """-k 1, only reads whose ids lie in two trees, one process per form of the fold: the answers are the oracle's, and the library's
    own count of where the reads went says which form folded them.  The team forms are counted directly.  The three single-lane forms
    have no counter of their own and are shown by exclusion: no read listed for the teams, none left to k_adjust_tail, and the
    process's switches decide which single-lane code the reads of that size take (registers in k_adjust_tail, registers in k_post_fast,
    pool scratch and d_tax_lca with the teams off).  d_tax_lca behind --expand-taxid has a positive check of its own below."""
    rows, stats = setup.child(site)
    sizes = FOLD_SITES[site][1]
    picked = _fold_reads(name, ends, sizes)
    assert len(picked) >= (1 if site.endswith("tops_only") else 4), (site, name, ends, len(picked))
    want = setup.want(name, 1, ends)
    if site.endswith("tops_only") and name == "seq_on_roots":           # [500, 1, 1, 500]: the first top that is not the root
        assert all(len(want[i][4]) == 1 and want[i][4][0][0] == 1 and want[i][4][0][2] == 500 for i in picked), [want[i][4] for i in picked]
    got = rows[f"{name} {ends}"]
    assert len(got) == len(picked)
    for i, g in zip(picked, got):
        assert (g[0], [tuple(m) for m in g[1]]) == (want[i][0], want[i][4]), f"{site} {name} {ends}: read {i}: got {g}, oracle {want[i]}"
    st = stats.get(f"{name} {ends}")
    print(site, name, ends, len(picked), "reads; post stage:", st)
    assert st is not None and st[0] == len(picked), st
    _, slow, small, large = st
    if site in ("tail_emit_small", "single_lane_pool"):
        assert (slow, small, large) == (0, 0, 0), st                 # nothing left for a second kernel, nothing listed for the teams
    elif site == "post_fast_registers":
        assert (slow, small, large) == (0, 0, 0), st                 # k_post_fast listed no read for k_adjust_tail: it folded them itself
    elif site == "small_teams_tops_only" or (site == "small_teams" and ends == "se"):
        assert small == len(picked) and large == 0, st
    elif site == "small_teams":                                         # (a pair of 2 x 40 rows starts with the large teams: more than 64 rows)
        assert small > 0 and small + large >= len(picked), st
    else:
        assert large > 0, st


@pytest.mark.parametrize("ends", ENDS)
@pytest.mark.parametrize("name", FOLD_WORLDS)
def test_expand_taxid_sends_cross_tree_reads_of_every_size_through_d_tax_lca(name, ends, setup):
    """--expand-taxid at -k 1.  A list of promoted children is written by d_tax_expand alone, behind d_tax_reduce -> d_tax_lca in the
    general form; the register and team forms write none and hand such reads on.  So for every subset size a cross-tree read whose
    answer is the root must come back with the root's children of at least two trees, as the oracle lists them: that list is the
    positive sign that d_tax_lca folded the read."""
    w = tw.make(name)
    _, xdev = setup.dev(name, 1, expand=True)
    res, mat, spans, xids = xdev.classify_expanded(*_reads(w, ends))
    want = setup.want(name, 1, ends, expand=True)
    _assert_same(res, mat, want, f"{name} -k 1 {ends} expanded", spans, xids)
    for size in tw.SIZES:
        at_root = [i for i in _fold_reads(name, ends, (size,)) if want[i][4] == [(1, want[i][4][0][1], w.info["root_taxid"])]]
        # (seq_on_roots, two ids: {second root, id below it} lies in one tree, and [id, second root] gives the id - none at the root)
        assert at_root or (name, size) == ("seq_on_roots", 2), (name, ends, size)
        for i in at_root:
            s = spans[int(res["match_begin"][i])]
            assert int(s["count"]) >= 2 and int(res["n_match"][i]) == 1, (name, ends, size, i, s)


# ------------------------------------------------------------------------------------------------ the other consumers
def _by_read(res, mat):
    return [(tuple(int(res[f][i]) for f in ("score", "secondary_score", "hit_length", "query_length", "n_match")),
             [tuple(int(x) for x in (m["kind"], m["id"], m["taxid"])) for m in mat[int(res["match_begin"][i]):int(res["match_begin"][i]) + max(0, int(res["n_match"][i]))]])
            for i in range(len(res))]


@pytest.mark.parametrize("level", pc.LEVELS)
@pytest.mark.parametrize("name", CONSUMER_WORLDS)
def test_promote_on_the_device_equals_host_twin(name, level, setup):
    k = KS[-1]
    res0, mat0 = setup.plain(name, k, "se")
    out = {}
    for device in (None, 0):
        res, mat = res0.copy(), mat0.copy()
        p = capi.Promote(setup.prefix[name], level, device=device)
        p.apply(res, mat)
        p.close()
        out[device] = _by_read(res, mat)
    assert out[0] == out[None], f"{name} {level}: capi.Promote"
    _, dev = setup.dev(name, k)
    dev.set_promote(level)
    try:
        res, mat = dev.classify(*_reads(tw.make(name), "se"))
    finally:
        dev.set_promote(None)
    assert _by_read(res, mat) == out[None], f"{name} {level}: set_promote"


@pytest.mark.parametrize("name", CONSUMER_WORLDS)
def test_kreport_on_the_device_equals_host_twin(name, setup):
    k = KS[-1]
    res, mat = setup.plain(name, k, "se")
    _, dev = setup.dev(name, k)
    if name == "no_tax_id_1":                                           # the report hangs on tax id 1 (cfr_kreport_core.hpp): refused everywhere
        for device in (None, 0):
            with pytest.raises(capi.CfrError):
                capi.Kreport(setup.prefix[name], device=device)
        with pytest.raises(capi.CfrError):
            dev.set_kreport(True)
        return
    out = {}
    for device in (None, 0):
        kr = capi.Kreport(setup.prefix[name], device=device, score_data=True)
        kr.add_results(res.copy(), mat.copy())
        own, clade, sc, csc, seq = kr.counts()
        out[device] = (own.tolist(), clade.tolist(), sc.tolist(), csc.tolist(), seq, kr.warnings().tolist())
        bins = kr.bins
        kr.close()
    assert out[0] == out[None] and out[None][4] == len(res)
    dev.set_kreport(True, score_data=True)
    try:
        dev.classify(*_reads(tw.make(name), "se"))
        own, sc, seq = dev.kreport_counts(bins)
    finally:
        dev.set_kreport(False)
    assert (own.tolist(), sc.tolist(), seq) == (out[None][0], out[None][2], out[None][4])


@pytest.mark.parametrize("name", CONSUMER_WORLDS)
def test_quant_on_the_device_equals_host_twin(name, setup):
    k = KS[-1]
    res, mat = setup.plain(name, k, "se")
    out = {}
    for device in (None, 0):
        q = capi.Quant(setup.prefix[name], device=device)
        q.add_results(res, mat)
        rounds = q.run()
        v = q.values()
        out[device] = (rounds, {key: val.view(np.uint64).tolist() for key, val in v.items() if key != "node_cnt"})
        q.close()
    assert out[0] == out[None], name


@pytest.mark.parametrize("name", CONSUMER_WORLDS)
def test_tsv_formatter_on_the_device_prints_phantom_nodes_as_the_reference(name, setup):
    """-k 1 (where a cross-tree read's one row is the root) and the largest -k of the run.  On orphan_subtree the root is the phantom
    tax id 0: its rows carry the rank string of code 0 and tax id 0, the host formatter's text holds such rows, the device's text is
    that text, and with the dust pre-step on (the reference's default) it is the reference classifier's committed stdout."""
    w = tw.make(name)
    for k in sorted({1, KS[-1]}):
        res, mat = setup.plain(name, k, "se")
        idx, dev = setup.dev(name, k)
        ids = [f"r{i}" for i in range(len(res))]
        want = b"".join(idx.format_tsv(ids[i], res[i], mat) for i in range(len(res)))
        phantom = sum(1 for line in want.split(b"\n") if line.split(b"\t")[1:3] == [b"no rank", b"0"])
        if name == "orphan_subtree" and k == 1:                        # (at -k 1 every cross-tree read's row is the root; a larger -k lists
            assert phantom >= 50, phantom                              #  sequences or ranked nodes, and no row need be the root)
        for device in (None, 0):
            t = capi.Tsv(idx, device=device)
            text, _ = t.format(res, mat, ids)
            t.close()
            assert text == want, (name, k, device)
        if name in tw.COMMITTED and k == 1:
            dev.set_dust(True)
            try:
                dres, dmat = dev.classify(*_reads(w, "se"))
            finally:
                dev.set_dust(False)
            t = capi.Tsv(idx, device=0)
            text, _ = t.format(dres, dmat, ids)
            t.close()
            assert capi.tsv_header() + text == gzip.open(os.path.join(TDIR, f"{name}.se_k1.tsv.gz"), "rb").read(), name


# ------------------------------------------------------------------------------------------------ the child process
def _child(root, out, sizes):
    sizes = tuple(int(s) for s in sizes.split(","))
    rows = {}
    for name in FOLD_WORLDS:
        idx = capi.Index(os.path.join(root, name), capi.default_params(max_result=1))
        dev = capi.DeviceIndex(idx)
        for ends in ENDS:
            z = np.load(os.path.join(root, f"reads_{ends}.npz"))
            picked = _fold_reads(name, ends, sizes)

            def take(b, o):
                parts = [b[int(o[i]):int(o[i + 1])] for i in picked]
                offs = np.zeros(len(parts) + 1, dtype=np.uint64)
                offs[1:] = np.cumsum([len(x) for x in parts])
                return np.concatenate(parts), offs
            b1, o1 = take(z["b1"], z["o1"])
            b2, o2 = take(z["b2"], z["o2"]) if "b2" in z else (None, None)
            sys.stderr.write(f"[case {name} {ends}]\n")
            sys.stderr.flush()
            res, mat = dev.classify(b1, o1, b2, o2)
            rows[f"{name} {ends}"] = [(int(res["score"][i]), [(int(m["kind"]), int(m["id"]), int(m["taxid"]))
                                                                for m in mat[int(res["match_begin"][i]):int(res["match_begin"][i]) + int(res["n_match"][i])]])
                                      for i in range(len(res))]
        dev.close()
    with open(out, "w") as f:
        json.dump(rows, f)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3])
