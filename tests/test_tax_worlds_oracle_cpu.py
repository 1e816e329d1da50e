"""The nine taxonomy worlds of tests/tax_worlds.py on the CPU: forests, a root other than tax id 1, sequences on the roots, a 300-node
chain, irregular ranks, an id outside the tree, 64-bit tax ids.  Every index is written by the Python writer (no GPU), which must give
the reference builder's files for the forest worlds (tests/golden/taxworlds).  Then, with the reference as the only authority:
  * each world provokes what it claims (tax_worlds.guards, from the C oracle alone);
  * Taxonomy::LCA on every ordered pair and triple of nodes: the oracle, the host tail's restatement and the fold the kernels use
    (csrc/cfr_tax_fold.hpp, through cfr_taxonomy_lca_probe) give one answer, and the fold's loop count stays within the depths of
    its ids - the proof that the device climb ends on a forest, which needs no GPU;
  * the oracle's TSV for the worlds' reads equals the reference classifier's committed stdout at -k 1, 2, 5, with and without
    --expand-taxid."""
import gzip
import itertools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as ora
import tax_worlds as tw
from centrifuger_amd import capi, indexbuild, synth
from cfr_fields import parse_1cfr
from conftest import GOLDEN, REF_DIR, have_ref

TDIR = os.path.join(GOLDEN, "taxworlds")
MANIFEST = json.load(open(os.path.join(TDIR, "manifest.json")))


@pytest.fixture(scope="module", params=tw.NAMES)
def built(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp(request.param))
    w = tw.make(request.param)
    g = w.genomes
    prefix = os.path.join(d, "own")
    indexbuild.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, prefix, device=torch.device("cpu"), **tw.build_kwargs(w))
    return w, d, prefix


def _same_index(own, ref1, ref2):
    mine, want = parse_1cfr(own + ".1.cfr"), parse_1cfr(ref1)
    assert len(mine) == len(want)
    for (na, va), (nb, vb) in zip(mine, want):
        assert na == nb and va == vb, f"field {na} differs"
    assert open(own + ".2.cfr", "rb").read() == open(ref2, "rb").read(), ".2.cfr differs"


def test_python_writer_equals_committed_reference_files(built):
    """the phantom nodes of ReadTaxonomyTree (Taxonomy.hpp:190-197): orphan_subtree has 30 nodes and the phantom id 0 as its root"""
    w, _, prefix = built
    name = w.info["name"]
    t = capi.Taxonomy(prefix)
    assert int(t.orig_taxid[t.root]) == w.info["root_taxid"]
    if name in tw.COMMITTED:
        _same_index(prefix, os.path.join(TDIR, "text.1.cfr"), os.path.join(TDIR, name + ".2.cfr"))
        assert (int(t.node_cnt), int(t.root)) == (MANIFEST["indexes"][name]["node_cnt"], MANIFEST["indexes"][name]["root"])
    if name == "orphan_subtree":
        orig = t.orig_taxid.tolist()
        assert orig[:2] == [0, 1] and 999 in orig and int(t.node_cnt) == 30
        for phantom in (0, 999):                                          # empty name, rank code 0, as the reference prints them
            c = orig.index(phantom)
            assert t.tax_name(c) == "" and int(t.rank[c]) == 0 and capi.tax_rank_string(int(t.rank[c])) == "no rank"
        assert int(t.parent[orig.index(999)]) == 0 and int(t.parent[orig.index(1)]) == orig.index(1)
    t.close()


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (compiled reference) not present")
def test_python_writer_equals_live_reference_build(built):
    w, d, prefix = built
    synth.write_reference_inputs(w.genomes, d)
    ref = os.path.join(d, "ref")
    subprocess.run([os.path.join(REF_DIR, "centrifuger-build"), "-t", "2", "-r", os.path.join(d, "ref.fa"), "--taxonomy-tree", os.path.join(d, "nodes.dmp"),
                    "--name-table", os.path.join(d, "names.dmp"), "--conversion-table", os.path.join(d, "seqid.map"), "-o", ref,
                    "--ftabchars", str(w.info["ftab_chars"])], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    _same_index(prefix, ref + ".1.cfr", ref + ".2.cfr")


def test_world_provokes_what_it_claims(built):
    w, _, prefix = built
    o = ora.OracleIndex(prefix, max_result=1)
    reached = tw.guards(w, o)
    print(w.info["name"], reached)
    o.close()


def _depths(parent):
    out = []
    for x in range(len(parent)):
        d = 0
        while int(parent[x]) != x:
            x = int(parent[x]); d += 1
        out.append(d)
    return out


def _nodes_for_tuples(w, t):
    """every node of the world; of deep_chain (305 nodes) the two ends of the chain, the tops, the nodes that carry sequences and 20
    seeded others"""
    nc = int(t.node_cnt)
    if w.info["name"] != "deep_chain":
        return list(range(nc))
    depth = _depths(t.parent)
    deepest = int(np.argmax(depth))
    keep = {x for x in range(nc) if int(t.parent[x]) == x} | {deepest, int(t.parent[deepest]), depth.index(3)}
    keep |= {int(x) for x in t.seq_to_tax.tolist()}
    rest = [x for x in range(nc) if x not in keep]
    keep |= {int(x) for x in np.random.default_rng(11).choice(rest, size=20, replace=False)}
    return sorted(keep)


def test_lca_of_every_pair_and_triple(built):
    w, _, prefix = built
    t = capi.Taxonomy(prefix)
    o = ora.OracleIndex(prefix, max_result=1)
    nodes = _nodes_for_tuples(w, t)
    assert len(nodes) == int(t.node_cnt) or w.info["name"] == "deep_chain"
    depth = _depths(t.parent)
    lists = [list(p) for r in (1, 2, 3) for p in itertools.product(nodes, repeat=r)]
    want = np.array(o.tax_lca(lists), dtype=np.uint64)
    twin, _ = t.lca(lists)
    fold, steps = t.lca(lists, fold=True)
    bad = np.flatnonzero(twin != want)
    assert len(bad) == 0, (w.info["name"], "host twin", [(lists[i], int(twin[i]), int(want[i])) for i in bad[:5]])
    bad = np.flatnonzero(fold != want)
    assert len(bad) == 0, (w.info["name"], "shared fold", [(lists[i], int(fold[i]), int(want[i])) for i in bad[:5]])
    for ids, st in zip(lists, steps.tolist()):
        bound = sum(depth[x] for x in ids) + 2                # (a pair: depth(a) + depth(b) + 2; a join never takes more than the deeper side)
        assert st <= bound, (w.info["name"], ids, st, bound)
    if w.info["name"] in tw.FOREST:
        root = int(t.root)
        tops = [x for x in nodes if int(t.parent[x]) == x and x != root]
        plain = [x for x in nodes if int(t.parent[x]) != x]
        assert tops and plain
        at = {tuple(l): int(v) for l, v in zip(lists, want.tolist())}
        for r2 in tops:                                       # Taxonomy.hpp:746-762: the order decides
            for a in plain:
                assert at[(r2, a)] == root and at[(a, r2)] == a and at[(r2,)] == r2 and at[(root, r2)] == r2
    o.close(); t.close()


def _ids(n):
    return [f"r{i}" for i in range(n)]


@pytest.mark.parametrize("expand", [False, True], ids=["plain", "expand"])
@pytest.mark.parametrize("ends", ["se", "pe"])
@pytest.mark.parametrize("k", MANIFEST["ks"])
def test_oracle_tsv_equals_committed_reference_tsv(built, k, ends, expand):
    w, _, prefix = built
    want = gzip.open(os.path.join(TDIR, f"{w.info['name']}.{ends}_k{k}{'.expand' if expand else ''}.tsv.gz"), "rb").read()
    o = ora.OracleIndex(prefix, max_result=k, expand=expand)
    if ends == "se":
        res = o.classify(w.reads.bases, w.reads.offsets, dust=True, threads=4)
        n = w.reads.n
    else:
        r1, r2 = w.pairs
        res = o.classify(r1.bases, r1.offsets, r2.bases, r2.offsets, dust=True, threads=4)
        n = r1.n
    own = o.tsv(_ids(n), res)
    assert want.count(b"\n") > n
    if own != want:
        a, b = own.split(b"\n"), want.split(b"\n")
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        assert False, f"{len(diff)} rows differ (oracle, reference), first: {diff[:3]}"
    o.close()


@pytest.mark.parametrize("k", [1, 2, 5])
def test_host_tail_equals_oracle_on_the_cassette_reads(built, k):
    """cfr_classify_from_hits_expanded (the host twin of the device tail: cfr_tail.cpp) on the oracle's hit list of every cassette read
    whose rows are all located at this k, with the rows' sequence ids from the oracle: matches and --expand-taxid lists equal the
    oracle's.  (A second top as the backbone is a child of the root in the reference's lcaChildTaxIds, Taxonomy.hpp:770.)"""
    w, _, prefix = built
    o = ora.OracleIndex(prefix, max_result=k, expand=True)
    idx = capi.Index(prefix, capi.default_params(max_result=k, output_expanded=1))
    rs = w.reads
    picked = [i for i, j in enumerate(w.info["read_cassette"]) if j >= 0 and w.info["cassettes"][j].size <= 40 * k]
    hits, hit_begin, row_begin, row_vals, qlen = [], [0], [0], [], []
    for i in picked:
        for h in o.query_hits(rs.get(i), None):
            hits.append((int(h["sp"]), int(h["ep"]), int(h["l"]), int(h["strand"]), int(h["offset"]), 0))
            row_vals += [o.locate(r)[0] for r in range(int(h["sp"]), int(h["ep"]) + 1)]
            row_begin.append(len(row_vals))
        hit_begin.append(len(hits))
        qlen.append(len(rs.get(i)))
    res, mat, spans, xids = idx.classify_from_hits_expanded(np.array(hits, dtype=capi.HIT_DTYPE), hit_begin, row_begin, row_vals, qlen, threads=2)
    ores = o.classify(rs.bases, rs.offsets, threads=4)
    assert len(picked) >= 100
    for n, i in enumerate(picked):
        r, b = ores[i], int(res["match_begin"][n])
        assert (int(res["score"][n]), int(res["n_match"][n])) == (int(r.score), int(r.nmatch)), (w.info["name"], i)
        got = [(int(m["kind"]), int(m["id"]), int(m["taxid"])) for m in mat[b:b + r.nmatch]]
        assert got == [(int(r.kind[q]), int(r.id[q]), int(r.taxid[q])) for q in range(r.nmatch)], (w.info["name"], i, got)
        lists = [[int(x) for x in xids[int(s["begin"]):int(s["begin"]) + int(s["count"])]] for s in spans[b:b + r.nmatch]]
        assert lists == [r.expanded_ids(q) for q in range(r.nmatch)], (w.info["name"], i, lists, [r.expanded_ids(q) for q in range(r.nmatch)])
    idx.close(); o.close()


# ------------------------------------------------------------------------------------------------ promote, kreport, quant: the host twins
def _script_inputs(built, tmp_path, monkeypatch):
    """pc.Tree / kc.Script read `<key>.taxonomy-tree.txt` and `<key>.name-table.txt` under pc.IDIR: here what bin/centrifuger-inspect
    prints for the world's own index"""
    import promote_cases as pc
    w, _, prefix = built
    for mode in ("taxonomy-tree", "name-table"):
        r = subprocess.run([pc.INSPECT, "-x", prefix, "--" + mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 0, r.stderr.decode()[-1000:]
        (tmp_path / f"world.{mode}.txt").write_bytes(r.stdout)
    monkeypatch.setattr(pc, "IDIR", str(tmp_path))
    return "world"


def _tax_id_lists(w, prefix, t):
    """the tax ids of the oracle's rows for the world's single reads at -k 1 and -k 5, and every ordered pair of (sampled) nodes"""
    out = []
    for k in (1, 5):
        o = ora.OracleIndex(prefix, max_result=k)
        res = o.classify(w.reads.bases, w.reads.offsets, threads=4)
        out += [[int(res[i].taxid[q]) for q in range(res[i].nmatch)] for i in range(w.reads.n)]
        o.close()
    nodes = [int(t.orig_taxid[x]) for x in _nodes_for_tuples(w, t)][:40]
    out += [[a, b] for a in nodes for b in nodes] + [[a, 424242, b] for a in nodes[:6] for b in nodes[-6:]]
    return out


def test_promote_host_twin_equals_script_restatement(built, tmp_path, monkeypatch):
    """every level of promote_cases.LEVELS; the tree and the levels are those bin/centrifuger-inspect prints for this index.  A walk
    stops at a node that is its own parent (cfr_promote_core.hpp:21-22): with a root above tax id 1 the script itself would not return."""
    import promote_cases as pc
    w, _, prefix = built
    tree = pc.Tree(_script_inputs(built, tmp_path, monkeypatch))
    t = capi.Taxonomy(prefix)
    nc = int(t.node_cnt)
    assert tree.orig == t.orig_taxid.tolist()
    reads = _tax_id_lists(w, prefix, t)
    res0, mat0 = pc.make_arrays(tree, reads, nc, seq_to_tax=t.seq_to_tax, rng=np.random.default_rng(3), gap=1)
    for level in pc.LEVELS:
        res, mat = res0.copy(), mat0.copy()
        p = capi.Promote(prefix, level, device=None)
        src = p.apply(res, mat, want_src=True)
        p.close()
        pc.check_against_script(tree, reads, level, res0, mat0, res, mat, src, nc)
    t.close()


@pytest.mark.parametrize("score_data", [False, True], ids=["plain", "score_data"])
def test_kreport_host_twin_equals_script_restatement(built, score_data, tmp_path, monkeypatch):
    import kreport_cases as kc
    w, _, prefix = built
    t = capi.Taxonomy(prefix)
    nc = int(t.node_cnt)
    if 1 not in t.orig_taxid.tolist():                        # the report hangs on tax id 1 (dfs_summation(1)): such an index is refused
        with pytest.raises(capi.CfrError):
            capi.Kreport(prefix, device=None)
        assert w.info["name"] == "no_tax_id_1"
        return
    s = kc.Script(_script_inputs(built, tmp_path, monkeypatch))
    rng = np.random.default_rng(17)
    reads = [(ids, int(rng.integers(0, 1 << 20)), int(rng.integers(0, 300))) for ids in _tax_id_lists(w, prefix, t) if not ids or ids[0] != 0 or all(x in s.tree.compact for x in ids)]
    counts, scores, seq, warn = s.count_reads(reads)
    clade, cscore = s.clades(counts, scores)
    k = capi.Kreport(prefix, device=None, score_data=score_data)
    res, mat = kc.arrays(s.tree, reads, nc, seq_to_tax=t.seq_to_tax, rng=np.random.default_rng(5), gap=1)
    k.add_results(res, mat)
    own, cl, sc, csc, seq_count = k.counts()
    assert seq_count == seq == len(reads) and int(own.sum()) == seq
    assert np.array_equal(own, s.bins(counts, nc)) and np.array_equal(cl, s.bins({a: v for a, v in clade.items() if a == 0 or a in s.tree.compact}, nc))
    if score_data:
        assert np.array_equal(sc, s.bins(scores, nc)) and np.array_equal(csc, s.bins(cscore, nc))
    assert k.warnings().tolist() == warn
    want = s.report(counts, scores, seq, score_data=score_data)
    k.write(str(tmp_path / "report.txt"))
    assert (tmp_path / "report.txt").read_bytes() == want
    k.close(); t.close()


@pytest.mark.parametrize("fmt", [0, 1])
def test_quant_host_twin_equals_reference_quantifier(built, fmt, tmp_path):
    """The reference classifier's rows at -k 5 through the quant host twin: it runs to the end on every world, and on the five
    single-rooted ones it prints the report the reference's centrifuger-quant printed for the same rows (tests/golden/taxworlds),
    byte for byte.

    On the four forests the reports differ, on purpose (cfr_quant.cpp, general_tree): ConvertToGeneralTree means to hang every further
    top below the root, but adds the edge root -> root first, after which the next top replaces the root's child list.  The committed
    reference reports show the loss - their root row counts about half of the classified reads, and the top of the tree that was
    lost gets abundance 0 - and this test reads that off them; the twin's root row counts every classified read, and each of its rows
    (both formats) is checked against the twin's own tables."""
    w, _, prefix = built
    tsv = str(tmp_path / "se_k5.tsv")
    open(tsv, "wb").write(gzip.open(os.path.join(TDIR, f"{w.info['name']}.se_k5.tsv.gz"), "rb").read())
    q = capi.Quant(prefix, device=None)
    q.add_tsv(tsv)
    assert q.run() >= 1
    q.write(str(tmp_path / "report.txt"), fmt)
    v = q.values()
    q.close()
    want = gzip.open(os.path.join(TDIR, f"{w.info['name']}.quant_fmt{fmt}.txt.gz"), "rb").read()
    own = (tmp_path / "report.txt").read_bytes()
    assert len(want) > 100
    if w.info["name"] not in tw.FOREST:
        assert own == want
        return
    assert own != want
    t = capi.Taxonomy(prefix)
    compact = {int(x): c for c, x in enumerate(t.orig_taxid.tolist())}
    rows = lambda text: [l.split(b"\t") for l in text.split(b"\n")[1:] if l]
    if fmt == 0:                                                  # name, taxID, taxRank, genomeSize, numReads, numUniqueReads, abundance
        classified = len({l.split(b"\t")[0] for l in open(tsv, "rb").read().split(b"\n")[1:] if l and l.split(b"\t")[2] != b"0"})
        root_row = lambda text: [r for r in rows(text) if int(r[1]) == w.info["root_taxid"]][0]
        assert int(root_row(own)[4]) == classified > 150 and float(root_row(own)[6]) == 1.0
        assert int(root_row(want)[4]) < 0.6 * classified and float(root_row(want)[6]) < 0.75
        # every row is the twin's own table: the read count rounded down, the abundance to seven places; and every other top's row
        # is there with a share of the abundance (the reference prints 0 for the top of the tree it lost)
        for r in rows(own):
            c = compact[int(r[1])]
            assert int(r[4]) == int(v["read_count"][c]) and abs(float(r[6]) - float(v["abund"][c])) < 1e-7, r
        others = [r for r in rows(own) if int(t.parent[compact[int(r[1])]]) == compact[int(r[1])] and int(r[1]) != w.info["root_taxid"]]
        assert others and all(0.2 < float(r[6]) < 0.8 for r in others), others
    else:                                                         # lineage by name, lineage by id, percentage, ...
        assert len(rows(own)) >= 20
        for r in rows(own):
            c = compact[int(r[1].split(b"|")[-1])]
            assert abs(float(r[2]) - 100.0 * float(v["abund"][c])) < 1e-5, r
        in_both = {r[1]: float(r[2]) for r in rows(want)}
        assert sum(1 for r in rows(own) if r[1] in in_both and abs(float(r[2]) - in_both[r[1]]) > 1.0) >= 5      # (the reference's shares are those of one tree)
    t.close()


def test_quant_read_counts_sum_to_the_read_count(built):
    """The read count that reaches the root equals the number of classified reads, on every world, forests included
    (every top hangs below the root in the quantifier's tree; before, a forest's root counted one tree alone - about half of the
    reads - and orphan_subtree's EM ran its full 1000 rounds).  The abundance at the root is 1 up to rounding (the M-step
    normalises: a few ulp per node), and the EM ends before its cap."""
    w, _, prefix = built
    o = ora.OracleIndex(prefix, max_result=5)
    ores = o.classify(w.reads.bases, w.reads.offsets, threads=4)
    t = capi.Taxonomy(prefix)
    nc = int(t.node_cnt)
    res = np.zeros(w.reads.n, dtype=capi.RESULT_DTYPE)
    mat = np.zeros(5 * w.reads.n, dtype=capi.MATCH_DTYPE)
    for i in range(w.reads.n):
        r = ores[i]
        res[i] = (r.score, r.secondaryScore, r.hitLength, r.queryLength, r.nmatch, 0, 5 * i)
        for q in range(r.nmatch):
            mat[5 * i + q] = (r.id[q], r.taxid[q], r.kind[q], 0)
    classified = int((res["n_match"] > 0).sum())
    q = capi.Quant(prefix, device=None)
    q.add_results(res, mat)
    rounds = q.run()
    v = q.values()
    assert rounds >= 1 and v["node_cnt"] == nc
    total = float(v["read_count"][int(t.root)])
    print(w.info["name"], "rounds", rounds, "classified", classified, "reads at the root", total, "abundance sum", float(v["abund"].sum()))
    assert abs(total - classified) < 1e-6 * max(1, classified), (total, classified)
    assert abs(float(v["abund"][int(t.root)]) - 1.0) < 1e-9 and rounds < 1000, (float(v["abund"][int(t.root)]), rounds)
    q.close(); o.close(); t.close()
