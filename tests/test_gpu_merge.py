"""--merge-readpair on the device (k_merge_decide / k_merge_write) against the host twin (cfr_merge_pairs, itself pinned to the
reference's ReadPairMerger by tests/test_merge_host_cpu.py), the classify entries that run it as a pre-step against the reference's
TSVs, and the command line.  The second fixture (tests/golden/merge_long) and the two seeded sweeps drive the kernels to their own
units: plane words 1..8 and the funnel shift into the last one, the 512-base switch to the byte path, offsets and overlaps at
multiples of 64, and every overlap length 32..600 exactly on the similarity threshold and one substitution past it.  -m gpu."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import merge_fixtures as mf
from centrifuger_amd import capi
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.full(256, ord("N"), dtype=np.uint8)
COMP[ACGT] = ACGT[::-1]


def _flat(seqs):
    o = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return (np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)).astype(np.uint8), o


def _random_pairs(rng, n):
    """mates of 0..300 bases cut from fragments that make them overlap by every size 0..150 (and not at all), read-through included,
    with substitutions, non-ACGT bytes, tandem overlaps; qualities with exact ties at q1 == qm - 14 and rcq2 == q1"""
    r1s, r2s, q1s, q2s = [], [], [], []
    for i in range(n):
        L1, L2 = int(rng.integers(0, 301)), int(rng.integers(0, 301))
        ov = i % 152                                           # 151: no overlap at all
        flen = L1 + L2 - ov if ov <= min(L1, L2) and ov < 151 else int(rng.integers(1, 700))
        if i % 4 == 3:                                         # a fragment shorter than both reads: read-through
            flen = int(rng.integers(1, max(2, min(L1, L2) + 1)))
        f = ACGT[rng.integers(0, 4, size=max(flen, 1))]
        if i % 11 == 0 and flen > 8:                            # a tandem repeat where the mates meet
            a = max(0, min(L1, flen) - int(rng.integers(0, 70)))
            f[a:a + 80] = np.resize(ACGT[rng.integers(0, 4, size=int(rng.integers(1, 4)))], len(f[a:a + 80]))
        r1 = np.concatenate([f, ACGT[rng.integers(0, 4, size=max(0, L1 - len(f)))]])[:L1].copy()
        r2 = np.concatenate([COMP[f[::-1]], ACGT[rng.integers(0, 4, size=max(0, L2 - len(f)))]])[:L2].copy()
        for r in (r1, r2):
            m = rng.random(len(r)) < 0.02
            r[m] = ACGT[rng.integers(0, 4, size=int(m.sum()))]
            if i % 5 == 0 and len(r):
                m = rng.random(len(r)) < 0.03
                r[m] = np.frombuffer(b"NnacgtRY.", dtype=np.uint8)[rng.integers(0, 9, size=int(m.sum()))]
        q1 = rng.integers(33, 74, size=L1).astype(np.uint8)
        q2 = rng.integers(33, 74, size=L2).astype(np.uint8)
        if i % 3 == 0 and i % 4 != 3 and ov <= min(L1, L2) and ov < 151:      # the overlap is r1[L1 - ov:] against rc(r2)[:ov]: ties on it
            rc = q2[::-1]
            rc[:ov] = q1[L1 - ov:] + (14 if i % 2 else 0)
        elif i % 3 == 1:
            m = min(L1, L2)
            q2[::-1][:m] = q1[:m]                               # read-through at offset 0: rcq2 == q1
        r1s.append(r1); r2s.append(r2); q1s.append(q1); q2s.append(q2)
    b1, o1 = _flat(r1s)
    b2, o2 = _flat(r2s)
    return b1, o1, _flat(q1s)[0], b2, o2, _flat(q2s)[0]


def _same(a, b):
    for k in ("kind", "overlap", "offset", "offsets1", "offsets2", "bases1", "bases2", "qual1", "qual2"):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def dev(golden_dir):
    out = {}

    def get(k):
        if k not in out:
            idx = capi.Index(os.path.join(golden_dir, "f6"), capi.default_params(max_result=k))
            out[k] = (idx, capi.DeviceIndex(idx))
        return out[k]
    yield get
    for _, d in out.values():
        d.close()


@pytest.fixture(scope="module")
def random_pairs():
    rng = np.random.default_rng(20261017)
    p = _random_pairs(rng, 20_000)
    host = {True: capi.merge_pairs(p[0], p[1], p[3], p[4], p[2], p[5], threads=16),
            False: capi.merge_pairs(p[0], p[1], p[3], p[4], threads=16)}
    return p, host


@pytest.mark.parametrize("fmt", ["fq", "fa"])
def test_device_merge_equals_reference_dump(dev, fmt):
    _, d = dev(1)
    p = mf.pairs(fmt)
    mf.check_against_dump(fmt, d.merge_pairs(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], p["q2"]))


@pytest.mark.parametrize("fmt", ["fq", "fa"])
def test_device_merge_equals_reference_dump_long(dev, fmt):
    _, d = dev(1)
    p = mf.pairs(fmt, "merge_long")
    mf.check_against_dump(fmt, d.merge_pairs(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], p["q2"]), "merge_long")


@pytest.mark.parametrize("with_qual", [True, False])
def test_device_merge_equals_host_merge(dev, random_pairs, with_qual):
    _, d = dev(1)
    (b1, o1, q1, b2, o2, q2), host = random_pairs
    want = host[with_qual]
    kinds = want["kind"].tolist()
    assert min(kinds.count(k) for k in (0, 1, 2)) > 1000            # the mix really merges both ways
    for shift in (0, 1, 2, 3, 5):                                  # the buffers' alignment
        pad = np.full(shift, ord("G"), dtype=np.uint8)
        sh = np.uint64(shift)
        got = d.merge_pairs(np.concatenate([pad, b1]), o1 + sh, np.concatenate([pad, b2]), o2 + sh,
                            np.concatenate([pad, q1]) if with_qual else None, np.concatenate([pad, q2]) if with_qual else None)
        _same(got, want)


def test_long_mates_take_the_byte_path(dev):
    """two 5 kbp mates that overlap by 2 kbp (beyond the bit planes kept in LDS), one pair whose mates differ, and short pairs around them"""
    _, d = dev(1)
    rng = np.random.default_rng(5)
    f = ACGT[rng.integers(0, 4, size=8000)]
    r1, r2 = f[:5000].copy(), COMP[f[::-1]][:5000].copy()
    r1[rng.random(5000) < 0.01] = ord("A")
    s = ACGT[rng.integers(0, 4, size=260)]
    pairs = [(s[:150], COMP[s[::-1]][:150]), (r1, r2), (r1, ACGT[rng.integers(0, 4, size=700)]), (f[:600], COMP[f[:450][::-1]]), (s[:150], COMP[s[::-1]][:150])]
    b1, o1 = _flat([p[0] for p in pairs])
    b2, o2 = _flat([p[1] for p in pairs])
    q1, q2 = rng.integers(33, 74, size=len(b1)).astype(np.uint8), rng.integers(33, 74, size=len(b2)).astype(np.uint8)
    want = capi.merge_pairs(b1, o1, b2, o2, q1, q2)
    assert want["kind"].tolist() == [1, 1, 0, 2, 1] and want["overlap"].tolist()[1] == 2000
    _same(d.merge_pairs(b1, o1, b2, o2, q1, q2), want)


EDGE_LENS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 447, 448, 449, 511, 512, 513, 514, 600, 1100)
EDGE_OFFSETS = (0, 1, 63, 64, 65, 128, 191, 192, 448)
EDGE_OVERLAPS = tuple(k + d for k in (64, 128, 192, 256, 320, 384, 448, 512) for d in (-1, 0, 1))


def _edge_pairs(rng):
    """every (len1, len2) of EDGE_LENS: the same fragment seen by both mates with the overlap K, or the true offset j, taken from the
    word-edge values that fit, in the plain and in the read-through pass, and mates that have nothing in common; more rounds where
    both mates are longer than the planes (16 length combinations only).  1 to 3 % substitutions, a twentieth of the pairs with N / lower case."""
    r1s, r2s, q1s, q2s = [], [], [], []

    def rnd(n):
        return ACGT[rng.integers(0, 4, size=n)]

    def put(r1, rc, tie):
        i = len(r1s)
        r1, rc = r1.copy(), rc.copy()
        for r in (r1, rc):
            m = rng.random(len(r)) < (0.005, 0.01, 0.015)[i % 3]      # per mate: 1, 2, 3 % between the two
            r[m] = ACGT[rng.integers(0, 4, size=int(m.sum()))]
            if i % 20 == 7:
                a, n = int(rng.integers(0, len(r))), int(rng.integers(1, 9))
                r[a:a + n] = ord("N") if i % 40 == 7 else np.frombuffer(bytes(r[a:a + n]).lower(), dtype=np.uint8)
        q1, rcq = rng.integers(33, 74, size=len(r1)).astype(np.uint8), rng.integers(33, 74, size=len(rc)).astype(np.uint8)
        if tie is not None and i % 3 == 0:                            # ties of both quality rules where the mates really align
            a1, a2, K = tie
            rcq[a2:a2 + K] = q1[a1:a1 + K] + (14 if i % 2 else 0)
        r1s.append(r1); r2s.append(COMP[rc[::-1]]); q1s.append(q1); q2s.append(rcq[::-1].copy())

    n = 0
    for L1 in EDGE_LENS:
        for L2 in EDGE_LENS:
            rounds = 1 if min(L1, L2) <= 512 else 6
            for _ in range(rounds):
                n += 1
                m = min(L1, L2)
                f = rnd(L1 + L2 + 600)
                # plain pass: r1 = f[:L1], rc(r2) = f[j:j + L2]
                Ks = [k for k in EDGE_OVERLAPS if k <= m]
                K = Ks[n % len(Ks)] if Ks else m
                put(f[:L1], f[L1 - K:L1 - K + L2], (L1 - K, 0, K))
                js = [j for j in EDGE_OFFSETS if 0 < j <= L1 - 33]
                j = js[n % len(js)]
                put(f[:L1], f[j:j + L2], (j, 0, min(L1 - j, L2)))
                # read-through pass: a fragment of F bases, rc(r2) = j adapter bases + the fragment, r1 = the fragment + adapter
                F = Ks[(n + 1) % len(Ks)] if Ks else m
                put(np.concatenate([f[:F], rnd(L1 - F)]), np.concatenate([rnd(L2 - F), f[:F]]), (0, L2 - F, F))
                js = [j for j in EDGE_OFFSETS if j <= L2 - 33]
                j = js[(n + 2) % len(js)]
                F = L2 - j
                put(np.concatenate([f[:F], rnd(max(0, L1 - F))])[:L1], np.concatenate([rnd(j), f[:F]]), (0, j, min(F, L1)))
                # nothing in common
                put(f[:L1], f[L1 + 300:L1 + 300 + L2], None)
                if max(L1, L2) > 512:
                    put(rnd(L1), rnd(L2), None)
    b1, o1 = _flat(r1s)
    b2, o2 = _flat(r2s)
    return b1, o1, _flat(q1s)[0], b2, o2, _flat(q2s)[0]


@pytest.fixture(scope="module")
def edge_pairs():
    p = _edge_pairs(np.random.default_rng(20261019))
    host = {True: capi.merge_pairs(p[0], p[1], p[3], p[4], p[2], p[5], threads=16),
            False: capi.merge_pairs(p[0], p[1], p[3], p[4], threads=16)}
    return p, host


@pytest.mark.parametrize("with_qual", [True, False])
def test_device_merge_equals_host_merge_at_the_word_edges(dev, edge_pairs, with_qual):
    _, d = dev(1)
    (b1, o1, q1, b2, o2, q2), host = edge_pairs
    want = host[with_qual]
    n = len(o1) - 1
    assert 2000 <= n <= 4000
    len1, len2 = np.diff(o1.astype(np.int64)), np.diff(o2.astype(np.int64))
    longs = (len1 > 512).astype(int) + (len2 > 512)
    for c, name in enumerate(("both at most 512", "mixed", "both above 512")):      # a kernel that never merges long pairs must fail
        kinds = want["kind"][longs == c].tolist()
        print(name, int((longs == c).sum()), "pairs, kinds 0/1/2:", [kinds.count(k) for k in (0, 1, 2)])
        assert min(kinds.count(k) for k in (0, 1, 2)) >= 50, (name, [kinds.count(k) for k in (0, 1, 2)])
    for shift in (0, 1, 2, 3, 5):                                  # the buffers' alignment
        pad = np.full(shift, ord("G"), dtype=np.uint8)
        sh = np.uint64(shift)
        got = d.merge_pairs(np.concatenate([pad, b1]), o1 + sh, np.concatenate([pad, b2]), o2 + sh,
                            np.concatenate([pad, q1]) if with_qual else None, np.concatenate([pad, q2]) if with_qual else None)
        _same(got, want)


THRESHOLD_LENGTHS = range(32, 601)


def _threshold_geometry(L):
    """offset j and the e bases behind the overlap: both mates within the 512 bases of the planes as long as L allows it (L <= 511),
    j over 1..67 so that it is 64 and 65 for some L"""
    j = 1 + L % 67
    return (min(j, 512 - L), min(60, 512 - L)) if L < 512 else (j, 60)


@pytest.fixture(scope="module")
def threshold_pairs():
    """per L four pairs: plain pass at L - T(L) substitutions and at one more, read-through pass the same; T from Python floats
    (merge_fixtures.threshold).  Substitutions spread over the overlap's words for one pass and packed into its end for the other,
    swapping with L."""
    rng = np.random.default_rng(20261020)
    r1s, r2s = [], []
    for L in THRESHOLD_LENGTHS:
        j, e = _threshold_geometry(L)
        n = L - mf.threshold(L)
        for rt in (False, True):
            for extra in (0, 1):
                r1, r2 = mf.threshold_pair(ACGT[rng.integers(0, 4, size=j + L + e)], L, rt, j, e, n + extra, bool(L & 1) != rt,
                                           ACGT[rng.integers(0, 4, size=j + e)])
                r1s.append(r1); r2s.append(r2)
    b1, o1 = _flat(r1s)
    b2, o2 = _flat(r2s)
    q1, q2 = rng.integers(33, 74, size=len(b1)).astype(np.uint8), rng.integers(33, 74, size=len(b2)).astype(np.uint8)
    return b1, o1, q1, b2, o2, q2


def test_device_merge_on_the_similarity_threshold(dev, threshold_pairs):
    """an offset passes iff L - mism >= int(L * t(L)): for every L in 32..600 the last number of substitutions that merges and the
    first that does not, in both passes - first that the host twin does as designed (so that the comparison is not between two
    empty answers), then device == twin on every field"""
    _, d = dev(1)
    b1, o1, q1, b2, o2, q2 = threshold_pairs
    assert len(o1) - 1 == 4 * 569
    for quals in ((q1, q2), (None, None)):
        want = capi.merge_pairs(b1, o1, b2, o2, quals[0], quals[1], threads=16)
        kind, ov, off = want["kind"].reshape(-1, 4), want["overlap"].reshape(-1, 4), want["offset"].reshape(-1, 4)
        Ls = np.array(THRESHOLD_LENGTHS)
        js = np.array([_threshold_geometry(L)[0] for L in THRESHOLD_LENGTHS])
        assert np.array_equal(kind, np.tile([1, 0, 2, 0], (len(Ls), 1))), np.nonzero((kind != [1, 0, 2, 0]).any(axis=1))[0] + 32
        assert np.array_equal(ov[:, 0], Ls) and np.array_equal(ov[:, 2], Ls) and (ov[:, [1, 3]] == -1).all()
        assert np.array_equal(off[:, 0], js) and np.array_equal(off[:, 2], js) and (off[:, [1, 3]] == -1).all()
        _same(d.merge_pairs(b1, o1, b2, o2, quals[0], quals[1]), want)


def _tsv(idx, ids, results, matches):
    return capi.tsv_header() + b"".join(idx.format_tsv(ids[i].decode(), results[i], matches) for i in range(len(ids)))


def _classify_merged_case(dev, case, which):
    import torch
    args = mf.manifest(which)["cases"][case]["args"]
    fmt = "fq" if case.startswith("fq") else "fa"
    k = int(args[args.index("-k") + 1]) if "-k" in args else 1
    idx, d = dev(k)
    p = mf.pairs(fmt, which)
    kinds = np.array([r[0] for r in mf.dump(fmt, which)], dtype=np.int32)
    want = mf.tsv(case, which)
    d.set_merge(True)
    try:
        # SDUST on the device behind the merge
        d.set_dust("--no-dust" not in args)
        res, mat, kind = d.classify_merged(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], p["q2"])
        assert np.array_equal(kind, kinds)
        assert _tsv(idx, p["ids"], res, mat) == want
        # the resident entry: the same bytes
        t = {n: torch.from_numpy(p[n].view(np.int64) if p[n].dtype == np.uint64 else p[n]).cuda() for n in ("b1", "o1", "b2", "o2") if p[n] is not None}
        tq = {n: torch.from_numpy(p[n]).cuda() for n in ("q1", "q2") if p[n] is not None}
        torch.cuda.synchronize()
        n = len(p["ids"])
        res2, mat2, kind2 = d.classify_resident_merged(t["b1"].data_ptr(), t["o1"].data_ptr(), n, int(p["o1"][n]), t["b2"].data_ptr(), t["o2"].data_ptr(),
                                                       int(p["o2"][n]), tq["q1"].data_ptr() if tq else 0, tq["q2"].data_ptr() if tq else 0)
        assert np.array_equal(kind2, kinds) and res2.tobytes() == res.tobytes() and mat2.tobytes() == mat.tobytes()
        assert torch.equal(t["b1"].cpu(), torch.from_numpy(p["b1"])) and torch.equal(t["b2"].cpu(), torch.from_numpy(p["b2"]))   # the caller's buffers stay
        # SDUST off on the device: the host masks the merged reads, the device classifies them as they are (merge off)
        d.set_dust(False)
        if "--no-dust" not in args:
            b1, o1, _, b2, o2, _ = mf.expected_reads(fmt, which)
            b1, b2 = b1.copy(), b2.copy()
            capi.dust_mask(b1, o1); capi.dust_mask(b2, o2)
            d.set_merge(False)
            res3, mat3, kind3 = d.classify_merged(b1, o1, b2, o2)
            assert not kind3.any() and _tsv(idx, p["ids"], res3, mat3) == want
    finally:
        d.set_dust(False)
        d.set_merge(False)


@pytest.mark.parametrize("case", ["fq_k1", "fq_k5", "fq_nodust", "fa_k1"])
def test_classify_merged_equals_reference_tsv(dev, case):
    _classify_merged_case(dev, case, "merge")


@pytest.mark.parametrize("case", ["fq_k1", "fq_nodust", "fa_k1"])
def test_classify_merged_equals_reference_tsv_long(dev, case):
    _classify_merged_case(dev, case, "merge_long")


def test_empty_mate_equals_single_end(dev):
    """a pair with an empty mate is Query(r, NULL): what the merged pairs rely on"""
    idx, d = dev(5)
    p = mf.pairs("fq")
    n = 400
    o1, o2 = p["o1"][:n + 1], p["o2"][:n + 1]
    b1, b2 = p["b1"][:int(o1[n])], p["b2"][:int(o2[n])]
    zero = np.zeros(n + 1, dtype=np.uint64)
    empty = np.zeros(1, dtype=np.uint8)
    se1, m1 = d.classify(b1, o1)
    se2, m2 = d.classify(b2, o2)
    a, ma = d.classify(b1, o1, empty, zero)                 # every second mate empty
    ids = p["ids"][:n]
    assert _tsv(idx, ids, a, ma) == _tsv(idx, ids, se1, m1)
    # empty first mates, and a mix: even pairs keep both mates, odd pairs lose the second / the first
    c, mc = d.classify(empty, zero, b2, o2)
    # (a lone second mate is searched as the pair's second read: the result equals the single-end one of that read)
    assert _tsv(idx, ids, c, mc) == _tsv(idx, ids, se2, m2)
    keep = np.arange(n) % 2 == 0
    l2 = np.where(keep, np.diff(o2.astype(np.int64)), 0)
    mo2 = np.concatenate([[0], np.cumsum(l2)]).astype(np.uint64)
    mb2 = np.concatenate([b2[int(o2[i]):int(o2[i + 1])] for i in range(n) if keep[i]])
    full, mf_ = d.classify(b1, o1, b2, o2)
    mix, mm = d.classify(b1, o1, mb2, mo2)
    for i in range(n):
        want = (full, mf_) if keep[i] else (se1, m1)
        assert idx.format_tsv(ids[i].decode(), mix[i], mm) == idx.format_tsv(ids[i].decode(), want[0][i], want[1]), i


def test_single_end_packed_and_protein(dev, golden_dir):
    idx, d = dev(1)
    p = mf.pairs("fq")
    d.set_merge(True)
    try:
        on, mon, kind = d.classify_merged(p["b1"], p["o1"], None, None, p["q1"], None)
        assert not kind.any()
        d.set_merge(False)
        off, moff, _ = d.classify_merged(p["b1"], p["o1"], None, None, p["q1"], None)
        assert on.tobytes() == off.tobytes() and mon.tobytes() == moff.tobytes()
        d.set_merge(True)
        with pytest.raises(capi.CfrError) as e:
            d.classify_packed(capi.pack_reads(p["b1"]), p["o1"], capi.pack_reads(p["b2"]), p["o2"])
        assert e.value.status == capi.CFR_ERR_ARG
        with pytest.raises(capi.CfrError) as e:
            d.classify_merged(p["b1"], p["o1"], p["b2"], p["o2"], p["q1"], None)
        assert e.value.status == capi.CFR_ERR_ARG
    finally:
        d.set_merge(False)
    pidx = capi.Index(os.path.join(GOLDEN, "prot", "p2"))
    pd = capi.DeviceIndex(pidx)
    try:
        with pytest.raises(capi.CfrError) as e:
            pd.set_merge(True)
        assert e.value.status == capi.CFR_ERR_ARG
    finally:
        pd.close()


def _cli(tmp_path, golden_dir, fmt, extra, which="merge"):
    files = []
    for m in (1, 2):
        f = tmp_path / (f"pairs_{m}.{fmt}" if which == "merge" else f"{which}_{m}.{fmt}")
        if not f.exists():
            f.write_bytes(gzip.open(os.path.join(mf.GOLDEN, which, f"pairs_{m}.{fmt}.gz"), "rb").read())
        files.append(str(f))
    exe = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
    r = subprocess.run([exe, "-x", os.path.join(golden_dir, "f6"), "-1", files[0], "-2", files[1], "--merge-readpair"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


@pytest.mark.parametrize("case", ["fq_k1", "fq_k5", "fq_nodust", "fa_k1"])
def test_cli_merge_readpair_equals_reference(tmp_path, golden_dir, case):
    args = mf.manifest()["cases"][case]["args"][4:]
    fmt = "fq" if case.startswith("fq") else "fa"
    assert _cli(tmp_path, golden_dir, fmt, args) == mf.tsv(case)
    if case == "fq_k5":                                        # merged and unmerged pairs on both sides of every batch boundary
        assert _cli(tmp_path, golden_dir, fmt, args + ["--gpu-batch", "256"]) == mf.tsv(case)


@pytest.mark.parametrize("case", ["fq_k1", "fq_nodust", "fa_k1"])
def test_cli_merge_readpair_equals_reference_long(tmp_path, golden_dir, case):
    args = mf.manifest("merge_long")["cases"][case]["args"][4:]
    fmt = "fq" if case.startswith("fq") else "fa"
    assert _cli(tmp_path, golden_dir, fmt, args, "merge_long") == mf.tsv(case, "merge_long")
    if case == "fq_k1":                                        # merged and unmerged long pairs on both sides of every batch boundary
        assert _cli(tmp_path, golden_dir, fmt, args + ["--gpu-batch", "64"], "merge_long") == mf.tsv(case, "merge_long")


@pytest.mark.parametrize("batch", [[], ["--gpu-batch", "256"]])
def test_cli_merge_readpair_dumps(tmp_path, golden_dir, batch):
    assert _cli(tmp_path, golden_dir, "fa", ["--un", "un", "--cl", "cl"] + batch) == mf.tsv("fa_dump")
    for name in mf.manifest()["dumps"]:
        got = tmp_path / name
        if not got.exists():
            got = tmp_path / (name + ".gz")
        raw = got.read_bytes()
        if raw[:2] == b"\x1f\x8b":
            raw = gzip.decompress(raw)
        assert raw == mf.golden(name), name
