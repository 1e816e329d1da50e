"""The chain hand-out of k_search_prot_sm and the sub-batches of the protein path.  The protein tests of tests/test_gpu_protein.py send at
most 5 400 chains: every lane of the resident grid gets one chain and the kernel ends.  Here batches hold more chains than the grid has
lanes (wave tiles drawn from tile_ctr, `chain + stride` with CFR_PROT_DYN=0, a lane set up for a second and a third chain, tiles that
reach past the last chain) and are cut into sub-batches (read0 != 0: the translated codes of read r live at prot_code_base(o, read0 + r)).

About 2 000 unique reads - the reads of the four protein worlds and the golden se.fa - are classified once by the C oracle; a batch
repeats them in a seeded permutation.  A read's answer does not depend on its neighbours, so every copy must give the records and the
match slots of its unique read (compared as arrays) and the unique reads' TSV rows must be the oracle's.

The library reads its switches once per process, so a switch set is a child process (a fresh `python -m pytest <this file> -k ..`, one
at a time, as tests/test_gpu_variants.py starts them); the tests that only mean something under a switch are defined in a process that
has it set, and the test that starts the child counts what passed there.  -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_lib as ora
import protein_worlds as pw
from centrifuger_amd import capi
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
ENV = os.environ
BLOCKS = int(ENV.get("CFR_PROT_BLOCKS", "0"))
SUBBATCH = int(ENV.get("CFR_SUBBATCH", "0"))
FIELDS = ("score", "secondary_score", "hit_length", "query_length", "n_match")


class Unique:
    """the unique reads (or pairs), one world's index and the oracle's answers for them: made once per module"""

    def __init__(self, d, world, k, paired):
        self.k, self.paired = k, paired
        w = pw.make(world)
        g = w.genomes
        self.prefix = os.path.join(d, f"{world}_{k}_{int(paired)}")
        capi.build_index(g.names, g.taxids, g.seqs, g.nodes, g.tax_names, self.prefix, **pw.build_kwargs(w))
        sets = []
        for name in pw.NAMES:
            x = pw.make(name)
            sets.append(x.pairs if paired else (x.reads,))
        gold = [ora.read_fastx(os.path.join(GOLDEN, "prot", f))[1:] for f in (("pe_1.fa", "pe_2.fa") if paired else ("se.fa",))]
        self.mates = []
        for m in range(2 if paired else 1):
            reads = [s[m].get(i) for s in sets for i in range(s[m].n)]
            b, o = gold[m]
            reads += [b[int(o[i]):int(o[i + 1])].tobytes() for i in range(len(o) - 1)]
            offs = np.zeros(len(reads) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(r) for r in reads])
            self.mates.append((np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offs))
        self.n = len(self.mates[0][1]) - 1
        o = ora.OracleIndex(self.prefix, max_result=k)
        (b1, o1), (b2, o2) = self.mates[0], self.mates[1] if paired else (None, None)
        res = o.classify(b1, o1, b2, o2, threads=16)
        self.rows = [o.format(f"u{u}", res[u]) for u in range(self.n)]
        self.want = np.array([[res[u].score, res[u].secondaryScore, res[u].hitLength, res[u].queryLength, res[u].nmatch] for u in range(self.n)], dtype=np.int64)
        o.close()
        self.index = capi.Index(self.prefix, capi.default_params(max_result=k))
        self.dev = capi.DeviceIndex(self.index)

    def batch(self, n, seed):
        """n reads: the unique ones again and again, each round in another seeded order -> (source of every read, mates)"""
        rng = np.random.default_rng(seed)
        src = np.concatenate([rng.permutation(self.n) for _ in range((n + self.n - 1) // self.n)])[:n]
        out = []
        for b, o in self.mates:
            o = o.astype(np.int64)
            lens = (o[1:] - o[:-1])[src]
            offs = np.zeros(n + 1, dtype=np.int64)
            offs[1:] = np.cumsum(lens)
            take = np.repeat(o[:-1][src] - offs[:-1], lens) + np.arange(int(offs[-1]), dtype=np.int64)
            out.append((b[take], offs.astype(np.uint64)))
        return src, out

    def check(self, src, res, mat, what):
        """every copy against its unique read's record (oracle), match slots equal among the copies, the first copies' TSV rows"""
        n, k = len(src), self.k
        got = np.stack([res[f].astype(np.int64) for f in FIELDS], axis=1)
        bad = np.nonzero((got != self.want[src]).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {n} records differ from the oracle's, first: read {bad[0]} (unique {src[bad[0]]}) got {got[bad[0]]} want {self.want[src[bad[0]]]}"
        assert len(mat) == n * k and np.array_equal(res["match_begin"], np.arange(n, dtype=np.uint64) * k)
        first = np.full(self.n, -1, dtype=np.int64)
        present, at = np.unique(src, return_index=True)
        first[present] = at                                                           # the first copy of every unique read in the batch
        live = np.arange(k)[None, :] < got[:, 4][:, None]
        for f in ("id", "taxid", "kind"):
            m = mat[f].reshape(n, k)
            assert np.array_equal(np.where(live, m, 0), np.where(live, m[first[src]], 0)), f"{what}: match slots ({f}) differ between copies of a read"
        for u in np.nonzero(first >= 0)[0]:
            row = self.index.format_tsv(f"u{u}", res[first[u]], mat)
            assert row == self.rows[u], f"{what}: unique read {u}: got {row!r} want {self.rows[u]!r}"

    def run(self, n, seed, what, entry="classify"):
        src, mates = self.batch(n, seed)
        (b1, o1), (b2, o2) = mates[0], mates[1] if self.paired else (None, None)
        if entry == "classify":
            res, mat = self.dev.classify(b1, o1, b2, o2)
        elif entry == "submit":
            res, mat = self.dev.wait(self.dev.submit(b1, o1, b2, o2))
        else:
            t = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (b1, o1) + ((b2, o2) if self.paired else ())]
            torch.cuda.synchronize()
            args = (t[0].data_ptr(), t[1].data_ptr(), n, int(o1[-1])) + ((t[2].data_ptr(), t[3].data_ptr(), int(o2[-1])) if self.paired else ())
            res, mat = self.dev.classify_resident(*args)
        self.check(src, res, mat, f"{what} ({entry})")
        return res, mat


@pytest.fixture(scope="module")
def uniques(tmp_path_factory):
    d, made = str(tmp_path_factory.mktemp("chains")), {}

    def get(world, k, paired):
        if (world, k, paired) not in made:
            made[(world, k, paired)] = Unique(d, world, k, paired)
        return made[(world, k, paired)]
    yield get
    for u in made.values():
        u.dev.close()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("ends", ["se", "pe"])
def test_more_chains_than_lanes(ends, uniques):
    """120 000 reads = 720 000 chains (60 000 pairs: the same): above CUs x 8 blocks x 256 lanes, the most k_search_prot_sm can have
    resident on 256 CUs - at least a quarter of the chains are a lane's second or later one."""
    paired = ends == "pe"
    u = uniques("shared", 5, paired)
    n = 60_000 if paired else 120_000
    if not BLOCKS and not SUBBATCH:
        assert n * (12 if paired else 6) > _cus() * 8 * 256
    u.run(n, 101 + paired, f"{n} reads {ends}")


def _live_slots(res, mat, k):
    """the match slots with everything behind a read's n_match zeroed: a slot a read does not use is not part of its answer - it holds
    what an earlier sub-batch left in the device buffer (tests/test_gpu_scale.py canon() reads the slots the same way)"""
    live = np.arange(k)[None, :] < res["n_match"].astype(np.int64)[:, None]
    return np.stack([np.where(live, mat[f].reshape(len(res), k).astype(np.int64), 0) for f in ("id", "taxid", "kind")], axis=2)


def test_same_batch_twice_gives_identical_bytes(uniques):
    """the result records byte for byte (padding included), the match slots in use byte for byte"""
    u = uniques("repeats", 5, False)
    a = u.run(30_000, 7, "first run")
    b = u.run(30_000, 7, "second run")
    assert a[0].tobytes() == b[0].tobytes()
    assert _live_slots(*a, u.k).tobytes() == _live_slots(*b, u.k).tobytes()


if BLOCKS == 1:
    def _stride_batches():
        """read counts whose chain counts are stride - 5, stride, stride + 1, + 63, + 65 and 3 x stride + 7 rounded to whole reads
        (stride = CUs x 256 lanes, six chains per read), moved by a read or two until their remainders modulo 64 all differ"""
        stride, out = _cus() * 256, []
        for chains in (stride - 5, stride, stride + 1, stride + 63, stride + 65, 3 * stride + 7):
            n = (chains + 5) // 6
            while any(n % 64 == m % 64 for m in out):
                n += 1
            out.append(n)
        return stride, out

    @pytest.mark.parametrize("which", range(6))
    def test_stride_batches(which, uniques):
        """One block per CU: the grid's lanes take the first CUs x 256 chains; what lies beyond them is a last tile that reaches past the
        last chain, one lane that draws, a whole wave that draws at once, several draws per lane."""
        stride, ns = _stride_batches()
        n = ns[which]
        assert abs(6 * n - (stride - 5, stride, stride + 1, stride + 63, stride + 65, 3 * stride + 7)[which]) <= 6 * 8
        uniques("frames", 1, False).run(n, 300 + which, f"{n} reads, stride {stride}")

    def test_stride_batch_of_pairs(uniques):
        stride = _cus() * 256
        n = (stride + 65 + 11) // 12 + 3
        uniques("ragged", 5, True).run(n, 310, f"{n} pairs, stride {stride}")


if SUBBATCH:
    @pytest.mark.parametrize("entry", ["classify", "submit", "resident"])
    @pytest.mark.parametrize("ends", ["se", "pe"])
    def test_sub_batches(ends, entry, uniques):
        """Several sub-batches (read0 != 0) through the three entries: the unique reads once for a small sub-batch, 20 000 reads for a
        large one."""
        paired = ends == "pe"
        u = uniques("ragged" if paired else "frames", 5, paired)
        n = max(u.n, 2 * SUBBATCH + 5) if SUBBATCH < 4000 else 20_000
        assert n > 2 * SUBBATCH
        u.run(n, 500 + SUBBATCH, f"{n} reads {ends}, sub-batches of {SUBBATCH}", entry=entry)


def _child(select, extra, want_passed):
    env = dict(ENV, CFR_DEBUG_ENV="1")
    env.update(extra)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", select],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT, timeout=600)
    tail = r.stdout.decode()[-2000:]
    assert r.returncode == 0, f"{extra}:\n{tail}"
    assert f"{want_passed} passed" in tail, tail


@pytest.mark.parametrize("hand_out", ["wave_tiles", "static"])
def test_one_block_per_cu_child_process(hand_out):
    """CFR_PROT_BLOCKS=1 (stride = CUs x 256) with the wave tiles and with CFR_PROT_DYN=0 (chain + stride): the seven batches around
    the stride."""
    _child("stride_batch", {"CFR_PROT_BLOCKS": "1", **({"CFR_PROT_DYN": "0"} if hand_out == "static" else {})}, 7)


@pytest.mark.parametrize("sub", [37, 1000, 4099])
def test_sub_batches_child_process(sub):
    _child("test_sub_batches and not child", {"CFR_SUBBATCH": str(sub), "CFR_TAPER_FLOOR": "0"}, 6)
