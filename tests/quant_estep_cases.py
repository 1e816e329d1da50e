"""Shared by tests/test_quant_host_cpu.py and tests/test_gpu_quant.py: inputs for cfr_quant_estep_probe and the yardstick they are
compared with bit for bit - a plain sequential restatement of the E-step loop of EMupdate (Quantifier.hpp:196-208) in numpy.float64
scalars (IEEE double, one rounding per operation, nothing fused): for every assignment in order, sum = the left-to-right sum of
abund[t]; then read_count[t] += (w * abund[t]) / sum slot by slot from 0.0; the init round adds w / cnt instead.

A case is (a_begin, a_target, a_weight, n_nodes, abund (rounds x n_nodes), init).  Cases and their yardsticks are made once per
process (lru_cache) and handed out read-only."""
import functools

import numpy as np

GRID_NODES = (1, 255, 256, 257, 1000)            # one lane per node, 256 lanes per block: one block, its last lane, the tail block
GRID_SLOTS = (0, 1, 255, 256, 257, 20011)        # one lane per slot likewise; 20011 = 78 blocks and 43 lanes


def restate(a_begin, a_target, a_weight, n_nodes, abund, init):
    out = []
    targets = [int(t) for t in a_target]
    begin = [int(b) for b in a_begin]
    weight = [np.float64(w) for w in a_weight]
    with np.errstate(all="ignore"):
        for r in range((1 if init else 0) + len(abund)):
            rc = [np.float64(0.0)] * n_nodes
            first = init and r == 0
            ab = None if first else [np.float64(x) for x in abund[r - (1 if init else 0)]]
            for i, w in enumerate(weight):
                t = targets[begin[i]:begin[i + 1]]
                if first:
                    term = w / np.float64(len(t))
                    for x in t:
                        rc[x] = rc[x] + term
                else:
                    s = np.float64(0.0)
                    for x in t:
                        s = s + ab[x]
                    for x in t:
                        rc[x] = rc[x] + (w * ab[x]) / s
            out.append(np.array(rc, dtype=np.float64))
    return np.array(out, dtype=np.float64).reshape(-1, n_nodes)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _case(lists, weight, n_nodes, abund, init):
    a_begin = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.uint64)
    a_target = np.concatenate([np.asarray(t, dtype=np.uint32) for t in lists] + [np.zeros(0, dtype=np.uint32)]).astype(np.uint32)
    abund = np.asarray(abund, dtype=np.float64).reshape(-1, n_nodes)
    a_begin, a_target, weight, abund = _frozen(a_begin, a_target, np.asarray(weight, dtype=np.float64), abund)
    return a_begin, a_target, weight, n_nodes, abund, init


def slot_pos(a_target, n_nodes):
    """slot -> position of its term in the node-major order (what quant_csr_finish computes)"""
    order = np.argsort(a_target, kind="stable")
    pos = np.empty(len(a_target), dtype=np.int64)
    pos[order] = np.arange(len(a_target))
    return pos


def grid_silent(n_nodes):
    """the nodes of a grid case that receive no term: a tenth of them (rounded up), never node 0 or the last one - which leaves
    none to choose from below three nodes"""
    if n_nodes < 3:
        return np.zeros(0, dtype=np.int64)
    rng = np.random.default_rng(n_nodes)
    return np.sort(rng.choice(np.arange(1, n_nodes - 1), size=-(-n_nodes // 10), replace=False))


@functools.lru_cache(maxsize=None)
def grid(n_nodes, n_slots):
    """lists of 1..6 targets that use n_slots slots in all; node 0 and node n_nodes - 1 both occur as soon as there are two slots
    (the single slot of n_slots = 1 is the last node: the tail lane); grid_silent(n_nodes) never occurs.  The init round and one round."""
    rng = np.random.default_rng(1000 * n_nodes + n_slots)
    allowed = np.setdiff1d(np.arange(n_nodes), grid_silent(n_nodes))
    targets = allowed[rng.integers(0, len(allowed), size=n_slots)]
    if n_slots >= 1:
        targets[rng.integers(0, n_slots)] = n_nodes - 1
    if n_slots >= 2:
        free = np.nonzero(targets != n_nodes - 1)[0] if n_nodes > 1 else np.arange(n_slots)
        targets[free[rng.integers(0, len(free))]] = 0
        assert (targets == 0).any() and (targets == n_nodes - 1).any()
    lists, at = [], 0
    while at < n_slots:
        k = min(int(rng.integers(1, 7)), n_slots - at)
        lists.append(targets[at:at + k]); at += k
    weight = rng.integers(1, 1 << 30, size=len(lists)) / float(1 << 22)       # what the coalesce hands over: units of 2^-22
    abund = rng.random(n_nodes) + 2.0 ** -30
    return _case(lists, weight, n_nodes, abund, True)


@functools.lru_cache(maxsize=None)
def order():
    """node 150 of 301 receives 100 000 terms whose magnitudes span 2^-60 .. 2^20 (the weights do; abund lies in [0.5, 1), so a
    term is its weight times a ratio in (1/6, 1]); the other 300 nodes share the remaining slots.  The assignments come in random
    order, so consecutive slots of one node are far apart in the slot order"""
    rng = np.random.default_rng(150)
    n_nodes, hot, n = 301, 150, 100000
    others = np.array([v for v in range(n_nodes) if v != hot])
    lists = []
    for i in range(n):
        k = int(rng.integers(1, 4))
        t = others[rng.integers(0, 300, size=k)]
        t[rng.integers(0, k)] = hot
        lists.append(t)
    weight = np.ldexp(1.0 + rng.random(n), rng.integers(-60, 20, size=n).astype(np.int32))
    weight[:2] = [2.0 ** -60, 2.0 ** 20]
    perm = rng.permutation(n)
    lists, weight = [lists[i] for i in perm], weight[perm]
    abund = 0.5 + rng.random(n_nodes) / 2
    return _case(lists, weight, n_nodes, abund, False)


@functools.lru_cache(maxsize=None)
def long_lists():
    """one assignment of 5000 targets over 40 of 300 nodes (every one of them repeats), beside assignments of 1, 2, 63, 64, 65"""
    rng = np.random.default_rng(5000)
    n_nodes = 300
    forty = rng.choice(n_nodes, size=40, replace=False)
    big = forty[rng.integers(0, 40, size=5000)]
    big[:40] = forty
    lists = [rng.integers(0, n_nodes, size=k) for k in (1, 2, 63)] + [big] + [rng.integers(0, n_nodes, size=k) for k in (64, 65, 1, 2)]
    weight = rng.integers(1, 1 << 30, size=len(lists)) / float(1 << 22)
    abund = rng.random((2, n_nodes)) + 2.0 ** -30
    return _case(lists, weight, n_nodes, abund, True)


def _by_exponent(rng, lo, hi, size):
    """random mantissa in [1, 2) times 2^e, e uniform over [lo, hi]; below -1022 the value is a denormal (never 0: 2^-1074 at least)"""
    v = np.ldexp(1.0 + rng.random(size), rng.integers(lo, hi + 1, size=size).astype(np.int32))
    assert (v > 0).all() and np.isfinite(v).all()
    return v


@functools.lru_cache(maxsize=None)
def value_range():
    """600 nodes.  abund of nodes 0..199 is drawn by exponent over [-1074, -1023]: denormals only; of nodes 200..599 over [-1074, 0],
    nodes 200..209 pinned to [0.5, 1).  Weights 2^-22 .. 2^40 (a power of two times a random mantissa).  Lists of 1..6 targets:
    200 of denormals alone, 200 of one normal (200..209) among denormals, 600 of anything, and 50 with the weight 2^-22 whose first
    target is node 200..209 and whose others are the denormals 100..149 - their terms come out denormal or 0, and nodes 100..149 stand
    in no other list, so their results are sums of denormals.  abund <= 1 (strictly below 2) and
    at most 6 targets: a sum stays below 12, a term below 2^41 - nothing overflows"""
    rng = np.random.default_rng(1074)
    n_nodes = 600
    abund = np.concatenate([_by_exponent(rng, -1074, -1023, 200), _by_exponent(rng, -1074, 0, 400)])
    abund[200:210] = 0.5 + rng.random(10) / 2
    abund[200] = 1.0
    abund[0], abund[1] = 2.0 ** -1074, 2.0 ** -1023 * (2 - 2.0 ** -51)        # the smallest and the largest denormal
    lists, weight = [], []

    def w(n, lo=-22, hi=40):
        return np.ldexp(1.0 + rng.random(n), rng.integers(lo, hi, size=n).astype(np.int32)).tolist()
    low = np.concatenate([np.arange(0, 100), np.arange(150, 200)])             # denormals other than 100..149
    for _ in range(200):
        lists.append(low[rng.integers(0, len(low), size=int(rng.integers(1, 7)))])
    weight += w(200)
    for _ in range(200):
        t = low[rng.integers(0, len(low), size=int(rng.integers(2, 7)))]
        t[rng.integers(0, len(t))] = 200 + int(rng.integers(0, 10))
        lists.append(t)
    weight += w(200)
    for _ in range(600):
        t = rng.integers(0, n_nodes, size=int(rng.integers(1, 7)))
        lists.append(np.where((t >= 100) & (t < 150), t + 50, t))
    weight += w(600)
    for _ in range(50):
        t = 100 + rng.integers(0, 50, size=int(rng.integers(2, 7)))
        t[0] = 200 + int(rng.integers(0, 10))
        lists.append(t)
    weight += [2.0 ** -22] * 50
    perm = rng.permutation(len(lists))
    return _case([lists[i] for i in perm], np.array(weight)[perm], n_nodes, abund, False)


ZERO_NODES = (3, 77, 299)


@functools.lru_cache(maxsize=None)
def zero_sum():
    """300 nodes of which ZERO_NODES have abund == 0.  One list holds these three alone: its sum is 0 and its three terms are 0 / 0.
    They also stand in lists with positive sums, where their terms are 0"""
    rng = np.random.default_rng(299)
    n_nodes = 300
    abund = rng.random(n_nodes) + 2.0 ** -30
    abund[list(ZERO_NODES)] = 0.0
    lists = [rng.integers(0, n_nodes, size=int(rng.integers(1, 7))) for _ in range(400)]
    lists = [t for t in lists if abund[t].sum() > 0]
    lists.insert(123, np.array(ZERO_NODES))
    lists.append(np.array([ZERO_NODES[0], 5, ZERO_NODES[2]]))
    weight = rng.integers(1, 1 << 30, size=len(lists)) / float(1 << 22)
    return _case(lists, weight, n_nodes, abund, False)


@functools.lru_cache(maxsize=None)
def reuse():
    """the init round and three different abundance vectors through one E-step object: 700 nodes, 3000 lists"""
    rng = np.random.default_rng(3)
    n_nodes = 700
    lists = [rng.integers(0, n_nodes, size=int(rng.integers(1, 7))) for _ in range(3000)]
    weight = rng.integers(1, 1 << 30, size=len(lists)) / float(1 << 22)
    abund = np.stack([rng.random(n_nodes) + 2.0 ** -30, _by_exponent(rng, -40, 0, n_nodes), rng.random(n_nodes) ** 8 + 2.0 ** -200])
    return _case(lists, weight, n_nodes, abund, True)


NAMED = {"order": order, "long_lists": long_lists, "value_range": value_range, "zero_sum": zero_sum, "reuse": reuse}


@functools.lru_cache(maxsize=None)
def want(name, *args):
    """the yardstick of a case, computed once"""
    case = grid(*args) if name == "grid" else NAMED[name]()
    out = restate(*case)
    out.setflags(write=False)
    return out


def get(name, *args):
    return grid(*args) if name == "grid" else NAMED[name]()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, ref, what, nan_ok=False):
    """bit for bit; nan_ok: where ref is NaN got must be NaN (the sign and payload of a default NaN are the platform's), and nowhere else"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    got, ref = got.ravel(), ref.ravel()
    if nan_ok:
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN at {np.nonzero(np.isnan(got))}, expected at {np.nonzero(np.isnan(ref))}"
        keep = ~np.isnan(ref)
        got, ref = got[keep], ref[keep]
    else:
        assert not np.isnan(ref).any(), what
    bad = np.nonzero(bits(got) != bits(ref))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {ref.size} values differ, first at {bad[0]}: {float(got[bad[0]]).hex()} != {float(ref[bad[0]]).hex()}"
