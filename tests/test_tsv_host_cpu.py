"""The batch formatter's host twin (cfr_tsv_open with device = -1) against cfr_format_tsv read after read: text and row_offsets, the
capacity rule and every argument refusal - the semantics stated in csrc/cfr_tsv_core.hpp.  Sequence names come from the f6 golden
index, the 811-node taxonomy (every rank the strings cover) from tests/golden/quant_wide.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import tsv_cases as tc
from centrifuger_amd import capi


@pytest.fixture(scope="module")
def indexes(tmp_path_factory):
    f6 = capi.Index(tc.F6)
    hy = capi.Index(tc.hybrid_prefix(str(tmp_path_factory.mktemp("hy"))))
    assert f6.info().seq_cnt > 0 and hy.info().node_cnt == 811
    yield f6, hy
    hy.close()
    f6.close()


@pytest.fixture(scope="module")
def edge(indexes):
    """(index, results, matches, ids, text, row_offsets) for both indexes: the reference is computed once"""
    out = []
    for idx in indexes:
        info = idx.info()
        res, mat, ids = tc.edge_batch(info.seq_cnt, info.node_cnt)
        out.append((idx, res, mat, ids) + tc.reference(idx, res, mat, ids))
    return out


def test_the_cases_cover_what_they_claim(edge):
    _idx, res, mat, ids, text, _off = edge[0]
    assert set(tc.N_MATCHES) <= set(res["n_match"].tolist()) and set(tc.ID_LENGTHS) <= {len(i) for i in ids}
    assert {0, 1} <= set(mat["kind"].tolist())
    assert len(tc.U64_EDGES) == 40 and str((1 << 64) - 1).encode() in text and b"-2147483648" in text and b"\t2147483647\t" in text
    assert b"out_seq\t\t7\t" in text and b"out_node\tno rank\t7\t" in text
    assert b"neg\tunclassified\t0\t0\t0\t0\t77\t1\n" in text


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("threads", [1, 3])
def test_host_twin_equals_format_tsv(edge, which, threads):
    idx, res, mat, ids, want, want_off = edge[which]
    t = capi.Tsv(idx, device=None, threads=threads)
    text, off = t.format(res, mat, ids, cap=len(want))
    assert text == want
    assert np.array_equal(off, want_off)
    st = t.stats()
    assert st.blocks == 0 and st.direct_blocks == 0
    t.close()


def test_the_ranks_of_the_wide_taxonomy_print_as_format_tsv_prints_them(indexes):
    _f6, hy = indexes
    b = tc.Batch()
    for node in range(812):                       # every node, and the one behind the last
        b.add(b"r%d" % node, [(node, node, 1)], score=node)
    res, mat, ids = b.arrays()
    want, want_off = tc.reference(hy, res, mat, ids)
    assert len({w.split(b"\t")[1] for w in want.split(b"\n") if w}) >= 4          # no rank, genus, species, strain
    t = capi.Tsv(hy, device=None)
    text, off = t.format(res, mat, ids)
    assert text == want and np.array_equal(off, want_off)


def test_n_0_and_1(indexes):
    f6, _hy = indexes
    t = capi.Tsv(f6, device=None, threads=3)
    res, mat, ids = tc.Batch().arrays()
    text, off = t.format(res, mat, ids, cap=0)
    assert text == b"" and off.tolist() == [0]
    b = tc.Batch()
    b.add(b"only", [(0, 5, 0)], score=3, qlen=9)
    res, mat, ids = b.arrays()
    text, off = t.format(res, mat, ids)
    assert text == f6.format_tsv("only", res[0], mat) and off.tolist() == [0, len(text)]


def test_capacity(edge):
    idx, res, mat, ids, want, want_off = edge[0]
    t = capi.Tsv(idx, device=None, threads=3)
    idb, ido = capi.pack_ids(ids)
    status, ln, _text, _off = t.format_raw(res, mat, idb, ido, len(want) - 1)
    assert status == capi.CFR_ERR_CAPACITY and ln == len(want)
    status, ln, text, off = t.format_raw(res, mat, idb, ido, len(want))
    assert status == capi.CFR_OK and ln == len(want) and text[:ln].tobytes() == want and np.array_equal(off, want_off)
    # no NUL is appended: a buffer with room to spare keeps what it held behind the text
    L = capi.lib()
    buf = np.full(len(want) + 8, 0x55, dtype=np.uint8)
    n = C.c_uint64(0)
    assert L.cfr_tsv_format(t._h, capi._p(res), capi._p(mat), C.c_size_t(len(mat)), C.c_size_t(len(res)), capi._p(idb), capi._p(ido), capi._p(buf),
                            C.c_uint64(len(buf)), C.byref(n), None) == capi.CFR_OK
    assert n.value == len(want) and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0x55).all()


def test_argument_refusals(indexes):
    f6, _hy = indexes
    L = capi.lib()
    t = capi.Tsv(f6, device=None)
    b = tc.Batch()
    for k in range(4):
        b.add(b"id%d" % k, [(0, 1, 0)] * 2)
    res, mat, ids = b.arrays()
    idb, ido = capi.pack_ids(ids)
    text = np.zeros(4096, dtype=np.uint8)
    n = C.c_uint64(0)

    def call(res=res, mat=mat, n_slots=len(mat), count=len(res), idb=idb, ido=ido, text=text, cap=4096, ln=n, handle=None):
        return L.cfr_tsv_format(t._h if handle is None else handle, capi._p(res), capi._p(mat), C.c_size_t(n_slots), C.c_size_t(count), capi._p(idb),
                                capi._p(ido), capi._p(text), C.c_uint64(cap), None if ln is None else C.byref(ln), None)

    assert call() == capi.CFR_OK
    assert call(res=None) == capi.CFR_ERR_ARG
    assert call(mat=None) == capi.CFR_ERR_ARG
    assert call(ido=None) == capi.CFR_ERR_ARG
    assert call(idb=None) == capi.CFR_ERR_ARG
    assert call(text=None) == capi.CFR_ERR_ARG
    assert call(ln=None) == capi.CFR_ERR_ARG
    assert call(handle=C.c_void_p(0)) == capi.CFR_ERR_ARG
    # the matches of read 2 end behind the slots: the message names the read
    assert call(n_slots=5) == capi.CFR_ERR_ARG and b"read 2" in L.cfr_last_error()
    bad = res.copy()
    bad["match_begin"][1] = (1 << 64) - 1                            # (no wrap-around in the check)
    assert call(res=bad) == capi.CFR_ERR_ARG and b"read 1" in L.cfr_last_error()
    bad = res.copy()
    bad["n_match"][3] = tc.INT32_MAX
    assert call(res=bad) == capi.CFR_ERR_ARG and b"read 3" in L.cfr_last_error()
    down = ido.copy()
    down[2] = down[1] - 1
    assert call(ido=down) == capi.CFR_ERR_ARG and b"read 1" in L.cfr_last_error()
    # a read without matches may point anywhere; no reads need no arrays
    free = res.copy()
    free["n_match"][1] = 0
    free["match_begin"][1] = 1 << 60
    assert call(res=free) == capi.CFR_OK
    assert call(res=None, mat=None, n_slots=0, count=0, idb=None, ido=np.zeros(1, dtype=np.uint64), text=None, cap=0) == capi.CFR_OK and n.value == 0
    raw = C.c_void_p(t._h.value)
    t.close()
    assert call(handle=raw) == capi.CFR_ERR_ARG                      # (a closed handle)
    L.cfr_tsv_close(raw)                                             # (a second close is ignored)
    # the options
    h = C.c_void_p()
    assert L.cfr_tsv_open(None, C.c_int(-1), None, C.byref(h)) == capi.CFR_ERR_ARG
    assert L.cfr_tsv_open(f6._h, C.c_int(-2), None, C.byref(h)) == capi.CFR_ERR_ARG
    o = capi.TsvOptions(-1, 0, 0, 0)
    assert L.cfr_tsv_open(f6._h, C.c_int(-1), C.byref(o), C.byref(h)) == capi.CFR_ERR_ARG
    assert L.cfr_tsv_open(f6._h, C.c_int(-1), None, C.byref(h)) == capi.CFR_OK and h.value
    assert L.cfr_tsv_get_stats(h, None) == capi.CFR_ERR_ARG
    L.cfr_tsv_close(h)
