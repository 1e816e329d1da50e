"""The batch formatter on the device (csrc/cfr_tsv.hip) against its host twin - text and row_offsets - at the block and wave edges, on
both paths of k_tsv_write (a span staged in LDS, a span written straight to HBM) and at every alignment of a span; and inside the
classifier: cfr_device_index_set_tsv / _tsv_last / _tsv_last_resident against cfr_format_tsv over the results the same call returned.
The twin itself is pinned to cfr_format_tsv by tests/test_tsv_host_cpu.py."""
import gzip
import os

import numpy as np
import pytest

import oracle_lib as ora
import quant_fixtures as qf
import tsv_cases as tc
from centrifuger_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def idx():
    i = capi.Index(tc.F6)
    yield i
    i.close()


@pytest.fixture(scope="module")
def handles(idx):
    host, dev = capi.Tsv(idx, device=None, threads=3), capi.Tsv(idx, device=0)
    yield host, dev
    dev.close()
    host.close()


def _same(host, dev, res, mat, ids):
    want, want_off = host.format(res, mat, ids)
    got, got_off = dev.format(res, mat, ids, cap=len(want))
    assert got == want
    assert np.array_equal(got_off, want_off)
    return want_off, dev.stats()


def _counts(idx):
    info = idx.info()
    return info.seq_cnt, info.node_cnt


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_device_equals_host_twin_at_the_wave_and_block_edges(idx, handles, n):
    res, mat, ids = tc.random_batch(n, *_counts(idx), seed=n)
    _off, st = _same(*handles, res, mat, ids)
    assert st.blocks == (n + 255) // 256 and st.direct_blocks == 0


def test_the_edge_cases_of_the_host_test(idx, handles):
    res, mat, ids = tc.edge_batch(*_counts(idx))
    _same(*handles, res, mat, ids)


def test_stride_loops(idx, handles):
    host, _dev = handles
    dev = capi.Tsv(idx, device=0, max_blocks=2)
    res, mat, ids = tc.random_batch(3000, *_counts(idx), seed=3000, stride=5)         # (the classifier's layout: unused slots between the reads)
    _off, st = _same(host, dev, res, mat, ids)
    assert st.blocks == 12
    dev.close()


def test_a_span_of_exactly_the_tile_one_less_and_one_more(idx, handles):
    host, _dev = handles
    res, mat, ids = tc.random_batch(256, *_counts(idx), seed=11)
    _text, off = host.format(res, mat, ids)
    span = int(off[256])
    for tile, direct in ((span, 0), (span + 1, 0), (span - 1, 1)):                    # span == tile, tile - 1, tile + 1
        dev = capi.Tsv(idx, device=0, tile_bytes=tile)
        _off, st = _same(host, dev, res, mat, ids)
        assert st.blocks == 1 and st.direct_blocks == direct, (tile, span)
        dev.close()


def test_a_direct_block_between_two_staged_ones(idx, handles):
    host, _dev = handles
    seq_cnt, node_cnt = _counts(idx)
    a = tc.random_batch(256, seq_cnt, node_cnt, seed=21, id_len=(0, 8))
    b = tc.random_batch(256, seq_cnt, node_cnt, seed=22, id_len=(40, 60))
    c = tc.random_batch(200, seq_cnt, node_cnt, seed=23, id_len=(0, 8))
    res = np.concatenate([a[0], b[0], c[0]])
    res["match_begin"][256:512] += len(a[1])
    res["match_begin"][512:] += len(a[1]) + len(b[1])
    mat = np.concatenate([a[1], b[1], c[1]])
    ids = a[2] + b[2] + c[2]
    _text, off = host.format(res, mat, ids)
    spans = [int(off[256] - off[0]), int(off[512] - off[256]), int(off[712] - off[512])]
    tile = max(spans[0], spans[2])
    assert tile < spans[1]
    dev = capi.Tsv(idx, device=0, tile_bytes=tile)
    _off, st = _same(host, dev, res, mat, ids)
    assert st.blocks == 3 and 0 < st.direct_blocks < st.blocks and st.direct_blocks == 1
    dev.close()


def test_long_reads_take_the_direct_path_with_the_default_tile(idx, handles):
    """reads of 64 matches with 300-byte ids among short ones: their block's span is longer than the default tile"""
    seq_cnt, node_cnt = _counts(idx)
    rng = np.random.default_rng(31)
    b = tc.Batch()
    for i in range(600):
        if 300 <= i < 305:
            b.add(tc.read_id(rng, 300), [(int(rng.integers(0, seq_cnt)), 1000 + k, k & 1) for k in range(64)], score=12345, second=77, hit=150, qlen=151)
        else:
            b.add(tc.read_id(rng, 6), [(0, 9, 0)] * int(rng.integers(0, 3)), score=int(rng.integers(0, 99999)), qlen=151)
    res, mat, ids = b.arrays()
    off, st = _same(*handles, res, mat, ids)
    assert int(off[512] - off[256]) > 80 * 1024 and st.blocks == 3 and st.direct_blocks == 1


def test_spans_at_every_alignment(idx, handles):
    """an id of 0..15 bytes in front moves the start of every later span through the residues modulo 16"""
    seq_cnt, node_cnt = _counts(idx)
    res, mat, ids = tc.random_batch(600, seq_cnt, node_cnt, seed=41)
    starts, ends = set(), set()
    for L in range(16):
        ids[0] = b"x" * L
        off, st = _same(*handles, res, mat, ids)
        starts.add(int(off[256]) % 16)
        ends.add(int(off[512]) % 16)
        assert st.direct_blocks == 0
    assert starts == set(range(16)) and ends == set(range(16))


def test_buffers_grow_on_the_same_handle(idx):
    host, dev = capi.Tsv(idx, device=None), capi.Tsv(idx, device=0)
    seq_cnt, node_cnt = _counts(idx)
    for n, id_len in ((10, (0, 4)), (5000, (30, 60)), (20, (0, 4))):
        _same(host, dev, *tc.random_batch(n, seq_cnt, node_cnt, seed=n, id_len=id_len))
    # the capacity rule on the device: len is set, and the next call is sound
    res, mat, ids = tc.random_batch(100, seq_cnt, node_cnt, seed=7)
    want, _ = host.format(res, mat, ids)
    idb, ido = capi.pack_ids(ids)
    status, ln, _t, _o = dev.format_raw(res, mat, idb, ido, len(want) - 1)
    assert status == capi.CFR_ERR_CAPACITY and ln == len(want)
    status, ln, text, _o = dev.format_raw(res, mat, idb, ido, len(want))
    assert status == capi.CFR_OK and text[:ln].tobytes() == want
    bad = res.copy()
    bad["match_begin"][5] = len(mat)
    bad["n_match"][5] = 1
    status, _ln, _t, _o = dev.format_raw(bad, mat, idb, ido, len(want) + 100)
    assert status == capi.CFR_ERR_ARG and b"read 5" in capi.lib().cfr_last_error()      # refused on the host: nothing was launched
    dev.close()
    host.close()


def test_no_device_is_an_error_not_a_fallback(idx):
    with pytest.raises(capi.CfrError) as e:
        capi.Tsv(idx, device=capi.device_count() + 7)
    assert e.value.status == capi.CFR_ERR_NO_DEVICE


# ---- inside the classifier ----
@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsv_reads")
    for f in ("reads_1.fq", "reads_2.fq"):
        (d / f).write_bytes(gzip.open(os.path.join(qf.QDIR, f + ".gz"), "rb").read())
    return d


def _rows(idx, ids, res, mat):
    return b"".join(idx.format_tsv(ids[i], res[i], mat) for i in range(len(res)))


def test_rows_inside_classify_batch(reads):
    """q8 on the device with sub-batches of 64 reads, 200 pairs (four sub-batches), -k 5: the shape of test_report_inside_classify_batch"""
    idx = capi.Index(qf.PREFIX, capi.default_params(max_result=5))
    dev = capi.DeviceIndex(idx, 0, capi.default_device_options(sub_batch=64))
    ids, b1, o1 = ora.read_fastx(str(reads / "reads_1.fq"))
    _, b2, o2 = ora.read_fastx(str(reads / "reads_2.fq"))
    n = 200
    ids = ids[:n]
    o1, o2 = o1[:n + 1].copy(), o2[:n + 1].copy()
    inputs = (b1[:int(o1[n])].copy(), o1, b2[:int(o2[n])].copy(), o2)
    res0, mat0 = dev.classify(*inputs)
    res0, mat0 = res0.copy(), mat0.copy()
    want = _rows(idx, ids, res0, mat0)
    assert int((res0["n_match"] > 1).sum()) > 0 and int((res0["n_match"] == 0).sum()) > 0
    # switched off: nothing ran, and there is nothing to format
    assert dev.last_tsv_ms() == 0
    with pytest.raises(capi.CfrError) as e:
        dev.tsv_last(ids)
    assert e.value.status == capi.CFR_ERR_ARG
    dev.set_tsv(True)
    with pytest.raises(capi.CfrError) as e:                                          # on, but no call has kept anything yet
        dev.tsv_last(ids)
    assert e.value.status == capi.CFR_ERR_ARG
    res, mat = dev.classify(*inputs)
    assert np.array_equal(res, res0)                                                 # the host copies are delivered as before
    text, off = dev.tsv_last(ids, want_offsets=True)
    assert text == _rows(idx, ids, res, mat) == want
    assert int(off[n]) == len(want) and int(off[1]) == len(idx.format_tsv(ids[0], res[0], mat))
    assert dev.last_tsv_ms() > 0
    assert dev.tsv_last(ids, cap=len(want)) == want                                  # again, from the same kept arrays
    # the same after submit / wait
    res, mat = dev.wait(dev.submit(*inputs))
    assert dev.tsv_last(ids) == _rows(idx, ids, res, mat) == want
    # under promotion the rows are the promoted ones
    dev.set_promote("genus")
    res, mat = dev.classify(*inputs)
    res, mat = res.copy(), mat.copy()
    promoted = dev.tsv_last(ids)
    dev.set_promote(None)
    assert not np.array_equal(res["n_match"], res0["n_match"])
    assert promoted == _rows(idx, ids, res, mat) and promoted != want
    # the compact entry refuses while the switch is on
    import torch
    tb = torch.from_numpy(inputs[0]).cuda()
    to = torch.from_numpy(o1.view(np.int64)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(capi.CfrError) as e:
        dev.classify_resident_compact(tb.data_ptr(), to.data_ptr(), n, int(o1[n]))
    assert e.value.status == capi.CFR_ERR_ARG and "cfr_device_index_set_tsv" in str(e.value)
    # off again: the next call keeps nothing
    dev.set_tsv(False)
    dev.classify(*inputs)
    assert dev.last_tsv_ms() == 0
    with pytest.raises(capi.CfrError) as e:
        dev.tsv_last(ids)
    assert e.value.status == capi.CFR_ERR_ARG
    assert len(dev.classify_resident_compact(tb.data_ptr(), to.data_ptr(), n, int(o1[n]))[0]) == n
    dev.close()
    idx.close()
    L = capi.lib()
    assert L.cfr_device_index_set_tsv(None, 1) == capi.CFR_ERR_ARG and L.cfr_last_tsv_ms(None, None) == capi.CFR_ERR_ARG


def test_ids_from_the_tokenisers_tables(reads):
    """tsv_last_resident takes the ids from the tokenised text in HBM: the same rows as with host ids"""
    idx = capi.Index(qf.PREFIX, capi.default_params(max_result=5))
    dev = capi.DeviceIndex(idx, 0, capi.default_device_options(sub_batch=64))
    tok1, tok2 = capi.Tokenizer(0), capi.Tokenizer(0)
    try:
        n = 200
        t1, t2 = ((reads / f).read_bytes() for f in ("reads_1.fq", "reads_2.fq"))
        i1, i2 = tok1.tokenize(t1, max_records=n), tok2.tokenize(t2, max_records=n)
        assert i1.n_records == i2.n_records == n
        rec, _o, _b = tok1.fetch()
        ids = capi.Tokenizer.ids(t1, rec)
        (d_b1, d_o1), (d_b2, d_o2) = tok1.device_reads(), tok2.device_reads()
        dev.set_tsv(True)
        res, mat = dev.classify_resident(d_b1, d_o1, n, i1.total_bases, d_b2, d_o2, i2.total_bases)
        want = _rows(idx, ids, res, mat)
        assert dev.tsv_last(ids) == want
        d_text, d_rec = tok1.device_records()
        text, off = dev.tsv_last_resident(d_text, d_rec, n, want_offsets=True)
        assert text == want and int(off[n]) == len(want)
        host = capi.Tokenizer(None)
        host.tokenize(t1, max_records=4)
        with pytest.raises(capi.CfrError) as e:
            host.device_records()
        assert e.value.status == capi.CFR_ERR_ARG
        host.close()
    finally:
        tok1.close()
        tok2.close()
        dev.close()
        idx.close()
