"""The barcode whitelist on the device (csrc/cfr_barcode.hip: k_bc_build, k_bc_count, k_bc_correct) against the host twin
(cfr_barcode_correct_host / a host-only handle), status for status and byte for byte, and against the reference's own dumps of
tests/golden/barcode."""
import numpy as np
import pytest

import barcode_fixtures as bf
from centrifuger_amd import capi

pytestmark = pytest.mark.gpu

N_BARCODES = 50000
CASES = [(1, 1), (1, 3), (5, 3), (5, 1000), (16, 1), (16, 1000), (16, 200000), (31, 1000), (32, 3), (32, 200000)]


@pytest.fixture(scope="module")
def handles(tmp_path_factory):
    """(L, entries) -> (device handle, host handle), both after the same background pass; made once"""
    d = tmp_path_factory.mktemp("barcode")
    made = {}

    def get(L, n_entries):
        if (L, n_entries) not in made:
            wl = bf.random_whitelist(L, n_entries)
            path = str(d / f"wl_{L}_{n_entries}.txt")
            bf.write_whitelist(path, wl, repeats=min(5, len(wl)))
            dev, host = capi.Barcode(path, device=0), capi.Barcode(path, device=None)
            b, o, _, _ = bf.random_barcodes(L, n_entries, N_BARCODES)
            for h in (dev, host):
                h.count(b, o, max_records=20000)
            made[(L, n_entries)] = (dev, host, len(wl))
        return made[(L, n_entries)]
    return get


@pytest.mark.parametrize("L,n_entries", CASES)
def test_device_correct_equals_host_twin(handles, L, n_entries):
    dev, host, n_wl = handles(L, n_entries)
    st = dev.stats()
    assert st.on_device == 1 and st.barcode_length == L and st.whitelist_size == n_wl and st.table_slots >= 2 * n_wl
    b, o, q, n_other = bf.random_barcodes(L, n_entries, N_BARCODES)
    for qual in (q, None):
        s_dev, b_dev = dev.correct(b, o, qual, threads=4)
        assert dev.stats().host_barcodes == n_other          # exactly the barcodes whose length is not L went to the host twin
        assert dev.stats().device_ms > 0
        s_twin, b_twin = dev.correct_host(b, o, qual, threads=4)
        s_host, b_host = host.correct(b, o, qual, threads=4)
        assert np.array_equal(s_twin, s_host) and np.array_equal(b_twin, b_host)
        assert np.array_equal(s_dev, s_host)
        assert np.array_equal(b_dev, b_host)
        if n_entries >= 1000 and L >= 5:
            assert all(int((s_dev == v).sum()) >= 100 for v in (-1, 0, 1))


@pytest.mark.parametrize("L,n_entries", [(16, 1000), (32, 200000)])
def test_device_counts_equal_host_counts(handles, L, n_entries):
    dev, host, _ = handles(L, n_entries)
    e_dev, c_dev = dev.counts()
    e_host, c_host = host.counts()
    assert e_dev == e_host and np.array_equal(c_dev, c_host) and int(c_dev.sum()) > len(e_dev) + 5


@pytest.mark.parametrize("n", [0, 1, 65])
def test_small_batches(handles, n):
    dev, host, _ = handles(16, 1000)
    b, o, q, _ = bf.random_barcodes(16, 1000, N_BARCODES)
    o = o[:n + 1]
    b, q = b[:int(o[n])], q[:int(o[n])]
    s_dev, b_dev = dev.correct(b, o, q)
    s_host, b_host = host.correct(b, o, q)
    assert len(s_dev) == n and np.array_equal(s_dev, s_host) and np.array_equal(b_dev, b_host)


def test_call_buffers_regrow_and_the_qualities_follow(tmp_path):
    """One fresh device handle, four calls whose sizes make upload() regrow: 3 without qualities; 300 with (more than one 256-lane
    block, both size classes regrown, the first quality buffer allocated after a regrow); 3 with; 700 without."""
    wl = bf.random_whitelist(16, 1000)
    path = str(tmp_path / "wl.txt")
    bf.write_whitelist(path, wl)
    dev, host = capi.Barcode(path, device=0), capi.Barcode(path, device=None)
    assert dev.stats().on_device == 1
    b, o, q, _ = bf.random_barcodes(16, 1000, N_BARCODES)
    for n, with_qual in [(3, False), (300, True), (3, True), (700, False)]:
        on, bn = o[:n + 1], b[:int(o[n])]
        qn = q[:int(o[n])] if with_qual else None
        s_dev, b_dev = dev.correct(bn, on, qn)
        s_host, b_host = host.correct(bn, on, qn)
        assert len(s_dev) == n and np.array_equal(s_dev, s_host) and np.array_equal(b_dev, b_host)


def test_count_one_barcode_many_times_a_cap_and_two_calls(tmp_path):
    wl = bf.random_whitelist(16, 1000)
    path = str(tmp_path / "wl.txt")
    bf.write_whitelist(path, wl, repeats=3)
    dev, host = capi.Barcode(path, device=0), capi.Barcode(path, device=None)
    b, o = bf.flat([wl[10]] * 100000)
    for h in (dev, host):
        h.count(b, o)                                   # 100 000 atomic adds on one slot
        h.count(b, o, max_records=7)                    # a cap smaller than n; the second call adds to the first
    e, c = dev.counts()
    assert c[e.index(wl[10])] == 1 + 100007 and int(c.sum()) == len(wl) + 3 + 100007
    assert np.array_equal(c, host.counts()[1])
    # barcodes of another length in the background: the twin counts them, the device does not see them
    mixed, mo = bf.flat([wl[0], wl[1][:9], wl[2] + b"A", b"", wl[0][:15] + b"N"])
    for h in (dev, host):
        h.count(mixed, mo)
    assert dev.stats().host_barcodes == 3
    assert np.array_equal(dev.counts()[1], host.counts()[1])
    s_dev, b_dev = dev.correct(mixed, mo)
    s_host, b_host = host.correct(mixed, mo)
    assert s_dev.tolist() == s_host.tolist() == [0, 0, -1, 0, 1] and np.array_equal(b_dev, b_host)


@pytest.mark.parametrize("name", ["wl5", "wl16", "wlmix"])
def test_device_handle_equals_reference_dump(name):
    w = bf.manifest()["whitelists"][name]
    dev = capi.Barcode(bf.whitelist_path(name), device=0)
    st = dev.stats()
    assert st.on_device == (0 if name == "wlmix" else 1)      # mixed lengths: host results through the same handle
    dev.count(*bf.background(name), max_records=w["background_cap"])
    assert (dev.counts()[0], dev.counts()[1].tolist()) == bf.counts(name)
    _, b, o, q = bf.barcodes(name)
    sq, bq, sn, bn = bf.corrected(name)
    s, out = dev.correct(b, o, q, threads=2)
    assert s.tolist() == sq and bf.unflat(out, o) == bq
    L = st.barcode_length
    n_other = sum(1 for i in range(len(sq)) if int(o[i + 1] - o[i]) != L)
    assert dev.stats().host_barcodes == (len(sq) if name == "wlmix" else n_other)
    s, out = dev.correct(b, o, None, threads=2)
    assert s.tolist() == sn and bf.unflat(out, o) == bn


def test_all_t_at_32_is_a_key_like_any_other(tmp_path):
    path = str(tmp_path / "wl.txt")
    bf.write_whitelist(path, [b"T" * 32, b"A" * 32, b"T" * 31 + b"G"])
    dev = capi.Barcode(path, device=0)
    s, out = dev.correct(*bf.flat([b"T" * 32, b"A" * 32, b"T" * 31 + b"C", b"A" * 31 + b"C", b"C" * 32, b"N" + b"T" * 31]))
    assert s.tolist() == [0, 0, 1, 1, -1, 1]
    assert bf.unflat(out, np.arange(0, 193, 32)) == [b"T" * 32, b"A" * 32, b"T" * 31 + b"G", b"A" * 32, b"C" * 32, b"T" * 32]   # G before T among equal counts
