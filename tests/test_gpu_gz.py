"""The device compressor and the device read dumps (csrc/cfr_gz.hip) against their host twin (csrc/cfr_gz.cpp), byte for byte, over the
texts and dumps of tests/gz_cases.py and both block sizes; the twin itself is checked with zlib in tests/test_gz_host_cpu.py.  The
twin's outputs are made once per module."""
import gzip

import pytest

import gz_cases as gc
from centrifuger_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    hs = {bb: (capi.Gz(device=0, block_bytes=bb), capi.Gz(block_bytes=bb, threads=4)) for bb in gc.BLOCKS}
    yield hs
    for d, h in hs.values():
        d.close()
        h.close()


def _counts(st):
    return (st.blocks, st.stored_blocks, st.bytes_in, st.bytes_out)


@pytest.mark.parametrize("block_bytes", gc.BLOCKS)
@pytest.mark.parametrize("name", list(gc.texts(65280)))
def test_compress_equals_the_host_twin(handles, name, block_bytes):
    dev, host = handles[block_bytes]
    text = gc.texts(block_bytes)[name]
    want = host.compress(text)
    got = dev.compress(text)
    assert got == want
    assert _counts(dev.stats()) == _counts(host.stats())
    assert gzip.decompress(got + capi.gz_eof()) == text


@pytest.mark.parametrize("block_bytes", gc.BLOCKS)
@pytest.mark.parametrize("name", list(gc.dump_cases()))
def test_dump_equals_the_host_twin(handles, name, block_bytes):
    dev, host = handles[block_bytes]
    ids, select, files = gc.dump_cases()[name]
    want = host.dump(ids, select, files)
    got = dev.dump(ids, select, files)
    assert got == want
    assert _counts(dev.stats()) == _counts(host.stats())
    for g, w in zip(got, gc.dump_expected(ids, select, files)):
        assert gzip.decompress(g + capi.gz_eof()) == w


def test_open_and_close_without_a_call():
    g = capi.Gz(device=0)
    st = g.stats()
    assert _counts(st) == (0, 0, 0, 0)
    g.close()
    g.close()


def test_second_text_shorter_than_the_first(handles):
    dev, host = handles[65280]
    long_, short = gc.texts(65280)["fastq_1mb"], gc.texts(65280)["all_bytes_x300"]
    assert dev.compress(long_) == host.compress(long_)
    assert dev.compress(short) == host.compress(short)
    assert dev.compress(b"") == b"" and _counts(dev.stats()) == (0, 0, 0, 0)
    assert dev.compress(short[:3]) == host.compress(short[:3])


def test_workgroups_that_stride_over_the_blocks_give_the_same_bytes(handles):
    """max_blocks = 3: every workgroup encodes several blocks in turn in the same LDS, and several reads' records in turn"""
    few = capi.Gz(device=0, block_bytes=251, max_blocks=3)
    _, host = handles[251]
    for name in ("fastq_1mb", "random_200k"):
        text = gc.texts(251)[name][:60000]
        assert few.compress(text) == host.compress(text)
    ids, select, files = gc.dump_cases()["select_alternating"]
    assert few.dump(ids, select, files) == host.dump(ids, select, files)
    few.close()


def test_no_such_device_is_an_error_not_a_fall_back():
    with pytest.raises(capi.CfrError) as e:
        capi.Gz(device=1000)
    assert e.value.status == capi.CFR_ERR_NO_DEVICE
