"""Dynamic mode of the device compressor (k_gzd_encode in csrc/cfr_gz.hip, capi.Gz(device=0, codes="dynamic")) against its host twin,
byte for byte and in the counts of its stats, over the texts of tests/gz_dyn_cases.py, the dumps of tests/gz_cases.py and both block
sizes; the twin itself is checked with zlib and a parser of the dynamic header in tests/test_gz_dyn_host_cpu.py."""
import gzip

import pytest

import gz_cases as gc
import gz_dyn_cases as gd
from centrifuger_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    hs = {bb: (capi.Gz(device=0, block_bytes=bb, codes="dynamic"), capi.Gz(block_bytes=bb, threads=4, codes="dynamic")) for bb in gd.BLOCKS}
    yield hs
    for d, h in hs.values():
        d.close()
        h.close()


def _counts(st):
    return (st.blocks, st.stored_blocks, st.dynamic_blocks, st.bytes_in, st.bytes_out)


@pytest.mark.parametrize("block_bytes", gd.BLOCKS)
@pytest.mark.parametrize("name", list(gd.texts(65280)))
def test_compress_equals_the_host_twin(handles, name, block_bytes):
    dev, host = handles[block_bytes]
    text = gd.texts(block_bytes)[name]
    want = host.compress(text)
    got = dev.compress(text)
    assert got == want
    assert _counts(dev.stats()) == _counts(host.stats())
    assert gzip.decompress(got + capi.gz_eof()) == text


@pytest.mark.parametrize("block_bytes", gd.BLOCKS)
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


def test_dynamic_members_come_from_the_device(handles):
    dev, _ = handles[65280]
    out = dev.compress(gd.texts(65280)["fastq_1mb"])
    st = dev.stats()
    assert st.dynamic_blocks == st.blocks == 15 and all((m[1][0] >> 1) & 3 == 2 for m in gc.walk(out))


def test_workgroups_that_stride_over_the_blocks_give_the_same_bytes(handles):
    """max_blocks = 3: every workgroup encodes several blocks in turn with the same histograms, tables, staging and token area"""
    few = capi.Gz(device=0, block_bytes=251, max_blocks=3, codes="dynamic")
    _, host = handles[251]
    for text in (gd.texts(251)["fastq_1mb"][:60000], gd.texts(251)["fibonacci_literals"]):
        assert few.compress(text) == host.compress(text)
        assert _counts(few.stats()) == _counts(host.stats())
    ids, select, files = gc.dump_cases()["select_alternating"]
    assert few.dump(ids, select, files) == host.dump(ids, select, files)
    few.close()


def test_second_text_shorter_than_the_first(handles):
    dev, host = handles[65280]
    long_, short = gd.texts(65280)["fastq_1mb"], gd.texts(65280)["all_bytes_x300"]
    assert dev.compress(long_) == host.compress(long_)
    assert dev.compress(short) == host.compress(short)
    assert dev.compress(b"") == b"" and _counts(dev.stats()) == (0, 0, 0, 0, 0)
    assert dev.compress(short[:3]) == host.compress(short[:3])


def test_a_fixed_and_a_dynamic_handle_side_by_side(handles):
    dyn, dyn_host = handles[65280]
    fixed, fixed_host = capi.Gz(device=0), capi.Gz(threads=4)
    for name in ("fastq_1mb", "acgt_40000_twice", "random_200k", "fastq_1mb"):
        text = gd.texts(65280)[name]
        assert fixed.compress(text) == fixed_host.compress(text) and fixed.stats().dynamic_blocks == 0
        assert dyn.compress(text) == dyn_host.compress(text)
    fixed.close()
    fixed_host.close()
