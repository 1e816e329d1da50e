"""The host twin of the block compressor and of the read dumps (csrc/cfr_gz.cpp through capi.Gz with device=None), checked with
Python's zlib / gzip: what the members inflate to, their framing, when a block is stored, and that the bytes do not depend on the
call or on the number of threads.  The record length at which a dump leaves a read out is pinned against zlib's gzprintf itself,
by a small C program that prints records of 8190 .. 8193 bytes the way ReadDump::put does.  No GPU."""
import gzip
import shutil
import subprocess

import numpy as np
import pytest

import gz_cases as gc
from centrifuger_amd import capi


@pytest.fixture(scope="module")
def twins():
    hs = {bb: capi.Gz(block_bytes=bb, threads=3) for bb in gc.BLOCKS}
    yield hs
    for h in hs.values():
        h.close()


def test_end_of_file_member_is_an_empty_gzip_file():
    eof = capi.gz_eof()
    assert len(eof) == 28 and gzip.decompress(eof) == b""
    assert gc.walk(eof) == [(28, b"\x03\x00", 0, 0)]


@pytest.mark.parametrize("block_bytes", gc.BLOCKS)
@pytest.mark.parametrize("name", list(gc.texts(65280)))
def test_members_inflate_to_the_text_and_are_framed(twins, name, block_bytes):
    text = gc.texts(block_bytes)[name]
    out = twins[block_bytes].compress(text)
    assert gzip.decompress(out + capi.gz_eof()) == text
    members, stored = gc.check_members(out, text, block_bytes)
    st = twins[block_bytes].stats()
    assert (st.blocks, st.stored_blocks, st.bytes_in, st.bytes_out) == (members, stored, len(text), len(out))
    if name == "empty":
        assert out == b""


def test_fastq_text_is_never_stored_and_shrinks(twins):
    text = gc.texts(65280)["fastq_1mb"]
    out = twins[65280].compress(text)
    assert twins[65280].stats().stored_blocks == 0 and len(out) < len(text)


@pytest.mark.parametrize("block_bytes", gc.BLOCKS)
def test_random_text_is_stored(twins, block_bytes):
    text = gc.texts(block_bytes)["random_200k"]
    out = twins[block_bytes].compress(text)
    st = twins[block_bytes].stats()
    assert st.stored_blocks == st.blocks == (len(text) + block_bytes - 1) // block_bytes
    assert len(out) == len(text) + 31 * st.blocks


def test_a_run_is_matched_in_pieces_of_258(twins):
    """1000 equal bytes: the first window is 64 literals; then matches of 258, 258, 258 and the remainder of 162, each against the last
    position of the window in front of its own: distances 1, 3, 5, 7.  Length 258 is 8 bits, 162 is 8 + 5; the distances take 5, 5,
    5 + 1, 5 + 1 bits: 3 + 512 + 13 + 13 + 14 + 19 + 7 bits"""
    out = twins[65280].compress(b"a" * 1000)
    assert len(gc.walk(out)[0][1]) == (3 + 512 + 13 + 13 + 14 + 19 + 7 + 7) // 8 == 73


@pytest.mark.parametrize("block_bytes", gc.BLOCKS)
def test_bytes_do_not_depend_on_the_call_or_the_threads(twins, block_bytes):
    one, seven = capi.Gz(block_bytes=block_bytes, threads=1), capi.Gz(block_bytes=block_bytes, threads=7)
    for name in ("fastq_1mb", "random_200k", "all_bytes_x300", "a_block_and_one"):
        text = gc.texts(block_bytes)[name]
        first = twins[block_bytes].compress(text)
        assert twins[block_bytes].compress(text) == first and one.compress(text) == first and seven.compress(text) == first
    one.close()
    seven.close()


@pytest.mark.parametrize("bad", [-1, 65281])
def test_block_bytes_outside_its_range_is_refused(bad):
    with pytest.raises(capi.CfrError):
        capi.Gz(block_bytes=bad)


@pytest.mark.parametrize("block_bytes", gc.BLOCKS)
@pytest.mark.parametrize("name", list(gc.dump_cases()))
def test_dump_inflates_to_the_records_python_builds(twins, name, block_bytes):
    ids, select, files = gc.dump_cases()[name]
    want = gc.dump_expected(ids, select, files)
    got = twins[block_bytes].dump(ids, select, files)
    assert len(got) == len(files)
    for g, w in zip(got, want):
        assert gzip.decompress(g + capi.gz_eof()) == w
        gc.check_members(g, w, block_bytes)
    st = twins[block_bytes].stats()
    assert st.bytes_in == sum(len(w) for w in want) and st.bytes_out == sum(len(g) for g in got)


def test_dump_drops_a_long_record_from_its_own_file_only():
    ids, select, files = gc.dump_cases()["drop_rule"]
    t1, t2 = gc.dump_expected(ids, select, files)
    in1 = [b"@" + i + b"\n" in t1 for i in ids]
    in2 = [b">" + i + b"\n" in t2 for i in ids]
    assert in1 == [True, True, True, False, False, True, True, False]
    assert in2 == [True, False, False, True, True, False, False, True]


def test_dump_refuses_offsets_that_decrease():
    g = capi.Gz()
    n = 3
    idb, ido = capi.pack_strings([b"a", b"b", b"c"])
    sb, so = capi.pack_strings([b"AC", b"GT", b"AA"])
    so[2] = 1
    f = (capi.GzFile * 1)()
    f[0].seq, f[0].seq_off = sb.ctypes.data, so.ctypes.data
    out, out_n = (capi.C.POINTER(capi.C.c_uint8) * 1)(), (capi.C.c_uint64 * 1)()
    sel = np.ones(n, dtype=np.uint8)
    status = capi.lib().cfr_gz_dump(g._h, capi._p(idb), capi._p(ido), capi._p(sel), capi.C.c_size_t(n), f, capi.C.c_int(1), out, out_n)
    assert status == capi.CFR_ERR_ARG and b"decrease at read 1" in capi.lib().cfr_last_error()
    g.close()


GZPRINTF_PROBE = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
/* records of argv[2..] bytes through gzprintf into argv[1], as ReadDump::put prints a read without a quality string */
int main(int argc, char **argv) {
  gzFile f = gzopen(argv[1], "w1");
  if (!f) return 2;
  for (int k = 2; k < argc; ++k) {
    int total = atoi(argv[k]), n = total - 3 - 5;          /* '>' id(5) '\n' seq '\n' */
    char id[8], *s = malloc((size_t)n + 1);
    snprintf(id, sizeof id, "%05d", total);
    memset(s, 'A', (size_t)n);
    gzprintf(f, ">%s\n%.*s\n", id, n, s);
    free(s);
  }
  return gzclose(f) == Z_OK ? 0 : 1;
}
"""


def test_record_limit_is_the_one_of_gzprintf(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text(GZPRINTF_PROBE)
    r = subprocess.run([cc, "-O1", "-o", str(tmp_path / "probe"), str(src), "-lz"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    sizes = [8190, 8191, 8192, 8193, 50]
    subprocess.run([str(tmp_path / "probe"), str(tmp_path / "probe.gz")] + [str(s) for s in sizes], check=True)
    text = gzip.open(tmp_path / "probe.gz").read()
    kept = [s for s in sizes if b">%05d\n" % s in text]
    assert kept == [s for s in sizes if s < gc.RECORD_LIMIT] == [8190, 8191, 50]
    # ... and the twin keeps and drops the same records
    ids = [b"%05d" % s for s in sizes]
    got = capi.Gz().dump(ids, np.ones(len(ids), np.uint8), [([b"A" * (s - 8) for s in sizes], None, None)])[0]
    assert gzip.decompress(got + capi.gz_eof()) == text
