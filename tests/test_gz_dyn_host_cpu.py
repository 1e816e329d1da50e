"""Dynamic mode of the compressor's host twin (csrc/cfr_gz.cpp through capi.Gz(codes="dynamic"), device=None): every member inflates to
its block with zlib, a dynamic member (BTYPE 10) has complete codes within the limits of deflate and is shorter than fixed mode's member
of the same block, and every other member has exactly fixed mode's bytes.  The texts of tests/gz_dyn_cases.py each carry the shape
their name says, read back from the parsed header.  No GPU."""
import gzip

import pytest

import gz_cases as gc
import gz_dyn_cases as gd
from centrifuger_amd import capi


@pytest.fixture(scope="module")
def twins():
    hs = {bb: (capi.Gz(block_bytes=bb, threads=3, codes="dynamic"), capi.Gz(block_bytes=bb, threads=3)) for bb in gd.BLOCKS}
    yield hs
    for d, f in hs.values():
        d.close()
        f.close()


def _counts(st):
    return (st.blocks, st.stored_blocks, st.dynamic_blocks, st.bytes_in, st.bytes_out)


@pytest.mark.parametrize("block_bytes", gd.BLOCKS)
@pytest.mark.parametrize("name", list(gd.texts(65280)))
def test_members_are_dynamic_and_shorter_or_fixed_modes_bytes(twins, name, block_bytes):
    dyn, fixed = twins[block_bytes]
    text = gd.texts(block_bytes)[name]
    out, fixed_out = dyn.compress(text), fixed.compress(text)
    assert gzip.decompress(out + capi.gz_eof()) == text
    members, stored, dynamic, _ = gd.check_members_dyn(out, fixed_out, text, block_bytes)
    assert _counts(dyn.stats()) == (members, stored, dynamic, len(text), len(out))
    assert len(out) <= len(fixed_out) and fixed.stats().dynamic_blocks == 0


@pytest.mark.parametrize("name", ["fastq_1mb", "acgt_40000_twice"])
def test_compressible_text_comes_out_dynamic_and_smaller(twins, name):
    dyn, fixed = twins[65280]
    text = gd.texts(65280)[name]
    out = dyn.compress(text)
    assert dyn.stats().dynamic_blocks > 0 and len(out) < len(fixed.compress(text))


@pytest.mark.parametrize("block_bytes", gd.BLOCKS)
def test_random_text_is_stored_as_in_fixed_mode(twins, block_bytes):
    dyn, fixed = twins[block_bytes]
    text = gd.texts(block_bytes)["random_200k"]
    assert dyn.compress(text) == fixed.compress(text)
    assert dyn.stats().dynamic_blocks == 0 and dyn.stats().stored_blocks == dyn.stats().blocks


@pytest.mark.parametrize("name", ["one_byte", "two_bytes"])
def test_tiny_blocks_stay_fixed(twins, name):
    dyn, fixed = twins[65280]
    out = dyn.compress(gd.texts(65280)[name])
    assert out == fixed.compress(gd.texts(65280)[name]) and (gc.walk(out)[0][1][0] >> 1) & 3 == 1
    assert _counts(dyn.stats())[1:3] == (0, 0)


def _headers(twins, name, block_bytes=65280):
    dyn, fixed = twins[block_bytes]
    text = gd.texts(block_bytes)[name]
    headers = gd.check_members_dyn(dyn.compress(text), fixed.compress(text), text, block_bytes)[3]
    assert headers, f"{name}: no dynamic member"
    return headers


def test_no_match_leaves_two_forced_distance_codes(twins):
    """no 4 bytes occur twice: no length symbol, no distance is used, and the distance code is symbols 0 and 1 with one bit each"""
    h, = _headers(twins, "no_match_16_symbols")
    assert h["hlit"] == 257 and h["dist"] == [1, 1]
    assert sum(1 for l in h["ll"][:256] if l) <= 16 and not any(h["ll"][257:])


def test_one_used_distance_gets_a_forced_partner(twins):
    """every match is at distance 512: distance symbol 17 and the forced symbol 0, one bit each"""
    h, = _headers(twins, "one_distance_code")
    assert h["hlit"] > 257, "no match in the text"
    assert [(d, l) for d, l in enumerate(h["dist"]) if l] == [(0, 1), (17, 1)]


def test_fibonacci_frequencies_reach_the_length_limit(twins):
    """fibonacci_tail: 20 rare bytes with Fibonacci frequencies under a bulk of 64 frequent ones - Huffman's tree puts the rarest 19
    levels below the subtree's root: without the limit the longest code would have more than 15 bits.  With it, bytes of different
    frequency share a length, which Huffman's code for Fibonacci frequencies never does below the two rarest.
    (fibonacci_literals, all 22 bytes Fibonacci, does NOT get there with this tokeniser: its frequent bytes leave in matches, and the
    longest code of the histogram that remains has 13 bits, for every one of 12 shuffles tried.  It runs through every other check.)"""
    h, = _headers(twins, "fibonacci_tail")
    assert max(h["ll"]) == 15, "no code of 15 bits: the limiter did not have to run"
    assert all(h["ll"][k] > 0 for k in range(1, 21)) and len(set(h["ll"][2:21])) < 19


def test_far_apart_literals_need_symbol_18_and_a_remainder(twins):
    """literals 0x00 and 0xff only: the 254 zero lengths between them are more than one symbol 18 can hold"""
    h, = _headers(twins, "far_apart_symbols")
    assert h["ll"][0] > 0 and h["ll"][255] > 0 and not any(h["ll"][1:255])
    at = h["sent"].index((18, 138))
    assert h["sent"][at - 1][0] == h["ll"][0] and h["sent"][at + 1] == (18, 254 - 138)


def test_runs_of_equal_lengths_use_symbol_16(twins):
    """all 256 byte values equally often: long runs of one length, sent once and then as repeats of up to 6"""
    headers = _headers(twins, "all_bytes_x300")
    assert any((16, 6) in h["sent"] for h in headers)
    for h in headers:
        for k, (s, count) in enumerate(h["sent"]):
            if s == 16:
                assert 3 <= count <= 6 and k > 0


@pytest.mark.parametrize("block_bytes", gd.BLOCKS)
@pytest.mark.parametrize("name", list(gc.dump_cases()))
def test_dump_inflates_to_the_records(twins, name, block_bytes):
    dyn, fixed = twins[block_bytes]
    ids, select, files = gc.dump_cases()[name]
    want = gc.dump_expected(ids, select, files)
    got, fixed_got = dyn.dump(ids, select, files), fixed.dump(ids, select, files)
    totals = [0, 0, 0]
    for g, f, w in zip(got, fixed_got, want):
        assert gzip.decompress(g + capi.gz_eof()) == w
        for k, v in enumerate(gd.check_members_dyn(g, f, w, block_bytes)[:3]):
            totals[k] += v
    st = dyn.stats()
    assert _counts(st) == (totals[0], totals[1], totals[2], sum(len(w) for w in want), sum(len(g) for g in got))
    assert st.bytes_out <= fixed.stats().bytes_out


@pytest.mark.parametrize("block_bytes", gd.BLOCKS)
def test_bytes_do_not_depend_on_the_threads(twins, block_bytes):
    one, seven = capi.Gz(block_bytes=block_bytes, threads=1, codes="dynamic"), capi.Gz(block_bytes=block_bytes, threads=7, codes="dynamic")
    for name in ("fastq_1mb", "all_bytes_x300", "fibonacci_literals"):
        text = gd.texts(block_bytes)[name]
        first = twins[block_bytes][0].compress(text)
        assert one.compress(text) == first and seven.compress(text) == first
    one.close()
    seven.close()


@pytest.mark.parametrize("bad", [2, -1])
def test_codes_outside_0_and_1_is_refused(bad):
    with pytest.raises(capi.CfrError) as e:
        capi.Gz(codes=bad)
    assert e.value.status == capi.CFR_ERR_ARG
    with pytest.raises(ValueError):
        capi.Gz(codes="static")
