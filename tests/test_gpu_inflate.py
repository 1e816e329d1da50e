"""The device inflater (csrc/cfr_inflate.hip) against its host twin (csrc/cfr_inflate.cpp) over the members of tests/inflate_cases.py:
text, text offsets, every status and every field of cfr_inflate_info, in one call and member by member; the twin itself is checked
with zlib in tests/test_inflate_host_cpu.py.  The malformed members are inputs the kernel must refuse cleanly: the bounds rules it
runs are the core header's, which tests/test_inflate_sanitized_cpu.py runs under AddressSanitizer over the same corpus.
Then the text that stays in HBM: cfr_tokenize_resident on a range of it against cfr_tokenize of the same bytes from the host, and
cfr_tokenizer_fetch_ids against the host twin's."""
import numpy as np
import pytest

import inflate_cases as ic
import tokenize_cases as tc
from centrifuger_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    dev, host = capi.Inflate(device=0), capi.Inflate()
    yield dev, host
    dev.close()
    host.close()


def _info(i):
    return (i.members, i.bad_members, i.first_bad, i.bytes_in, i.bytes_out, i.first_bad_status)


def same_as_host(handles, members):
    dev, host = handles
    want, winfo = host.inflate(members)
    wst, woff = host.member_status()
    got, ginfo = dev.inflate(members)
    gst, goff = dev.member_status()
    assert _info(ginfo) == _info(winfo)
    assert np.array_equal(gst, wst) and np.array_equal(goff, woff)
    assert got == want
    return got, gst


@pytest.mark.parametrize("name", ic.case_names())
def test_device_equals_the_host_twin(handles, name):
    _, members, text, status = ic.case(name)
    got, st = same_as_host(handles, members)
    assert got == text and list(st) == status
    ms = ic.members_of(members)
    if len(ms) > 1:
        for m in ms:
            same_as_host(handles, m)


def test_one_call_of_300_mixed_members(handles):
    members, text, status = ic.mixed_call()
    got, st = same_as_host(handles, members)
    assert got == text and list(st) == status


def test_more_members_than_workgroups_fit_the_device(handles):
    """the workgroups stride: 12 000 small members, every 7th refused, end-of-file members between them"""
    good, eof = ic.good()["one_byte"][0], ic.EOF
    bad = ic.malformed()["distance_in_front_of_the_member"][0]
    members = (good * 5 + eof + bad) * (12000 // 7)
    got, st = same_as_host(handles, members)
    assert got == (b"x" * 5 + bytes(4)) * (12000 // 7)
    assert list(st[:7]) == [0] * 6 + [ic.BAD_SYMBOL]


def test_a_smaller_then_a_larger_input_on_the_same_handle(handles):
    g = ic.good()
    for name in ("fastq_65280_l6", "one_byte", "eof_member", "fastq_997_l1", "fastq_65280_l9"):
        got, _ = same_as_host(handles, g[name][0])
        assert got == g[name][1]
    dev, _ = handles
    text, info = dev.inflate(b"")
    assert text == b"" and _info(info) == (0, 0, 0, 0, 0, 0)
    assert dev.device_text()[1] == 0


def test_input_that_does_not_frame_is_refused_before_a_launch(handles):
    dev, _ = handles
    good = ic.good()["one_byte"][0]
    for what in (good[:-1], good + b"\x1f\x8b\x08\x00" + good[4:]):
        with pytest.raises(capi.CfrError) as e:
            dev.inflate(what)
        assert e.value.status == capi.CFR_ERR_ARG
    assert dev.inflate(good)[0] == b"x"


def test_text_that_stays_in_hbm_is_tokenised_there(handles):
    dev, _ = handles
    members, text = ic.good()["fastq_65280_l6"]
    none, info = dev.inflate(members, fetch_text=False)
    assert none is None and info.bad_members == 0
    d_text, n = dev.device_text()
    assert d_text and n == len(text)
    tok, ref, host_tok = capi.Tokenizer(device=0), capi.Tokenizer(device=0), capi.Tokenizer()
    starts = [i + 1 for i in range(len(text) - 1) if text[i] == 10 and text[i + 1] == 64 and text[i + 2:i + 3] == b"r"]
    lo, hi = starts[3], starts[-5]
    # (range, final): whole records; the last line without its '\n'; text cut inside a record, to be continued
    for a, b, final in ((0, len(text), True), (lo, hi, True), (lo, hi - 1, True), (lo, hi - 40, False), (lo, hi, False), (lo, lo + 20, False)):
        sub = text[a:b]
        want = tc.run(ref, sub, final=final)
        info = tok.tokenize_resident(d_text + a, b - a, final=final)
        got = (info,) + tok.fetch()
        tc.assert_same(want, got, (a, b, final))
        tc.run(host_tok, sub, final=final)
        ids, id_off = tok.fetch_ids()
        hids, hid_off = host_tok.fetch_ids()
        assert ids.tobytes() == hids.tobytes() and np.array_equal(id_off, hid_off), (a, b, final)
        assert [ids[int(id_off[i]):int(id_off[i + 1])].tobytes() for i in range(info.n_records)] == [i for _, i, _ in tc.delivered(sub, *got[1:])]
    assert tok.tokenize_resident(d_text, 0).n_records == 0
    with pytest.raises(capi.CfrError) as e:                            # text that starts inside a record
        tok.tokenize_resident(d_text + lo + 1, 100)
    assert e.value.status == capi.CFR_ERR_ARG
    tok.tokenize_resident(d_text + lo, hi - lo)
    with pytest.raises(capi.CfrError) as e:
        tok.fetch_ids(cap=3)
    assert e.value.status == capi.CFR_ERR_CAPACITY
    for t in (tok, ref, host_tok):
        t.close()


def test_no_such_device_is_an_error_not_a_fall_back():
    with pytest.raises(capi.CfrError) as e:
        capi.Inflate(device=1000)
    assert e.value.status == capi.CFR_ERR_NO_DEVICE
