"""The inflater's host twin (csrc/cfr_inflate.cpp) against zlib over the members of tests/inflate_cases.py: it accepts exactly the
members zlib accepts (the case builder asserts zlib's verdict on every one), the text comes back byte for byte, every malformed
member has the status the core header names and costs nothing but its own text, the text offsets are the exclusive sum of the
ISIZEs, and input that does not frame is refused before anything is inflated.  Also cfr_tokenizer_fetch_ids on the tokeniser's host
twin against ids cut in Python.  No GPU."""
import numpy as np
import pytest

import inflate_cases as ic
import tokenize_cases as tc
from centrifuger_amd import capi


@pytest.fixture(scope="module")
def host():
    h = capi.Inflate()
    yield h
    h.close()


def check_call(h, members, text, status, fetch_text=True):
    got, info = h.inflate(members, fetch_text=fetch_text)
    st, off = h.member_status()
    ms = ic.members_of(members)
    sizes = [i if i <= 65536 else 0 for i in (ic.split(m)[2] for m in ms)]
    assert list(st) == list(status)
    assert list(off) == [0] + list(np.cumsum(sizes, dtype=np.uint64)) if sizes else list(off) == [0]
    bad = [i for i, s in enumerate(status) if s]
    assert (info.members, info.bad_members, info.bytes_in, info.bytes_out) == (len(ms), len(bad), len(members), sum(sizes))
    if bad:
        assert (info.first_bad, info.first_bad_status) == (bad[0], status[bad[0]])
    if fetch_text:
        assert got == text
    return got, info


@pytest.mark.parametrize("name", ic.case_names())
def test_host_twin_agrees_with_zlib(host, name):
    _, members, text, status = ic.case(name)
    ok = all(ic.verdict(m) is not None for m in ic.members_of(members))
    assert ok == all(s == ic.OK for s in status)                      # the builder's bookkeeping
    check_call(host, members, text, status)


def test_one_call_of_300_mixed_members(host):
    members, text, status = ic.mixed_call()
    assert len(status) >= 300 and any(status) and ic.EOF in members
    check_call(host, members, text, status)


def test_member_by_member(host):
    members, text, status = ic.mixed_call()
    for m in ic.members_of(members)[:40]:                              # member by member: one thread
        want = ic.verdict(m)
        got, info = host.inflate(m)
        assert (got == want and info.bad_members == 0) if want is not None else (info.bad_members == 1 and not any(got))


def test_input_that_does_not_frame_is_refused(host):
    good = ic.good()["one_byte"][0]
    plain_gzip = b"\x1f\x8b\x08\x00" + good[4:]
    for what in (b"no gzip at all, but more than eighteen bytes", good[:-1], good + good[:20], good + plain_gzip, plain_gzip, good + b"\0"):
        with pytest.raises(capi.CfrError) as e:
            host.inflate(what)
        assert e.value.status == capi.CFR_ERR_ARG
    text, info = host.inflate(good)                                    # the handle is as good as before
    assert text == b"x" and info.members == 1


def test_no_input_is_no_text(host):
    text, info = host.inflate(b"")
    assert text == b"" and (info.members, info.bad_members, info.bytes_out) == (0, 0, 0)
    st, off = host.member_status()
    assert len(st) == 0 and list(off) == [0]


def test_device_text_is_refused_on_the_host_twin(host):
    with pytest.raises(capi.CfrError) as e:
        host.device_text()
    assert e.value.status == capi.CFR_ERR_ARG


def test_fetch_ids_of_the_host_tokeniser_equals_ids_cut_in_python():
    tok = capi.Tokenizer()
    texts = list(tc.REGULAR.items()) + tc.mutation_corpus()[::7]
    for name, text in texts:
        info, rec, off, bases = tc.run(tok, text)
        want = [i for _, i, _ in tc.delivered(text, rec, off, bases)]
        ids, id_off = tok.fetch_ids()
        assert len(id_off) == info.n_records + 1 and id_off[0] == 0
        assert [ids[int(id_off[i]):int(id_off[i + 1])].tobytes() for i in range(info.n_records)] == want, name
    with pytest.raises(capi.CfrError) as e:                            # resident text is a device matter
        tok.tokenize_resident(4096, 10)
    assert e.value.status == capi.CFR_ERR_ARG
    info = tok.tokenize(tc.THREE_FQ)
    with pytest.raises(capi.CfrError) as e:
        tok.fetch_ids(cap=1)
    assert e.value.status == capi.CFR_ERR_CAPACITY
    tok.close()
