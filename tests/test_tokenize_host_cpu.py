"""The host twin of the tokeniser (cfr_tokenize with a handle opened on device -1) against a restatement of the sequential grammar of
SeqReader::read_record (tokenize_cases.sequential_parse).  The safety property: whatever the tokeniser delivers is a prefix of what
the sequential grammar reads from the same text, and the sequential grammar started at `consumed` reads the rest.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import tokenize_cases as tc
from centrifuger_amd import capi


@pytest.fixture(scope="module")
def tok():
    t = capi.Tokenizer(None)
    yield t
    t.close()


def line_starts(text):
    return {0} | {i + 1 for i in range(len(text)) if text[i:i + 1] == b"\n"} | {len(text)}


@pytest.mark.parametrize("name", sorted(tc.REGULAR))
def test_regular_text_gives_the_sequential_grammars_records(tok, name):
    text = tc.REGULAR[name]
    want = tc.sequential_parse(text)
    info, rec, off, bases = tc.run(tok, text)
    assert info.irregular == 0 and info.irregular_at == 0 and info.fastq == (text[:1] == b"@")
    assert tc.delivered(text, rec, off, bases) == want
    assert info.n_records == len(want) and info.consumed == len(text) and info.total_bases == sum(len(s) for _, _, s in want) == len(bases)
    assert int(off[0]) == 0 and int(off[-1]) == info.total_bases
    for r in rec:      # the header line's content, and for FASTQ the quality line
        h = int(r["header"])
        assert text[h:h + 1] in (b">", b"@") and text[h:h + int(r["header_len"])] == text[h:].split(b"\n")[0].rstrip(b"\r")
        assert (int(r["qual"]) == 0) == (not info.fastq)
    assert capi.Tokenizer.ids(text, rec) == [i.decode("latin-1") for _, i, _ in want]


def test_ids_drop_the_mate_suffix_and_stop_at_a_blank(tok):
    info, rec, off, bases = tc.run(tok, tc.REGULAR["fq"])
    assert capi.Tokenizer.ids(tc.REGULAR["fq"], rec) == ["r0", "r1", "r2", "", "a", "plus", "long.id.with.dots/3", "r7"]
    q = [int(r["qual"]) for r in rec]
    assert tc.REGULAR["fq"][q[4]:q[4] + 1] == b"@" and tc.REGULAR["fq"][q[5]:q[5] + 1] == b"+"      # quality lines that look like headers


def test_mutations_deliver_a_prefix_and_the_sequential_reader_continues_at_consumed(tok):
    corpus = tc.mutation_corpus()
    assert len(corpus) >= 250
    n_irregular = 0
    for name, text in corpus:
        want = tc.sequential_parse(text)
        info, rec, off, bases = tc.run(tok, text)
        got = tc.delivered(text, rec, off, bases)
        assert got == want[:len(got)], name
        assert info.consumed in line_starts(text), name
        rest = [(o + info.consumed, i, s) for o, i, s in tc.sequential_parse(text[info.consumed:])]
        assert got + rest == want, name
        if info.irregular:
            n_irregular += 1
            assert info.consumed == info.irregular_at, name
        else:
            assert got == want and info.consumed == len(text), name
    assert n_irregular >= 100       # (the mutations do hit)


@pytest.mark.parametrize("text", [tc.THREE_FQ, tc.THREE_FA], ids=["fastq", "fasta"])
def test_text_cut_at_every_byte_without_final_then_the_rest_with_final(tok, text):
    one_shot = tc.delivered(text, *tc.run(tok, text)[1:])
    assert len(one_shot) == 3
    for cut in range(1, len(text) + 1):
        info, rec, off, bases = tc.run(tok, text[:cut], final=False)
        assert info.irregular == 0
        got = tc.delivered(text, rec, off, bases)
        c = info.consumed
        assert c <= cut and (info.n_records > 0 or c == 0)
        info2, rec2, off2, bases2 = tc.run(tok, text[c:], final=True)
        assert info2.irregular == 0 and info2.consumed == len(text) - c
        got += [(h + c, i, s) for h, i, s in tc.delivered(text[c:], rec2, off2, bases2)]
        assert got == one_shot, cut


@pytest.mark.parametrize("name", ["fq", "fa_w60", "fq_empty_last"])
def test_max_records(tok, name):
    text = tc.REGULAR[name]
    want = tc.sequential_parse(text)
    n = len(want)
    for cap in (1, n - 1, n, n + 1):
        info, rec, off, bases = tc.run(tok, text, max_records=cap)
        k = min(cap, n)
        assert info.n_records == k and info.irregular == 0
        assert tc.delivered(text, rec, off, bases) == want[:k]
        assert info.consumed == (want[k][0] if k < n else len(text))
        assert info.total_bases == sum(len(s) for _, _, s in want[:k])


def test_argument_errors():
    L = capi.lib()
    h = C.c_void_p()
    assert L.cfr_tokenizer_open(C.c_int(-1), C.byref(h)) == capi.CFR_OK
    info = capi.TokenInfo()
    bad = np.frombuffer(b"ACGT\n", dtype=np.uint8)
    assert L.cfr_tokenize(h, capi._p(bad), C.c_uint64(len(bad)), C.c_int(1), C.c_uint64(0), C.byref(info)) == capi.CFR_ERR_ARG
    # len >= 2^32 is refused before a byte is read: the buffer behind the pointer is 8 bytes long
    small = np.frombuffer(b">a\nACGT\n", dtype=np.uint8)
    assert L.cfr_tokenize(h, capi._p(small), C.c_uint64(1 << 32), C.c_int(1), C.c_uint64(0), C.byref(info)) == capi.CFR_ERR_ARG
    assert b"2^32" in L.cfr_last_error()
    assert L.cfr_tokenize(h, capi._p(small), C.c_uint64(len(small)), C.c_int(1), C.c_uint64(0), C.byref(info)) == capi.CFR_OK and info.n_records == 1
    d_b, d_o = C.c_void_p(), C.c_void_p()
    assert L.cfr_tokenizer_device_reads(h, C.byref(d_b), C.byref(d_o)) == capi.CFR_ERR_ARG       # the host twin has no device buffers
    assert L.cfr_tokenize(h, None, C.c_uint64(0), C.c_int(1), C.c_uint64(0), C.byref(info)) == capi.CFR_OK and info.n_records == 0 and info.consumed == 0
    L.cfr_tokenizer_close(h)
    assert L.cfr_tokenize(h, capi._p(small), C.c_uint64(len(small)), C.c_int(1), C.c_uint64(0), C.byref(info)) == capi.CFR_ERR_ARG
    assert L.cfr_tokenizer_fetch(h, None, None, None) == capi.CFR_ERR_ARG
    L.cfr_tokenizer_close(h)        # (a second close is ignored)
    assert np.dtype(capi.READ_RECORD_DTYPE).itemsize == 24 and C.sizeof(capi.TokenInfo) == 48 and C.sizeof(capi.TokenStats) == 16


def test_fetch_before_the_first_call_gives_nothing():
    t = capi.Tokenizer(None)
    rec, off, bases = t.fetch()
    assert len(rec) == 0 and off.tolist() == [0] and len(bases) == 0
    st = t.stats()
    assert st.copy_in_ms == 0.0 and st.kernel_ms == 0.0          # (the host twin has one clock)
    t.close()
