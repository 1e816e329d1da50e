"""The device form of the tokeniser (csrc/cfr_tokenize.hip) against its host twin: every field - cfr_token_info but the clock, the
records, the offsets, the bases.  Sizes sit at the edges of the kernels' units: a lane's 16 bytes, a block's 4096, the tiles of
the scans over block counts and unit weights (hipcub picks the tile: unit counts around multiples of 2048 cover its choices), a read
and a record far longer than a block.  -m gpu."""
import os
import random

import numpy as np
import pytest

import tokenize_cases as tc
from centrifuger_amd import capi
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SPAN = 4096           # bytes per block of k_tok_count / k_tok_lines (kBlock * kLaneBytes)


@pytest.fixture(scope="module")
def toks():
    host, dev = capi.Tokenizer(None), capi.Tokenizer(0)
    yield host, dev
    host.close()
    dev.close()


def both(toks, text, what="", **kw):
    h, d = tc.run(toks[0], text, **kw), tc.run(toks[1], text, **kw)
    tc.assert_same(h, d, what)
    return h


def test_open_and_close_without_a_call():
    t = capi.Tokenizer(0)
    t.close()
    with pytest.raises(capi.CfrError) as e:
        capi.Tokenizer(4096)
    assert e.value.status == capi.CFR_ERR_NO_DEVICE


@pytest.mark.parametrize("name", ["se.fq", "pe_1.fq", "pe_2.fq", "edge.fa"])
def test_golden_files(toks, name):
    text = open(os.path.join(GOLDEN, name), "rb").read()
    info = both(toks, text, name)[0]
    assert info.irregular == 0 and info.n_records == len(tc.sequential_parse(text)) and info.consumed == len(text)


def test_regular_texts_and_mutations(toks):
    for name, text in tc.REGULAR.items():
        assert both(toks, text, name)[0].irregular == 0
    corpus = tc.mutation_corpus()
    for name, text in random.Random(7).sample(corpus, 50):
        both(toks, text, name)


def _seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def test_line_lengths_at_the_edges_of_a_lane_and_a_block(toks):
    rng = random.Random(3)
    lens = [0, 1, 15, 16, 17, SPAN - 1, SPAN, SPAN + 1, 31, 2 * SPAN - 1]
    fq = b"".join(b"@r%d c\n" % i + _seq(rng, n) + b"\n+\n" + b"I" * n + b"\n" for i, n in enumerate(lens))
    fa = b"".join(b">r%d c\n" % i + _seq(rng, n) + b"\n" for i, n in enumerate(lens))
    for text in (fq, fa, fq.replace(b"\n", b"\r\n"), fa.replace(b"\n", b"\r\r\r\n")):
        h = both(toks, text)
        assert h[0].irregular == 0 and h[0].n_records == len(lens) and [int(b - a) for a, b in zip(h[2], h[2][1:])] == lens
    # a run of '\r' that crosses the end of a lane's bytes and the end of a block's: the '\n' sits at 16 k and at SPAN
    for at in (16, 32, SPAN, 2 * SPAN):
        for run in (1, 2, 17):
            head = b">x\n"
            run = min(run, at - len(head))
            text = head + b"A" * (at - len(head) - run) + b"\r" * run + b"\n" + b"CC\n>y\n\r\r\nG\n"
            assert text[at:at + 1] == b"\n"
            h = both(toks, text, (at, run))
            assert bytes(h[3]) == b"A" * (at - len(head) - run) + b"CCG"


def test_a_read_and_a_record_longer_than_any_block(toks):
    rng = random.Random(5)
    s = _seq(rng, 70000)
    for text in (b"@a\nACGT\n+\nIIII\n@long/1\n" + s + b"\n+\n" + b"F" * 70000 + b"\n@b\nGG\n+\nII\n", b">a\nACGT\n>long\n" + s + b"\n>b\nGG\n"):
        h = both(toks, text)
        assert h[0].n_records == 3 and bytes(h[3]) == b"ACGT" + s + b"GG"
    text = b">a\nAC\n>many\n" + b"\n".join(s[i:i + 1] for i in range(70000)) + b"\n>b\nGG"
    h = both(toks, text)
    assert h[0].n_records == 3 and bytes(h[3]) == b"AC" + s + b"GG" and h[0].consumed == len(text)


@pytest.mark.parametrize("units", [2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 8193])
def test_unit_counts_around_the_scan_tiles(toks, units):
    # FASTA: a unit is a line.  Two-line records, then one-base lines up to the wanted number of lines
    n_rec = units // 3
    text = b"".join(b">%d\nAC\n" % i for i in range(n_rec)) + b">t\n" + b"G\n" * (units - 2 * n_rec - 1)
    h = both(toks, text)
    assert h[0].n_records == n_rec + 1 and h[0].total_bases == 2 * n_rec + (units - 2 * n_rec - 1)
    # FASTQ: a unit is a record
    fq = b"".join(b"@%d\nACG\n+\nIII\n" % i for i in range(units))
    assert both(toks, fq)[0].n_records == units


@pytest.fixture(scope="module")
def two_mb():
    rng = np.random.default_rng(11)
    n = 6400
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 150))]
    return [b"@read.%d/1 len=150\n" % i + seqs[i].tobytes() + b"\n+\n" + b"I" * 150 + b"\n" for i in range(n)]


def test_two_megabytes_of_150_bp_reads(toks, two_mb):
    text = b"".join(two_mb)
    assert len(text) > 2_000_000
    h = both(toks, text)
    assert h[0].n_records == len(two_mb) and h[0].total_bases == 150 * len(two_mb) and h[0].irregular == 0
    fa = b"".join(b">" + r.split(b"\n")[0][1:] + b"\n" + r.split(b"\n")[1] + b"\n" for r in two_mb)
    assert both(toks, fa)[0].n_records == len(two_mb)
    st = toks[1].stats()                                       # the parts of device_ms, from events inside the call
    assert st.copy_in_ms > 0 and st.kernel_ms > 0 and st.copy_in_ms + st.kernel_ms <= toks[1]._last.device_ms * 1.001
    h = both(toks, text, max_records=1000)
    assert h[0].n_records == 1000 and h[0].consumed == sum(len(r) for r in two_mb[:1000])
    cut = len(text) - 100
    h = both(toks, text[:cut], final=False)
    assert h[0].n_records == len(two_mb) - 1 and h[0].consumed == len(text) - len(two_mb[-1])


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_an_irregular_record_first_in_the_middle_and_last(toks, two_mb, where):
    recs = list(two_mb[:3000])
    k = {"first": 0, "middle": 1500, "last": 2999}[where]
    lines = recs[k].split(b"\n")
    recs[k] = b"\n".join([lines[0], lines[1][:70], lines[1][70:], lines[2], lines[3], b""])       # multi-line FASTQ
    text = b"".join(recs)
    h = both(toks, text, where)
    assert h[0].irregular == 1 and h[0].n_records == k and h[0].consumed == h[0].irregular_at == sum(len(r) for r in recs[:k])
    fa = [b">" + r.split(b"\n")[0][1:] + b"\n" + r.split(b"\n")[1] + b"\n" for r in two_mb[:3000]]
    fa[k] = fa[k].split(b"\n")[0] + b"\nACGT\n+not a sequence\nACGT\n"
    h = both(toks, b"".join(fa), where)
    assert h[0].irregular == 1 and h[0].n_records == k and h[0].irregular_at == sum(len(r) for r in fa[:k])


@pytest.mark.parametrize("text", [tc.THREE_FQ, tc.THREE_FA], ids=["fastq", "fasta"])
def test_text_cut_at_every_byte_without_final(toks, text):
    one_shot = tc.delivered(text, *both(toks, text)[1:])
    for cut in range(1, len(text) + 1):
        h = both(toks, text[:cut], cut, final=False)
        c = h[0].consumed
        h2 = both(toks, text[c:], cut, final=True)
        got = tc.delivered(text, *h[1:]) + [(o + c, i, s) for o, i, s in tc.delivered(text[c:], *h2[1:])]
        assert got == one_shot, cut


def test_a_larger_text_second_grows_the_buffers(two_mb):
    host, dev = capi.Tokenizer(None), capi.Tokenizer(0)
    try:
        for text in (tc.REGULAR["fq"], b"".join(two_mb[:2000]), tc.REGULAR["fa_w60"], b"".join(two_mb)):
            tc.assert_same(tc.run(host, text), tc.run(dev, text))
    finally:
        host.close()
        dev.close()


@pytest.fixture(scope="module")
def dev_index(golden_dir):
    idx = capi.Index(os.path.join(golden_dir, "f6"), capi.default_params(max_result=5))
    return capi.DeviceIndex(idx, 0)


def test_resident_hand_off_to_classify(toks, dev_index):
    """the pointers of cfr_tokenizer_device_reads go straight into cfr_classify_batch_resident"""
    host, dev = toks
    text = open(os.path.join(GOLDEN, "se.fq"), "rb").read()
    _, _, off, bases = tc.run(host, text)
    want_r, want_m = dev_index.classify(bases, off)
    info = dev.tokenize(text)
    d_b, d_o = dev.device_reads()
    got_r, got_m = dev_index.classify_resident(d_b, d_o, info.n_records, info.total_bases)
    assert info.n_records == len(off) - 1 and got_r.tobytes() == want_r.tobytes() and got_m.tobytes() == want_m.tobytes()
    assert int((got_r["n_match"] > 0).sum()) > 0


def test_resident_hand_off_of_pairs(toks, dev_index):
    host, dev = toks
    dev2 = capi.Tokenizer(0)
    try:
        t1, t2 = (open(os.path.join(GOLDEN, f), "rb").read() for f in ("pe_1.fq", "pe_2.fq"))
        _, _, o1, b1 = tc.run(host, t1)
        _, _, o2, b2 = tc.run(host, t2)
        want_r, want_m = dev_index.classify(b1, o1, b2, o2)
        i1, i2 = dev.tokenize(t1), dev2.tokenize(t2)
        assert i1.n_records == i2.n_records == len(o1) - 1
        (d_b1, d_o1), (d_b2, d_o2) = dev.device_reads(), dev2.device_reads()
        got_r, got_m = dev_index.classify_resident(d_b1, d_o1, i1.n_records, i1.total_bases, d_b2, d_o2, i2.total_bases)
        assert got_r.tobytes() == want_r.tobytes() and got_m.tobytes() == want_m.tobytes()
    finally:
        dev2.close()
