"""The kernels of the reference-text front end (csrc/cfr_refseq.hip) against the Python statement of the grammar and against the host
twin: records, the stream U and drawn assemblies T over the whole corpus of tests/refseq_cases.py, every text fed whole (several blocks
in a chunk) and in chunks of 4096, 1024 and 256 bytes.  -m gpu."""
import numpy as np
import pytest

import refseq_cases as rc
from centrifuger_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("log2", rc.CHUNK_LOG2)
def test_device_records_and_stream_equal_the_statement_and_the_host_twin(log2):
    for name in sorted(rc.CASES):
        out = []
        for make in (lambda: capi.Refseq(0), lambda: capi.Refseq(None)):
            h, pieces, want_u = rc.check_feed(make, rc.CASES[name], 1 << log2)
            text = b""
            if pieces:
                h.assemble([(s, ln, d) for (s, ln), d in zip(pieces, np.cumsum([0] + [p[1] for p in pieces[:-1]]))])
                text = h.text()
                assert text == b"".join(want_u), name
            out.append((pieces, text))
            h.close()
        assert out[0] == out[1], name


@pytest.mark.parametrize("log2", rc.CHUNK_LOG2)
def test_device_assembles_drawn_segment_lists(log2):
    rc.check_assemblies(lambda: capi.Refseq(0), 1 << log2)


def test_device_segments_one_symbol_long_and_many_in_a_word():
    u = b"ACGTACGTACGTACGTACGTACGTACGTACGTAAAACCCCGGGGTTTT" * 3
    order = [47, 0, 33, 1, 2, 40, 5, 5, 5] + list(range(10, 140)) + [3] + list(range(143, 60, -1))
    out = []
    for dev in (0, None):
        h = capi.Refseq(dev)
        info = h.feed(b">a\n" + u + b"\n")
        h.assemble([(info.u_start + s, 1, d) for d, s in enumerate(order)])
        out.append(h.text())
        h.close()
    assert out[0] == bytes(u[s] for s in order) == out[1]


def test_device_refuses_what_the_host_twin_refuses():
    h = capi.Refseq(0)
    with pytest.raises(capi.CfrError) as e:
        h.feed(b">a header line that does not end in this chunk", True, False)
    assert e.value.status == capi.CFR_ERR_CAPACITY
    assert h.feed(b">a\nACGTACGT\n").kept == 8
    for segs, n in (([(0, 4, 0), (4, 4, 5)], 9), ([(4, 4, 4), (0, 4, 0)], 8), ([(0, 9, 0)], 9), ([(0, 8, 0)], 9), ([(0, 0, 0), (0, 8, 0)], 8)):
        with pytest.raises(capi.CfrError):
            h.assemble(segs, n)
    h.assemble([(0, 8, 0)])
    assert h.text() == b"ACGTACGT"
    st = h.stats()
    assert st.feed_ms > 0 and st.assemble_ms > 0
    h.close()
