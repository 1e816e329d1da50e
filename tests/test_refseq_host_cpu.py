"""The host twin of the reference-text front end (csrc/cfr_refseq.cpp behind cfr_refseq_open(-1)) against the plain Python statement of
the grammar in tests/refseq_cases.py: records, the stream U (read back through an assembly in feed order) and drawn assemblies T.  Also
the stand-alone tools/refseq_sanitize.cpp over the corpus under ASan + UBSan.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import refseq_cases as rc
from centrifuger_amd import capi
from conftest import ROOT


@pytest.mark.parametrize("log2", rc.CHUNK_LOG2)
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_host_twin_records_and_stream_equal_the_python_statement(name, log2):
    h, pieces, want_u = rc.check_feed(lambda: capi.Refseq(None), rc.CASES[name], 1 << log2)
    if pieces:
        dst, segs = 0, []
        for s, ln in pieces:
            segs.append((s, ln, dst))
            dst += ln
        h.assemble(segs)
        assert h.text() == b"".join(want_u)
    h.close()


@pytest.mark.parametrize("name", sorted(rc.PROTEIN_CASES))
def test_host_twin_keeps_the_protein_letters(name):
    h, pieces, want_u = rc.check_feed(lambda: capi.Refseq(None, protein=True), rc.PROTEIN_CASES[name], 256, rc.AA)
    h.assemble([(s, ln, d) for (s, ln), d in zip(pieces, np.cumsum([0] + [p[1] for p in pieces[:-1]]))])
    assert h.text() == b"".join(want_u)
    h.close()


@pytest.mark.parametrize("log2", rc.CHUNK_LOG2)
def test_host_twin_assembles_drawn_segment_lists(log2):
    rc.check_assemblies(lambda: capi.Refseq(None), 1 << log2)


def test_segments_inside_records_one_symbol_long_and_three_in_a_word():
    h = capi.Refseq(None)
    info = h.feed(b">a\nACGTACGTACGTACGTACGTACGTACGTACGTAAAACCCCGGGGTTTT\n")
    u = b"ACGTACGTACGTACGTACGTACGTACGTACGTAAAACCCCGGGGTTTT"
    order = [47, 0, 33, 1, 2, 40, 5, 5, 5] + list(range(10, 48)) + [3]
    h.assemble([(info.u_start + s, 1, d) for d, s in enumerate(order)])
    assert h.text() == bytes(u[s] for s in order)


def test_feed_and_assemble_refuse_what_the_header_says_they_refuse():
    h = capi.Refseq(None)
    with pytest.raises(capi.CfrError) as e:
        h.feed(b">a header line that does not end in this chunk", True, False)
    assert e.value.status == capi.CFR_ERR_CAPACITY
    info = h.feed(b">a\nACGTACGT\n")
    assert info.kept == 8
    for segs, n in (([(0, 4, 0), (4, 4, 5)], 9), ([(4, 4, 4), (0, 4, 0)], 8), ([(0, 9, 0)], 9), ([(0, 8, 0)], 9), ([(0, 0, 0), (0, 8, 0)], 8)):
        with pytest.raises(capi.CfrError):
            h.assemble(segs, n)
    h.assemble([(0, 8, 0)])
    assert h.text() == b"ACGTACGT"
    with pytest.raises(capi.CfrError):
        capi.Refseq(None, protein=True).feed(b">p\nARND$\n")
    with pytest.raises(capi.CfrError):
        capi.Refseq(0, protein=True)


def test_host_twin_under_address_and_undefined_sanitizers(tmp_path):
    """tools/refseq_sanitize.cpp: a program of its own with the twin compiled in, over the corpus at every chunk size."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "refseq_sanitize")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tools", "refseq_sanitize.cpp"), os.path.join(ROOT, "centrifuger_amd", "csrc", "cfr_refseq.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    corpus = str(tmp_path / "corpus.bin")
    with open(corpus, "wb") as f:
        for name in sorted(rc.CASES):
            f.write(struct.pack("<IB", len(rc.CASES[name]), 0) + rc.CASES[name])
        for name in sorted(rc.PROTEIN_CASES):
            f.write(struct.pack("<IB", len(rc.PROTEIN_CASES[name]), 1) + rc.PROTEIN_CASES[name])
    r = subprocess.run([exe, corpus], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    assert b"no report" in r.stdout
