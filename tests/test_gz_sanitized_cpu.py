"""The compressor's host twin under AddressSanitizer and UBSan: tools/gz_sanitize.cpp (a program of its own, with its own main) is
compiled together with csrc/cfr_gz.cpp, with the sanitizers' runtimes linked statically (so the program starts whatever the
environment preloads, and the test leaves the environment as it is), and run over the texts and dumps of tests/gz_cases.py: every
input in a heap block of exactly its size, so that a read one byte in front of a block's start or behind its end is a report.  The
program inflates what the twin made with a decoder of its own.  No Python process loads sanitized code.  No GPU."""
import os
import shutil
import subprocess

import pytest

import gz_cases as gc
from conftest import ROOT


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = tmp_path / "gz_sanitize"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tools", "gz_sanitize.cpp"), os.path.join(ROOT, "centrifuger_amd", "csrc", "cfr_gz.cpp"), "-o", str(exe), "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    text_items = [(bb, t) for bb in gc.BLOCKS for t in gc.texts(bb).values()]
    dump_items = [(bb, ids, sel, files, gc.dump_expected(ids, sel, files)) for bb in gc.BLOCKS for ids, sel, files in gc.dump_cases().values()]
    corpus = tmp_path / "corpus.bin"
    gc.write_corpus(corpus, text_items, dump_items)
    r = subprocess.run([str(exe), str(corpus)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-3000:])
    assert f"{len(text_items) + len(dump_items)} items".encode() in r.stdout
