"""The inflater's host twin under AddressSanitizer and UBSan: tools/inflate_sanitize.cpp (a program of its own, with its own main) is
compiled together with csrc/cfr_inflate.cpp, with the sanitizers' runtimes linked statically (so the program starts whatever the
environment preloads, and the test leaves the environment as it is), and run over every member of tests/inflate_cases.py, the
malformed ones included: every input in a heap block of exactly its size, the text in one of exactly the sum of the ISIZEs, so that
an access one byte off either is a report.  The decoder and its bounds rules are the core header's, which the kernel shares.  No
Python process loads sanitized code.  No GPU."""
import os
import shutil
import subprocess

import pytest

import inflate_cases as ic
from conftest import ROOT


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = tmp_path / "inflate_sanitize"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tools", "inflate_sanitize.cpp"), os.path.join(ROOT, "centrifuger_amd", "csrc", "cfr_inflate.cpp"), "-o", str(exe), "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    items = [(ms, text, status) for _, ms, text, status in ic.corpus()] + [ic.mixed_call()]
    corpus = tmp_path / "corpus.bin"
    ic.write_corpus(corpus, items)
    r = subprocess.run([str(exe), str(corpus)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-3000:])
    assert f"{len(items)} items".encode() in r.stdout
