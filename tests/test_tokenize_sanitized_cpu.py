"""The tokeniser's host twin under AddressSanitizer and UBSan: tools/tokenize_sanitize.cpp (a program of its own, with its own main)
is compiled together with csrc/cfr_tokenize_host.cpp, with the sanitizers' runtimes linked statically (so the program starts whatever
the environment preloads, and the test leaves the environment as it is), and run over the regular texts (every truncation of them too) and the mutation
corpus of tests/tokenize_cases.py.  No Python process loads sanitized code.  No GPU."""
import os
import shutil
import struct
import subprocess

import pytest

import tokenize_cases as tc
from conftest import ROOT


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = tmp_path / "tokenize_sanitize"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tools", "tokenize_sanitize.cpp"), os.path.join(ROOT, "centrifuger_amd", "csrc", "cfr_tokenize_host.cpp"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    corpus = tmp_path / "corpus.bin"
    texts = [(t, 1) for t in tc.REGULAR.values()] + [(tc.THREE_FQ, 1), (tc.THREE_FA, 1)] + [(t, 0) for _, t in tc.mutation_corpus()]
    texts += [(b">", 1), (b"@", 1), (b">\n", 1), (b"@\n\n+\n\n", 1), (b"@a\r\r\n\r\n+\r\n\r", 1), (b">a\n\n\n", 1)]
    with open(corpus, "wb") as f:
        for t, sweep in texts:
            f.write(struct.pack("<IB", len(t), sweep) + t)
    r = subprocess.run([str(exe), str(corpus)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-3000:])
    assert f"{len(texts)} texts".encode() in r.stdout
