"""The batch formatter's host twin under AddressSanitizer and UBSan: tools/tsv_sanitize.cpp (a program of its own, with its own main) is
compiled together with csrc/cfr_tsv.cpp, with the sanitizers' runtimes linked statically (so the program starts whatever the
environment preloads, and the test leaves the environment as it is), and run over the cases of tests/test_tsv_host_cpu.py: every
array in a heap block of exactly its size, the text in one of exactly the expected length.  No Python process loads sanitized code.
No GPU."""
import os
import shutil
import subprocess

import pytest

import tsv_cases as tc
from centrifuger_amd import capi
from conftest import ROOT


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = tmp_path / "tsv_sanitize"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tools", "tsv_sanitize.cpp"), os.path.join(ROOT, "centrifuger_amd", "csrc", "cfr_tsv.cpp"), "-o", str(exe), "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    idx = capi.Index(tc.F6)
    tax = capi.Taxonomy(tc.F6)
    names = [s.encode() for s in tax.seq_names]
    ranks = tax.rank.tobytes()
    info = idx.info()
    assert len(names) == info.seq_cnt and len(ranks) == info.node_cnt
    batches = []
    for res, mat, ids in (tc.edge_batch(info.seq_cnt, info.node_cnt), tc.random_batch(0, info.seq_cnt, info.node_cnt, 1),
                          tc.random_batch(1, info.seq_cnt, info.node_cnt, 2), tc.random_batch(777, info.seq_cnt, info.node_cnt, 3, stride=5)):
        batches.append((res, mat, ids, tc.reference(idx, res, mat, ids)[0]))
    corpus = tmp_path / "corpus.bin"
    tc.write_corpus(corpus, (names, ranks), batches)
    r = subprocess.run([str(exe), str(corpus)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-3000:])
    assert f"{len(batches)} batches".encode() in r.stdout
    tax.close()
    idx.close()
