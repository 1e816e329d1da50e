"""The code build of the compressor's dynamic mode under AddressSanitizer and UBSan, in two programs of their own (each with its own
main, the sanitizers' runtimes linked statically as in tests/test_gz_sanitized_cpu.py; no Python process loads sanitized code):
tools/gz_codes_check.cpp drives gz_code_lengths, gz_canonical, gz_dyn_build and gz_put_dyn_header of csrc/cfr_gz_core.hpp directly, on
the histograms where a length-limited code build goes wrong, from workspaces of exactly their sizes; tools/gz_sanitize.cpp with
`dynamic` runs the host twin with codes = 1 over the texts and dumps and inflates the members with a decoder of its own.  No GPU."""
import os
import shutil
import subprocess

import pytest

import gz_cases as gc
import gz_dyn_cases as gd
from conftest import ROOT

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"]


def _compile(tmp_path, name, sources):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = tmp_path / name
    r = subprocess.run([gxx] + FLAGS + sources + ["-o", str(exe), "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def test_code_build_is_clean_and_its_codes_are_complete(tmp_path):
    exe = _compile(tmp_path, "gz_codes_check", [os.path.join(ROOT, "tools", "gz_codes_check.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-3000:])
    assert b"every one held" in r.stdout


def test_host_twin_in_dynamic_mode_is_clean_under_asan_and_ubsan(tmp_path):
    exe = _compile(tmp_path, "gz_sanitize", [os.path.join(ROOT, "tools", "gz_sanitize.cpp"), os.path.join(ROOT, "centrifuger_amd", "csrc", "cfr_gz.cpp")])
    text_items = [(bb, t) for bb in gd.BLOCKS for t in gd.texts(bb).values()]
    dump_items = [(bb, ids, sel, files, gc.dump_expected(ids, sel, files)) for bb in gd.BLOCKS for ids, sel, files in gc.dump_cases().values()]
    corpus = tmp_path / "corpus.bin"
    gc.write_corpus(corpus, text_items, dump_items)
    r = subprocess.run([str(exe), str(corpus), "dynamic"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-3000:])
    assert f"{len(text_items) + len(dump_items)} items".encode() in r.stdout
    dynamic = int(r.stdout.split(b" members with dynamic codes")[0].split()[-1])
    assert dynamic > 4000                      # fastq_1mb at 251 bytes a block alone has 3880 such members
