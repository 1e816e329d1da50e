"""The command line's read-file code (csrc/cfr_cli_reads.hpp: SeqReader with its inflaters, the cutters of mapped files, parse_piece)
under AddressSanitizer and UBSan: tools/reads_sanitize.cpp (a program of its own, with its own main) is compiled with the sanitizers'
runtimes linked statically and run over the awkward inputs of test_cli_read_parser, a .gz of each, and a BGZF file read with several
inflate threads.  The program itself checks that the sequential reader, the byte-cut pieces and the record-cut pieces give the same
records.  No Python process loads sanitized code.  No GPU."""
import gzip
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_host_cpu import CASES, _py_parse, write_bgzf


def test_read_files_are_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = tmp_path / "reads_sanitize"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tools", "reads_sanitize.cpp"), "-o", str(exe), "-lz", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    files = []
    for name, data in CASES.items():
        (tmp_path / (name + ".txt")).write_bytes(data)
        with gzip.open(tmp_path / (name + ".txt.gz"), "wb", compresslevel=1) as f:
            f.write(data)
        files += [str(tmp_path / (name + ".txt")), str(tmp_path / (name + ".txt.gz"))]
    r = subprocess.run([str(exe)] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-3000:])
    rows = [ln.split("\t") for ln in r.stdout.decode().splitlines()]
    assert [row[0] for row in rows] == files
    for (name, data), plain, gz in zip(CASES.items(), rows[0::2], rows[1::2]):
        assert int(plain[1]) == len(_py_parse(data)) and plain[1:3] == gz[1:3], name      # the same records from the file and from its .gz
        assert gz[3] == "", name                                                           # (a .gz is not cut)
    how = {os.path.basename(row[0])[:-4]: row[3] for row in rows[0::2]}
    assert how["fastq4"] == "bytes+records" and how["huge_line"] == "bytes+records" and how["mixed_blank"] == "", how
    # BGZF: blocks inflated side by side by 4 threads, and the same file through gzread (1 thread)
    data = CASES["fastq4"] * 150                                                           # ~9 MB of text: two groups of blocks
    write_bgzf(tmp_path / "blocks.fq.gz", data)
    sums = []
    for t in ("4", "1"):
        r = subprocess.run([str(exe), "-t", t, str(tmp_path / "blocks.fq.gz")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, (t, r.returncode, r.stderr.decode()[-3000:])
        sums.append(r.stdout.decode().split("\t")[1:3])
    assert sums[0] == sums[1] and sums[0][0] == "30000"
