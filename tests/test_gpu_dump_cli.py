"""`centrifuger --gpu-dump`: the --un / --cl read dumps made and compressed on the GPU (cfr_gz_dump) against the same command line
without the switch (gzprintf on the writer thread, itself compared with the reference in tests/test_gpu_cli.py): every file
inflates to the same bytes, stdout is the same, and the new files are BGZF members closed by the end-of-file member.  -m gpu."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import barcode_fixtures as bf
import gz_cases as gc
from centrifuger_amd import capi
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
CDIR = os.path.join(bf.BARCODE, "cli")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _run(golden_dir, cwd, reads, extra=(), index="f6"):
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([CLI, "-x", os.path.join(golden_dir, index), "-t", "3"] + list(reads) + ["--un", "un", "--cl", "cl"] + list(extra),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(cwd))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _both(golden_dir, tmp_path, reads, extra=(), files=("un.fq.gz", "cl.fq.gz")):
    """the run with and without --gpu-dump -> {file: inflated bytes}; asserts that stdout and every file agree"""
    host = _run(golden_dir, tmp_path / "host", reads, extra)
    dev = _run(golden_dir, tmp_path / "dev", reads, list(extra) + ["--gpu-dump"])
    assert dev.stdout == host.stdout
    assert sorted(os.listdir(tmp_path / "dev")) == sorted(os.listdir(tmp_path / "host")) == sorted(files)
    texts = {}
    for name in files:
        raw = (tmp_path / "dev" / name).read_bytes()
        assert raw.endswith(EOF), name
        members = gc.walk(raw)                      # (asserts that the file is BGZF members and nothing else)
        assert members[-1] == (28, b"\x03\x00", 0, 0) and all(m[3] > 0 for m in members[:-1])
        texts[name] = gzip.decompress(raw)
        assert texts[name] == gzip.open(tmp_path / "host" / name).read(), name
    return texts, host.stdout


def test_end_of_file_member_is_the_one_of_the_library():
    assert capi.gz_eof() == EOF


def test_single_end_fasta_dumps(golden_dir, tmp_path):
    texts, _ = _both(golden_dir, tmp_path, ["-u", os.path.join(golden_dir, "edge.fa")])
    assert texts["un.fq.gz"].startswith(b">") or texts["cl.fq.gz"].startswith(b">")
    assert len(texts["un.fq.gz"]) + len(texts["cl.fq.gz"]) > 0


def test_paired_fastq_dumps_in_several_batches(golden_dir, tmp_path):
    reads = ["-1", os.path.join(golden_dir, "pe_1.fq"), "-2", os.path.join(golden_dir, "pe_2.fq")]
    names = ("un_1.fq.gz", "un_2.fq.gz", "cl_1.fq.gz", "cl_2.fq.gz")
    texts, _ = _both(golden_dir, tmp_path, reads, ["--gpu-batch", "70", "-k", "5"], names)
    assert texts["cl_1.fq.gz"].startswith(b"@") and texts["cl_1.fq.gz"].count(b"\n") == texts["cl_2.fq.gz"].count(b"\n") > 4 * 70
    one_batch, _ = _both(golden_dir, tmp_path / "one", reads, ["-k", "5"], names)
    assert one_batch == texts


def test_record_beyond_the_gzprintf_buffer_is_left_out(golden_dir, tmp_path):
    rng = np.random.default_rng(1)
    long_read = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=9000)])
    (tmp_path / "long.fa").write_bytes(b">short\nACGTACGTACGTAAAAAAAAAAAAAAAAAAAAAACGT\n>long9k\n" + long_read + b"\n>tail\nGGGGCCCCAAAATTTTACGTACGT\n")
    texts, _ = _both(golden_dir, tmp_path, ["-u", str(tmp_path / "long.fa")])
    both = texts["un.fq.gz"] + texts["cl.fq.gz"]
    assert b"long9k" not in both and b">short\n" in both and b">tail\n" in both


def test_single_cell_dumps_with_barcode_and_umi_files(golden_dir, tmp_path):
    man = json.load(open(os.path.join(CDIR, "manifest.json")))
    args = [a.format(G=GOLDEN, B=bf.BARCODE, C=CDIR, M=os.path.join(GOLDEN, "merge")) for a in man["cases"]["dump"]["args"]]
    assert args[-4:] == ["--un", "un", "--cl", "cl"]
    names = ("un.fq.gz", "un_bc.fa.gz", "un_um.fa.gz", "cl.fq.gz", "cl_bc.fa.gz", "cl_um.fa.gz")
    texts, _ = _both(golden_dir, tmp_path, args[:-4], ["--gpu-batch", "61"], names)
    for name in names:
        assert texts[name] == gzip.open(os.path.join(CDIR, name), "rb").read(), name
    assert texts["cl_bc.fa.gz"].startswith(b">")


def test_dump_read_back_gives_the_rows_of_those_reads(golden_dir, tmp_path):
    """the --cl file of a --gpu-dump run, fed back with -u (this tool's BGZF reader inflates its members in parallel), classifies to
    exactly the rows the first run printed for the classified reads"""
    se = os.path.join(golden_dir, "se.fq")
    first = _run(golden_dir, tmp_path / "first", ["-u", se], ["--gpu-dump", "--no-dust", "--gpu-batch", "40"])
    rows = first.stdout.split(b"\n")
    header, body = rows[0], [r for r in rows[1:] if r]
    want = [r for r in body if r.split(b"\t")[1] != b"unclassified"]
    assert 0 < len(want)
    again = subprocess.run([CLI, "-x", os.path.join(golden_dir, "f6"), "-u", str(tmp_path / "first" / "cl.fq.gz"), "--no-dust"], check=True, stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL).stdout
    assert again == b"\n".join([header] + want) + b"\n"


def test_nothing_classified_gives_an_empty_cl_file(golden_dir, tmp_path):
    (tmp_path / "n.fa").write_bytes(b"".join(b">n%d\n%s\n" % (i, b"N" * (40 + i)) for i in range(9)))
    texts, _ = _both(golden_dir, tmp_path, ["-u", str(tmp_path / "n.fa")])
    assert texts["cl.fq.gz"] == b"" and (tmp_path / "dev" / "cl.fq.gz").read_bytes() == EOF
    assert texts["un.fq.gz"].count(b">") == 9


def test_merge_readpair_keeps_the_host_writer(golden_dir, tmp_path):
    reads = ["-1", os.path.join(golden_dir, "pe_1.fq"), "-2", os.path.join(golden_dir, "pe_2.fq"), "--merge-readpair"]
    names = ("un_1.fq.gz", "un_2.fq.gz", "cl_1.fq.gz", "cl_2.fq.gz")
    host = _run(golden_dir, tmp_path / "host", reads)
    dev = _run(golden_dir, tmp_path / "dev", reads, ["--gpu-dump"])
    assert b"--gpu-dump is not used, the dumps are written on the host" in dev.stderr and b"--gpu-dump" not in host.stderr
    assert dev.stdout == host.stdout
    for name in names:
        assert (tmp_path / "dev" / name).read_bytes() == (tmp_path / "host" / name).read_bytes(), name


def test_switch_without_dumps_says_so_and_changes_nothing(golden_dir, tmp_path):
    base = [CLI, "-x", os.path.join(golden_dir, "f6"), "-u", os.path.join(golden_dir, "se.fq")]
    plain = subprocess.run(base, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(tmp_path))
    r = subprocess.run(base + ["--gpu-dump"], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(tmp_path))
    assert r.stdout == plain.stdout and b"--gpu-dump has no effect" in r.stderr and os.listdir(tmp_path) == []


def test_two_devices_each_compress_their_own_batches(golden_dir, tmp_path):
    if capi.device_count() < 2:
        pytest.skip("one GPU visible")
    reads = ["-1", os.path.join(golden_dir, "pe_1.fq"), "-2", os.path.join(golden_dir, "pe_2.fq")]
    _both(golden_dir, tmp_path, reads, ["--gpu", "0,1", "--gpu-batch", "20", "-k", "5"], ("un_1.fq.gz", "un_2.fq.gz", "cl_1.fq.gz", "cl_2.fq.gz"))
