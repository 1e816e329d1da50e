"""`centrifuger --gpu-dump --gpu-dump-codes dynamic` against the same command line without --gpu-dump (the host writer) and with
--gpu-dump alone: stdout is the same, every file inflates to the same bytes and is BGZF closed by the end-of-file member, some member
has a dynamic block, and no file is larger than the fixed code's.  -m gpu."""
import gzip
import os
import subprocess

import pytest

import gz_cases as gc
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _run(golden_dir, cwd, reads, extra=()):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "3"] + list(reads) + ["--un", "un", "--cl", "cl"] + list(extra),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(cwd))


def _three(golden_dir, tmp_path, reads, extra, files):
    host = _run(golden_dir, tmp_path / "host", reads, extra)
    fixed = _run(golden_dir, tmp_path / "fixed", reads, list(extra) + ["--gpu-dump"])
    dyn = _run(golden_dir, tmp_path / "dyn", reads, list(extra) + ["--gpu-dump", "--gpu-dump-codes", "dynamic"])
    for r in (host, fixed, dyn):
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert dyn.stdout == host.stdout == fixed.stdout
    assert sorted(os.listdir(tmp_path / "dyn")) == sorted(files)
    dynamic_members = 0
    for name in files:
        raw = (tmp_path / "dyn" / name).read_bytes()
        assert raw.endswith(EOF), name
        members = gc.walk(raw)
        assert members[-1] == (28, b"\x03\x00", 0, 0) and all(m[3] > 0 for m in members[:-1])
        dynamic_members += sum(1 for m in members if (m[1][0] >> 1) & 3 == 2)
        assert gzip.decompress(raw) == gzip.open(tmp_path / "host" / name).read(), name
        assert len(raw) <= os.path.getsize(tmp_path / "fixed" / name), name
    assert dynamic_members > 0
    assert b"--gpu-dump-codes" not in dyn.stderr


def test_single_end_fasta_dumps(golden_dir, tmp_path):
    _three(golden_dir, tmp_path, ["-u", os.path.join(golden_dir, "edge.fa")], [], ("un.fq.gz", "cl.fq.gz"))


def test_paired_fastq_dumps_in_several_batches(golden_dir, tmp_path):
    reads = ["-1", os.path.join(golden_dir, "pe_1.fq"), "-2", os.path.join(golden_dir, "pe_2.fq")]
    _three(golden_dir, tmp_path, reads, ["--gpu-batch", "70", "-k", "5"], ("un_1.fq.gz", "un_2.fq.gz", "cl_1.fq.gz", "cl_2.fq.gz"))


def test_fixed_is_the_default_and_may_be_named(golden_dir, tmp_path):
    reads = ["-u", os.path.join(golden_dir, "edge.fa")]
    a = _run(golden_dir, tmp_path / "a", reads, ["--gpu-dump"])
    b = _run(golden_dir, tmp_path / "b", reads, ["--gpu-dump", "--gpu-dump-codes", "fixed"])
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout
    for name in ("un.fq.gz", "cl.fq.gz"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()


def test_a_bad_value_is_a_usage_error(golden_dir, tmp_path):
    r = _run(golden_dir, tmp_path, ["-u", os.path.join(golden_dir, "edge.fa")], ["--gpu-dump", "--gpu-dump-codes", "best"])
    assert r.returncode != 0 and b"--gpu-dump-codes is 'fixed' or 'dynamic'" in r.stderr and r.stdout == b""


def test_dynamic_without_gpu_dump_says_so_and_changes_nothing(golden_dir, tmp_path):
    reads = ["-u", os.path.join(golden_dir, "edge.fa")]
    plain = _run(golden_dir, tmp_path / "plain", reads)
    r = _run(golden_dir, tmp_path / "dyn", reads, ["--gpu-dump-codes", "dynamic"])
    assert plain.returncode == 0 and r.returncode == 0 and r.stdout == plain.stdout
    assert r.stderr.count(b"--gpu-dump-codes dynamic has no effect") == 1 and b"--gpu-dump-codes" not in plain.stderr
    for name in ("un.fq.gz", "cl.fq.gz"):
        assert (tmp_path / "dyn" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
