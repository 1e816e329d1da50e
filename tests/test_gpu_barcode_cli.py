"""Single-cell input through the command line (centrifuger_amd/bin/centrifuger: --barcode, --UMI, --read-format, --barcode-whitelist,
--barcode-translate) against what the reference's own command line printed for the same files (tests/golden/barcode/cli,
make_golden_barcode.py): TSV and --un / --cl dumps byte for byte, and the refusals.  -m gpu."""
import gzip
import json
import os
import subprocess

import pytest

import barcode_fixtures as bf
from centrifuger_amd import capi
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
CDIR = os.path.join(bf.BARCODE, "cli")
MAN = json.load(open(os.path.join(CDIR, "manifest.json")))
WHERE = {"G": GOLDEN, "M": os.path.join(GOLDEN, "merge"), "B": bf.BARCODE, "C": CDIR}


def _run(golden_dir, args, extra=(), cwd=None):
    return subprocess.run([CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "3"] + list(extra) + [a.format(**WHERE) for a in args],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=cwd)


def _want(case):
    return gzip.open(os.path.join(CDIR, "tsv", case + ".tsv.gz"), "rb").read()


@pytest.mark.parametrize("case", sorted(c for c in MAN["cases"] if c != "dump"))
def test_cli_equals_reference_tsv_with_two_batch_sizes(case, golden_dir):
    want = _want(case)
    assert want.count(b"\n") > 300
    for batch in ("97", "100000"):
        r = _run(golden_dir, MAN["cases"][case]["args"], ["--gpu-batch", batch])
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == want, (case, batch)
        assert b"can be classified." in r.stderr and b"Centrifuger finishes." in r.stderr


def test_cli_dumps_equal_reference(golden_dir, tmp_path):
    r = _run(golden_dir, MAN["cases"]["dump"]["args"], ["--gpu-batch", "61"], cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == _want("dump")
    assert len(MAN["dumps"]) == 6
    for name in MAN["dumps"]:
        assert gzip.open(tmp_path / name, "rb").read() == gzip.open(os.path.join(CDIR, name), "rb").read(), name


def test_cli_on_every_gpu_equals_one_gpu(golden_dir):
    if capi.device_count() < 2:
        pytest.skip("one GPU visible")
    for case in ("whitelist_fq", "pe_merge_k5"):
        r = _run(golden_dir, MAN["cases"][case]["args"], ["--gpu", "all", "--gpu-batch", "53"])
        assert r.returncode == 0 and r.stdout == _want(case), case


@pytest.mark.parametrize("name", sorted(MAN["refusals"]))
def test_cli_refuses_like_the_reference(name, golden_dir):
    c = MAN["refusals"][name]
    r = _run(golden_dir, c["args"])
    assert r.returncode == c["returncode"] != 0
    assert c["message"].encode() in r.stderr


def test_cli_refusals_of_its_own(golden_dir):
    r = _run(golden_dir, ["-u", "{G}/se.fq", "--barcode", "{C}/bc_hd.fq.gz", "--read-format", "bc:hd:CB:5:-1", "--barcode-whitelist", "{B}/wl16.txt.gz"])
    assert r.returncode != 0 and b"bc:hd:" in r.stderr and r.stdout == b""
    r = _run(golden_dir, ["-u", "{G}/se.fq", "--barcode-whitelist", "{B}/wl16.txt.gz"])
    assert r.returncode != 0 and b"Barcode whitelist has to be used with --barcode option" in r.stderr
    r = _run(golden_dir, ["--sample-sheet", "sheet.txt"])
    assert r.returncode != 0 and b"--sample-sheet" in r.stderr
    r = _run(golden_dir, ["-u", "{G}/se.fq", "--UMI", "{C}/bc_short.fq.gz"])
    assert r.returncode != 0 and b"The UMI file and read file have different number of reads." in r.stderr


def test_cli_missing_translation_exits_255(golden_dir, tmp_path):
    table = tmp_path / "tr.txt"
    table.write_text("cellA\tACGTACGTACGTACGT\n")
    r = _run(golden_dir, ["-u", "{G}/se.fq", "--barcode", "{C}/bc.fq.gz", "--barcode-translate", str(table)])
    assert r.returncode == 255 and b"does not exist in the translation table." in r.stderr
