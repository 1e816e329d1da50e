"""`centrifuger --gpu-format`: the TSV rows made on the GPU that classified the reads (cfr_device_index_set_tsv -> _tsv_last, with
--gpu-parse _tsv_last_resident: the read ids never leave the device).  Where the switch applies the TSV must be the golden one byte for
byte; where it does not, the output must be that of the run without the switch and stderr carries one line that says why.  -m gpu."""
import gzip
import json
import os
import subprocess

import pytest

import barcode_fixtures as bf
import quant_fixtures as qf
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
CASES = sorted(c for c, v in MAN["cases"].items() if any(a in ("se.fq", "edge.fa", "pe_1.fq") for a in v["args"]))      # those of tests/test_gpu_parse_cli.py
RERUN = {"CFR_DEBUG_ENV": "1", "CFR_POOL_INIT": "3", "CFR_SUBBATCH": "50", "CFR_TAPER_FLOOR": "0"}      # tests/test_gpu_kreport.py: sub-batches computed again


def _args(args, gd):
    return [os.path.join(gd, a) if a.endswith((".fq", ".fa")) else a for a in args]


def _run(args, env=None):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr


def _lines(stderr, what):
    return [l for l in stderr.split(b"\n") if what in l]


@pytest.mark.parametrize("case", CASES)
def test_gpu_format_prints_the_golden_tsv(case, golden_dir):
    c = MAN["cases"][case]
    want = open(os.path.join(GOLDEN, "tsv", case + ".tsv"), "rb").read()
    base = [CLI, "-x", os.path.join(golden_dir, c["index"]), "-t", "3"]
    out, err = _run(base + ["--gpu-format", "--gpu-batch", "97"] + _args(c["args"], golden_dir))
    assert out == want
    assert not _lines(err, b"--gpu-format") and b"can be classified." in err and b"Centrifuger finishes." in err
    # with --gpu-parse the ids come from the tokeniser's tables in HBM; two workers on one device keep the input order
    out, err = _run(base + ["--gpu-format", "--gpu-parse", "--gpu", "0,0", "--gpu-batch", "23"] + _args(c["args"], golden_dir))
    assert out == want
    assert not _lines(err, b"--gpu-format") and not _lines(err, b"--gpu-parse"), err


@pytest.fixture(scope="module")
def q8_reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("format_reads")
    for f in ("reads_se.fq", "reads_1.fq", "reads_2.fq"):
        (d / f).write_bytes(gzip.open(os.path.join(qf.QDIR, f + ".gz"), "rb").read())
    return d


OTHERS = {"promote": ("pe", ["--promote", "genus"], None), "kreport": ("pe", ["--kreport", "{d}/k.txt"], "k.txt"),
          "kreport_promote": ("se", ["--kreport", "{d}/k.txt", "--promote", "species"], "k.txt"), "quant": ("pe", ["--quant", "{d}/q.tsv"], "q.tsv"),
          "nodust": ("se", ["--no-dust"], None), "un": ("se", ["--un", "{d}/un"], "un.fq.gz")}


@pytest.mark.parametrize("parse", [[], ["--gpu-parse"]], ids=["host_parse", "gpu_parse"])
@pytest.mark.parametrize("name", sorted(OTHERS))
def test_the_other_switches_work_as_without_it(name, parse, q8_reads, tmp_path):
    """--promote, --kreport, --quant, --no-dust and --un: output and side files equal the run without --gpu-format"""
    which, extra, side = OTHERS[name]
    reads = ["-1", str(q8_reads / "reads_1.fq"), "-2", str(q8_reads / "reads_2.fq"), "-k", "5"] if which == "pe" else ["-u", str(q8_reads / "reads_se.fq")]
    base = [CLI, "-x", qf.PREFIX, "-t", "2", "--gpu-batch", "300"]
    outs = []
    for tag, switch in (("a", []), ("b", ["--gpu-format"] + parse)):
        d = tmp_path / tag
        d.mkdir()
        out, err = _run(base + reads + [e.format(d=d) for e in extra] + switch)
        data = (d / side).read_bytes() if side else b""
        outs.append((out, gzip.decompress(data) if side and side.endswith(".gz") else data, err))
    assert outs[0][0] == outs[1][0] and outs[0][0].count(b"\n") > 100
    assert outs[0][1] == outs[1][1] and (not side or outs[0][1])
    assert not _lines(outs[1][2], b"--gpu-format")
    counts = [[l[l.index(b"Processed"):] for l in _lines(o[2], b"can be classified.")] for o in outs]          # (behind the time stamp)
    assert counts[0] == counts[1] and len(counts[0]) == 1                                                    # the count of classified reads


@pytest.mark.parametrize("key", ["se_k1", "pe_k5"])
def test_recomputed_sub_batches_overwrite_their_rows(key, q8_reads):
    """a fresh child under the re-run recipe: sub-batches whose scratch pool ran dry are computed again after copy_out has kept them"""
    reads = ["-u", str(q8_reads / "reads_se.fq"), "-k", "1"] if key == "se_k1" else ["-1", str(q8_reads / "reads_1.fq"), "-2", str(q8_reads / "reads_2.fq"), "-k", "5"]
    out, _err = _run([CLI, "-x", qf.PREFIX, "-t", "2", "--gpu-format"] + reads, env=RERUN)
    assert out == gzip.open(qf.tsv_path(key), "rb").read()


def test_what_the_switch_does_not_cover_runs_as_without_it(golden_dir):
    se = os.path.join(golden_dir, "se.fq")
    x = [CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "3", "--gpu-batch", "97"]
    cdir = os.path.join(bf.BARCODE, "cli")
    for name, reads in (("expand", ["-u", se, "--expand-taxid"]),
                        ("barcode", ["-u", se, "--barcode", os.path.join(cdir, "bc.fq.gz"), "--UMI", os.path.join(cdir, "um.fq.gz")])):
        want, err0 = _run(x + reads)
        for parse in ([], ["--gpu-parse"]):
            out, err = _run(x + reads + ["--gpu-format"] + parse)
            assert out == want and want.count(b"\n") > 20, name
            assert not _lines(err0, b"--gpu-format") and len(_lines(err, b"--gpu-format is not used")) == 1 and len(_lines(err, b"--gpu-format")) == 1, (name, err)


def test_help_lists_the_switch():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--gpu-format" in r.stdout + r.stderr
