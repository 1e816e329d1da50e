"""`centrifuger --gpu-parse`: the read files tokenised on the GPU that classifies them (cfr_tokenize -> cfr_classify_batch_resident).
Where the switch applies the TSV must be the golden one byte for byte and stderr must not speak of a fall-back; where it does not
apply the output must be that of the run without the switch, and stderr carries one line that says why.  -m gpu."""
import gzip
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
CASES = sorted(c for c, v in MAN["cases"].items() if any(a in ("se.fq", "edge.fa", "pe_1.fq") for a in v["args"]))


def _args(args, gd):
    return [os.path.join(gd, a) if a.endswith((".fq", ".fa")) else a for a in args]


def _run(args):
    r = subprocess.run(args, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return r.stdout, r.stderr


def _fallback_lines(stderr):
    return [l for l in stderr.split(b"\n") if b"--gpu-parse" in l]


@pytest.mark.parametrize("case", CASES)
def test_gpu_parse_prints_the_golden_tsv(case, golden_dir):
    c = MAN["cases"][case]
    out, err = _run([CLI, "-x", os.path.join(golden_dir, c["index"]), "-t", "3", "--gpu-parse", "--gpu-batch", "97"] + _args(c["args"], golden_dir))
    assert out == open(os.path.join(GOLDEN, "tsv", case + ".tsv"), "rb").read()
    assert not _fallback_lines(err), err
    assert b"can be classified." in err and b"Centrifuger finishes." in err


@pytest.mark.parametrize("case", ["f6.se_default", "f6.pe_k5", "f6.edge_default"])
def test_two_workers_on_one_device_keep_input_order(case, golden_dir):
    c = MAN["cases"][case]
    out, err = _run([CLI, "-x", os.path.join(golden_dir, c["index"]), "-t", "4", "--gpu-parse", "--gpu-batch", "23", "--gpu", "0,0"] + _args(c["args"], golden_dir))
    assert out == open(os.path.join(GOLDEN, "tsv", case + ".tsv"), "rb").read()
    assert not _fallback_lines(err), err


@pytest.mark.parametrize("reads", [["-u", "se.fq"], ["-1", "pe_1.fq", "-2", "pe_2.fq", "-k", "5"], ["-u", "edge.fa"]], ids=["se", "pe_k5", "edge"])
@pytest.mark.parametrize("extra", [["--promote", "genus"], ["--promote", "genus", "--no-dust"], ["--no-dust"]], ids=["promote", "promote_nodust", "nodust"])
def test_promote_and_dust_work_as_without_the_switch(reads, extra, golden_dir):
    base = [CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "2", "--gpu-batch", "97"] + _args(reads, golden_dir) + extra
    want, _ = _run(base)
    out, err = _run(base + ["--gpu-parse"])
    assert out == want and want.count(b"\n") > 20
    assert not _fallback_lines(err), err


def test_what_the_switch_does_not_cover_runs_as_without_it(golden_dir, tmp_path):
    se = os.path.join(golden_dir, "se.fq")
    text = open(se, "rb").read()
    gz = tmp_path / "se.fq.gz"
    with gzip.open(gz, "wb") as f:
        f.write(text)
    lines = text.split(b"\n")[:-1]
    multi = tmp_path / "multi.fq"          # multi-line FASTQ: sequence and quality on two lines each
    multi.write_bytes(b"".join(b"\n".join([h, s[:70], s[70:], p, q[:70], q[70:]]) + b"\n" for h, s, p, q in zip(*[iter(lines)] * 4)))
    one_bad = tmp_path / "one_bad.fq"      # 4-line FASTQ but for one record in the middle, the line count still a multiple of 4:
    recs = [b"\n".join(r) + b"\n" for r in zip(*[iter(lines)] * 4)]      # the cutter accepts the file, a piece comes back irregular
    h, s, p, q = lines[4 * 200:4 * 201]
    recs[200] = b"\n".join([h, s[:50], s[50:100], s[100:], p, q[:50], q[50:100], q[100:]]) + b"\n"
    one_bad.write_bytes(b"".join(recs))
    x = ["-x", os.path.join(golden_dir, "f6"), "-t", "3", "--gpu-batch", "97"]
    for name, reads in (("un", ["-u", se, "--un", str(tmp_path / "un")]), ("gz", ["-u", str(gz)]), ("multi", ["-u", str(multi)]), ("one_bad", ["-u", str(one_bad)]),
                        ("interleaved", ["-i", se]), ("merge", ["-1", os.path.join(golden_dir, "pe_1.fq"), "-2", os.path.join(golden_dir, "pe_2.fq"), "--merge-readpair"])):
        want, err0 = _run([CLI] + x + reads)
        out, err = _run([CLI] + x + reads + ["--gpu-parse"])
        assert out == want, name
        assert not _fallback_lines(err0) and len(_fallback_lines(err)) == 1, (name, err)
    assert want.count(b"\n") > 20
    golden = open(os.path.join(GOLDEN, "tsv", "f6.se_default.tsv"), "rb").read()
    for f in (gz, multi, one_bad):
        assert _run([CLI] + x + ["-u", str(f), "--gpu-parse"])[0] == golden
