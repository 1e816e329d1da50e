"""`centrifuger --gpu-inflate`: -u files that are BGZF throughout go to the GPU compressed, are inflated there (cfr_inflate_bgzf) and
tokenised where the text lies (cfr_tokenize_resident).  The BGZF files are made here from the golden read files, with 997 text bytes
per member - records straddle members and pieces, long.fq's records force scouts over several members - and with 65280.  Where the
switch applies the TSV must be the golden one byte for byte and stderr must not speak of it; where it does not apply the output is
that of the run without the switch and stderr carries exactly one line that says why.  -m gpu."""
import gzip
import os
import struct
import subprocess
import zlib

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "centrifuger_amd", "bin", "centrifuger")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FILES = {"se.fq": "f6.se_default", "edge.fa": "f6.edge_default", "long.fq": "f6.long_default"}


def member(text, crc=None):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = c.compress(text) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(d) + 8 - 1) + d +
            struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text)))


def bgzf(text, per_member, flip_crc_of=None):
    ms = [member(text[i:i + per_member], None if k != flip_crc_of else zlib.crc32(text[i:i + per_member]) ^ 4) for k, i in enumerate(range(0, len(text), per_member))]
    return b"".join(ms) + EOF


def _run(args, check=True):
    r = subprocess.run(args, check=check, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return r.stdout, r.stderr, r.returncode


def _lines(stderr, what=b"--gpu-inflate"):
    return [l for l in stderr.split(b"\n") if what in l]


@pytest.fixture(scope="module")
def made(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf")
    out = {}
    for name in FILES:
        text = open(os.path.join(golden_dir, name), "rb").read()
        for per in (997, 65280):
            p = d / f"{name}.{per}.gz"
            p.write_bytes(bgzf(text, per))
            assert gzip.decompress(p.read_bytes()) == text
            out[name, per] = str(p)
    return out


@pytest.mark.parametrize("extra", [[], ["--gpu-format"], ["--gpu", "0,0"]], ids=["plain", "gpu_format", "two_workers"])
@pytest.mark.parametrize("per", [997, 65280])
@pytest.mark.parametrize("name", list(FILES))
def test_gpu_inflate_prints_the_golden_tsv(name, per, extra, made, golden_dir):
    out, err, _ = _run([CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "3", "--gpu-inflate", "--gpu-batch", "97", "-u", made[name, per]] + extra)
    assert out == open(os.path.join(GOLDEN, "tsv", FILES[name] + ".tsv"), "rb").read()
    assert not _lines(err) and not _lines(err, b"--gpu-parse"), err
    assert b"can be classified." in err and b"Centrifuger finishes." in err


def test_long_records_force_scouts_over_several_members(made, golden_dir):
    out, err, _ = _run([CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "3", "--gpu-inflate", "--gpu-batch", "5", "-u", made["long.fq", 997]])
    assert out == open(os.path.join(GOLDEN, "tsv", "f6.long_default.tsv"), "rb").read() and not _lines(err), err


def test_plain_and_bgzf_files_may_be_mixed(made, golden_dir):
    x = [CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "3", "--gpu-batch", "97", "-u", os.path.join(golden_dir, "se.fq"), "-u", made["se.fq", 997]]
    want, _, _ = _run(x)
    out, err, _ = _run(x + ["--gpu-inflate"])
    assert out == want and want.count(b"\n") > 40 and not _lines(err), err


def test_what_the_switch_does_not_cover_runs_as_without_it(made, golden_dir, tmp_path):
    se = open(os.path.join(golden_dir, "se.fq"), "rb").read()
    gz = tmp_path / "plain.fq.gz"
    with gzip.open(gz, "wb") as f:
        f.write(se)
    mixed = tmp_path / "bgzf_then_plain.fq.gz"                          # BGZF followed by a plain member
    half = se.index(b"\n@", len(se) // 2) + 1
    mixed.write_bytes(bgzf(se[:half], 997)[:-len(EOF)] + gzip.compress(se[half:]))
    mates = {}
    for m in ("pe_1.fq", "pe_2.fq"):
        mates[m] = tmp_path / (m + ".gz")
        mates[m].write_bytes(bgzf(open(os.path.join(golden_dir, m), "rb").read(), 997))
    x = ["-x", os.path.join(golden_dir, "f6"), "-t", "3", "--gpu-batch", "97"]
    for name, reads in (("gz", ["-u", str(gz)]), ("bgzf_then_plain", ["-u", str(mixed)]), ("mates", ["-1", str(mates["pe_1.fq"]), "-2", str(mates["pe_2.fq"])]),
                        ("un", ["-u", made["se.fq", 997], "--un", str(tmp_path / "un")])):
        want, err0, _ = _run([CLI] + x + reads)
        out, err, _ = _run([CLI] + x + reads + ["--gpu-inflate"])
        assert out == want and want.count(b"\n") > 20, name
        lines = _lines(err)
        assert not _lines(err0) and len(lines) == 1 and b"--gpu-inflate is not used, the file is inflated on the host:" in lines[0], (name, err)
        assert not _lines(err, b"--gpu-parse"), (name, err)
    # --gpu-parse alone on a .gz file is what it was: its one fall-back line
    _, err, _ = _run([CLI] + x + ["-u", str(gz), "--gpu-parse"])
    assert len(_lines(err, b"--gpu-parse is not used")) == 1 and not _lines(err)


def test_a_member_with_a_wrong_crc_ends_the_run_with_the_files_name(golden_dir, tmp_path):
    se = open(os.path.join(golden_dir, "se.fq"), "rb").read()
    bad = tmp_path / "crc_flipped.fq.gz"
    bad.write_bytes(bgzf(se, 997, flip_crc_of=40))
    x = [CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "3", "--gpu-batch", "97", "-u", str(bad)]
    for switch in ([], ["--gpu-inflate"]):
        _, err, rc = _run(x + switch, check=False)
        assert rc != 0, switch
        lines = [l for l in err.split(b"\n") if b"ERROR:" in l]
        assert lines and str(bad).encode() in lines[0] and b"does not inflate to what its trailer says" in lines[0], err


def test_an_irregular_record_sends_the_rest_to_the_host(golden_dir, tmp_path):
    """the one_bad shape of tests/test_gpu_parse_cli.py: 4-line FASTQ but for one multi-line record in the middle"""
    lines = open(os.path.join(golden_dir, "se.fq"), "rb").read().split(b"\n")[:-1]
    recs = [b"\n".join(r) + b"\n" for r in zip(*[iter(lines)] * 4)]
    h, s, p, q = lines[4 * 200:4 * 201]
    recs[200] = b"\n".join([h, s[:50], s[50:100], s[100:], p, q[:50], q[50:100], q[100:]]) + b"\n"
    one_bad = tmp_path / "one_bad.fq.gz"
    one_bad.write_bytes(bgzf(b"".join(recs), 997))
    x = [CLI, "-x", os.path.join(golden_dir, "f6"), "-t", "3", "--gpu-batch", "97", "-u", str(one_bad)]
    want, _, _ = _run(x)
    out, err, _ = _run(x + ["--gpu-inflate"])
    assert out == want == open(os.path.join(GOLDEN, "tsv", "f6.se_default.tsv"), "rb").read()
    assert len(_lines(err)) == 1 and b"--gpu-inflate stops here" in _lines(err)[0], err
