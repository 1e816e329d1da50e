"""Writes tests/golden/buildsel: what the reference's centrifuger-build (oracle/_ref, compiled by `make -C oracle`) writes for the runs of
tests/buildsel_world.py - .1.cfr (gzipped), .2.cfr, .3.cfr - and what the reference's classifier prints on each index for the world's
reads.  Data only.  Run from the repository root: python tests/golden/buildsel/make_golden_buildsel.py"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import buildsel_world as bw  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        p = bw.write_inputs(tmp)
        for name, args in bw.runs(p).items():
            prefix = os.path.join(tmp, name)
            subprocess.run([os.path.join(REF, "centrifuger-build"), "-t", "1"] + args + bw.common(p, prefix), check=True, stderr=subprocess.DEVNULL)
            with open(prefix + ".1.cfr", "rb") as fi, gzip.GzipFile(os.path.join(HERE, name + ".1.cfr.gz"), "wb", mtime=0) as fo:
                fo.write(fi.read())
            for k in (2, 3):
                open(os.path.join(HERE, f"{name}.{k}.cfr"), "wb").write(open(f"{prefix}.{k}.cfr", "rb").read())
            tsv = subprocess.run([os.path.join(REF, "centrifuger"), "-x", prefix, "-u", p["reads"], "-t", "1"], check=True, stdout=subprocess.PIPE,
                                 stderr=subprocess.DEVNULL).stdout
            open(os.path.join(HERE, name + ".tsv"), "wb").write(tsv)
            print(name, os.path.getsize(prefix + ".1.cfr"), "bytes of .1.cfr,", tsv.count(b"\n") - 1, "TSV rows")


if __name__ == "__main__":
    main()
