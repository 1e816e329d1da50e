#!/usr/bin/env python3
"""Regenerate tests/golden/taxworlds/*: what the REAL reference wrote for the worlds of tests/tax_worlds.py.  Dev container only (needs
oracle/_ref/centrifuger-build and oracle/_ref/centrifuger, which `make -C oracle ref` compiles where the reference's source lies):
    python tests/golden/make_golden_taxworlds.py

  text.1.cfr / text.4.cfr, <world>.2.cfr          the reference builder's index (--ftabchars 6) for the worlds of tax_worlds.COMMITTED:
                                                  forests, on which the native writers used to differ from it.  The worlds share
                                                  their text, so .1.cfr and .4.cfr are byte-equal among them and stored once
  <world>.<se|pe>_k<1|2|5>[.expand].tsv.gz        the reference classifier's stdout for the worlds' reads, every world
  <world>.quant_fmt<0|1>.txt.gz                   the reference centrifuger-quant's stdout for <world>.se_k5.tsv (CentrifugerQuant.cpp is
                                                  compiled where the reference's source lies, into the temporary directory)
  manifest.json                                   md5 of every file, and the node count and root of every committed index
The inputs (FASTA, nodes.dmp, names.dmp, seqid.map, FASTQ) are written from tax_worlds into a temporary directory; committed: data only."""
import gzip
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
REF_SRC = os.environ.get("CFR_REFERENCE_SRC", "/root/reference")
OUT = os.path.join(HERE, "taxworlds")
KS = (1, 2, 5)


def run(cmd, **kw):
    print("+", " ".join(cmd), file=sys.stderr)
    return subprocess.run(cmd, check=True, **kw)


def gz_write(path, data):
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(data)


def main():
    import tax_worlds as tw
    from centrifuger_amd import synth
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    tmp = tempfile.mkdtemp(prefix="cfr_golden_taxworlds_")
    indexes = {}
    quant = os.path.join(tmp, "centrifuger-quant")
    run(["g++", "-O3", "-msse4.2", "-w", f"-I{REF_SRC}", "-o", quant, os.path.join(REF_SRC, "CentrifugerQuant.cpp"), "-lpthread", "-lz"])
    for name in tw.NAMES:
        w = tw.make(name)
        d = os.path.join(tmp, name)
        synth.write_reference_inputs(w.genomes, d)
        tw.write_reads(w, d)
        prefix = os.path.join(d, "ref")
        run([os.path.join(REF_DIR, "centrifuger-build"), "-t", "2", "-r", os.path.join(d, "ref.fa"), "--taxonomy-tree", os.path.join(d, "nodes.dmp"),
             "--name-table", os.path.join(d, "names.dmp"), "--conversion-table", os.path.join(d, "seqid.map"), "-o", prefix,
             "--ftabchars", str(w.info["ftab_chars"])], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        if name in tw.COMMITTED:
            shutil.copy(prefix + ".2.cfr", os.path.join(OUT, name + ".2.cfr"))
            for ext in ("1", "4"):                                      # the worlds share their text: one copy
                dst = os.path.join(OUT, f"text.{ext}.cfr")
                if not os.path.exists(dst):
                    shutil.copy(f"{prefix}.{ext}.cfr", dst)
                assert open(dst, "rb").read() == open(f"{prefix}.{ext}.cfr", "rb").read(), (name, ext)
            raw = open(prefix + ".2.cfr", "rb").read()
            node_cnt = struct.unpack_from("<Q", raw, 0)[0]
            parents = [struct.unpack_from("<Q", raw, 24 + 16 * i)[0] for i in range(node_cnt)]
            indexes[name] = {"node_cnt": node_cnt, "root": next(i for i, p in enumerate(parents) if p == i)}
        for k in KS:
            for ends, files in (("se", ["-u", os.path.join(d, "se.fq")]), ("pe", ["-1", os.path.join(d, "p_1.fq"), "-2", os.path.join(d, "p_2.fq")])):
                for expand in (False, True):
                    r = run([os.path.join(REF_DIR, "centrifuger"), "-x", prefix, "-t", "2", "-k", str(k)] + files + (["--expand-taxid"] if expand else []),
                            stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
                    gz_write(os.path.join(OUT, f"{name}.{ends}_k{k}{'.expand' if expand else ''}.tsv.gz"), r.stdout)
                    if (k, ends, expand) == (5, "se", False):
                        tsv = os.path.join(d, "se_k5.tsv")
                        open(tsv, "wb").write(r.stdout)
        for fmt in (0, 1):                                              # the reference quantifier on its classifier's rows
            r = run([quant, "-x", prefix, "-c", tsv, "--output-format", str(fmt)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            gz_write(os.path.join(OUT, f"{name}.quant_fmt{fmt}.txt.gz"), r.stdout)
    manifest = {"ks": list(KS), "indexes": indexes,
                "md5": {f: hashlib.md5(open(os.path.join(OUT, f), "rb").read()).hexdigest() for f in sorted(os.listdir(OUT))}}
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    shutil.rmtree(tmp)
    print("wrote", OUT, file=sys.stderr)


if __name__ == "__main__":
    main()
