"""The inputs of the selection tests (tests/test_build_select_cpu.py, tests/test_gpu_build_select.py) and of the golden set
tests/golden/buildsel: a world of 3 species x 2 strains x 3 kbp (centrifuger_amd/synth.py), every strain cut into two contigs of its own
tax id, as one FASTA and as one file per strain; and the runs of the reference builder the goldens come from."""
import os

import numpy as np

from centrifuger_amd import synth

SEED, FTAB = 77, 6
GENUS0 = 1000                       # Genus0: species0 and species1 (make_genomes numbers the nodes from 1000 on)


def genomes():
    return synth.make_genomes(n_species=3, n_strains=2, genome_len=3000, seed=SEED)


def _record(name, s, width=70):
    s = bytes(s)
    return b">" + name.encode() + b" a contig\n" + b"".join(s[a:a + width] + b"\n" for a in range(0, len(s), width))


def write_inputs(outdir):
    """-> dict of the paths: nodes, names, seqid.map, ref.fa, ref_uncat.fa, files.list (file -> strain tax id), species.list (file -> species tax id)"""
    g = genomes()
    os.makedirs(outdir, exist_ok=True)
    synth.write_reference_inputs(g, outdir)
    parent = {t: p for t, p, _ in g.nodes}
    contigs, files = [], []
    rng = np.random.default_rng(SEED)
    for name, tid, s in zip(g.names, g.taxids, g.seqs):
        stem = name[:-2]
        a, b = _record(stem + ".1", s[:1400]), _record(stem + ".2", s[1400:])
        contigs += [(stem + ".1", tid, a), (stem + ".2", tid, b)]
        # the extensions GetFileBaseName strips: .fna, .fa, .fasta, and a second one behind them
        ext = [".fna", ".fa", ".fasta.txt", ".fna", ".faa", ".fa"][len(files)]
        path = os.path.join(outdir, stem + ext)
        open(path, "wb").write(a + b)
        files.append((path, tid, parent[tid]))
    p = {k: os.path.join(outdir, v) for k, v in dict(nodes="nodes.dmp", names="names.dmp", map="contigs.map", ref="contigs.fa", uncat="contigs_uncat.fa",
                                                    files="files.list", species="species.list").items()}
    open(p["ref"], "wb").write(b"".join(c[2] for c in contigs))
    extra = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=900)])
    open(p["uncat"], "wb").write(b"".join(c[2] for c in contigs[:5]) + _record("uncategorized_contig", extra) + b"".join(c[2] for c in contigs[5:]))
    open(p["map"], "w").write("".join(f"{n}\t{t}\n" for n, t, _ in contigs))
    open(p["files"], "w").write("".join(f"{f}\t{t}\n" for f, t, _ in files))
    open(p["species"], "w").write("".join(f"{f}\t{sp}\n" for f, _, sp in files))
    reads = synth.make_reads(g, 60, 100, seed=5)
    p["reads"] = os.path.join(outdir, "reads.fq")
    synth.write_fastq(reads, p["reads"])
    return p


# name -> the builder's arguments behind "--taxonomy-tree .. --name-table .. --ftabchars 6 -o .."
def runs(p):
    return {
        "concat": ["-r", p["ref"], "--conversion-table", p["map"], "--concat-tax-genome"],
        "subset": ["-r", p["ref"], "--conversion-table", p["map"], "--subset-tax", str(GENUS0)],
        "filelist": ["-l", p["files"]],
        "filelist_concat": ["-l", p["species"], "--concat-tax-genome"],
        "concat_uncat": ["-r", p["uncat"], "--conversion-table", p["map"], "--concat-tax-genome"],
    }


def common(p, prefix):
    return ["--taxonomy-tree", p["nodes"], "--name-table", p["names"], "--ftabchars", str(FTAB), "-o", prefix]


# the same runs for tools/dbg/select_writer_host.cpp: TABLE FILE_LEVEL CONCAT SUBSET_TAX IGNORE_UNCATEGORIZED, FASTA...
def host_runs(p):
    files = [ln.split("\t")[0] for ln in open(p["files"]).read().splitlines()]
    return {
        "concat": ([p["map"], "0", "1", "0", "0"], [p["ref"]]),
        "subset": ([p["map"], "0", "0", str(GENUS0), "0"], [p["ref"]]),
        "filelist": ([p["files"], "1", "0", "0", "0"], files),
        "filelist_concat": ([p["species"], "1", "1", "0", "0"], files),
        "concat_uncat": ([p["map"], "0", "1", "0", "0"], [p["uncat"]]),
    }
