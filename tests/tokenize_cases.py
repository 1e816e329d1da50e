"""Texts for the tokeniser's tests (cfr_tokenize): a restatement of the sequential grammar, regular texts, seeded mutations of them.
Shared by tests/test_tokenize_host_cpu.py, tests/test_tokenize_sanitized_cpu.py and tests/test_gpu_tokenize.py."""
import random

import numpy as np


def _lines(text):
    """SeqReader::next_line at the end of a file: (offset, content) of every line; content without '\\n' and trailing '\\r's; a last
    line without '\\n' only when something is left of it"""
    pos, n = 0, len(text)
    while True:
        nl = text.find(b"\n", pos)
        if nl < 0:
            tail = text[pos:].rstrip(b"\r")
            if pos < n and tail:
                yield pos, tail
            return
        yield pos, text[pos:nl].rstrip(b"\r")
        pos = nl + 1


def sequential_parse(text):
    """The sequential grammar (SeqReader::read_record, kseq's): [(header offset, id, bases)].  A sequence runs until a line that starts
    with '>', '@' or '+'; after '+' quality lines are read until they are as long as the sequence (at least one line)."""
    it = _lines(bytes(text))
    recs, hdr = [], None
    while True:
        while hdr is None:
            x = next(it, None)
            if x is None:
                return recs
            if x[1][:1] in (b">", b"@"):
                hdr = x
        off, h = hdr
        hdr = None
        e = 1
        while e < len(h) and h[e:e + 1] not in (b" ", b"\t"):
            e += 1
        idn = e - 1
        if idn >= 2 and h[e - 2:e - 1] == b"/" and h[e - 1:e] in (b"1", b"2"):
            idn -= 2
        seq = b""
        for x in it:
            line = x[1]
            if not line:
                continue
            if line[:1] in (b">", b"@"):
                hdr = x
                break
            if line[:1] == b"+":
                qn = 0
                for y in it:
                    qn += len(y[1])
                    if qn >= len(seq):
                        break
                break
            seq += line
        recs.append((off, h[1:1 + idn], seq))


def _fastq(recs, eol=b"\n", last_eol=True):
    t = b"".join(b"@" + h + eol + s + eol + b"+" + eol + q + eol for h, s, q in recs)
    return t if last_eol else t[:len(t) - len(eol)]


def _fasta(recs, width, eol=b"\n", last_eol=True):
    out = []
    for h, s, _ in recs:
        out.append(b">" + h + eol)
        out.extend(s[i:i + width] + eol for i in range(0, len(s), width))
    t = b"".join(out)
    return t if last_eol else t[:len(t) - len(eol)]


_rng = random.Random(20240611)


def _seq(n):
    return bytes(_rng.choice(b"ACGTacgtN") for _ in range(n))


RECS = [(b"r0", _seq(37), b"I" * 37), (b"r1/1 extra words", _seq(150), b"5" * 150), (b"r2\tcomment/2", _seq(61), b"#" * 61),
        (b"/1", _seq(5), b"IIIII"), (b"a/2", _seq(16), b"@" + b"F" * 15), (b"plus/2", _seq(17), b"+" + b"F" * 16),
        (b"long.id.with.dots/3", _seq(1), b"!"), (b"r7", _seq(95), b"@" * 95)]
EMPTY = [(b"e0", b"", b""), (b"e1 c", _seq(9), b"G" * 9), (b"e2", b"", b"")]

# name -> text; every one is regular: the tokeniser must give all of the sequential grammar's records
REGULAR = {
    "fq": _fastq(RECS),
    "fq_crlf": _fastq(RECS, b"\r\n"),
    "fq_crcrlf": _fastq(RECS, b"\r\r\n"),
    "fq_no_final_newline": _fastq(RECS, last_eol=False),
    "fq_crlf_no_final_newline": _fastq(RECS, b"\r\n", last_eol=False),
    "fq_empty_reads": _fastq(EMPTY + RECS[:2]),
    "fq_empty_last": _fastq(RECS[:2] + EMPTY),
    "fq_trailing_blank_lines": _fastq(RECS[:3]) + b"\n\r\n\n",
    "fa_1line": _fasta(RECS, 1 << 20),
    "fa_w1": _fasta(RECS[:4], 1),
    "fa_w60": _fasta(RECS, 60),
    "fa_w60_crlf": _fasta(RECS, 60, b"\r\n"),
    "fa_w60_crcrlf": _fasta(RECS, 60, b"\r\r\n"),
    "fa_no_final_newline": _fasta(RECS, 60, last_eol=False),
    "fa_empty_reads": _fasta(EMPTY + RECS[:2] + EMPTY, 60),
    "fa_blank_lines": _fasta(RECS[:3], 60).replace(b"\n>", b"\n\n>") + b"\n\n",
}
THREE_FQ = _fastq(RECS[:3])
THREE_FA = _fasta(RECS[:3], 20)

MUTATIONS = ("blank", "split_seq", "seq_plus", "seq_at", "seq_gt", "qual_short", "qual_long", "gt_header", "truncate")


def mutate(text, kind, rng):
    """one mutation of a regular text; lines are picked by their role in 4-line FASTQ, for FASTA among the lines that are no headers"""
    if kind == "truncate":
        return text[:rng.randrange(1, len(text))]
    lines = text.split(b"\n")
    body = lines[:-1] if lines[-1] == b"" else lines
    fq = text[:1] == b"@"
    role = (lambda want: [i for i in range(len(body)) if i % 4 == want]) if fq else (lambda want: [i for i in range(len(body)) if (body[i][:1] == b">") == (want in (0, 2))])
    if kind == "blank":
        body.insert(rng.randrange(len(body) + 1), rng.choice([b"", b"\r"]))
    elif kind == "split_seq":
        i = rng.choice(role(1))
        k = rng.randrange(len(body[i]) + 1)
        body[i:i + 1] = [body[i][:k], body[i][k:]]
    elif kind in ("seq_plus", "seq_at", "seq_gt"):
        i = rng.choice(role(1))
        body[i] = {"seq_plus": b"+", "seq_at": b"@", "seq_gt": b">"}[kind] + body[i][1:]
    elif kind == "qual_short":
        i = rng.choice(role(3))
        body[i] = body[i][1:]
    elif kind == "qual_long":
        i = rng.choice(role(3))
        body[i] = b"I" + body[i]
    elif kind == "gt_header":
        i = rng.choice(role(0))
        body[i] = (b">" if fq else b"@") + body[i][1:]
    return b"\n".join(body) + (b"\n" if lines[-1] == b"" else b"")


def mutation_corpus():
    """[(name, text)]: every regular text under every mutation, two seeds each (about 300)"""
    out = []
    for name, text in REGULAR.items():
        for kind in MUTATIONS:
            for seed in (1, 2):
                rng = random.Random(f"{name}:{kind}:{seed}")
                m = mutate(text, kind, rng)
                if m and m[:1] in (b">", b"@"):
                    out.append((f"{name}:{kind}:{seed}", m))
    return out


def run(tok, text, final=True, max_records=0):
    """tokenize + fetch -> (info, records, offsets, bases)"""
    info = tok.tokenize(text, final=final, max_records=max_records)
    rec, off, bases = tok.fetch()
    return info, rec, off, bases


def delivered(text, rec, off, bases):
    """what a tokeniser delivered, in the form of sequential_parse"""
    return [(int(r["header"]), text[int(r["header"]) + 1:int(r["header"]) + 1 + int(r["id_len"])], bytes(bases[int(off[i]):int(off[i + 1])]))
            for i, r in enumerate(rec)]


def info_fields(info):
    return (info.n_records, info.consumed, info.total_bases, info.irregular_at, info.fastq, info.irregular)


def assert_same(host, dev, what=""):
    """every field of two runs: cfr_token_info but the clock, records, offsets, bases"""
    assert info_fields(host[0]) == info_fields(dev[0]), what
    assert host[1].tobytes() == dev[1].tobytes(), what
    assert np.array_equal(host[2], dev[2]), what
    assert host[3].tobytes() == dev[3].tobytes(), what

