"""The texts and read dumps the compressor tests share (tests/test_gz_host_cpu.py, test_gz_sanitized_cpu.py, test_gpu_gz.py), the
walk over BGZF members that checks their framing, the dump texts as plain Python builds them, and the corpus file of
tools/gz_sanitize.cpp.  Everything is made once per process and handed out unchanged."""
import functools
import struct
import zlib

import numpy as np

# htslib's block size, and one that gives many blocks and a short last one.  (A random byte costs 8.44 bits on average in the fixed code, so
# a random block is stored only from about 70 bytes on: 251 leaves the 200 000 random bytes a last block of 204 bytes, 8 standard deviations
# above that; 257 would leave 54 bytes, which the fixed code may well undercut.)
BLOCKS = (65280, 251)
RECORD_LIMIT = 8192            # gzprintf drops a record of this many bytes or more (test_gz_host_cpu.py pins it against zlib)


def _rand(rng, n, lo=0, hi=256):
    return rng.integers(lo, hi, n).astype(np.uint8).tobytes()


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def fastq_like(rng, n_reads, read_len=150):
    """reads drawn from one 20 kbp random genome with 1% substitutions, qualities from a short alphabet: text that deflate can shorten"""
    genome = np.frombuffer(_acgt(rng, 20000), dtype=np.uint8)
    out = []
    for i in range(n_reads):
        at = int(rng.integers(0, len(genome) - read_len))
        s = genome[at:at + read_len].copy()
        flip = rng.random(read_len) < 0.01
        s[flip] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(flip.sum()))]
        q = np.frombuffer(b"FFFF:,#", dtype=np.uint8)[np.minimum(rng.geometric(0.6, read_len) - 1, 6)]
        out.append(b"@r%d/1 sim:%07d\n" % (i, at) + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    return b"".join(out)


def _planted(rng, distance, length=300):
    """text over ACGT whose last `length` bytes repeat the bytes `distance` in front of them"""
    a = _acgt(rng, distance)
    return a + a[:length]


@functools.lru_cache(maxsize=None)
def texts(block_bytes):
    """name -> text, for one block size"""
    rng = np.random.default_rng(20260 + block_bytes)
    r40 = _rand(rng, 40000)
    a40 = _acgt(rng, 40000)
    t = {
        "empty": b"",
        "one_byte": b"x",
        "two_bytes": b"xy",
        "exactly_a_block": _acgt(rng, block_bytes),
        "a_block_and_one": _acgt(rng, block_bytes + 1),
        "equal_1000": b"a" * 1000,
        "all_bytes_x300": bytes(range(256)) * 300,
        "random_40000_twice": (r40 + r40)[:65280],
        "acgt_40000_twice": (a40 + a40)[:65280],
        "repeat_at_32768": _planted(rng, 32768),
        "repeat_at_32769": _planted(rng, 32769),
        "random_200k": _rand(rng, 200000),
        "fastq_1mb": fastq_like(rng, 3000),
    }
    return t


def walk(data):
    """the members of a BGZF byte string -> [(member size, deflate bytes, crc32, isize)]; asserts the framing"""
    out, at = [], 0
    while at < len(data):
        assert len(data) - at >= 26, "a member needs 26 bytes at least"
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04", f"no gzip header with FEXTRA at {at}"
        xlen, = struct.unpack_from("<H", data, at + 10)
        assert xlen == 6 and data[at + 12:at + 16] == b"BC\x02\x00", f"no BC field at {at}"
        bsize, = struct.unpack_from("<H", data, at + 16)
        size = bsize + 1
        assert size <= 65536 and at + size <= len(data)
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        out.append((size, data[at + 18:at + size - 8], crc, isize))
        at += size
    return out


def check_members(out, text, block_bytes):
    """every member of `out` frames and encodes its block of `text` -> (members, stored members)"""
    members = walk(out)
    assert len(members) == (len(text) + block_bytes - 1) // block_bytes
    stored = 0
    for k, (size, deflate, crc, isize) in enumerate(members):
        piece = text[k * block_bytes:(k + 1) * block_bytes]
        assert isize == len(piece) and crc == zlib.crc32(piece), f"member {k}: CRC32 / ISIZE"
        d = zlib.decompressobj(-15)
        assert d.decompress(deflate) == piece and d.eof and d.unused_data == b"", f"member {k}: the deflate part"
        assert deflate[0] & 1 == 1, f"member {k}: BFINAL"
        if (deflate[0] >> 1) & 3 == 0:
            stored += 1
            assert len(deflate) == 5 + len(piece)
        else:
            assert (deflate[0] >> 1) & 3 == 1 and len(deflate) < 5 + len(piece), f"member {k}: a fixed stream no smaller than a stored block"
    return len(members), stored


# ---- read dumps: (ids, select, files); a file is (sequences, qualities or None, has_qual or None) ----
def _reads(rng, n, lens, with_qual=True, has=None):
    seqs = [_acgt(rng, int(l)) for l in lens]
    if not with_qual:
        return (seqs, None, None)
    has = np.ones(n, dtype=np.uint8) if has is None else np.asarray(has, dtype=np.uint8)
    quals = [_rand(rng, len(s), 33, 74) if h else b"" for s, h in zip(seqs, has)]
    return (seqs, quals, has)


def _record_seq_len(total, id_len, qual):
    """the sequence length that makes a record of `total` bytes"""
    return (total - id_len - 6) // 2 if qual else total - id_len - 3


@functools.lru_cache(maxsize=None)
def dump_cases():
    rng = np.random.default_rng(4711)
    n = 300
    ids = [b"read.%d" % i for i in range(n)]
    lens = rng.integers(30, 200, n)
    pe = [_reads(rng, n, lens), _reads(rng, n, rng.integers(30, 200, n))]
    cases = {
        "select_all": (ids, np.ones(n, np.uint8), pe),
        "select_none": (ids, np.zeros(n, np.uint8), pe),
        "select_alternating": (ids, (np.arange(n) % 2).astype(np.uint8), pe),
        "no_reads": ([], np.zeros(0, np.uint8), [([], [], np.zeros(0, np.uint8))]),
    }
    # reads of length 0, ids of length 0 and 1, mixed has_qual
    m = 40
    ids2 = [b"", b"a"] + [b"id%d" % i for i in range(m - 2)]
    has = (rng.random(m) < 0.5).astype(np.uint8)
    lens2 = rng.integers(0, 3, m) * rng.integers(0, 60, m)
    cases["edges_mixed_qual"] = (ids2, (rng.random(m) < 0.8).astype(np.uint8), [_reads(rng, m, lens2, has=has), _reads(rng, m, lens2[::-1], with_qual=False)])
    # the drop rule, per file and per record: mate 1 of 8191 bytes beside mate 2 of 8192, 8193, 9000; and the other way round; FASTA records too
    tot1 = [8190, 8191, 8191, 8192, 8193, 100, 8191, 12001]
    tot2 = [8191, 8192, 9001, 8191, 8190, 8192, 8193, 100]
    # (a FASTQ record is its id, 6 bytes and twice the sequence: the id's length takes the parity of the total)
    ids3 = [(b"b%d" if t % 2 == 0 else b"bb%d") % i for i, t in enumerate(tot1)]
    f1 = _reads(rng, 8, [_record_seq_len(t, len(i), True) for t, i in zip(tot1, ids3)])
    f2 = _reads(rng, 8, [_record_seq_len(t, len(i), False) for t, i in zip(tot2, ids3)], with_qual=False)
    assert [len(record(i, s, q)) for i, s, q in zip(ids3, f1[0], f1[1])] == tot1 and [len(record(i, s, None)) for i, s in zip(ids3, f2[0])] == tot2
    cases["drop_rule"] = (ids3, np.ones(8, np.uint8), [f1, f2])
    # barcode / UMI descriptors: strings, never a quality
    k = 100
    ids4 = [b"cell%d" % i for i in range(k)]
    cases["barcode_umi"] = (ids4, (np.arange(k) % 3 != 0).astype(np.uint8),
                            [_reads(rng, k, rng.integers(20, 90, k)), _reads(rng, k, np.full(k, 16), with_qual=False), _reads(rng, k, np.full(k, 10), with_qual=False),
                             _reads(rng, k, rng.integers(0, 12, k), with_qual=False)])
    return cases


def record(id_, seq, qual):
    return b">" + id_ + b"\n" + seq + b"\n" if qual is None else b"@" + id_ + b"\n" + seq + b"\n+\n" + qual + b"\n"


def dump_expected(ids, select, files):
    """the text of every file, as ReadDump::put / put_extra print it record by record"""
    out = []
    for seqs, quals, has in files:
        parts = []
        for i, id_ in enumerate(ids):
            if not select[i]:
                continue
            r = record(id_, seqs[i], quals[i] if quals is not None and has[i] else None)
            if len(r) < RECORD_LIMIT:
                parts.append(r)
        out.append(b"".join(parts))
    return out


# ---- the corpus of tools/gz_sanitize.cpp (little-endian) ----
def _strings(strings):
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    if strings:
        off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return b"".join(strings), off.tobytes()


def write_corpus(path, text_items, dump_items):
    """text_items: (block_bytes, text); dump_items: (block_bytes, ids, select, files, expected texts).
    'T' <u32 block_bytes> <u64 n> text
    'D' <u32 block_bytes> <u64 n reads> <u32 files> <u64 id bytes> ids, n + 1 id offsets, n select bytes; per file: <u64 seq bytes> <u64 qual bytes, or
        2^64 - 1 for none> seq, n + 1 offsets, [qual, n + 1 offsets, n has_qual bytes], <u64 expected bytes> expected text"""
    with open(path, "wb") as f:
        for bb, text in text_items:
            f.write(b"T" + struct.pack("<IQ", bb, len(text)) + text)
        for bb, ids, select, files, expected in dump_items:
            n = len(ids)
            idb, ido = _strings(list(ids))
            f.write(b"D" + struct.pack("<IQIQ", bb, n, len(files), len(idb)) + idb + ido + np.asarray(select, dtype=np.uint8).tobytes())
            for (seqs, quals, has), want in zip(files, expected):
                sb, so = _strings(list(seqs))
                if quals is None:
                    f.write(struct.pack("<QQ", len(sb), 2 ** 64 - 1) + sb + so)
                else:
                    qb, qo = _strings(list(quals))
                    f.write(struct.pack("<QQ", len(sb), len(qb)) + sb + so + qb + qo + np.asarray(has, dtype=np.uint8).tobytes())
                f.write(struct.pack("<Q", len(want)) + want)
