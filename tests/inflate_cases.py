"""The BGZF members the inflater's tests share (tests/test_inflate_host_cpu.py, test_inflate_sanitized_cpu.py, test_gpu_inflate.py):
good members made with zlib's raw deflate (wbits = -15) in its strategies, or assembled here bit by bit, framed by hand; malformed
members as mutations of good ones, each with the status csrc/cfr_inflate_core.hpp names for it; the corpus file of
tools/inflate_sanitize.cpp.  For every member the builder itself asserts zlib's verdict: zlib.decompressobj(-15) takes the deflate
stream and consumes it exactly - and the trailer fits - or the member is one that must be refused.  Everything is made once per
process and handed out unchanged."""
import functools
import struct
import zlib

import numpy as np

import gz_cases as gc
from centrifuger_amd import capi

OK, BAD_HEADER, BAD_BLOCK_TYPE, BAD_STORED_LEN, BAD_CODE_SET, BAD_SYMBOL, INPUT, OUTPUT_LONG, OUTPUT_SHORT, BAD_CRC = range(10)
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- framing ----
def frame(deflate, text=b"", crc=None, isize=None, extra_front=b""):
    """one BGZF member around a deflate stream; extra_front: other subfields of the extra field in front of BC"""
    xlen = len(extra_front) + 6
    size = 12 + xlen + len(deflate) + 8
    assert size <= 65536, size
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_front + b"BC\x02\0" + struct.pack("<H", size - 1) + deflate +
            struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize))


def raw(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if not flush_every:
        return c.compress(text) + c.flush()
    return b"".join(c.compress(text[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(text), flush_every)) + c.flush()


def split(m):
    """a member -> (deflate stream, crc, isize)"""
    xlen, = struct.unpack_from("<H", m, 10)
    crc, isize = struct.unpack_from("<II", m, len(m) - 8)
    return m[12 + xlen:len(m) - 8], crc, isize


def zlib_text(deflate):
    """what zlib makes of a raw deflate stream: its text when it takes the stream and consumes it exactly, else None"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(deflate)
    except zlib.error:
        return None
    return out if d.eof and d.unused_data == b"" else None


def verdict(m):
    """the text of a member that zlib inflates to what its trailer says (ISIZE at most 65536), else None"""
    deflate, crc, isize = split(m)
    text = zlib_text(deflate)
    return text if text is not None and isize <= 65536 and len(text) == isize and zlib.crc32(text) == crc else None


# ---- deflate by hand ----
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                      # least significant bit first
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):                      # a Huffman code: most significant bit first
        self.put(int(format(code, "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951, 3.2.2); the set need not be complete"""
    codes, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = {d: (d, 5) for d in range(32)}
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def put_tokens(b, tokens, lit, dist):
    """tokens: a byte value, ("m", length, distance), ("sym", literal/length symbol), ("d", distance symbol) or "eob" """
    for t in tokens:
        if t == "eob":
            b.code(*lit[256])
        elif isinstance(t, int):
            b.code(*lit[t])
        elif t[0] == "sym":
            b.code(*lit[t[1]])
        elif t[0] == "d":
            b.code(*dist[t[1]])
        else:
            _, length, distance = t
            ls = max(i for i in range(29) if LEN_BASE[i] <= length and (i < 28 or length == 258))
            b.code(*lit[257 + ls])
            b.put(length - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = max(i for i in range(30) if DIST_BASE[i] <= distance)
            b.code(*dist[ds])
            b.put(distance - DIST_BASE[ds], DIST_EXTRA[ds])


def fixed_block(tokens, final=True):
    b = Bits()
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    put_tokens(b, tokens, FIXED_LIT, FIXED_DIST)
    return b.bytes()


def dynamic_block(lit_lens, dist_lens, ops, tokens, final=True):
    """lit_lens (257 .. 286 entries) and dist_lens (1 .. 30) say what HLIT / HDIST are and which codes the tokens get; ops is how the
    lengths are sent: (symbol 0 .. 15,) or (16 | 17 | 18, run).  The code-length code gives every used symbol the same length and
    is padded with unused symbols until it is complete."""
    seq = []
    for op in ops:
        seq += [op[0]] if op[0] < 16 else [seq[-1]] * op[1] if op[0] == 16 else [0] * op[1]
    assert seq == list(lit_lens) + list(dist_lens), "the ops do not spell the lengths"
    used = sorted({op[0] for op in ops})
    bits = max(1, (len(used) - 1).bit_length())
    used += [s for s in range(19) if s not in used][:(1 << bits) - len(used)]
    cl_lens = [bits if s in used else 0 for s in range(19)]
    cl = canonical(cl_lens)
    hclen = max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]) + 1
    b = Bits()
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(len(lit_lens) - 257, 5)
    b.put(len(dist_lens) - 1, 5)
    b.put(max(hclen, 4) - 4, 4)
    for s in CL_ORDER[:max(hclen, 4)]:
        b.put(cl_lens[s], 3)
    for op in ops:
        b.code(*cl[op[0]])
        if op[0] == 16:
            b.put(op[1] - 3, 2)
        elif op[0] == 17:
            b.put(op[1] - 3, 3)
        elif op[0] == 18:
            b.put(op[1] - 11, 7)
    put_tokens(b, tokens, canonical(lit_lens), canonical(dist_lens))
    return b.bytes()


def zero_runs(n):
    """ops for n zeros"""
    out = []
    while n >= 11:
        out.append((18, min(n, 138)))
        n -= min(n, 138)
    if n >= 3:
        out.append((17, n))
        n = 0
    return out + [(0,)] * n


def dynamic_header_lengths(deflate):
    """the code lengths a stream's first block (BTYPE 10) sends -> (literal/length lengths, distance lengths)"""
    v = int.from_bytes(deflate, "little")
    pos = 0

    def take(n):
        nonlocal pos
        r = (v >> pos) & ((1 << n) - 1)
        pos += n
        return r

    take(1)
    assert take(2) == 2, "not a dynamic block"
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl_lens = [0] * 19
    for s in CL_ORDER[:hclen]:
        cl_lens[s] = take(3)
    decode = {(c, l): s for s, (c, l) in canonical(cl_lens).items()}
    lens = []
    while len(lens) < hlit + hdist:
        code, l = 0, 0
        while (code, l) not in decode:
            code, l = (code << 1) | take(1), l + 1
            assert l <= 7
        s = decode[(code, l)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        else:
            lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
    return lens[:hlit], lens[hlit:hlit + hdist]


# ---- the good members: name -> (members back to back, their text) ----
def _cut(text, per_member, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    return b"".join(frame(raw(text[i:i + per_member], level, strategy), text[i:i + per_member]) for i in range(0, len(text), per_member))


@functools.lru_cache(maxsize=None)
def good():
    rng = np.random.default_rng(1951)
    g = {}
    g["eof_member"] = (EOF, b"")
    g["one_byte"] = (frame(raw(b"x"), b"x"), b"x")
    g["two_bytes"] = (frame(raw(b"xy"), b"xy"), b"xy")
    g["two_bytes_eof_between"] = (frame(raw(b"x"), b"x") + EOF + frame(raw(b"y"), b"y"), b"xy")
    a = b"a" * 65280
    g["equal_65280"] = (frame(raw(a), a), a)                                   # overlapping copies of length 258
    g["equal_65280_rle"] = (frame(raw(a, 6, zlib.Z_RLE), a), a)                # distance-1 copies
    allb = bytes(range(256)) * 255
    g["all_bytes_x255"] = (frame(raw(allb), allb), allb)
    r = gc._rand(rng, 65280)
    m = frame(raw(r, 0), r)                                                    # stored
    assert len(m) <= 65536 and split(m)[0][0] & 6 == 0
    g["random_65280_stored"] = (m, r)
    g["random_65280_level6"] = (frame(raw(r), r), r)
    p = gc._planted(rng, 32768)
    g["repeat_at_32768"] = (frame(raw(p, 9), p), p)
    fq = gc.fastq_like(rng, 600)
    for level in (1, 6, 9):
        g[f"fastq_65280_l{level}"] = (_cut(fq, 65280, level), fq)
        g[f"fastq_997_l{level}"] = (_cut(fq[:30000], 997, level), fq[:30000])
        g[f"fastq_251_l{level}"] = (_cut(fq[:12000], 251, level), fq[:12000])
    g["fastq_fixed"] = (_cut(fq[:60000], 20000, 6, zlib.Z_FIXED), fq[:60000])                          # BTYPE 01
    assert all(split(x)[0][0] & 7 == 3 for x in members_of(g["fastq_fixed"][0]))
    g["fastq_huffman_only"] = (_cut(fq[:60000], 60000, 6, zlib.Z_HUFFMAN_ONLY), fq[:60000])            # a dynamic block without matches
    t = fq[:50000]
    g["fastq_full_flush_7000"] = (frame(raw(t, 6, flush_every=7000), t), t)                            # many blocks, empty stored blocks between
    # Fibonacci-like frequencies: Huffman's tree is a chain, deeper than 15, so zlib's limited lengths reach 15
    # (1 3 4 7 11 ...: no two weights are ever equal while the tree is made, so the chain does not depend on how ties are broken)
    fib = [1, 3]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    t = np.repeat(np.arange(len(fib), dtype=np.uint8) + 65, fib)
    rng.shuffle(t)
    t = t.tobytes()
    d = raw(t, 6, zlib.Z_HUFFMAN_ONLY)
    assert max(dynamic_header_lengths(d)[0]) == 15, "no literal code of 15 bits"
    g["fibonacci_15_bit_codes"] = (frame(d, t), t)
    # by hand: code 18 runs over the end of the literal/length lengths into the distance lengths; no distance code at all
    lit = [0] * 260
    lit[65], lit[256] = 1, 1
    ops = zero_runs(65) + [(1,)] + zero_runs(190) + [(1,), (18, 3 + 10)]
    d = dynamic_block(lit, [0] * 10, ops, [65] * 40 + ["eob"])
    g["hand_run_crosses_alphabets"] = (frame(d, b"A" * 40), b"A" * 40)
    # by hand: a single distance code (an incomplete set that zlib allows), used; a match that overlaps its source
    lit = [0] * 258
    lit[97], lit[256], lit[257] = 2, 2, 1
    ops = zero_runs(97) + [(2,)] + zero_runs(158) + [(2,), (1,), (1,)]
    d = dynamic_block(lit, [1], ops, [97, ("m", 3, 1), ("m", 3, 1), "eob"])
    g["hand_single_distance_code"] = (frame(d, b"a" * 7), b"a" * 7)
    # by hand: 65536 bytes of text in one member (BGZF writers stop at 65280; the format's limit is what ISIZE may say)
    t = (fq * 2)[:65536]
    g["hand_65536_bytes"] = (frame(raw(t, 9), t), t)
    # BC behind another subfield of the extra field
    g["bc_behind_another_subfield"] = (frame(raw(b"field"), b"field", extra_front=b"XY\x03\0abc"), b"field")
    for name, (ms, text) in g.items():
        assert b"".join(verdict(x) for x in members_of(ms)) == text, name
    return g


OWN_NAMES = ("own_fixed", "own_dynamic")


@functools.lru_cache(maxsize=None)
def own():
    """the output of the project's own compressor (host twin), fixed and dynamic codes.  Apart from good(): this loads the library,
    which a test module must not do while it is collected (tests/conftest.py: torch initialises HIP first)."""
    fq = good()["fastq_65280_l6"][1]
    g = {}
    for name in OWN_NAMES:
        h = capi.Gz(block_bytes=20000, threads=2, codes=name[4:])
        g[name] = (h.compress(fq[:90000]), fq[:90000])
        h.close()
        assert b"".join(verdict(x) for x in members_of(g[name][0])) == g[name][1], name
    assert any(split(m)[0][0] & 6 == 4 for m in members_of(g["own_dynamic"][0])), "no member with dynamic codes"
    return g


def members_of(data):
    return [data[at:at + size] for at, size in _walk(data)]


def _walk(data):
    at = 0
    while at < len(data):
        xlen, = struct.unpack_from("<H", data, at + 10)
        o = at + 12
        while data[o:o + 2] != b"BC":
            o += 4 + struct.unpack_from("<H", data, o + 2)[0]
        size = struct.unpack_from("<H", data, o + 4)[0] + 1
        yield at, size
        at += size


# ---- malformed members: name -> (member, the status the core header names) ----
def _reframe(m, deflate=None, crc=None, isize=None):
    d, c, i = split(m)
    return frame(d if deflate is None else deflate, b"", c if crc is None else crc, i if isize is None else isize)


@functools.lru_cache(maxsize=None)
def malformed():
    g = good()
    fixed = members_of(g["fastq_fixed"][0])[0]
    stored = g["random_65280_stored"][0]
    dyn = members_of(g["fastq_65280_l6"][0])[0]
    d_fixed, d_stored = split(fixed)[0], split(stored)[0]
    bad = {}
    bad["btype_11"] = (_reframe(fixed, bytes([d_fixed[0] | 6]) + d_fixed[1:]), BAD_BLOCK_TYPE)
    bad["nlen_wrong"] = (_reframe(stored, d_stored[:3] + bytes([d_stored[3] ^ 1]) + d_stored[4:]), BAD_STORED_LEN)
    lit = [0] * 257
    lit[65], lit[66], lit[256] = 1, 1, 1
    ops = zero_runs(65) + [(1,), (1,)] + zero_runs(189) + [(1,), (0,)]
    bad["oversubscribed_lengths"] = (frame(dynamic_block(lit, [0], ops, [65, "eob"]), b"A"), BAD_CODE_SET)
    lit = [0] * 257
    lit[65], lit[256] = 1, 2
    ops = zero_runs(65) + [(1,)] + zero_runs(190) + [(2,), (0,)]
    bad["incomplete_lengths"] = (frame(dynamic_block(lit, [0], ops, [65, "eob"]), b"A"), BAD_CODE_SET)
    bad["distance_in_front_of_the_member"] = (frame(fixed_block([97, ("m", 3, 2), "eob"]), b"aaaa"), BAD_SYMBOL)
    bad["distance_symbol_30"] = (frame(fixed_block([97, ("sym", 257), ("d", 30), "eob"]), b"aaaa"), BAD_SYMBOL)
    bad["truncated_by_its_last_byte"] = (_reframe(fixed, d_fixed[:-1]), INPUT)
    _, crc, isize = split(dyn)
    bad["isize_one_too_large"] = (_reframe(dyn, isize=isize + 1), OUTPUT_SHORT)
    bad["isize_one_too_small"] = (_reframe(dyn, isize=isize - 1), OUTPUT_LONG)
    bad["crc_bit_flipped"] = (_reframe(dyn, crc=crc ^ (1 << 13)), BAD_CRC)
    bad["isize_65537"] = (_reframe(dyn, isize=65537), BAD_HEADER)
    for name, (m, status) in bad.items():
        assert verdict(m) is None and status != OK, name
    # zlib's own word on the streams whose deflate part is at fault
    for name in ("btype_11", "nlen_wrong", "oversubscribed_lengths", "incomplete_lengths", "distance_in_front_of_the_member", "distance_symbol_30",
                 "truncated_by_its_last_byte"):
        assert zlib_text(split(bad[name][0])[0]) is None, name
    return bad


@functools.lru_cache(maxsize=None)
def corpus():
    """every case as one call: [(name, members, expected text, expected statuses)]; a refused member's text is zeros"""
    out = []
    for name, (ms, text) in list(good().items()) + list(own().items()):
        out.append((name, ms, text, [OK] * len(members_of(ms))))
    for name, (m, status) in malformed().items():
        _, _, isize = split(m)
        out.append((name, m, bytes(isize if isize <= 65536 else 0), [status]))
    return out


def case_names():
    """the names of corpus(), without loading the library"""
    return list(good()) + list(OWN_NAMES) + list(malformed())


def case(name):
    return next(c for c in corpus() if c[0] == name)


@functools.lru_cache(maxsize=None)
def mixed_call():
    """about 300 members of every kind in one call, end-of-file members and refused members in the middle"""
    ms, text, status = [], [], []
    items = corpus()
    while len(status) < 300:
        for _, m, t, s in items:
            if len(m) > 40000 and len(status) > 60:          # the large ones once
                continue
            ms += [m, EOF]
            text.append(t)
            status += s + [OK]
    return b"".join(ms), b"".join(text), status


def write_corpus(path, items):
    """items: (members, expected text, expected statuses) -> 'M' <u64 bytes> members <u64 text bytes> text <u64 n> statuses (little-endian)"""
    with open(path, "wb") as f:
        for ms, text, status in items:
            f.write(b"M" + struct.pack("<Q", len(ms)) + ms + struct.pack("<Q", len(text)) + text + struct.pack("<Q", len(status)) + bytes(status))
