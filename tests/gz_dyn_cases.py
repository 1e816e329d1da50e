"""Dynamic mode of the compressor (cfr_gz_options.codes = 1; tests/test_gz_dyn_host_cpu.py, test_gz_codes_cpu.py, test_gpu_gz_dyn.py):
the texts whose codes have the shapes where a code build can go wrong, a parser of the header of a dynamic deflate block
(RFC 1951, 3.2.7), and the walk over the members that checks them against fixed mode's members of the same text.  The texts of
tests/gz_cases.py are taken as they are.  Everything is made once per process and handed out unchanged."""
import functools
import zlib
from fractions import Fraction

import numpy as np

import gz_cases as gc

BLOCKS = gc.BLOCKS
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence over k symbols of order n (joined Lyndon words)"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return seq


def _no_repeated_4mer(b):
    return len({b[i:i + 4] for i in range(len(b) - 3)}) == len(b) - 3


@functools.lru_cache(maxsize=None)
def new_texts():
    """name -> text: the same for every block size"""
    rng = np.random.default_rng(1951)
    t = {}
    # no 4 bytes occur twice: no match, an empty distance histogram
    db = bytes(0x41 + v for v in _de_bruijn(16, 4))
    t["no_match_16_symbols"] = db[:600]
    assert _no_repeated_4mer(t["no_match_16_symbols"]) and len(set(t["no_match_16_symbols"])) <= 16
    # a chunk without a repeated 4-mer (its wrap into the next copy included), eight times: every match is at distance 512
    while True:
        at = int(rng.integers(1000, len(db) - 600))
        chunk = db[at:at + 512]
        if _no_repeated_4mer(chunk + chunk[:3]):
            break
    t["one_distance_code"] = chunk * 8
    # byte value k occurs F(k) times, k = 1 .. 22
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    a = np.repeat(np.arange(1, 23, dtype=np.uint8), fib)
    assert len(a) == 46367
    rng.shuffle(a)
    t["fibonacci_literals"] = a.tobytes()
    # ... the frequent bytes of that text repeat so often that most of them leave in matches, and the histogram the code is built
    # from is flatter than the text's.  Here the Fibonacci frequencies are those of the RARE bytes only (k = 1 .. 20: 17710 bytes, a
    # Huffman subtree 19 levels deep), and the bulk is 47 000 bytes drawn from 64 other values, where 4 bytes seldom occur twice.
    a = np.concatenate([np.repeat(np.arange(1, 21, dtype=np.uint8), fib[:20]), rng.integers(64, 128, 47000).astype(np.uint8)])
    rng.shuffle(a)
    t["fibonacci_tail"] = a.tobytes()
    # 254 unused literals between the two used ones
    t["far_apart_symbols"] = (rng.integers(0, 2, 3000).astype(np.uint8) * 255).tobytes()
    return t


@functools.lru_cache(maxsize=None)
def texts(block_bytes):
    """the texts of gz_cases and the new ones"""
    t = dict(gc.texts(block_bytes))
    t.update(new_texts())
    return t


class _Bits:
    def __init__(self, data):
        self.data, self.at = data, 0

    def low_first(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.at >> 3] >> (self.at & 7)) & 1) << i
            self.at += 1
        return v


def kraft(lengths):
    return sum(Fraction(1, 1 << l) for l in lengths if l)


def parse_dynamic_header(deflate):
    """the header of a final dynamic block -> dict(hlit, hdist, hclen, cl = the 19 lengths of the code-length code, ll, dist = the two
    codes' lengths, sent = [(code-length symbol, how many lengths it stands for)], bits = the header's bits, the first 3 included)"""
    b = _Bits(deflate)
    assert b.low_first(1) == 1 and b.low_first(2) == 2
    hlit, hdist, hclen = b.low_first(5) + 257, b.low_first(5) + 1, b.low_first(4) + 4
    assert hlit <= 286 and hdist <= 30
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = b.low_first(3)
    # canonical codes of the code-length code: (length, code) -> symbol
    decode, code = {}, 0
    for length in range(1, 8):
        for s in range(19):
            if cl[s] == length:
                decode[(length, code)] = s
                code += 1
        code <<= 1
    seq, sent = [], []
    while len(seq) < hlit + hdist:
        length, code = 0, 0
        while (length, code) not in decode:
            code = (code << 1) | b.low_first(1)
            length += 1
            assert length <= 7, "no code of the code-length code matches"
        s = decode[(length, code)]
        if s < 16:
            seq.append(s)
            sent.append((s, 1))
            continue
        if s == 16:
            assert seq, "a repeat with nothing in front of it"
            count, value = 3 + b.low_first(2), seq[-1]
        else:
            count, value = (3 + b.low_first(3), 0) if s == 17 else (11 + b.low_first(7), 0)
        seq += [value] * count
        sent.append((s, count))
    assert len(seq) == hlit + hdist, "a repeat runs over the end of the lengths"
    return dict(hlit=hlit, hdist=hdist, hclen=hclen, cl=cl, ll=seq[:hlit], dist=seq[hlit:], sent=sent, bits=b.at)


def check_members_dyn(out, fixed_out, text, block_bytes):
    """every member of `out` (dynamic mode) frames and encodes its block of `text`; a dynamic member has codes within their limits whose
    Kraft sums are 1 and is shorter than fixed mode's member of the block (in fixed_out), any other member has fixed mode's bytes
    -> (members, stored members, dynamic members, the parsed headers of the dynamic members)"""
    members, fixed = gc.walk(out), gc.walk(fixed_out)
    assert len(members) == len(fixed) == (len(text) + block_bytes - 1) // block_bytes
    stored, headers = 0, []
    for k, ((size, deflate, crc, isize), (fsize, fdeflate, _, _)) in enumerate(zip(members, fixed)):
        piece = text[k * block_bytes:(k + 1) * block_bytes]
        assert isize == len(piece) and crc == zlib.crc32(piece), f"member {k}: CRC32 / ISIZE"
        d = zlib.decompressobj(-15)
        assert d.decompress(deflate) == piece and d.eof and d.unused_data == b"", f"member {k}: the deflate part"
        assert deflate[0] & 1 == 1, f"member {k}: BFINAL"
        btype = (deflate[0] >> 1) & 3
        if btype != 2:
            assert deflate == fdeflate and size == fsize, f"member {k}: not dynamic, and not fixed mode's bytes"
            stored += btype == 0
            continue
        h = parse_dynamic_header(deflate)
        assert max(h["ll"]) <= 15 and max(h["dist"]) <= 15 and max(h["cl"]) <= 7, f"member {k}: a code longer than its limit"
        assert kraft(h["ll"]) == 1 and kraft(h["dist"]) == 1 and kraft(h["cl"]) == 1, f"member {k}: a Kraft sum that is not 1"
        assert h["ll"][256] > 0, f"member {k}: no end-of-block code"
        assert h["ll"][-1] > 0 or h["hlit"] == 257, f"member {k}: HLIT is not trimmed"
        assert h["dist"][-1] > 0, f"member {k}: HDIST is not trimmed"
        assert h["hclen"] == 4 or h["cl"][CL_ORDER[h["hclen"] - 1]] > 0, f"member {k}: HCLEN is not trimmed"
        assert size < fsize and size <= 65311, f"member {k}: dynamic, and not shorter than fixed mode's"
        headers.append(h)
    return len(members), stored, len(headers), headers
