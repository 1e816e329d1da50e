"""The corpus of the reference-text front end (csrc/cfr_refseq_core.hpp) and a plain statement of its grammar, line by line, that the
host twin and the kernels are compared with.  Texts of a few KB; they are fed whole (several 4096-byte blocks in one chunk) and in chunks
of 4096, 1024 and 256 bytes, the sizes the command line takes through CFR_REFSEQ_CHUNK_LOG2."""
import numpy as np

CHUNK_LOG2 = (20, 12, 10, 8)          # 2^20: every text of the corpus in one chunk
SPAN = 4096                           # the bytes of one block of the device kernels
NT, AA = b"ACGT", b"ARNDCEQGHILKMFPSTWYV"


def _seq(rng, n, alphabet=NT):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)])


def _wrap(s, width):
    return b"".join(s[a:a + width] + b"\n" for a in range(0, len(s), width))


def _cases():
    rng = np.random.default_rng(20240611)
    c = {}
    c["wrapped"] = b"".join(b">w%d some text\n" % k + _wrap(_seq(rng, 900 + 37 * k), 70) for k in range(4))
    c["unwrapped"] = b"".join(b">u%d\n" % k + _seq(rng, 700 + k) + b"\n" for k in range(5))
    c["line_longer_than_a_chunk"] = b">long\n" + _seq(rng, 9000) + b"\n>after\n" + _seq(rng, 50) + b"\n"
    # the header line ends exactly where a chunk of 256 / 1024 / 4096 bytes ends, and the next one is cut by the following chunk end
    for size in (256, 1024, 4096):
        head = b">first\n" + _wrap(_seq(rng, 3 * size), 60)
        a = head[:size - 20] + b"\n"
        a += b">" + b"h" * (size - len(a) - 2) + b"\n"
        assert len(a) == size
        a += _wrap(_seq(rng, size - 130), 60)
        a = a[:2 * size - 9]
        if a[-1:] != b"\n":
            a += b"\n"
        a += b">cut_by_the_chunk_end with words\n" + _wrap(_seq(rng, 200), 50)
        c["header_at_chunk_end_%d" % size] = a
    c["crlf"] = b"".join(b">c%d desc\r\n" % k + _wrap(_seq(rng, 333), 60).replace(b"\n", b"\r\n") for k in range(3)) + b">only_cr\r\nACGTACGTAC\r\n"
    c["block_keeps_nothing"] = (b">masked\n" + _wrap(_seq(rng, 500), 80) + _wrap(_seq(rng, 2 * SPAN + 300).lower(), 80) + _wrap(_seq(rng, 90), 80) +
                                b"N" * (SPAN + 700) + b"\n" + _wrap(_seq(rng, 64), 80) + b">next\n" + _wrap(b"N" * 5000, 100) + b"ACGTTGCA\n")
    c["gt_inside_lines"] = b">a>b >c\nAC>GT\nACGT>\n >not_a_header\nAC\n>d\n>>e\nTTTT>AAAA\n"
    c["empty_records"] = b">e1\n>e2\n\n>e3\nACGT\n>e4\n\n\n>e5\nNNNN\n>e6\nGG\n"
    c["leading_bytes"] = b"ACGTACGT\n;comment\nGGCC\n>r1\nACGTACGTACGT\n"
    c["no_final_newline"] = b">n1\nACGTACGT\nACG"
    c["ends_inside_a_header"] = b">h1\nACGTAC\n>h2 the file ends he"
    c["only_a_header"] = b">alone"
    c["no_header_at_all"] = _wrap(_seq(rng, 300), 60)
    c["empty_file"] = b""
    c["tab_in_header"] = b">id\twith a tab\nACGTACGTAC\n>id2 \nAC\n>\nACGTA\n> spaced\nACGTT\n"
    # records of 1 .. 40 kept symbols: several segments meet in one word of T
    c["tiny_records"] = b"".join(b">t%d\n" % k + _seq(rng, k) + b"\n" for k in range(1, 41))
    # total lengths of 31 / 32 / 33 and 63 / 64 / 65 symbols past a word boundary
    for extra in (31, 32, 33, 63, 64, 65):
        c["total_%d_past_a_word" % extra] = b">x\n" + _wrap(_seq(rng, 640), 64) + b">y\n" + _seq(rng, extra) + b"\n"
    c["lower_case_and_n_mixed"] = b">m\n" + _wrap(bytes(rng.choice(np.frombuffer(b"ACGTacgtNnRYKM-*", dtype=np.uint8), size=6000)), 61)
    return c


CASES = _cases()
PROTEIN_CASES = {
    "proteins": b"".join(b">p%d desc\n" % k + _wrap(_seq(np.random.default_rng(k), 150 + k, AA), 60) for k in range(5)),
    "proteins_other_letters": b">p\nARNDXBZJUO*arnd\nCEQG\n>q\nMKV-\n",
}


class Capacity(Exception):
    pass


def effective_len(text, at_line_start, final):
    if final or not text:
        return len(text)
    tail = text.rfind(b"\n") + 1
    starts_line = True if tail else at_line_start
    if tail < len(text) and starts_line and text[tail:tail + 1] == b">":
        if tail == 0:
            raise Capacity()
        return tail
    return len(text)


def feed(text, at_line_start=True, final=True, alphabet=NT):
    """One chunk -> (consumed, [(header, header_len, id_len, kept)], lead_kept, kept symbols, at_line_start of the next chunk)"""
    eff = effective_len(text, at_line_start, final)
    t = text[:eff]
    records, kept, lead, pos = [], bytearray(), 0, 0
    lines = t.split(b"\n")
    if t.endswith(b"\n"):
        lines.pop()
    for j, line in enumerate(lines):
        begins = at_line_start if j == 0 else True
        if begins and line.startswith(b">"):
            id_len = len(line) - 1
            for k in range(1, len(line)):
                if line[k:k + 1] in (b" ", b"\t", b"\r"):
                    id_len = k - 1
                    break
            records.append([pos, len(line), id_len, 0])
        else:
            k = bytes(x for x in line if x in alphabet)
            kept += k
            if records:
                records[-1][3] += len(k)
            else:
                lead += len(k)
        pos += len(line) + 1
    nxt = t.endswith(b"\n") if t else at_line_start
    return eff, [tuple(r) for r in records], lead, bytes(kept), nxt


def feed_file(data, chunk, alphabet=NT):
    """-> per chunk (chunk bytes, at_line_start, final, feed(...)) as the command line cuts a file"""
    out, at, als = [], 0, True
    while True:
        piece = data[at:at + chunk]
        final = at + chunk >= len(data)
        r = feed(piece, als, final, alphabet)
        out.append((piece, als, final, r))
        at += r[0]
        als = r[4]
        if final:
            return out


def file_records(data, alphabet=NT):
    """The records of a whole file -> [(id, kept symbols)]"""
    _, recs, lead, kept, _ = feed(data, True, True, alphabet)
    out, at = [], lead
    for h, hl, il, k in recs:
        out.append((data[h + 1:h + 1 + il].decode("latin-1"), kept[at:at + k]))
        at += k
    return out


def draw_segment_lists(pieces, rng):
    """pieces: [(src, len)] of the records of a fed corpus, in feed order -> segment lists [(src, len, dst)]: everything in order, some
    records dropped, a permutation by group"""
    pieces = [p for p in pieces if p[1]]
    lists = []

    def lay(ps):
        out, dst = [], 0
        for s, ln in ps:
            out.append((s, ln, dst))
            dst += ln
        return out
    lists.append(lay(pieces))
    if len(pieces) > 2:
        keep = rng.random(len(pieces)) < 0.6
        keep[rng.integers(0, len(pieces))] = True
        lists.append(lay([p for p, k in zip(pieces, keep) if k]))
        group = rng.integers(0, 3, size=len(pieces))
        lists.append(lay([p for g in range(3) for p, q in zip(pieces, group) if q == g]))
    return [l for l in lists if l]


# ---- the checks the host twin (tests/test_refseq_host_cpu.py) and the kernels (tests/test_gpu_refseq.py) both go through; make(): a capi.Refseq
def check_feed(make, data, chunk, alphabet=NT):
    """Feeds one file chunk by chunk into make()'s handle beside the Python statement -> (handle, [(src, len)] per kept run, expected U symbols)"""
    h = make()
    pieces, want_u, u_len = [], [], 0
    for piece, als, final, (eff, recs, lead, kept, nxt) in feed_file(data, chunk, alphabet):
        info = h.feed(piece, als, final)
        u_start = (u_len + 31) // 32 * 32
        assert (info.consumed, info.n_records, info.lead_kept, info.kept, bool(info.at_line_start)) == (eff, len(recs), lead, len(kept), nxt)
        assert info.u_start == u_start
        got = h.fetch()
        assert [tuple(int(x) for x in r) for r in got] == recs
        if kept:
            pieces.append((u_start, len(kept)))
            want_u.append(kept)
            u_len = u_start + len(kept)
    return h, pieces, want_u


def feed_corpus(make, chunk):
    """every case as one file into one handle -> (handle, the kept run of every record in feed order [(src, len)], U as {src: symbols})"""
    h = make()
    pieces, sym = [], {}
    for name in sorted(CASES):
        data = CASES[name]
        want = file_records(data)
        got = h.feed_file(data, chunk)
        assert [g[0] for g in got] == [w[0] for w in want], name
        for (_, pcs), (_, kept) in zip(got, want):
            assert sum(p[1] for p in pcs) == len(kept), name
            at = 0
            for s, ln in pcs:
                pieces.append((s, ln))
                sym[s] = kept[at:at + ln]
                at += ln
    return h, pieces, sym


def check_assemblies(make, chunk):
    h, pieces, sym = feed_corpus(make, chunk)
    h.close()
    for k, segs in enumerate(draw_segment_lists(pieces, np.random.default_rng(chunk))):
        h, _, _ = feed_corpus(make, chunk)
        h.assemble(segs)
        assert h.text() == b"".join(sym[s] for s, _, _ in segs), f"segment list {k}"
        h.close()
