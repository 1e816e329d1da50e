"""ctypes binding of libcfr_hip.so (include/cfr_hip.h).  Thin: numpy arrays in, numpy arrays out.

The library is the product; there is no Python/CPU fallback here - if the shared object is
missing or no HIP device is usable, calls raise CfrError.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcfr_hip.so")

CFR_OK, CFR_ERR_IO, CFR_ERR_FORMAT, CFR_ERR_NO_DEVICE, CFR_ERR_HIP, CFR_ERR_ARG, CFR_ERR_CAPACITY, CFR_ERR_BUSY = range(8)


class CfrError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"cfr status {status}: {msg}")
        self.status = status


class Params(C.Structure):
    _fields_ = [("max_result", C.c_int32), ("min_hit_len", C.c_int32), ("max_result_per_hit_factor", C.c_int32),
                ("output_expanded", C.c_int32), ("consider_secondary_hit_len", C.c_uint64),
                ("consider_secondary_score_factor", C.c_double)]


class IndexInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("first_isa", C.c_uint64), ("block_size", C.c_uint64), ("precompute_width", C.c_uint64),
                ("sample_rate", C.c_uint64), ("selected_cnt", C.c_uint64), ("seq_cnt", C.c_uint64), ("node_cnt", C.c_uint64),
                ("min_hit_len", C.c_int32), ("last_chr", C.c_char), ("is_protein", C.c_uint8), ("pad", C.c_char * 2), ("device_bytes", C.c_uint64)]


class BatchStats(C.Structure):
    _fields_ = [("pack_ms", C.c_float), ("search_ms", C.c_float), ("adjust_ms", C.c_float), ("rows_ms", C.c_float),
                ("locate_ms", C.c_float), ("tail_ms", C.c_float), ("total_ms", C.c_float),
                ("n_chains", C.c_uint64), ("n_hits", C.c_uint64), ("n_rows", C.c_uint64)]


HIT_DTYPE = np.dtype([("sp", "<u8"), ("ep", "<u8"), ("l", "<i4"), ("strand", "<i4"), ("offset", "<i4"), ("pad", "<i4")])
RESULT_DTYPE = np.dtype([("score", "<u8"), ("secondary_score", "<u8"), ("hit_length", "<i4"), ("query_length", "<i4"),
                         ("n_match", "<i4"), ("pad", "<i4"), ("match_begin", "<u8")])
MATCH_DTYPE = np.dtype([("id", "<u8"), ("taxid", "<u8"), ("kind", "<i4"), ("pad", "<i4")])
SPAN_DTYPE = np.dtype([("begin", "<u8"), ("count", "<u8")])      # cfr_span: the --expand-taxid list of a match slot
# the narrow layout of cfr_classify_batch_resident_compact (20 + 12 bytes)
RESULT_COMPACT_DTYPE = np.dtype([("score", "<u4"), ("secondary_score", "<u4"), ("hit_length", "<u4"), ("query_length", "<u4"),
                                 ("n_match", "u1"), ("flags", "u1"), ("pad", "<u2")])
MATCH_COMPACT_DTYPE = np.dtype([("id_kind", "<u4"), ("taxid_lo", "<u4"), ("taxid_hi", "<u4")])
COMPACT_WIDE = 1


def expand_compact(cres, cmatch, max_result, wide=None):
    """cfr_result_compact / cfr_match_compact arrays -> the wide arrays (RESULT_DTYPE, MATCH_DTYPE) with match_begin = i * max_result.
    wide: DeviceIndex.compact_wide() of the same call - the reads flagged CFR_COMPACT_WIDE (values that do not fit the narrow
    layout) are patched in from it; without it a flagged read raises."""
    flagged = (cres["flags"] & COMPACT_WIDE) != 0
    if flagged.any() and wide is None:
        raise ValueError("a read of the batch does not fit the compact result layout (CFR_COMPACT_WIDE): pass DeviceIndex.compact_wide()")
    n = len(cres)
    res = np.zeros(n, dtype=RESULT_DTYPE)
    for f in ("score", "secondary_score", "hit_length", "query_length", "n_match"):
        res[f] = cres[f]
    res["match_begin"] = np.arange(n, dtype=np.uint64) * np.uint64(max_result)
    mat = np.zeros(len(cmatch), dtype=MATCH_DTYPE)
    mat["id"] = cmatch["id_kind"] & np.uint32(0x7fffffff)
    mat["kind"] = (cmatch["id_kind"] >> np.uint32(31)).astype(np.int32)
    mat["taxid"] = cmatch["taxid_lo"].astype(np.uint64) | (cmatch["taxid_hi"].astype(np.uint64) << np.uint64(32))
    if flagged.any():
        widx, wres, wmat = wide
        assert set(np.nonzero(flagged)[0].tolist()) <= set(int(x) for x in widx), "flagged reads missing from the wide side list"
        for j, i in enumerate(widx):
            i = int(i)
            if i >= n:
                continue
            mb = res["match_begin"][i]
            res[i] = wres[j]
            res["match_begin"][i] = mb
            src = int(wres[j]["match_begin"])
            mat[int(mb):int(mb) + max_result] = wmat[src:src + max_result]
    return res, mat

EXPORTS = [
    "cfr_classify_batch_resident_compact", "cfr_params_default", "cfr_last_error", "cfr_version", "cfr_index_open", "cfr_index_destroy", "cfr_index_get_info",
    "cfr_device_count", "cfr_device_index_create", "cfr_device_index_create_ex", "cfr_device_options_default",
    "cfr_device_index_destroy", "cfr_device_index_get_info", "cfr_device_index_set_dust", "cfr_dust_mask_device",
    "cfr_dust_mask_batch_literal",
    "cfr_selfcheck_tables", "cfr_build_index", "cfr_build_options_default",
    "cfr_rank_batch", "cfr_backward_search_batch", "cfr_locate_rows", "cfr_search_batch", "cfr_classify_batch",
    "cfr_classify_batch_resident", "cfr_last_batch_stats", "cfr_classify_from_hits", "cfr_dust_mask_batch",
    "cfr_format_tsv", "cfr_tsv_header", "cfr_host_alloc", "cfr_host_free",
    "cfr_classify_batch_submit", "cfr_classify_batch_wait", "cfr_compact_wide_reads", "cfr_index_digest", "cfr_index_mapped_bytes", "cfr_pack_reads", "cfr_classify_batch_packed",
    "cfr_classify_batch_expanded", "cfr_classify_from_hits_expanded", "cfr_format_tsv_expanded", "cfr_tsv_header_expanded",
    "cfr_merge_pairs", "cfr_merge_pairs_device", "cfr_device_index_set_merge", "cfr_classify_batch_merged",
    "cfr_classify_batch_resident_merged", "cfr_last_merge_ms",
    "cfr_quant_options_default", "cfr_quant_open", "cfr_quant_add_tsv", "cfr_quant_add_results", "cfr_quant_assignments", "cfr_quant_run",
    "cfr_quant_values", "cfr_quant_write", "cfr_quant_get_stats", "cfr_quant_destroy", "cfr_quant_estep_probe",
    "cfr_read_format_parse", "cfr_read_format_info", "cfr_read_format_extract", "cfr_read_format_destroy",
    "cfr_barcode_open", "cfr_barcode_count", "cfr_barcode_correct", "cfr_barcode_correct_host", "cfr_barcode_counts", "cfr_barcode_get_stats",
    "cfr_barcode_destroy", "cfr_barcode_translate_open", "cfr_barcode_translate_apply", "cfr_barcode_translate_destroy",
    "cfr_tsv_header_ex", "cfr_format_tsv_ex",
    "cfr_taxonomy_open", "cfr_taxonomy_get_tables", "cfr_taxonomy_tax_name", "cfr_taxonomy_seq_name", "cfr_tax_rank_string", "cfr_taxonomy_close",
    "cfr_taxonomy_lca_probe",
    "cfr_promote_open", "cfr_promote_apply", "cfr_promote_lca_warnings", "cfr_promote_get_stats", "cfr_promote_close",
    "cfr_device_index_set_promote", "cfr_last_promote_ms",
    "cfr_kreport_options_default", "cfr_kreport_open", "cfr_kreport_add_results", "cfr_kreport_add_tsv", "cfr_kreport_add_count_table",
    "cfr_kreport_add_counts", "cfr_kreport_bins", "cfr_kreport_counts", "cfr_kreport_warnings", "cfr_kreport_write", "cfr_kreport_get_stats",
    "cfr_kreport_close", "cfr_kreport_scan_warnings", "cfr_device_index_set_kreport", "cfr_device_index_kreport_counts", "cfr_last_kreport_ms",
    "cfr_tokenizer_open", "cfr_tokenize", "cfr_tokenizer_fetch", "cfr_tokenizer_device_reads", "cfr_tokenizer_get_stats", "cfr_tokenizer_close",
    "cfr_tsv_options_default", "cfr_tsv_open", "cfr_tsv_format", "cfr_tsv_get_stats", "cfr_tsv_close", "cfr_device_index_set_tsv",
    "cfr_device_index_tsv_last", "cfr_device_index_tsv_last_resident", "cfr_tokenizer_device_records", "cfr_last_tsv_ms",
    "cfr_gz_options_default", "cfr_gz_open", "cfr_gz_compress", "cfr_gz_dump", "cfr_gz_eof", "cfr_gz_get_stats", "cfr_gz_close",
    "cfr_inflate_open", "cfr_inflate_bgzf", "cfr_inflate_member_status", "cfr_inflate_device_text", "cfr_inflate_get_stats", "cfr_inflate_close",
    "cfr_tokenize_resident", "cfr_tokenizer_fetch_ids",
    "cfr_refseq_open", "cfr_refseq_feed", "cfr_refseq_fetch", "cfr_refseq_assemble", "cfr_refseq_text", "cfr_refseq_get_stats", "cfr_refseq_close",
    "cfr_build_select", "cfr_build_selection_get", "cfr_build_selection_free", "cfr_file_base_name", "cfr_build_index_assembled",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CfrError(-1, f"{LIB_PATH} not built (run `python -c 'import __graft_entry__ as g; g.build()'` or make -C centrifuger_amd/csrc)")
        L = C.CDLL(LIB_PATH)
        L.cfr_last_error.restype = C.c_char_p
        L.cfr_version.restype = C.c_char_p
        L.cfr_tsv_header.restype = C.c_char_p
        L.cfr_format_tsv.restype = C.c_size_t
        L.cfr_format_tsv_expanded.restype = C.c_size_t
        L.cfr_tsv_header_expanded.restype = C.c_char_p
        L.cfr_host_alloc.restype = C.c_void_p
        L.cfr_host_alloc.argtypes = [C.c_size_t]
        L.cfr_host_free.argtypes = [C.c_void_p]
        for name in EXPORTS:
            if name not in ("cfr_last_error", "cfr_version", "cfr_tsv_header", "cfr_format_tsv", "cfr_index_destroy", "cfr_format_tsv_expanded", "cfr_tsv_header_expanded",
                            "cfr_device_index_destroy", "cfr_params_default", "cfr_host_alloc", "cfr_host_free", "cfr_build_options_default",
                            "cfr_quant_options_default", "cfr_quant_destroy", "cfr_read_format_destroy", "cfr_barcode_destroy",
                            "cfr_barcode_translate_destroy", "cfr_tsv_header_ex", "cfr_format_tsv_ex",
                            "cfr_taxonomy_tax_name", "cfr_taxonomy_seq_name", "cfr_tax_rank_string", "cfr_taxonomy_close",
                            "cfr_tokenizer_close", "cfr_kreport_options_default", "cfr_tsv_options_default", "cfr_tsv_close",
                            "cfr_gz_options_default", "cfr_gz_eof", "cfr_gz_close", "cfr_inflate_close", "cfr_refseq_close",
                            "cfr_build_selection_free", "cfr_file_base_name"):
                getattr(L, name).restype = C.c_int
        for name in ("cfr_quant_destroy", "cfr_read_format_destroy", "cfr_barcode_destroy", "cfr_barcode_translate_destroy"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [C.c_void_p]
        L.cfr_tsv_header_ex.restype = C.c_char_p
        for name in ("cfr_taxonomy_tax_name", "cfr_taxonomy_seq_name"):
            getattr(L, name).restype = C.c_char_p
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64]
        L.cfr_tax_rank_string.restype = C.c_char_p
        L.cfr_tax_rank_string.argtypes = [C.c_uint8]
        L.cfr_taxonomy_close.restype = None
        L.cfr_taxonomy_close.argtypes = [C.c_void_p]
        L.cfr_format_tsv_ex.restype = C.c_size_t
        L.cfr_tokenizer_close.restype = None
        L.cfr_tokenizer_close.argtypes = [C.c_void_p]
        L.cfr_tsv_close.restype = None
        L.cfr_tsv_close.argtypes = [C.c_void_p]
        L.cfr_tsv_options_default.restype = None
        L.cfr_gz_close.restype = None
        L.cfr_gz_close.argtypes = [C.c_void_p]
        L.cfr_gz_options_default.restype = None
        L.cfr_gz_eof.restype = None
        L.cfr_inflate_close.restype = None
        L.cfr_inflate_close.argtypes = [C.c_void_p]
        for name in ("cfr_refseq_close", "cfr_build_selection_free"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [C.c_void_p]
        L.cfr_file_base_name.restype = C.c_size_t
        L.cfr_file_base_name.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


def _check(status):
    if status != CFR_OK:
        raise CfrError(status, lib().cfr_last_error().decode())


def _p(a, t=C.c_void_p):
    return None if a is None else a.ctypes.data_as(t)


def default_params(**kw) -> Params:
    p = Params()
    lib().cfr_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8)


def _u64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint64)


class BuildInput(C.Structure):
    _fields_ = [("n_seqs", C.c_uint64), ("seq_names", C.POINTER(C.c_char_p)), ("seq_taxids", C.c_void_p), ("seq_lens", C.c_void_p),
                ("text", C.c_void_p), ("n_nodes", C.c_uint64), ("node_taxid", C.c_void_p), ("node_parent", C.c_void_p),
                ("node_rank", C.POINTER(C.c_char_p)), ("n_names", C.c_uint64), ("name_taxid", C.c_void_p), ("name_text", C.POINTER(C.c_char_p)),
                ("n_genomes", C.c_uint64), ("genome_seq", C.c_void_p), ("genome_lens", C.c_void_p), ("n_extra", C.c_uint64),
                ("n_present_taxids", C.c_uint64), ("present_taxids", C.c_void_p), ("selection", C.c_void_p)]


class BuildOptions(C.Structure):
    _fields_ = [("ftab_chars", C.c_int32), ("offrate", C.c_int32), ("device", C.c_int32), ("threads", C.c_int32), ("rbbwt_b", C.c_uint64),
                ("verbose", C.c_int32), ("protein", C.c_int32)]


class BuildReport(C.Structure):
    _fields_ = [("n", C.c_uint64), ("block_size", C.c_uint64), ("first_isa", C.c_uint64), ("seconds_sa", C.c_double),
                ("seconds_total", C.c_double), ("rounds", C.c_int32), ("pad", C.c_int32)]


def build_index(names, taxids, seqs, nodes, tax_names, out_prefix, ftab_chars=10, offrate=4, rbbwt_b=0, device=0, threads=0, verbose=False,
                genome_seq=None, n_extra=0, protein=False):
    """cfr_build_index: the native writer (suffix array on the MI355X).  seqs: list of np.uint8 ASCII arrays, or one
    concatenated array together with the lengths given as (text, lens).  genome_seq: sequence id (index into names) of every
    genome of the text in text order when that is not 0, 1, 2, ... over all names; the last n_extra names have no tax id.
    protein: seqs are amino-acid strings (letters of ARNDCEQGHILKMFPSTWYV), the index is the one centrifuger-build --protein writes."""
    if isinstance(seqs, tuple):
        text, lens = seqs
        text = np.ascontiguousarray(text, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
    else:
        lens = np.array([len(x) for x in seqs], dtype=np.uint64)
        text = np.ascontiguousarray(np.concatenate(seqs), dtype=np.uint8)

    def strs(items):
        arr = (C.c_char_p * len(items))()
        arr[:] = [x.encode() if isinstance(x, str) else x for x in items]
        return arr
    inp = BuildInput()
    keep = [strs(list(names)), _u64(np.array(taxids, dtype=np.uint64)), lens, text,
            _u64(np.array([t for t, _, _ in nodes], dtype=np.uint64)), _u64(np.array([p for _, p, _ in nodes], dtype=np.uint64)),
            strs([r for _, _, r in nodes]), _u64(np.array([t for t, _ in tax_names], dtype=np.uint64)), strs([x for _, x in tax_names])]
    inp.n_seqs = len(names)
    inp.seq_names = keep[0]
    inp.seq_taxids = _p(keep[1]); inp.seq_lens = _p(keep[2]); inp.text = _p(keep[3])
    inp.n_nodes = len(nodes); inp.node_taxid = _p(keep[4]); inp.node_parent = _p(keep[5]); inp.node_rank = keep[6]
    inp.n_names = len(tax_names); inp.name_taxid = _p(keep[7]); inp.name_text = keep[8]
    if genome_seq is not None:
        keep.append(_u64(np.array(genome_seq, dtype=np.uint64)))
        inp.n_genomes = len(keep[-1]); inp.genome_seq = _p(keep[-1]); inp.genome_lens = _p(keep[2]); inp.seq_lens = None
        inp.n_extra = n_extra
    opt = BuildOptions()
    lib().cfr_build_options_default(C.byref(opt))
    opt.ftab_chars, opt.offrate, opt.device, opt.threads, opt.rbbwt_b, opt.verbose = ftab_chars, offrate, device, threads, rbbwt_b, int(verbose)
    opt.protein = int(protein)
    rep = BuildReport()
    _check(lib().cfr_build_index(C.byref(inp), C.byref(opt), out_prefix.encode(), C.byref(rep)))
    return {"n": rep.n, "b": rep.block_size, "first_isa": rep.first_isa, "seconds_sa": rep.seconds_sa, "seconds_total": rep.seconds_total,
            "rounds": rep.rounds}


# ---- the reference text of the index writer (cfr_refseq_*, cfr_build_select, cfr_build_index_assembled) ----
REFSEQ_RECORD_DTYPE = np.dtype([("header", "<u4"), ("header_len", "<u4"), ("id_len", "<u4"), ("kept", "<u4")])
REFSEQ_SEGMENT_DTYPE = np.dtype([("src", "<u8"), ("len", "<u8"), ("dst", "<u8")])


class RefseqInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("consumed", C.c_uint64), ("lead_kept", C.c_uint64), ("kept", C.c_uint64), ("u_start", C.c_uint64),
                ("at_line_start", C.c_int32), ("pad", C.c_int32), ("device_ms", C.c_double)]


class RefseqStats(C.Structure):
    _fields_ = [("feed_ms", C.c_double), ("copy_in_ms", C.c_double), ("assemble_ms", C.c_double)]


class SelectRecord(C.Structure):
    _fields_ = [("id", C.c_char_p), ("file", C.c_char_p), ("first_piece", C.c_uint64), ("n_pieces", C.c_uint64)]


class SelectOptions(C.Structure):
    _fields_ = [("file_level", C.c_int32), ("concat_tax_genome", C.c_int32), ("ignore_uncategorized", C.c_int32), ("protein", C.c_int32),
                ("subset_tax", C.c_uint64), ("ftab_chars", C.c_int32), ("pad", C.c_int32)]


def file_base_name(path: str) -> str:
    """cfr_file_base_name: Utils::GetFileBaseName(path, "fna|fa|fasta|faa")"""
    buf = C.create_string_buffer(len(path.encode()) + 1)
    lib().cfr_file_base_name(path.encode(), buf, C.c_size_t(len(buf)))
    return buf.value.decode()


class Refseq:
    """cfr_refseq: the bytes of reference FASTA files -> records and the stream U of kept symbols; assemble() copies segments of U into
    the text T of the index.  device=None: the host twin, no GPU is touched (the only path with protein=True)."""

    def __init__(self, device=None, protein=False):
        self._h = C.c_void_p()
        self._last = RefseqInfo()
        self._n = 0
        _check(lib().cfr_refseq_open(C.c_int(-1 if device is None else device), C.c_int(int(bool(protein))), C.byref(self._h)))

    def feed(self, text, at_line_start=True, final=True) -> RefseqInfo:
        a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else _u8(text)
        info = RefseqInfo()
        _check(lib().cfr_refseq_feed(self._h, _p(a), C.c_uint64(len(a)), C.c_int(int(bool(at_line_start))), C.c_int(int(bool(final))), C.byref(info)))
        self._last = info
        return info

    def fetch(self):
        """-> REFSEQ_RECORD_DTYPE[n_records] of the last feed()"""
        rec = np.zeros(self._last.n_records, dtype=REFSEQ_RECORD_DTYPE)
        _check(lib().cfr_refseq_fetch(self._h, _p(rec)))
        return rec

    def feed_file(self, data: bytes, chunk: int):
        """The bytes of one file in chunks of `chunk` bytes, as the command line feeds them -> [(id, [(src, len), ...]), ...]: every record
        with the pieces of U that hold its kept symbols (symbols before a file's first header belong to no record)."""
        out, at, line_start = [], 0, True
        while True:
            piece = data[at:at + chunk]
            final = at + chunk >= len(data)
            info = self.feed(piece, line_start, final)
            recs = self.fetch()
            src = info.u_start
            if info.lead_kept and out:
                out[-1][1].append((src, int(info.lead_kept)))
            src += info.lead_kept
            for r in recs:
                h = int(r["header"])
                out.append((bytes(piece[h + 1:h + 1 + int(r["id_len"])]).decode("latin-1"), [(src, int(r["kept"]))] if r["kept"] else []))
                src += int(r["kept"])
            at += info.consumed
            line_start = bool(info.at_line_start)
            if final:
                return out

    def assemble(self, segments, n=None):
        """segments: REFSEQ_SEGMENT_DTYPE array or a list of (src, len, dst)"""
        seg = np.ascontiguousarray(np.array(segments, dtype=REFSEQ_SEGMENT_DTYPE) if not isinstance(segments, np.ndarray) else segments)
        if n is None:
            n = int(seg["len"].sum())
        _check(lib().cfr_refseq_assemble(self._h, _p(seg), C.c_uint64(len(seg)), C.c_uint64(n)))
        self._n = n

    def text(self) -> bytes:
        out = np.zeros(max(self._n, 1), dtype=np.uint8)
        _check(lib().cfr_refseq_text(self._h, _p(out)))
        return out[:self._n].tobytes()

    def stats(self) -> RefseqStats:
        st = RefseqStats()
        _check(lib().cfr_refseq_get_stats(self._h, C.byref(st)))
        return st

    def close(self):
        if self._h:
            lib().cfr_refseq_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _build_input(names, taxids, nodes, tax_names, present_taxids=None):
    def strs(items):
        arr = (C.c_char_p * max(len(items), 1))()
        arr[:len(items)] = [x.encode() if isinstance(x, str) else x for x in items]
        return arr
    inp = BuildInput()
    keep = [strs(list(names)), _u64(np.array(taxids, dtype=np.uint64)),
            _u64(np.array([t for t, _, _ in nodes], dtype=np.uint64)), _u64(np.array([p for _, p, _ in nodes], dtype=np.uint64)),
            strs([r for _, _, r in nodes]), _u64(np.array([t for t, _ in tax_names], dtype=np.uint64)), strs([x for _, x in tax_names]),
            _u64(np.array(present_taxids if present_taxids is not None else [], dtype=np.uint64))]
    inp.n_seqs = len(names); inp.seq_names = keep[0]; inp.seq_taxids = _p(keep[1])
    inp.n_nodes = len(nodes); inp.node_taxid = _p(keep[2]); inp.node_parent = _p(keep[3]); inp.node_rank = keep[4]
    inp.n_names = len(tax_names); inp.name_taxid = _p(keep[5]); inp.name_text = keep[6]
    inp.n_present_taxids = len(keep[7]); inp.present_taxids = _p(keep[7])
    return inp, keep


class BuildSelection:
    """cfr_build_select: records -> genomes and segments.  names / taxids: the conversion table (file_level: the file list, base names);
    records: [(id, file, [(src, len), ...]), ...] in reading order."""

    def __init__(self, names, taxids, nodes, tax_names, records, ftab_chars=10, file_level=False, concat=False, ignore_uncategorized=False,
                 subset_tax=0, protein=False, present_taxids=None):
        self._h = C.c_void_p()
        self.inp, self._keep = _build_input(names, taxids, nodes, tax_names, present_taxids)
        recs = (SelectRecord * max(len(records), 1))()
        pieces = []
        for k, (rid, f, pcs) in enumerate(records):
            recs[k].id, recs[k].file, recs[k].first_piece, recs[k].n_pieces = rid.encode("latin-1"), f.encode(), len(pieces), len(pcs)
            pieces.extend(pcs)
        pc = np.ascontiguousarray(np.array(pieces, dtype=np.uint64).reshape(-1, 2))
        so = SelectOptions(int(file_level), int(concat), int(ignore_uncategorized), int(protein), subset_tax, ftab_chars, 0)
        _check(lib().cfr_build_select(C.byref(self.inp), C.byref(so), recs, C.c_uint64(len(records)), _p(pc), C.c_uint64(len(pc)), C.byref(self._h)))
        self.inp.selection = self._h
        seg, ns, n, ng, nx = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().cfr_build_selection_get(self._h, C.byref(seg), C.byref(ns), C.byref(n), C.byref(ng), C.byref(nx)))
        self.n, self.n_genomes, self.n_extra = n.value, ng.value, nx.value
        self.segments = np.ctypeslib.as_array(C.cast(seg, C.POINTER(C.c_uint64)), shape=(ns.value * 3,)).copy().view(REFSEQ_SEGMENT_DTYPE) if ns.value else np.zeros(0, dtype=REFSEQ_SEGMENT_DTYPE)

    def close(self):
        if self._h:
            lib().cfr_build_selection_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_index_assembled(refseq: Refseq, selection: BuildSelection, out_prefix, ftab_chars=10, offrate=4, rbbwt_b=0, device=0, threads=0, verbose=False,
                          protein=False):
    """cfr_build_index_assembled: the writer on the text the handle has assembled from selection.segments"""
    opt = BuildOptions()
    lib().cfr_build_options_default(C.byref(opt))
    opt.ftab_chars, opt.offrate, opt.device, opt.threads, opt.rbbwt_b, opt.verbose = ftab_chars, offrate, device, threads, rbbwt_b, int(verbose)
    opt.protein = int(protein)
    rep = BuildReport()
    _check(lib().cfr_build_index_assembled(refseq._h, C.byref(selection.inp), C.byref(opt), out_prefix.encode(), C.byref(rep)))
    return {"n": rep.n, "b": rep.block_size, "first_isa": rep.first_isa, "seconds_sa": rep.seconds_sa, "seconds_total": rep.seconds_total,
            "rounds": rep.rounds}


class Index:
    """cfr_index: host copy of <prefix>.{1,2,4}.cfr (Classifier::Init, Classifier.hpp:902-947)."""

    def __init__(self, prefix: str, params: Params | None = None):
        self._h = C.c_void_p()
        self.params = params if params is not None else default_params()
        _check(lib().cfr_index_open(prefix.encode(), C.byref(self.params), C.byref(self._h)))

    def info(self) -> IndexInfo:
        info = IndexInfo()
        _check(lib().cfr_index_get_info(self._h, C.byref(info)))
        return info

    def digest(self) -> int:
        """cfr_index_digest: 64-bit digest of everything the parser produced"""
        d = C.c_uint64(0)
        _check(lib().cfr_index_digest(self._h, C.byref(d)))
        return d.value

    def mapped_bytes(self):
        """cfr_index_mapped_bytes: (bytes of bit strings read from the file's mapping, bytes held as private copies)"""
        m, c = C.c_uint64(0), C.c_uint64(0)
        _check(lib().cfr_index_mapped_bytes(self._h, C.byref(m), C.byref(c)))
        return m.value, c.value

    def close(self):
        if self._h:
            lib().cfr_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def format_tsv(self, read_id: str, result, matches) -> bytes:
        r = np.ascontiguousarray(result).reshape(1)
        buf = C.create_string_buffer(1 << 16)
        n = lib().cfr_format_tsv(self._h, read_id.encode(), _p(r), _p(matches), buf, C.c_size_t(len(buf)))
        if n >= len(buf):
            buf = C.create_string_buffer(n + 1)
            lib().cfr_format_tsv(self._h, read_id.encode(), _p(r), _p(matches), buf, C.c_size_t(len(buf)))
        return buf.raw[:n]

    def format_tsv_ex(self, read_id: str, result, matches, has_barcode=False, barcode=None, has_umi=False, umi=None, expanded=False,
                      spans=None, ids=None) -> bytes:
        """cfr_format_tsv_ex: the row(s) of one read with the barcode / UMI columns (barcode / umi: bytes, None = a bare tab)"""
        r = np.ascontiguousarray(result).reshape(1)
        buf = C.create_string_buffer(1 << 16)
        args = (self._h, read_id.encode(), _p(r), _p(matches), C.c_int(int(has_barcode)), C.c_char_p(barcode), C.c_int(int(has_umi)), C.c_char_p(umi),
                C.c_int(int(expanded)), _p(spans), _p(ids))
        n = lib().cfr_format_tsv_ex(*args, buf, C.c_size_t(len(buf)))
        if n >= len(buf):
            buf = C.create_string_buffer(n + 1)
            lib().cfr_format_tsv_ex(*args, buf, C.c_size_t(len(buf)))
        return buf.raw[:n]

    def format_tsv_expanded(self, read_id: str, result, matches, spans, ids) -> bytes:
        """cfr_format_tsv_expanded: the row(s) of one read with the expandedTaxIDs column"""
        r = np.ascontiguousarray(result).reshape(1)
        buf = C.create_string_buffer(1 << 16)
        n = lib().cfr_format_tsv_expanded(self._h, read_id.encode(), _p(r), _p(matches), _p(spans), _p(ids), buf, C.c_size_t(len(buf)))
        if n >= len(buf):
            buf = C.create_string_buffer(n + 1)
            lib().cfr_format_tsv_expanded(self._h, read_id.encode(), _p(r), _p(matches), _p(spans), _p(ids), buf, C.c_size_t(len(buf)))
        return buf.raw[:n]

    def classify_from_hits_expanded(self, hits, hit_begin, row_begin, row_vals, query_len, threads=1):
        """cfr_classify_from_hits_expanded -> (results, matches, spans, ids)"""
        n = len(hit_begin) - 1
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        hit_begin, row_begin, row_vals = _u64(hit_begin), _u64(row_begin), _u64(row_vals)
        query_len = np.ascontiguousarray(query_len, dtype=np.int32)
        results = np.zeros(n, dtype=RESULT_DTYPE)
        cap, icap = max(16, 4 * n), max(16, 4 * n)
        while True:
            matches = np.zeros(cap, dtype=MATCH_DTYPE)
            spans = np.zeros(cap, dtype=SPAN_DTYPE)
            ids = np.zeros(icap, dtype=np.uint64)
            nm, ni = C.c_size_t(0), C.c_size_t(0)
            st = lib().cfr_classify_from_hits_expanded(self._h, _p(hits), _p(hit_begin), _p(row_begin), _p(row_vals), _p(query_len),
                                                       C.c_size_t(n), C.c_int(threads), _p(results), _p(matches), _p(spans), C.c_size_t(cap),
                                                       C.byref(nm), _p(ids), C.c_size_t(icap), C.byref(ni))
            if st == CFR_ERR_CAPACITY:
                cap, icap = max(cap, int(nm.value) + 16), max(icap, int(ni.value) + 16)
                continue
            _check(st)
            return results, matches[:nm.value], spans[:nm.value], ids[:ni.value]

    def classify_from_hits(self, hits, hit_begin, row_begin, row_vals, query_len, threads=1):
        n = len(hit_begin) - 1
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        hit_begin, row_begin, row_vals = _u64(hit_begin), _u64(row_begin), _u64(row_vals)
        query_len = np.ascontiguousarray(query_len, dtype=np.int32)
        results = np.zeros(n, dtype=RESULT_DTYPE)
        cap = max(16, 4 * n)
        while True:
            matches = np.zeros(cap, dtype=MATCH_DTYPE)
            nm = C.c_size_t(0)
            st = lib().cfr_classify_from_hits(self._h, _p(hits), _p(hit_begin), _p(row_begin), _p(row_vals), _p(query_len),
                                              C.c_size_t(n), C.c_int(threads), _p(results), _p(matches), C.c_size_t(cap), C.byref(nm))
            if st == CFR_ERR_CAPACITY:
                cap = int(nm.value) + 16
                continue
            _check(st)
            return results, matches[:nm.value]


class DeviceOptions(C.Structure):
    """cfr_device_options (include/cfr_hip.h)."""
    _fields_ = [("profile", C.c_int32), ("ftabx_width", C.c_int32), ("text_mode", C.c_int32), ("run_block_layout", C.c_int32),
                ("loc_memo_gb", C.c_double), ("sub_batch", C.c_uint64)]


PROFILE_THROUGHPUT, PROFILE_FAST_LOAD = 0, 1


def default_device_options(**kw) -> DeviceOptions:
    o = DeviceOptions()
    lib().cfr_device_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class DeviceIndex:
    """cfr_dev_index: the flat index image in one GPU's HBM + the batch entry points."""

    def __init__(self, index: Index, device: int = 0, options: DeviceOptions | None = None):
        self.index = index
        self._d = C.c_void_p()
        if options is None:
            _check(lib().cfr_device_index_create(index._h, C.c_int(device), C.byref(self._d)))
        else:
            _check(lib().cfr_device_index_create_ex(index._h, C.c_int(device), C.byref(options), C.byref(self._d)))

    def info(self) -> IndexInfo:
        info = IndexInfo()
        _check(lib().cfr_device_index_get_info(self._d, C.byref(info)))
        return info

    def set_dust(self, on: bool):
        """SDUST on the device before every following classify call (the caller hands over unmasked reads)."""
        _check(lib().cfr_device_index_set_dust(self._d, C.c_int(1 if on else 0)))

    def dust_mask(self, bases, offsets):
        """The device SDUST scan alone: masks `bases` (uint8 numpy, host) in place."""
        assert bases.dtype == np.uint8 and bases.flags["C_CONTIGUOUS"] and bases.flags["WRITEABLE"]
        offsets = _u64(offsets)
        _check(lib().cfr_dust_mask_device(self._d, _p(bases), _p(offsets), C.c_size_t(len(offsets) - 1)))

    def set_merge(self, on: bool):
        """--merge-readpair: classify_merged / classify_resident_merged merge overlapping pairs in HBM first (nucleotide indexes)."""
        _check(lib().cfr_device_index_set_merge(self._d, C.c_int(1 if on else 0)))

    def merge_pairs(self, bases1, offsets1, bases2, offsets2, qual1=None, qual2=None):
        """The device merge kernels alone (cfr_merge_pairs_device), host arrays in and out: see merge_pairs()."""
        return _merge_pairs(lambda *a: lib().cfr_merge_pairs_device(self._d, *a), bases1, offsets1, bases2, offsets2, qual1, qual2, None)

    def classify_merged(self, bases1, offsets1, bases2=None, offsets2=None, qual1=None, qual2=None):
        """cfr_classify_batch_merged -> (results, matches, merge_kind)"""
        bases1, offsets1, bases2, offsets2, qual1, qual2 = _u8(bases1), _u64(offsets1), _u8(bases2), _u64(offsets2), _u8(qual1), _u8(qual2)
        n = len(offsets1) - 1
        results = np.zeros(n, dtype=RESULT_DTYPE)
        kind = np.zeros(n, dtype=np.int32)
        cap = max(16, max(1, self.index.params.max_result) * n)
        while True:
            matches = np.zeros(cap, dtype=MATCH_DTYPE)
            nm = C.c_size_t(0)
            st = lib().cfr_classify_batch_merged(self._d, _p(bases1), _p(offsets1), _p(qual1), _p(bases2), _p(offsets2), _p(qual2), C.c_size_t(n),
                                                 _p(results), _p(matches), C.c_size_t(cap), C.byref(nm), _p(kind))
            if st == CFR_ERR_CAPACITY:
                cap = int(nm.value) + 16
                continue
            _check(st)
            return results, matches[:nm.value], kind

    def classify_resident_merged(self, d_bases1: int, d_offsets1: int, n: int, total1: int, d_bases2: int = 0, d_offsets2: int = 0,
                                 total2: int = 0, d_qual1: int = 0, d_qual2: int = 0, results=None, matches=None):
        """cfr_classify_batch_resident_merged: device pointers in (ints, qualities included) -> (results, matches, merge_kind)"""
        if results is None:
            results = np.zeros(n, dtype=RESULT_DTYPE)
        if matches is None:
            matches = np.zeros(max(16, max(1, self.index.params.max_result) * n), dtype=MATCH_DTYPE)
        kind = np.zeros(n, dtype=np.int32)
        nm = C.c_size_t(0)
        _check(lib().cfr_classify_batch_resident_merged(self._d, C.c_void_p(d_bases1), C.c_void_p(d_offsets1), C.c_void_p(d_qual1 or None),
                                                        C.c_void_p(d_bases2 or None), C.c_void_p(d_offsets2 or None), C.c_void_p(d_qual2 or None),
                                                        C.c_size_t(n), C.c_uint64(total1), C.c_uint64(total2), _p(results), _p(matches),
                                                        C.c_size_t(len(matches)), C.byref(nm), _p(kind)))
        return results, matches[:nm.value], kind

    def set_promote(self, level):
        """cfr_device_index_set_promote: every following wide classify call promotes its results to `level` ("lca" or a rank string) in
        HBM before they are copied out; None switches it off"""
        _check(lib().cfr_device_index_set_promote(self._d, None if level is None else level.encode()))

    def set_kreport(self, on=True, **options):
        """cfr_device_index_set_kreport: every following wide classify call counts its reads into the image's bins (options as
        kreport_options(); on=False switches it off).  Switching it on zeroes the bins."""
        if not on:
            _check(lib().cfr_device_index_set_kreport(self._d, None))
            return
        o = kreport_options(**options)
        _check(lib().cfr_device_index_set_kreport(self._d, C.byref(o)))

    def kreport_counts(self, bins: int):
        """(own, own_score, seq_count) of the image's bins; bins = node_cnt + 1 (Kreport.bins)"""
        own, sc = np.zeros(bins, dtype=np.uint64), np.zeros(bins, dtype=np.uint64)
        seq = C.c_double(0)
        _check(lib().cfr_device_index_kreport_counts(self._d, _p(own), _p(sc), C.c_size_t(bins), C.byref(seq)))
        return own, sc, seq.value

    def set_tsv(self, on: bool = True):
        """cfr_device_index_set_tsv: every following wide classify call keeps its final results in HBM for tsv_last()"""
        _check(lib().cfr_device_index_set_tsv(self._d, C.c_int(int(bool(on)))))

    def _tsv_last(self, call, a, b, cap, want_offsets, n):
        text = np.zeros(max(cap, 1), dtype=np.uint8)
        ln = C.c_uint64(0)
        off = np.zeros(n + 1, dtype=np.uint64) if want_offsets else None
        status = call(self._d, a, b, _p(text), C.c_uint64(cap), C.byref(ln), _p(off))
        if status == CFR_ERR_CAPACITY and cap < ln.value:
            return self._tsv_last(call, a, b, ln.value, want_offsets, n)
        _check(status)
        out = text[:ln.value].tobytes()
        return (out, off) if want_offsets else out

    def tsv_last(self, ids, cap=1 << 16, want_offsets=False):
        """the rows of the last classify call (set_tsv on) as bytes; ids: the read ids (str or bytes), uploaded by the call"""
        id_bytes, id_off = pack_ids(ids)
        return self._tsv_last(lib().cfr_device_index_tsv_last, _p(id_bytes), _p(id_off), cap, want_offsets, len(ids))

    def tsv_last_resident(self, d_text: int, d_records: int, n: int, cap=1 << 16, want_offsets=False):
        """the same with the ids where Tokenizer.device_records() says they are: nothing but the text crosses PCIe"""
        return self._tsv_last(lib().cfr_device_index_tsv_last_resident, C.c_void_p(d_text), C.c_void_p(d_records), cap, want_offsets, n)

    def last_tsv_ms(self) -> float:
        ms = C.c_float(0)
        _check(lib().cfr_last_tsv_ms(self._d, C.byref(ms)))
        return ms.value

    def last_kreport_ms(self) -> float:
        ms = C.c_float(0)
        _check(lib().cfr_last_kreport_ms(self._d, C.byref(ms)))
        return ms.value

    def last_promote_ms(self) -> float:
        ms = C.c_float(0)
        _check(lib().cfr_last_promote_ms(self._d, C.byref(ms)))
        return ms.value

    def last_merge_ms(self) -> float:
        ms = C.c_float(0)
        _check(lib().cfr_last_merge_ms(self._d, C.byref(ms)))
        return ms.value

    def close(self):
        if self._d:
            lib().cfr_device_index_destroy(self._d)
            self._d = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- probes
    def rank(self, chars, pos, inclusive):
        chars = np.ascontiguousarray(np.frombuffer(chars, dtype=np.uint8) if isinstance(chars, (bytes, bytearray)) else chars, dtype=np.uint8)
        pos, inclusive = _u64(pos), _u8(inclusive)
        n = len(pos)
        out_r = np.zeros(n, dtype=np.uint64)
        out_a = np.zeros(n, dtype=np.uint8)
        _check(lib().cfr_rank_batch(self._d, _p(chars), _p(pos), _p(inclusive), C.c_size_t(n), _p(out_r), _p(out_a)))
        return out_r, out_a

    def backward_search(self, bases, offsets, m):
        bases, offsets = _u8(bases), _u64(offsets)
        m = np.ascontiguousarray(m, dtype=np.uint32)
        n = len(m)
        l, sp, ep = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        _check(lib().cfr_backward_search_batch(self._d, _p(bases), _p(offsets), _p(m), C.c_size_t(n), _p(l), _p(sp), _p(ep)))
        return l, sp, ep

    def locate(self, rows):
        rows = _u64(rows)
        n = len(rows)
        val = np.zeros(n, dtype=np.uint64)
        steps = np.zeros(n, dtype=np.uint32)
        _check(lib().cfr_locate_rows(self._d, _p(rows), C.c_size_t(n), _p(val), _p(steps)))
        return val, steps

    def selfcheck(self):
        """dict of the derived-table self-check (all bad_* must be 0)"""
        out = np.zeros(6, dtype=np.uint64)
        _check(lib().cfr_selfcheck_tables(self._d, _p(out)))
        return {"bad_sa_isa": int(out[0]), "bad_text": int(out[1]), "bad_lf": int(out[2]), "bad_memo": int(out[3]),
                "text_tables": bool(out[4]), "memo": int(out[5])}

    # ---- the path
    def search(self, bases1, offsets1, bases2=None, offsets2=None):
        bases1, offsets1, bases2, offsets2 = _u8(bases1), _u64(offsets1), _u8(bases2), _u64(offsets2)
        n = len(offsets1) - 1
        hit_begin = np.zeros(n + 1, dtype=np.uint64)
        cap = max(64, 16 * n)
        while True:
            hits = np.zeros(cap, dtype=HIT_DTYPE)
            st = lib().cfr_search_batch(self._d, _p(bases1), _p(offsets1), _p(bases2), _p(offsets2), C.c_size_t(n),
                                        _p(hits), C.c_size_t(cap), _p(hit_begin))
            if st == CFR_ERR_CAPACITY:
                cap = int(hit_begin[n]) + 16
                continue
            _check(st)
            return hits[:int(hit_begin[n])], hit_begin

    def classify(self, bases1, offsets1, bases2=None, offsets2=None, results=None, matches=None):
        """Host buffers in, host buffers out (cfr_classify_batch).  results / matches: caller-provided arrays (e.g. PinnedArray
        views; matches must hold max_result slots per read) instead of fresh numpy arrays."""
        bases1, offsets1, bases2, offsets2 = _u8(bases1), _u64(offsets1), _u8(bases2), _u64(offsets2)
        n = len(offsets1) - 1
        if results is not None and matches is not None:
            nm = C.c_size_t(0)
            _check(lib().cfr_classify_batch(self._d, _p(bases1), _p(offsets1), _p(bases2), _p(offsets2), C.c_size_t(n),
                                            _p(results), _p(matches), C.c_size_t(len(matches)), C.byref(nm)))
            return results, matches[:nm.value]
        results = np.zeros(n, dtype=RESULT_DTYPE)
        cap = max(16, max(1, self.index.params.max_result) * n)
        while True:
            matches = np.zeros(cap, dtype=MATCH_DTYPE)
            nm = C.c_size_t(0)
            st = lib().cfr_classify_batch(self._d, _p(bases1), _p(offsets1), _p(bases2), _p(offsets2), C.c_size_t(n),
                                          _p(results), _p(matches), C.c_size_t(cap), C.byref(nm))
            if st == CFR_ERR_CAPACITY:
                cap = int(nm.value) + 16
                continue
            _check(st)
            return results, matches[:nm.value]

    def classify_expanded(self, bases1, offsets1, bases2=None, offsets2=None, ids_cap=None):
        """cfr_classify_batch_expanded (the index must have been opened with output_expanded=1) -> (results, matches, spans, ids)"""
        bases1, offsets1, bases2, offsets2 = _u8(bases1), _u64(offsets1), _u8(bases2), _u64(offsets2)
        n = len(offsets1) - 1
        results = np.zeros(n, dtype=RESULT_DTYPE)
        cap = max(16, max(1, self.index.params.max_result) * n)
        icap = ids_cap if ids_cap is not None else max(16, 4 * n)
        while True:
            matches = np.zeros(cap, dtype=MATCH_DTYPE)
            spans = np.zeros(cap, dtype=SPAN_DTYPE)
            ids = np.zeros(max(icap, 1), dtype=np.uint64)
            nm, ni = C.c_size_t(0), C.c_size_t(0)
            st = lib().cfr_classify_batch_expanded(self._d, _p(bases1), _p(offsets1), _p(bases2), _p(offsets2), C.c_size_t(n), _p(results), _p(matches),
                                                   _p(spans), C.c_size_t(cap), C.byref(nm), _p(ids), C.c_size_t(icap), C.byref(ni))
            if st == CFR_ERR_CAPACITY:
                cap, icap = max(cap, int(nm.value) + 16), max(icap, int(ni.value))
                continue
            _check(st)
            return results, matches[:nm.value], spans[:nm.value], ids[:ni.value]

    def classify_packed(self, packed1, offsets1, packed2=None, offsets2=None, results=None, matches=None):
        """cfr_classify_batch_packed: the bases as packed blocks (pack_reads) instead of ASCII; same results as classify()"""
        packed1, offsets1, packed2, offsets2 = _u64(packed1), _u64(offsets1), _u64(packed2), _u64(offsets2)
        n = len(offsets1) - 1
        if results is None:
            results = np.zeros(n, dtype=RESULT_DTYPE)
        if matches is None:
            matches = np.zeros(max(16, max(1, self.index.params.max_result) * n), dtype=MATCH_DTYPE)
        while True:
            nm = C.c_size_t(0)
            st = lib().cfr_classify_batch_packed(self._d, _p(packed1), _p(offsets1), _p(packed2), _p(offsets2), C.c_size_t(n),
                                                 _p(results), _p(matches), C.c_size_t(len(matches)), C.byref(nm))
            if st == CFR_ERR_CAPACITY:
                matches = np.zeros(int(nm.value) + 16, dtype=MATCH_DTYPE)
                continue
            _check(st)
            return results, matches[:nm.value]

    def compact_wide(self):
        """cfr_compact_wide_reads: (read_index, results, matches) of the reads the last compact call flagged CFR_COMPACT_WIDE"""
        n = C.c_size_t(0)
        pi, pr, pm = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().cfr_compact_wide_reads(self._d, C.byref(n), C.byref(pi), C.byref(pr), C.byref(pm)))
        k = max(1, self.index.params.max_result)
        if n.value == 0:
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=RESULT_DTYPE), np.zeros(0, dtype=MATCH_DTYPE)
        idx = np.ctypeslib.as_array(C.cast(pi, C.POINTER(C.c_uint32)), shape=(n.value,)).copy()
        res = np.frombuffer(C.string_at(pr, n.value * RESULT_DTYPE.itemsize), dtype=RESULT_DTYPE).copy()
        mat = np.frombuffer(C.string_at(pm, n.value * k * MATCH_DTYPE.itemsize), dtype=MATCH_DTYPE).copy()
        return idx, res, mat

    def submit(self, bases1, offsets1, bases2=None, offsets2=None, results=None, matches=None):
        """cfr_classify_batch_submit: queue a batch, return a ticket object for wait().  The arrays are kept alive by the ticket."""
        bases1, offsets1, bases2, offsets2 = _u8(bases1), _u64(offsets1), _u8(bases2), _u64(offsets2)
        n = len(offsets1) - 1
        if results is None:
            results = np.zeros(n, dtype=RESULT_DTYPE)
        if matches is None:
            matches = np.zeros(max(16, max(1, self.index.params.max_result) * n), dtype=MATCH_DTYPE)
        t = C.c_uint64(0)
        _check(lib().cfr_classify_batch_submit(self._d, _p(bases1), _p(offsets1), _p(bases2), _p(offsets2), C.c_size_t(n),
                                               _p(results), _p(matches), C.c_size_t(len(matches)), C.byref(t)))
        return {"ticket": t.value, "keep": (bases1, offsets1, bases2, offsets2), "results": results, "matches": matches}

    def wait(self, job):
        """cfr_classify_batch_wait: the (results, matches) of a submitted batch"""
        nm = C.c_size_t(0)
        _check(lib().cfr_classify_batch_wait(self._d, C.c_uint64(job["ticket"]), C.byref(nm)))
        return job["results"], job["matches"][:nm.value]

    def classify_resident(self, d_bases1: int, d_offsets1: int, n: int, total1: int, d_bases2: int = 0, d_offsets2: int = 0,
                          total2: int = 0, results=None, matches=None):
        """Device pointers in (ints), host numpy out.  Caller must have synchronised the producer stream."""
        if results is None:
            results = np.zeros(n, dtype=RESULT_DTYPE)
        if matches is None:
            matches = np.zeros(max(16, max(1, self.index.params.max_result) * n), dtype=MATCH_DTYPE)
        nm = C.c_size_t(0)
        st = lib().cfr_classify_batch_resident(self._d, C.c_void_p(d_bases1), C.c_void_p(d_offsets1),
                                               C.c_void_p(d_bases2 or None), C.c_void_p(d_offsets2 or None), C.c_size_t(n),
                                               C.c_uint64(total1), C.c_uint64(total2), _p(results), _p(matches),
                                               C.c_size_t(len(matches)), C.byref(nm))
        _check(st)
        return results, matches[:nm.value]

    def classify_resident_compact(self, d_bases1: int, d_offsets1: int, n: int, total1: int, d_bases2: int = 0, d_offsets2: int = 0,
                                  total2: int = 0, results=None, matches=None):
        """classify_resident with the narrow result layout (RESULT_COMPACT_DTYPE / MATCH_COMPACT_DTYPE arrays; max_result > 0);
        expand_compact() gives the wide arrays."""
        k = max(1, self.index.params.max_result)
        if results is None:
            results = np.zeros(n, dtype=RESULT_COMPACT_DTYPE)
        if matches is None:
            matches = np.zeros(max(16, k * n), dtype=MATCH_COMPACT_DTYPE)
        nm = C.c_size_t(0)
        st = lib().cfr_classify_batch_resident_compact(self._d, C.c_void_p(d_bases1), C.c_void_p(d_offsets1),
                                                       C.c_void_p(d_bases2 or None), C.c_void_p(d_offsets2 or None), C.c_size_t(n),
                                                       C.c_uint64(total1), C.c_uint64(total2), _p(results), _p(matches),
                                                       C.c_size_t(len(matches)), C.byref(nm))
        _check(st)
        return results, matches[:nm.value]

    def last_stats(self) -> BatchStats:
        st = BatchStats()
        _check(lib().cfr_last_batch_stats(self._d, C.byref(st)))
        return st


def device_count() -> int:
    c = C.c_int(0)
    st = lib().cfr_device_count(C.byref(c))
    return c.value if st == CFR_OK else 0


def dust_mask(bases, offsets, threads=1, literal=False):
    """In-place SDUST masking of a flat read buffer (cfr_dust_mask_batch; literal=True: the reference's own data structure)."""
    assert bases.dtype == np.uint8 and bases.flags["C_CONTIGUOUS"] and bases.flags["WRITEABLE"]
    offsets = _u64(offsets)
    fn = lib().cfr_dust_mask_batch_literal if literal else lib().cfr_dust_mask_batch
    _check(fn(_p(bases), _p(offsets), C.c_size_t(len(offsets) - 1), C.c_int(threads)))
    return bases


def _merge_pairs(call, bases1, offsets1, bases2, offsets2, qual1, qual2, threads):
    bases1, offsets1, bases2, offsets2, qual1, qual2 = _u8(bases1), _u64(offsets1), _u8(bases2), _u64(offsets2), _u8(qual1), _u8(qual2)
    n = len(offsets1) - 1
    t1, t2 = int(offsets1[n]), int(offsets2[n])
    ob1, ob2 = np.zeros(t1 + t2 + 1, dtype=np.uint8), np.zeros(t2 + 1, dtype=np.uint8)
    oq1 = np.zeros(t1 + t2 + 1, dtype=np.uint8) if qual1 is not None else None
    oq2 = np.zeros(t2 + 1, dtype=np.uint8) if qual1 is not None else None
    oo1, oo2 = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    kind, overlap, offset = (np.zeros(n, dtype=np.int32) for _ in range(3))
    args = [_p(bases1), _p(offsets1), _p(qual1), _p(bases2), _p(offsets2), _p(qual2), C.c_size_t(n)]
    if threads is not None:
        args.append(C.c_int(threads))
    _check(call(*args, _p(ob1), _p(oo1), _p(oq1), _p(ob2), _p(oo2), _p(oq2), _p(kind), _p(overlap), _p(offset)))
    m1, m2 = int(oo1[n]), int(oo2[n])
    return {"bases1": ob1[:m1], "offsets1": oo1, "qual1": None if oq1 is None else oq1[:m1],
            "bases2": ob2[:m2], "offsets2": oo2, "qual2": None if oq2 is None else oq2[:m2],
            "kind": kind, "overlap": overlap, "offset": offset}


def merge_pairs(bases1, offsets1, bases2, offsets2, qual1=None, qual2=None, threads=1):
    """cfr_merge_pairs (ReadPairMerger::Merge per pair, on the host): dict of the new reads (merged pair: read 1 = the merged read,
    read 2 = empty), their qualities when given, and kind / overlap / offset per pair."""
    return _merge_pairs(lib().cfr_merge_pairs, bases1, offsets1, bases2, offsets2, qual1, qual2, threads)


def pack_reads(bases, threads=1, out=None):
    """cfr_pack_reads: uint64 blocks of 16 characters (2-bit codes + validity bits) of a flat ASCII read buffer"""
    bases = _u8(bases)
    nblk = (len(bases) + 15) // 16
    if out is None:
        out = np.empty(max(nblk, 1), dtype=np.uint64)
    _check(lib().cfr_pack_reads(_p(bases), C.c_uint64(len(bases)), C.c_int(threads), _p(out)))
    return out[:nblk]


def tsv_header() -> bytes:
    return lib().cfr_tsv_header()


def tsv_header_ex(has_barcode=False, has_umi=False, expanded=False) -> bytes:
    return lib().cfr_tsv_header_ex(C.c_int(int(has_barcode)), C.c_int(int(has_umi)), C.c_int(int(expanded)))


class PinnedArray:
    """numpy view over cfr_host_alloc memory (pinned: D2H lands at PCIe rate)."""

    def __init__(self, count: int, dtype):
        self.dtype = np.dtype(dtype)
        self.nbytes = max(16, count * self.dtype.itemsize)
        self._p = lib().cfr_host_alloc(C.c_size_t(self.nbytes))
        if not self._p:
            raise CfrError(-1, "cfr_host_alloc failed")
        buf = (C.c_uint8 * self.nbytes).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=count)

    def free(self):
        if self._p:
            self.array = None
            lib().cfr_host_free(C.c_void_p(self._p))
            self._p = None


class QuantOptions(C.Structure):
    _fields_ = [("min_score", C.c_uint64), ("min_length", C.c_int32), ("device", C.c_int32), ("table_slots", C.c_uint64),
                ("threads", C.c_int32), ("pad", C.c_int32)]


class QuantStats(C.Structure):
    _fields_ = [("reader_ms", C.c_double), ("coalesce_ms", C.c_double), ("em_ms", C.c_double), ("grow_count", C.c_uint64),
                ("table_slots", C.c_uint64), ("em_rounds", C.c_int32), ("pad", C.c_int32)]


class Quant:
    """cfr_quant: abundance estimation (centrifuger-quant).  device=None: the host twin, no GPU is touched."""

    def __init__(self, prefix: str, device=0, min_score=0, min_length=0, table_slots=0, threads=0):
        opt = QuantOptions()
        lib().cfr_quant_options_default(C.byref(opt))
        opt.min_score, opt.min_length, opt.table_slots, opt.threads = min_score, min_length, table_slots, threads
        opt.device = -1 if device is None else device
        self._q = C.c_void_p()
        _check(lib().cfr_quant_open(prefix.encode(), C.byref(opt), C.byref(self._q)))

    def add_tsv(self, path: str):
        _check(lib().cfr_quant_add_tsv(self._q, path.encode()))

    def add_results(self, results, matches):
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        matches = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        _check(lib().cfr_quant_add_results(self._q, _p(results), _p(matches), C.c_size_t(len(results))))

    def assignments(self):
        """(lists, weight, count, uniq): lists = tuples of compact tax ids in the reference's order"""
        n = C.c_size_t()
        pb, pt, pw, pc, pu = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        _check(lib().cfr_quant_assignments(self._q, C.byref(n), C.byref(pb), C.byref(pt), C.byref(pw), C.byref(pc), C.byref(pu)))
        n = n.value
        begin = np.ctypeslib.as_array(pb, shape=(n + 1,)).copy()
        targets = np.ctypeslib.as_array(pt, shape=(max(int(begin[n]), 1),))[:int(begin[n])].copy() if n else np.zeros(0, dtype=np.uint32)
        lists = [tuple(int(x) for x in targets[int(begin[i]):int(begin[i + 1])]) for i in range(n)]
        arr = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0)   # noqa: E731
        return lists, arr(pw), arr(pc), arr(pu)

    def run(self) -> int:
        rounds = C.c_int32()
        _check(lib().cfr_quant_run(self._q, C.byref(rounds)))
        return rounds.value

    def values(self):
        """dict of abund, read_count, uniq_count (float64) and taxid_length (uint64), node_cnt + 1 entries each"""
        pa, pr, pu, pl, nc = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)(), C.c_uint64()
        _check(lib().cfr_quant_values(self._q, C.byref(pa), C.byref(pr), C.byref(pu), C.byref(pl), C.byref(nc)))
        n = nc.value + 1
        return {"abund": np.ctypeslib.as_array(pa, shape=(n,)).copy(), "read_count": np.ctypeslib.as_array(pr, shape=(n,)).copy(),
                "uniq_count": np.ctypeslib.as_array(pu, shape=(n,)).copy(), "taxid_length": np.ctypeslib.as_array(pl, shape=(n,)).copy(),
                "node_cnt": nc.value}

    def write(self, path: str, fmt: int = 0):
        _check(lib().cfr_quant_write(self._q, C.c_int(fmt), path.encode()))

    def stats(self) -> QuantStats:
        st = QuantStats()
        _check(lib().cfr_quant_get_stats(self._q, C.byref(st)))
        return st

    def close(self):
        if self._q:
            lib().cfr_quant_destroy(self._q)
            self._q = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def quant_estep_probe(a_begin, a_target, a_weight, n_nodes, abund=None, init=False, device=None):
    """cfr_quant_estep_probe: one E-step object (device=None: the host twin) runs the init round if asked and then one round per row of
    abund (rounds x n_nodes); returns every round's readCount, (init + rounds) x n_nodes float64"""
    a_begin = _u64(a_begin)
    a_target = np.ascontiguousarray(a_target, dtype=np.uint32)
    a_weight = np.ascontiguousarray(a_weight, dtype=np.float64)
    assert len(a_begin) == len(a_weight) + 1
    abund = np.zeros((0, n_nodes)) if abund is None else np.ascontiguousarray(abund, dtype=np.float64).reshape(-1, n_nodes)
    out = np.full(((1 if init else 0) + len(abund), n_nodes), -1.0, dtype=np.float64)
    _check(lib().cfr_quant_estep_probe(C.c_int32(-1 if device is None else device), _p(a_begin), _p(a_target), _p(a_weight), C.c_size_t(len(a_weight)),
                                       C.c_uint64(n_nodes), C.c_int32(1 if init else 0), _p(abund), C.c_size_t(len(abund)), _p(out)))
    return out


FORMAT_READ1, FORMAT_READ2, FORMAT_BARCODE, FORMAT_UMI = 0, 1, 2, 3


class TaxonomyTables(C.Structure):
    _fields_ = [("node_cnt", C.c_uint64), ("seq_cnt", C.c_uint64), ("extra_seq_cnt", C.c_uint64), ("root", C.c_uint64),
                ("n_seq_names", C.c_uint64), ("n_seq_lengths", C.c_uint64),
                ("parent", C.c_void_p), ("orig_taxid", C.c_void_p), ("seq_to_tax", C.c_void_p), ("rank", C.c_void_p),
                ("taxid_length", C.c_void_p), ("length_seq_id", C.c_void_p), ("length_value", C.c_void_p)]


def tax_rank_string(rank: int) -> str:
    return lib().cfr_tax_rank_string(C.c_uint8(rank)).decode()


class Taxonomy:
    """cfr_taxonomy: the taxonomy tables (and, with_lengths, the sequence and genome lengths) of an index prefix; never reads .1.cfr"""

    def __init__(self, prefix: str, with_lengths: bool = False):
        self._t = C.c_void_p()
        _check(lib().cfr_taxonomy_open(prefix.encode(), C.c_int(1 if with_lengths else 0), C.byref(self._t)))
        t = TaxonomyTables()
        _check(lib().cfr_taxonomy_get_tables(self._t, C.byref(t)))
        self.node_cnt, self.seq_cnt, self.extra_seq_cnt, self.root = t.node_cnt, t.seq_cnt, t.extra_seq_cnt, t.root

        def arr(ptr, n, ct, dt):
            if not ptr or n == 0:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n,)).copy()
        self.parent = arr(t.parent, t.node_cnt, C.c_uint64, np.uint64)
        self.orig_taxid = arr(t.orig_taxid, t.node_cnt, C.c_uint64, np.uint64)
        self.rank = arr(t.rank, t.node_cnt, C.c_uint8, np.uint8)
        self.seq_to_tax = arr(t.seq_to_tax, t.seq_cnt, C.c_uint64, np.uint64)
        self.taxid_length = arr(t.taxid_length, t.node_cnt + 1, C.c_uint64, np.uint64) if with_lengths else None
        self.length_seq_id = arr(t.length_seq_id, t.n_seq_lengths, C.c_uint64, np.uint64) if with_lengths else None
        self.length_value = arr(t.length_value, t.n_seq_lengths, C.c_uint64, np.uint64) if with_lengths else None
        self.seq_names = [lib().cfr_taxonomy_seq_name(self._t, C.c_uint64(i)).decode() for i in range(t.n_seq_names)]

    def tax_name(self, ctid: int) -> str:
        return lib().cfr_taxonomy_tax_name(self._t, C.c_uint64(ctid)).decode()

    def lca(self, lists, fold=False):
        """Taxonomy::LCA of every list of compact tax ids: the host tail's restatement, or (fold) the fold the kernels use -> (results,
        the fold's loop iterations per list)"""
        begin = np.zeros(len(lists) + 1, dtype=np.uint64)
        begin[1:] = np.cumsum([len(x) for x in lists])
        ids = _u64(np.array([t for x in lists for t in x], dtype=np.uint64))
        out = np.zeros(len(lists), dtype=np.uint64)
        steps = np.zeros(len(lists), dtype=np.uint32)
        _check(lib().cfr_taxonomy_lca_probe(self._t, _p(ids), _p(begin), C.c_size_t(len(lists)), C.c_int32(1 if fold else 0), _p(out), _p(steps)))
        return out, steps

    def close(self):
        if self._t:
            lib().cfr_taxonomy_close(self._t)
            self._t = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PromoteStats(C.Structure):
    _fields_ = [("table_ms", C.c_float), ("reads_ms", C.c_float)]


class Promote:
    """cfr_promote: centrifuger-promote on result arrays.  level: "lca" or a rank string.  device=None: the host twin, no GPU is touched."""

    def __init__(self, prefix: str, level: str, device=0):
        self._h = C.c_void_p()
        _check(lib().cfr_promote_open(prefix.encode(), level.encode(), C.c_int(-1 if device is None else device), C.byref(self._h)))

    def apply(self, results, matches, want_src=False):
        """in place on RESULT_DTYPE / MATCH_DTYPE arrays; returns src_slot (the slot every kept slot came from) when asked"""
        assert results.dtype == RESULT_DTYPE and matches.dtype == MATCH_DTYPE and results.flags.c_contiguous and matches.flags.c_contiguous
        src = np.full(len(matches), np.uint64(0xffffffffffffffff), dtype=np.uint64) if want_src else None
        _check(lib().cfr_promote_apply(self._h, _p(results), _p(matches), C.c_size_t(len(results)), _p(src)))
        return src

    def lca_warnings(self, results, matches):
        """tax ids of the script's "Couldn't find parent of taxID" lines for these (unpromoted) reads"""
        n = C.c_size_t(0)
        st = lib().cfr_promote_lca_warnings(self._h, _p(results), _p(matches), C.c_size_t(len(results)), None, C.c_size_t(0), C.byref(n))
        if st == CFR_OK:
            return np.zeros(0, dtype=np.uint64)
        if st != CFR_ERR_CAPACITY:
            _check(st)
        out = np.zeros(n.value, dtype=np.uint64)
        _check(lib().cfr_promote_lca_warnings(self._h, _p(results), _p(matches), C.c_size_t(len(results)), _p(out), C.c_size_t(len(out)), C.byref(n)))
        return out

    def stats(self) -> PromoteStats:
        st = PromoteStats()
        _check(lib().cfr_promote_get_stats(self._h, C.byref(st)))
        return st

    def close(self):
        if self._h:
            lib().cfr_promote_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KreportOptions(C.Structure):
    _fields_ = [("has_min_score", C.c_int32), ("has_min_length", C.c_int32), ("min_score", C.c_uint64), ("min_length", C.c_int64),
                ("no_lca", C.c_int32), ("show_zeros", C.c_int32), ("score_data", C.c_int32), ("max_blocks", C.c_uint32), ("lds_slots", C.c_uint32),
                ("threads", C.c_int32), ("pad", C.c_int32)]


class KreportStats(C.Structure):
    _fields_ = [("fold_ms", C.c_float), ("accumulate_ms", C.c_float), ("parse_ms", C.c_float)]


def kreport_options(min_score=None, min_length=None, no_lca=False, show_zeros=False, score_data=False, max_blocks=0, lds_slots=0, threads=0) -> KreportOptions:
    o = KreportOptions()
    lib().cfr_kreport_options_default(C.byref(o))
    if min_score is not None:
        o.has_min_score, o.min_score = 1, min_score
    if min_length is not None:
        o.has_min_length, o.min_length = 1, min_length
    o.no_lca, o.show_zeros, o.score_data, o.max_blocks, o.lds_slots, o.threads = int(no_lca), int(show_zeros), int(score_data), max_blocks, lds_slots, threads
    return o


class Kreport:
    """cfr_kreport: centrifuger-kreport, reads counted per taxon.  Options as kreport_options().  device=None: the host twin, no GPU is
    touched.  Bins: node_cnt + 1, the compact nodes and then "unclassified"."""

    def __init__(self, prefix: str, device=0, **options):
        self._h = C.c_void_p()
        o = kreport_options(**options)
        _check(lib().cfr_kreport_open(prefix.encode(), C.byref(o), C.c_int(-1 if device is None else device), C.byref(self._h)))
        n = C.c_size_t(0)
        _check(lib().cfr_kreport_bins(self._h, C.byref(n)))
        self.bins = n.value

    def add_results(self, results, matches):
        assert results.dtype == RESULT_DTYPE and matches.dtype == MATCH_DTYPE and results.flags.c_contiguous and matches.flags.c_contiguous
        _check(lib().cfr_kreport_add_results(self._h, _p(results), _p(matches), C.c_size_t(len(results))))

    def add_tsv(self, path: str):
        _check(lib().cfr_kreport_add_tsv(self._h, path.encode()))

    def add_count_table(self, path: str):
        _check(lib().cfr_kreport_add_count_table(self._h, path.encode()))

    def add_counts(self, own, own_score=None):
        own, own_score = _u64(own), _u64(own_score)
        _check(lib().cfr_kreport_add_counts(self._h, _p(own), _p(own_score), C.c_size_t(len(own))))

    def counts(self):
        """(own, clade, own_score, clade_score, seq_count)"""
        a = [np.zeros(self.bins, dtype=np.uint64) for _ in range(4)]
        seq = C.c_double(0)
        _check(lib().cfr_kreport_counts(self._h, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), C.c_size_t(self.bins), C.byref(seq)))
        return a[0], a[1], a[2], a[3], seq.value

    def warnings(self):
        """tax ids of the script's "Couldn't find parent of taxID" lines for everything added so far, in its order"""
        n = C.c_size_t(0)
        st = lib().cfr_kreport_warnings(self._h, None, C.c_size_t(0), C.byref(n))
        if st == CFR_OK:
            return np.zeros(0, dtype=np.uint64)
        if st != CFR_ERR_CAPACITY:
            _check(st)
        out = np.zeros(n.value, dtype=np.uint64)
        _check(lib().cfr_kreport_warnings(self._h, _p(out), C.c_size_t(len(out)), C.byref(n)))
        return out

    def write(self, path=None):
        _check(lib().cfr_kreport_write(self._h, None if path is None else path.encode()))

    def stats(self) -> KreportStats:
        st = KreportStats()
        _check(lib().cfr_kreport_get_stats(self._h, C.byref(st)))
        return st

    def close(self):
        if self._h:
            lib().cfr_kreport_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


READ_RECORD_DTYPE = np.dtype([("header", "<u8"), ("qual", "<u8"), ("header_len", "<u4"), ("id_len", "<u4")])


class TokenInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("consumed", C.c_uint64), ("total_bases", C.c_uint64), ("irregular_at", C.c_uint64),
                ("fastq", C.c_int32), ("irregular", C.c_int32), ("device_ms", C.c_double)]


class TokenStats(C.Structure):
    _fields_ = [("copy_in_ms", C.c_double), ("kernel_ms", C.c_double)]


class Tokenizer:
    """cfr_tokenizer: raw FASTA/FASTQ text -> records, 64-bit offsets, flat ASCII bases.  device=None: the host twin, no GPU is touched."""

    def __init__(self, device=None):
        self._h = C.c_void_p()
        self._last = TokenInfo()
        _check(lib().cfr_tokenizer_open(C.c_int(-1 if device is None else device), C.byref(self._h)))

    def tokenize(self, text, final=True, max_records=0) -> TokenInfo:
        """text: bytes or a uint8 array (kept alive by the caller for ids())"""
        a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else _u8(text)
        info = TokenInfo()
        _check(lib().cfr_tokenize(self._h, _p(a), C.c_uint64(len(a)), C.c_int(int(bool(final))), C.c_uint64(max_records), C.byref(info)))
        self._last = info
        return info

    def fetch(self):
        """-> (records READ_RECORD_DTYPE[n], offsets uint64[n + 1], bases uint8[total_bases]) of the last tokenize()"""
        info = self._last
        rec = np.zeros(info.n_records, dtype=READ_RECORD_DTYPE)
        off = np.zeros(info.n_records + 1, dtype=np.uint64)
        bases = np.zeros(info.total_bases, dtype=np.uint8)
        _check(lib().cfr_tokenizer_fetch(self._h, _p(rec), _p(off), _p(bases)))
        return rec, off, bases

    def stats(self) -> TokenStats:
        st = TokenStats()
        _check(lib().cfr_tokenizer_get_stats(self._h, C.byref(st)))
        return st

    def device_reads(self):
        """-> (d_bases, d_offsets) as ints, for DeviceIndex.classify_resident; valid until the next tokenize() / close()"""
        b, o = C.c_void_p(), C.c_void_p()
        _check(lib().cfr_tokenizer_device_reads(self._h, C.byref(b), C.byref(o)))
        return b.value or 0, o.value or 0

    def device_records(self):
        """-> (d_text, d_records) as ints, for DeviceIndex.tsv_last_resident; valid until the next tokenize() / close()"""
        t, r = C.c_void_p(), C.c_void_p()
        _check(lib().cfr_tokenizer_device_records(self._h, C.byref(t), C.byref(r)))
        return t.value or 0, r.value or 0

    def tokenize_resident(self, d_text: int, length: int, final=True, max_records=0) -> TokenInfo:
        """cfr_tokenize_resident: the text is `length` bytes at the device address d_text (Inflate.device_text(), or a range inside it)"""
        info = TokenInfo()
        _check(lib().cfr_tokenize_resident(self._h, C.c_void_p(d_text), C.c_uint64(length), C.c_int(int(bool(final))), C.c_uint64(max_records), C.byref(info)))
        self._last = info
        return info

    def fetch_ids(self, cap=None):
        """cfr_tokenizer_fetch_ids -> (ids uint8[total], id_off uint64[n + 1]) of the last call; cap: the bytes offered (default: asked for first)"""
        n = self._last.n_records
        off = np.zeros(n + 1, dtype=np.uint64)
        if cap is None:
            _check(lib().cfr_tokenizer_fetch_ids(self._h, None, C.c_uint64(0), _p(off)))
            cap = int(off[n])
        ids = np.zeros(max(cap, 1), dtype=np.uint8)
        _check(lib().cfr_tokenizer_fetch_ids(self._h, _p(ids), C.c_uint64(cap), _p(off)))
        return ids[:int(off[n])], off

    @staticmethod
    def ids(text, records):
        t = bytes(text)
        return [t[int(r["header"]) + 1:int(r["header"]) + 1 + int(r["id_len"])].decode("latin-1") for r in records]

    def close(self):
        if self._h:
            lib().cfr_tokenizer_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TsvOptions(C.Structure):
    _fields_ = [("tile_bytes", C.c_int32), ("max_blocks", C.c_int32), ("threads", C.c_int32), ("pad", C.c_int32)]


class TsvStats(C.Structure):
    _fields_ = [("upload_ms", C.c_float), ("len_ms", C.c_float), ("scan_ms", C.c_float), ("write_ms", C.c_float), ("download_ms", C.c_float),
                ("blocks", C.c_uint64), ("direct_blocks", C.c_uint64)]


def pack_ids(ids):
    """read ids (str or bytes) -> (uint8 bytes back to back, uint64 offsets[n + 1])"""
    raw = [i.encode("latin-1") if isinstance(i, str) else bytes(i) for i in ids]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    if raw:
        off[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
    return np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy(), off


class Tsv:
    """cfr_tsv: the rows of a batch as one text, the bytes of Index.format_tsv read after read.  device=None: the host twin."""

    def __init__(self, index: Index, device=None, tile_bytes=0, max_blocks=0, threads=0):
        self._h = C.c_void_p()
        self._index = index
        o = TsvOptions(tile_bytes, max_blocks, threads, 0)
        _check(lib().cfr_tsv_open(index._h, C.c_int(-1 if device is None else device), C.byref(o), C.byref(self._h)))

    def format_raw(self, results, matches, id_bytes, id_off, cap, n=None, n_slots=None, want_offsets=True):
        """one cfr_tsv_format call -> (status, len, text uint8[cap], row_offsets or None); raises nothing"""
        n = len(results) if n is None else n
        text = np.zeros(max(cap, 1), dtype=np.uint8)
        ln = C.c_uint64(0)
        off = np.zeros(n + 1, dtype=np.uint64) if want_offsets else None
        status = lib().cfr_tsv_format(self._h, _p(results), _p(matches), C.c_size_t(len(matches) if n_slots is None else n_slots), C.c_size_t(n),
                                      _p(id_bytes), _p(id_off), _p(text), C.c_uint64(cap), C.byref(ln), _p(off))
        return status, ln.value, text, off

    def format(self, results, matches, ids, cap=1 << 16):
        """-> (text bytes, row_offsets uint64[n + 1]); grows the buffer when the text needs more than cap"""
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        matches = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        id_bytes, id_off = pack_ids(ids)
        status, ln, text, off = self.format_raw(results, matches, id_bytes, id_off, cap)
        if status == CFR_ERR_CAPACITY and ln > cap:
            status, ln, text, off = self.format_raw(results, matches, id_bytes, id_off, ln)
        _check(status)
        return text[:ln].tobytes(), off

    def stats(self) -> TsvStats:
        st = TsvStats()
        _check(lib().cfr_tsv_get_stats(self._h, C.byref(st)))
        return st

    def close(self):
        if self._h:
            lib().cfr_tsv_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GZ_CODES = {"fixed": 0, "dynamic": 1}


class GzOptions(C.Structure):
    _fields_ = [("block_bytes", C.c_int32), ("max_blocks", C.c_int32), ("threads", C.c_int32), ("codes", C.c_int32)]


class GzStats(C.Structure):
    _fields_ = [("upload_ms", C.c_float), ("format_ms", C.c_float), ("deflate_ms", C.c_float), ("pack_ms", C.c_float), ("download_ms", C.c_float),
                ("dynamic_blocks", C.c_uint32), ("blocks", C.c_uint64), ("stored_blocks", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64)]


class GzFile(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("seq_off", C.c_void_p), ("qual", C.c_void_p), ("qual_off", C.c_void_p), ("has_qual", C.c_void_p)]


def gz_eof() -> bytes:
    """cfr_gz_eof: the BGZF end-of-file member"""
    p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    lib().cfr_gz_eof(C.byref(p), C.byref(n))
    return bytes(p[:n.value])


def pack_strings(strings):
    """byte strings -> (uint8 bytes back to back, uint64 offsets[n + 1])"""
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    if strings:
        off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer(b"".join(strings) or b"\0", dtype=np.uint8).copy(), off


class Gz:
    """cfr_gz: a text as BGZF members, and read dumps made and compressed in one call.  device=None: the host twin.
    codes: "fixed" (the fixed Huffman code, or stored) or "dynamic" (each block's own codes where they are smaller); an integer goes
    to cfr_gz_options.codes as it is."""

    def __init__(self, device=None, block_bytes=0, max_blocks=0, threads=0, codes="fixed"):
        self._h = C.c_void_p()
        if isinstance(codes, str):
            if codes not in GZ_CODES:
                raise ValueError("codes is 'fixed' or 'dynamic'")
            codes = GZ_CODES[codes]
        o = GzOptions(block_bytes, max_blocks, threads, codes)
        _check(lib().cfr_gz_open(C.c_int(-1 if device is None else device), C.byref(o), C.byref(self._h)))

    def compress(self, text) -> bytes:
        """the members of text (bytes or a uint8 array), without the end-of-file member"""
        a = np.frombuffer(bytes(text) or b"\0", dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, dtype=np.uint8)
        n = len(text)
        out, out_n = C.POINTER(C.c_uint8)(), C.c_uint64()
        _check(lib().cfr_gz_compress(self._h, _p(a), C.c_uint64(n), C.byref(out), C.byref(out_n)))
        return C.string_at(out, out_n.value) if out_n.value else b""

    def dump_arrays(self, id_bytes, id_off, select, files, copy=True):
        """cfr_gz_dump on flat arrays: files is a list of (seq uint8, seq_off uint64[n + 1], qual uint8 or None, qual_off, has_qual uint8[n])
        -> the members of every file (bytes; copy=False: their sizes only)"""
        n = len(id_off) - 1
        keep, arr = [_u8(id_bytes), _u64(id_off), _u8(select)], (GzFile * len(files))()
        for k, (seq, seq_off, qual, qual_off, has_qual) in enumerate(files):
            a = [_u8(seq), _u64(seq_off), _u8(qual), _u64(qual_off), _u8(has_qual)]
            keep += a
            arr[k].seq, arr[k].seq_off = a[0].ctypes.data, a[1].ctypes.data
            if qual is not None:
                arr[k].qual, arr[k].qual_off, arr[k].has_qual = a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data
        out, out_n = (C.POINTER(C.c_uint8) * len(files))(), (C.c_uint64 * len(files))()
        _check(lib().cfr_gz_dump(self._h, _p(keep[0]), _p(keep[1]), _p(keep[2]), C.c_size_t(n), arr, C.c_int(len(files)), out, out_n))
        if not copy:
            return [int(out_n[k]) for k in range(len(files))]
        return [C.string_at(out[k], out_n[k]) if out_n[k] else b"" for k in range(len(files))]

    def dump(self, ids, select, files):
        """ids: byte strings; select: n bytes; files: a list of (seqs, quals or None, has_qual or None), each a list of byte strings
        (quals) or n bytes (has_qual) -> the members of every file, as a list of bytes"""
        n = len(ids)
        id_bytes, id_off = pack_strings([i.encode("latin-1") if isinstance(i, str) else bytes(i) for i in ids])
        flat = []
        for seqs, quals, has_qual in files:
            sb, so = pack_strings(list(seqs))
            qb, qo = pack_strings(list(quals)) if quals is not None else (None, None)
            flat.append((sb, so, qb, qo, None if quals is None else (np.ascontiguousarray(has_qual, dtype=np.uint8) if n else np.zeros(1, dtype=np.uint8))))
        return self.dump_arrays(id_bytes, id_off, np.ascontiguousarray(select, dtype=np.uint8) if n else np.zeros(1, dtype=np.uint8), flat)

    def stats(self) -> GzStats:
        st = GzStats()
        _check(lib().cfr_gz_get_stats(self._h, C.byref(st)))
        return st

    def close(self):
        if self._h:
            lib().cfr_gz_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


INF_STATUS = {"ok": 0, "bad_header": 1, "bad_block_type": 2, "bad_stored_len": 3, "bad_code_set": 4, "bad_symbol": 5, "input": 6, "output_long": 7,
              "output_short": 8, "bad_crc": 9}


class InflateInfo(C.Structure):
    _fields_ = [("members", C.c_uint64), ("bad_members", C.c_uint64), ("first_bad", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64),
                ("first_bad_status", C.c_int32)]


class InflateStats(C.Structure):
    _fields_ = [("upload_ms", C.c_float), ("inflate_ms", C.c_float), ("download_ms", C.c_float)]


class Inflate:
    """cfr_inflate: BGZF members back into text, every member with a status.  device=None: the host twin."""

    def __init__(self, device=None):
        self._h = C.c_void_p()
        self._members = 0
        _check(lib().cfr_inflate_open(C.c_int(-1 if device is None else device), C.byref(self._h)))

    def inflate(self, members, fetch_text=True, copy=True):
        """members: bytes or a uint8 array of whole BGZF members -> (text bytes or None, InflateInfo); copy=False: (text size, info)"""
        a = np.frombuffer(bytes(members) or b"\0", dtype=np.uint8) if not isinstance(members, np.ndarray) else np.ascontiguousarray(members, dtype=np.uint8)
        text, text_n, info = C.POINTER(C.c_uint8)(), C.c_uint64(), InflateInfo()
        _check(lib().cfr_inflate_bgzf(self._h, _p(a), C.c_uint64(len(members)), C.c_int(int(bool(fetch_text))), C.byref(text), C.byref(text_n), C.byref(info)))
        self._members = info.members
        if not copy:
            return text_n.value, info
        if not fetch_text or not text:
            return (b"" if fetch_text else None), info
        return (C.string_at(text, text_n.value) if text_n.value else b""), info

    def member_status(self):
        """-> (status uint8[members], text_off uint64[members + 1]) of the last inflate()"""
        status = np.zeros(max(self._members, 1), dtype=np.uint8)
        off = np.zeros(self._members + 1, dtype=np.uint64)
        _check(lib().cfr_inflate_member_status(self._h, _p(status), _p(off), C.c_uint64(self._members)))
        return status[:self._members], off

    def device_text(self):
        """-> (device address, bytes) of the last call's text; valid until the next inflate() / close()"""
        d, n = C.c_void_p(), C.c_uint64()
        _check(lib().cfr_inflate_device_text(self._h, C.byref(d), C.byref(n)))
        return d.value or 0, n.value

    def stats(self) -> InflateStats:
        st = InflateStats()
        _check(lib().cfr_inflate_get_stats(self._h, C.byref(st)))
        return st

    def close(self):
        if self._h:
            lib().cfr_inflate_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReadFormat:
    """cfr_read_format: a --read-format string (ReadFormatter).  CfrError(CFR_ERR_FORMAT, "Format description error in ...") for a bad one."""

    def __init__(self, spec: str):
        self._f = C.c_void_p()
        _check(lib().cfr_read_format_parse(spec.encode(), C.byref(self._f)))

    def info(self, category: int):
        """(segment count, NeedExtract, IsInComment)"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().cfr_read_format_info(self._f, C.c_int(category), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, bool(b.value), bool(c.value)

    def extract(self, category: int, bases, offsets, qual=None, comments=None, comment_offsets=None, inplace=True):
        """cfr_read_format_extract -> (bases, offsets, qual or None)"""
        bases, offsets, qual, comments, comment_offsets = _u8(bases), _u64(offsets), _u8(qual), _u8(comments), _u64(comment_offsets)
        n = len(offsets if offsets is not None else comment_offsets) - 1
        out_off = np.zeros(n + 1, dtype=np.uint64)
        head = (self._f, C.c_int(category), C.c_int(int(inplace)), _p(bases), _p(offsets), _p(qual), _p(comments), _p(comment_offsets), C.c_size_t(n))
        _check(lib().cfr_read_format_extract(*head, None, _p(out_off), None))
        out = np.zeros(max(int(out_off[n]), 1), dtype=np.uint8)
        oq = np.zeros(len(out), dtype=np.uint8) if qual is not None and not self.info(category)[2] else None
        _check(lib().cfr_read_format_extract(*head, _p(out), _p(out_off), _p(oq)))
        total = int(out_off[n])
        return out[:total], out_off, (None if oq is None else oq[:total])

    def close(self):
        if self._f:
            lib().cfr_read_format_destroy(self._f)
            self._f = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BarcodeStats(C.Structure):
    _fields_ = [("whitelist_size", C.c_uint64), ("table_slots", C.c_uint64), ("host_barcodes", C.c_uint64), ("host_barcodes_total", C.c_uint64),
                ("device_ms", C.c_double), ("barcode_length", C.c_int32), ("on_device", C.c_int32)]


class Barcode:
    """cfr_barcode: a barcode whitelist (BarcodeCorrector).  device=None: the host twin only, no GPU is touched."""

    def __init__(self, whitelist_path: str, device=0):
        self._b = C.c_void_p()
        _check(lib().cfr_barcode_open(whitelist_path.encode(), C.c_int(-1 if device is None else device), C.byref(self._b)))

    def count(self, bases, offsets, max_records=2000000):
        bases, offsets = _u8(bases), _u64(offsets)
        _check(lib().cfr_barcode_count(self._b, _p(bases), _p(offsets), C.c_size_t(len(offsets) - 1), C.c_size_t(max_records)))

    def _correct(self, fn, bases, offsets, qual, threads):
        bases, offsets, qual = _u8(bases), _u64(offsets), _u8(qual)
        n = len(offsets) - 1
        status = np.zeros(n, dtype=np.int8)
        out = np.zeros(max(len(bases), 1), dtype=np.uint8)
        _check(fn(self._b, _p(bases), _p(offsets), _p(qual), C.c_size_t(n), C.c_int(threads), _p(status), _p(out)))
        return status, out[:len(bases)]

    def correct(self, bases, offsets, qual=None, threads=1):
        """cfr_barcode_correct (the handle's path) -> (status int8[n], bases after the call)"""
        return self._correct(lib().cfr_barcode_correct, bases, offsets, qual, threads)

    def correct_host(self, bases, offsets, qual=None, threads=1):
        """cfr_barcode_correct_host: always the host twin"""
        return self._correct(lib().cfr_barcode_correct_host, bases, offsets, qual, threads)

    def counts(self):
        """(entries as a list of bytes, counts uint32) in sorted order"""
        n, pb, po, pc = C.c_size_t(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
        _check(lib().cfr_barcode_counts(self._b, C.byref(n), C.byref(pb), C.byref(po), C.byref(pc)))
        n = n.value
        off = np.ctypeslib.as_array(po, shape=(n + 1,)).copy()
        total = int(off[n])
        flat = bytes(np.ctypeslib.as_array(pb, shape=(max(total, 1),))[:total]) if n else b""
        cnt = np.ctypeslib.as_array(pc, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint32)
        return [flat[int(off[i]):int(off[i + 1])] for i in range(n)], cnt

    def stats(self) -> BarcodeStats:
        st = BarcodeStats()
        _check(lib().cfr_barcode_get_stats(self._b, C.byref(st)))
        return st

    def close(self):
        if self._b:
            lib().cfr_barcode_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BarcodeTranslate:
    """cfr_barcode_translate: a --barcode-translate table (BarcodeTranslator)."""

    def __init__(self, path: str):
        self._t = C.c_void_p()
        _check(lib().cfr_barcode_translate_open(path.encode(), C.byref(self._t)))

    def apply(self, bases, offsets, status=None):
        """-> (bases, offsets); CfrError with the reference's message for a piece that is not in the table"""
        bases, offsets = _u8(bases), _u64(offsets)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int8)
        n = len(offsets) - 1
        out_off = np.zeros(n + 1, dtype=np.uint64)
        _check(lib().cfr_barcode_translate_apply(self._t, _p(bases), _p(offsets), _p(status), C.c_size_t(n), None, _p(out_off)))
        out = np.zeros(max(int(out_off[n]), 1), dtype=np.uint8)
        _check(lib().cfr_barcode_translate_apply(self._t, _p(bases), _p(offsets), _p(status), C.c_size_t(n), _p(out), _p(out_off)))
        return out[:int(out_off[n])], out_off

    def close(self):
        if self._t:
            lib().cfr_barcode_translate_destroy(self._t)
            self._t = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
