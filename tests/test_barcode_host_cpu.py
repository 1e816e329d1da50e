"""Single-cell input on the host: the twins of ReadFormatter, BarcodeCorrector and BarcodeTranslator (csrc/cfr_barcode.cpp) against
what the reference's own headers did with the cases of tests/golden/barcode, byte for byte.  No GPU."""
import numpy as np
import pytest

import barcode_fixtures as bf
from centrifuger_amd import capi

WHITELISTS = ["wl5", "wl16", "wlmix"]


def test_fixture_holds_every_class_and_every_return_value():
    m = bf.manifest()
    assert all(m["returns"][k] >= 100 for k in ("-1", "0", "1"))
    for c in ("exact", "sub_first", "sub_last", "one_n", "two_n", "n_plus_sub", "cand2_lower", "cand2_equal", "cand2_higher", "cand3_lower",
              "cand3_equal", "cand3_higher", "prefix", "empty", "longer"):
        assert m["classes"][c] >= 20, c
    assert sum(w["quality_changes_the_choice"] for w in m["whitelists"].values()) >= 20


@pytest.mark.parametrize("name", WHITELISTS)
def test_background_counts_equal_reference(name):
    w = bf.manifest()["whitelists"][name]
    bc = capi.Barcode(bf.whitelist_path(name), device=None)
    b, o = bf.background(name)
    assert len(o) - 1 == w["n_background"] > w["background_cap"]
    bc.count(b, o, max_records=w["background_cap"])
    entries, cnt = bc.counts()
    want_e, want_c = bf.counts(name)
    assert entries == want_e and cnt.tolist() == want_c
    st = bc.stats()
    assert st.whitelist_size == w["n_entries"] == len(want_e) and st.on_device == 0 and st.table_slots == 0
    assert st.barcode_length == {"wl5": 5, "wl16": 16, "wlmix": 0}[name]


@pytest.mark.parametrize("name", WHITELISTS)
@pytest.mark.parametrize("threads", [1, 3])
def test_correct_equals_reference_with_and_without_qualities(name, threads):
    w = bf.manifest()["whitelists"][name]
    bc = capi.Barcode(bf.whitelist_path(name), device=None)
    bc.count(*bf.background(name), max_records=w["background_cap"])
    _, b, o, q = bf.barcodes(name)
    sq, bq, sn, bn = bf.corrected(name)
    st, out = bc.correct(b, o, q, threads=threads)
    assert st.tolist() == sq and bf.unflat(out, o) == bq
    st, out = bc.correct_host(b, o, None, threads=threads)
    assert st.tolist() == sn and bf.unflat(out, o) == bn
    assert bc.stats().host_barcodes == len(sq)


def test_two_count_calls_add_up_and_a_cap_of_zero_counts_nothing():
    name = "wl16"
    cap = bf.manifest()["whitelists"][name]["background_cap"]
    b, o = bf.background(name)
    bc = capi.Barcode(bf.whitelist_path(name), device=None)
    bc.count(b, o, max_records=0)
    assert sum(bc.counts()[1]) == sum(capi.Barcode(bf.whitelist_path(name), device=None).counts()[1])
    half = cap // 2
    bc.count(b, o[:half + 1], max_records=cap)
    bc.count(b, o[half:], max_records=cap - half)
    assert bc.counts()[1].tolist() == bf.counts(name)[1]


def test_a_barcode_of_256_bytes_is_refused():
    bc = capi.Barcode(bf.whitelist_path("wl5"), device=None)
    b, o = bf.flat([b"ACGTA", b"A" * 256])
    with pytest.raises(capi.CfrError) as e:
        bc.correct(b, o)
    assert e.value.status == capi.CFR_ERR_ARG and "256" in str(e.value)
    st, _ = bc.correct(*bf.flat([b"ACGTA", b"A" * 255]))
    assert st.tolist() == [0, -1]


def test_bytes_outside_acgt_are_not_found():
    bc = capi.Barcode(bf.whitelist_path("wl5"), device=None)
    st, out = bc.correct(*bf.flat([b"acgta", b"ACGT\xff", b"ACG\x00A", b"ACGTa"]))
    assert st.tolist() == [-1, 1, 1, 1] and bf.unflat(out, np.arange(0, 21, 5))[1] == b"ACGTA"


@pytest.mark.parametrize("k", range(len(bf.formats())))
def test_read_format_equals_reference(k):
    entry = bf.formats()[k]
    recs = bf.format_records()
    use = entry["records"] if entry["records"] is not None else list(range(len(recs)))
    recs = [recs[i] for i in use]
    f = capi.ReadFormat(entry["spec"])
    b, o = bf.flat([r[0] for r in recs])
    q = bf.flat([r[1] for r in recs])[0]
    cm, co = bf.flat([r[2] for r in recs])
    rows = bf.format_dump(entry)
    cats = [c for c in range(4) if f.info(c)[0] > 0]
    assert len(rows) == len(recs) * len(cats)
    for ci, cat in enumerate(cats):
        want = rows[ci::len(cats)]
        assert all(int(r[0]) == cat for r in want)
        if f.info(cat)[2]:
            gb, go, gq = f.extract(cat, None, None, None, cm, co)
            assert bf.unflat(gb, go) == [r[1] for r in want] and gq is None
            continue
        gb, go, gq = f.extract(cat, b, o, q, inplace=False)
        assert bf.unflat(gb, go) == [r[1] for r in want] and bf.unflat(gq, go) == [r[2] for r in want]
        gb, go, gq = f.extract(cat, b, o, q, inplace=True)
        assert bf.unflat(gb, go) == [r[3] for r in want] and bf.unflat(gq, go) == [r[4] for r in want]
        gb2, go2, gq2 = f.extract(cat, b, o, None, inplace=True)
        assert np.array_equal(gb, gb2) and np.array_equal(go, go2) and gq2 is None


def test_read_format_info():
    f = capi.ReadFormat("r1:0:-1,bc:0:15;um:hd:UB:5:-1")
    assert f.info(capi.FORMAT_READ1) == (1, False, False) and f.info(capi.FORMAT_READ2) == (0, False, False)
    assert f.info(capi.FORMAT_BARCODE) == (1, True, False) and f.info(capi.FORMAT_UMI) == (1, True, True)


def test_bad_format_strings_are_refused_with_the_reference_message():
    for spec, msg in bf.manifest()["bad_formats"].items():
        with pytest.raises(capi.CfrError) as e:
            capi.ReadFormat(spec)
        assert e.value.status == capi.CFR_ERR_FORMAT and str(e.value).endswith(msg.strip()), spec


def test_translate_equals_reference(tmp_path):
    import os
    t = capi.BarcodeTranslate(os.path.join(bf.BARCODE, "translate.txt"))
    rows = bf.translations()
    b, o = bf.flat([r[0] for r in rows])
    gb, go = t.apply(b, o)
    assert bf.unflat(gb, go) == [r[1] for r in rows]
    assert any(b"-" in r[1] for r in rows) and any(r[1] == b"" for r in rows) and rows[-1][1] == b"again"
    # a barcode whose correction failed becomes "N" and is not looked up (CentrifugerClass.cpp:189-205)
    status = np.zeros(len(rows), dtype=np.int8)
    status[::7] = -1
    gb, go = t.apply(b, o, status)
    assert bf.unflat(gb, go) == [b"N" if status[i] == -1 else r[1] for i, r in enumerate(rows)]
    m = bf.manifest()["translate"]
    with pytest.raises(capi.CfrError) as e:
        t.apply(*bf.flat([rows[1][0], m["missing_barcode"].encode()]))
    assert m["returncode"] == 255 and str(e.value).endswith(m["stderr"].strip())
    bad = tmp_path / "bad.txt"
    bad.write_text("cell1,ACGT\nno_separator\n")
    with pytest.raises(capi.CfrError):
        capi.BarcodeTranslate(str(bad))


def test_tsv_ex_without_columns_equals_the_plain_entries(golden_dir):
    idx = capi.Index(golden_dir + "/f6")
    res = np.zeros(2, dtype=capi.RESULT_DTYPE)
    mat = np.zeros(2, dtype=capi.MATCH_DTYPE)
    res[0]["query_length"] = 77
    res[1]["query_length"] = 150; res[1]["n_match"] = 2; res[1]["score"] = 900; res[1]["hit_length"] = 60; res[1]["match_begin"] = 0
    mat[0]["taxid"] = 11; mat[1]["taxid"] = 12; mat[1]["id"] = 1
    assert capi.tsv_header_ex() == capi.tsv_header()
    assert capi.tsv_header_ex(True, True, True) == capi.tsv_header()[:-1] + b"\tbarcode\tUMI\texpandedTaxIDs\n"
    assert capi.tsv_header_ex(False, True, False) == capi.tsv_header()[:-1] + b"\tUMI\n"
    for i in range(2):
        plain = idx.format_tsv("read", res[i], mat)
        assert idx.format_tsv_ex("read", res[i], mat) == plain
        rows = plain.split(b"\n")[:-1]
        assert idx.format_tsv_ex("read", res[i], mat, True, b"ACGT", True, b"TT") == b"".join(r + b"\tACGT\tTT\n" for r in rows)
        assert idx.format_tsv_ex("read", res[i], mat, True, None, False, b"TT") == b"".join(r + b"\t\n" for r in rows)   # PrintExtraCol(NULL)
        assert idx.format_tsv_ex("read", res[i], mat, False, None, True, b"GG", True) == b"".join(r + b"\tGG\t\n" for r in rows)
