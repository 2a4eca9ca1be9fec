"""zng_rocm_gzip_headers_dev: the gzip header fields of the members of a device-resident file (inflateGetHeader), through the C
ABI.  Oracles: what was set when the file was written (gzip_header_batch.py), zng_rocm_gzip_header_parse on the same bytes in
host memory (itself held to zng_rocm_wrapper_parse and to CPython by tests/test_gzip_header_plan_cpu.py), and members made here
with struct, zlib.crc32 and CPython's deflate whose fields begin and end around the 16-byte lines and the 4096-byte steps of
the wavefront's zero search."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gzip_files
import gzip_header_batch as gb
import gzip_header_cases as cases

pytestmark = pytest.mark.gpu
EINVAL, BUF_ERROR = -3, -5
PLAIN = b"what the member holds does not matter here\n" * 3


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.deflate"), importlib.import_module("zlib-ng_amd.inflate"), zr


def to_dev(torch, data, shift=0):
    """the bytes on the device, `shift` bytes behind a 16-byte line, with 0xAB around them"""
    arena = torch.from_numpy(np.frombuffer(b"\xab" * (16 + shift) + data + b"\xab" * 64, dtype=np.uint8).copy()).cuda()
    assert arena.data_ptr() % 16 == 0
    return arena[16 + shift:16 + shift + len(data)]


def table(spans):
    return [(off, n, 0, 0, 0, 0) for off, n in spans]


def check_rows(inf, data, spans, rows, text, kws=None):
    """every row against zng_rocm_gzip_header_parse on the member's bytes (offsets moved to the file's), text_off as the running
    sum over the accepted members, the text's bytes, and -- where given -- the fields that were set"""
    at = 0
    for k, ((off, n), row) in enumerate(zip(spans, rows)):
        member = data[off:off + n]
        st, want = inf.gzip_header_parse(member)
        for key in ("extra_off", "name_off", "comment_off"):
            if want[key]:
                want[key] += off
        want["text_off"] = at
        assert row == want, (k, off, n)
        if st != 0:
            continue
        for key in ("extra", "name", "comment"):
            o, ln = row[key + "_off"], row[key + "_len"]
            if kws is not None:
                v = kws[k].get(key)
                assert (o != 0) == (v is not None) and (v is None or data[o:o + ln] == v), (k, key)
            if o:
                assert text[at:at + ln] == data[o:o + ln], (k, key)
                at += ln
                if key != "extra":
                    assert text[at] == 0
                    at += 1
        if kws is not None:
            kw = kws[k]
            assert (row["time"], row["os"], row["text"], row["hcrc"]) == (kw.get("time", 0), kw.get("os", 3) & 0xff,
                                                                         int(kw.get("text", False)), int(kw.get("hcrc", False)))
    assert at == len(text)


def test_rows_of_the_written_file_are_what_was_set(mods):
    torch, _, inf, _ = mods
    b = gb.batch(mods)
    f, _ = gb.written(mods, 9, 0, 15)
    spans = [(f.off[i], f.off[i + 1] - f.off[i]) for i in range(b.n)]
    st, rows, text, need = inf.gzip_headers_dev(f.dev[:len(f.data)], table(spans))
    assert st == 0 and need == len(text) == sum(len(kw.get(k, b"")) + (k != "extra" and k in kw) for kw in b.kws for k in
                                                 ("extra", "name", "comment"))
    check_rows(inf, f.data, spans, rows, text, b.kws)
    assert [r["xflags"] for r in rows] == [2] * b.n and [r["header_len"] for r in rows][32:] == list(gb.EDGE_HEADS) + [196621]


def test_text_cap_at_need_below_it_and_zero(mods):
    torch, _, inf, zr = mods
    lib = zr.rocm.lib()
    b = gb.batch(mods)
    f, _ = gb.written(mods)
    spans = [(f.off[i], f.off[i + 1] - f.off[i]) for i in range(b.n)]
    members = inf.member_table(table(spans))
    _, want_rows, want_text, need = inf.gzip_headers_dev(f.dev[:len(f.data)], members)
    for cap in (need, need - 1, 0, need + 5):
        rows = (inf.GzipHeaderRow * b.n)()
        text = (C.c_uint8 * (need + 8))(*([0xa5] * (need + 8)))
        got = C.c_size_t(123)
        st = lib.zng_rocm_gzip_headers_dev(f.dev.data_ptr(), len(f.data), C.cast(members, C.c_void_p), b.n, C.cast(rows, C.c_void_p),
                                           C.cast(text, C.c_void_p) if cap else None, cap, C.byref(got), None)
        assert st == (0 if cap >= need else BUF_ERROR) and got.value == need
        assert [rows[k].as_dict() for k in range(b.n)] == want_rows            # the rows are delivered either way
        if cap >= need:
            assert bytes(text)[:need] == want_text and bytes(text)[need:] == b"\xa5" * 8
        else:
            assert bytes(text) == b"\xa5" * (need + 8)                         # untouched


def edge_members():
    """members whose name and comment begin and end around 16-byte lines and around the 4096-byte step of the zero search, at
    every file offset modulo 16; some with an extra field in front, some with FHCRC"""
    lens = (0, 1, 2, 14, 15, 16, 17, 31, 32, 33, 4079, 4080, 4081, 4095, 4096, 4097, 8191, 8192, 8193)
    pat = bytes(range(1, 256)) * 40
    out = []
    for k, n in enumerate(lens):
        for which in range(3):
            kw = {"time": k * 3 + which, "hcrc": bool((k + which) & 1)}
            if which != 1:
                kw["name"] = pat[k:k + n]
            if which != 0:
                kw["comment"] = pat[2 * k:2 * k + lens[(k + 5) % len(lens)]] if which == 2 else pat[k:k + n]
            if k % 4 == 1:
                kw["extra"] = bytes(range(k)) + b"\0\0"
            out.append(kw)
    return out


def test_fields_around_the_lines_and_steps_of_the_zero_search_at_odd_offsets(mods):
    torch, _, inf, _ = mods
    kws = edge_members()
    data, spans = bytearray(), []
    for k, kw in enumerate(kws):
        data += b"\x1f\x8b\x00" * (k % 3)                                               # garbage between the members
        data += b"\xee" * ((k * 7 + 1 - len(data)) % 16)
        member = cases.gzip_member(cases.model_header(6, 0, **kw), PLAIN)
        spans.append((len(data), len(member)))
        data += member
    assert sorted({off % 16 for off, _ in spans}) == list(range(16))
    data = bytes(data)
    for shift in (0, 9):
        src = to_dev(torch, data, shift)
        st, rows, text, need = inf.gzip_headers_dev(src, table(spans))
        assert st == 0 and need == len(text)
        check_rows(inf, data, spans, rows, text, kws)


def test_a_header_above_4_kib_that_gunzip_members_still_decodes(mods):
    torch, _, inf, _ = mods
    kw = {"name": b"n" * 5000, "comment": b"c" * 3000, "extra": bytes(2000), "hcrc": True, "time": 77}
    data = cases.gzip_member(cases.model_header(6, 0, **kw), PLAIN) + cases.gzip_member(cases.model_header(6, 0, name=b"b"), PLAIN * 2)
    src = to_dev(torch, data, 3)
    dst = torch.zeros(3 * len(PLAIN) + 64, dtype=torch.uint8, device="cuda")
    st, out_len, in_used, members, nmembers, _ = inf.gunzip_members_dev(src, dst[:3 * len(PLAIN)])
    assert (st, out_len, in_used, nmembers) == (1, 3 * len(PLAIN), len(data), 2)
    spans = [(m[0], m[1]) for m in members]
    st, rows, text, need = inf.gzip_headers_dev(src, members)
    assert st == 0 and rows[0]["header_len"] == 10 + 2 + 2000 + 5001 + 3001 + 2 > 4096
    check_rows(inf, data, spans, rows, text, [kw, {"name": b"b"}])
    assert text == bytes(2000) + b"n" * 5000 + b"\0" + b"c" * 3000 + b"\0" + b"b\0"


def test_cut_refused_and_bad_fhcrc_members_between_good_ones(mods):
    torch, _, inf, _ = mods
    good = [cases.gzip_member(cases.model_header(6, 0, **cases.fields(flg, 1, flg)), PLAIN) for flg in (31, 8, 30, 16, 12, 27)]
    bad_crc = bytearray(good[2])
    bad_crc[len(cases.model_header(6, 0, **cases.fields(30, 1, 30))) - 2] ^= 0x81
    reserved = bytearray(good[1])
    reserved[3] |= 0x40
    method = bytearray(good[3])
    method[2] = 9
    parts = [good[0], bytes(bad_crc), good[1], bytes(reserved), good[4], bytes(method), good[5], good[3]]
    data, spans = b"", []
    for p in parts:
        spans.append((len(data) + 1, len(p)))
        data += b"\x00" + p
    # cut members: the table says they end inside the extra field, the name, the comment, the FHCRC, the fixed ten bytes
    head0 = len(cases.model_header(6, 0, **cases.fields(31, 1, 31)))
    cuts = [(spans[0][0], n) for n in (0, 1, 3, 9, 11, 14, 25, head0 - 3, head0 - 1)]
    spans = spans[:4] + cuts[:5] + spans[4:6] + cuts[5:] + spans[6:]
    src = to_dev(torch, data, 5)
    st, rows, text, need = inf.gzip_headers_dev(src, table(spans))
    assert st == 0
    check_rows(inf, data, spans, rows, text)
    assert [(r["status"], r["msg"]) for r in rows] == [
        (0, None), (-3, "header crc mismatch"), (0, None), (-3, "unknown header flags set")] + [(-5, None)] * 5 + [
        (0, None), (-3, "unknown compression method")] + [(-5, None)] * 4 + [(0, None), (0, None)]
    # the neighbours' rows and places are those of a table of the good members alone
    keep = [k for k, r in enumerate(rows) if r["status"] == 0]
    st, alone, text_alone, _ = inf.gzip_headers_dev(src, table([spans[k] for k in keep]))
    assert st == 0 and alone == [rows[k] for k in keep] and text_alone == text


def test_refusals_launch_nothing_and_write_nothing(mods):
    torch, _, inf, zr = mods
    lib = zr.rocm.lib()
    data = cases.gzip_member(cases.model_header(6, 0, name=b"a"), PLAIN)
    src = to_dev(torch, data)
    for spans in ([(0, len(data) + 1)], [(0, len(data)), (len(data) + 1, 0)], [(1 << 63, 1 << 63)]):
        members = inf.member_table(table(spans))
        rows = (C.c_uint8 * (96 * len(spans)))(*([0xa5] * 96 * len(spans)))
        text = (C.c_uint8 * 16)(*([0xa5] * 16))
        need = C.c_size_t(99)
        st = lib.zng_rocm_gzip_headers_dev(src.data_ptr(), len(data), C.cast(members, C.c_void_p), len(spans), C.cast(rows, C.c_void_p),
                                           C.cast(text, C.c_void_p), 16, C.byref(need), None)
        assert st == EINVAL and need.value == 0 and bytes(rows) == b"\xa5" * len(rows) and bytes(text) == b"\xa5" * 16
    st, rows, text, need = inf.gzip_headers_dev(src, [])
    assert (st, rows, text, need) == (0, [], b"", 0)
    st, rows, text, need = inf.gzip_headers_dev(src, table([(0, len(data)), (len(data), 0)]))      # an empty member at the end: cut
    assert st == 0 and [r["status"] for r in rows] == [0, -5] and text == b"a\0"


def test_bgzf_members_table_reports_the_bc_subfield(mods):
    torch, _, inf, _ = mods
    plain = bytes(range(256)) * 12
    data = gzip_files.bgzf_file(plain, block=1000)
    src = to_dev(torch, data, 7)
    st, members, nmembers, plain_len, in_used = inf.bgzf_index_dev(src)
    assert st == 0 and nmembers == len(members) == 4 + 1 and plain_len == len(plain) and in_used == len(data)
    st, rows, text, need = inf.gzip_headers_dev(src, members)
    assert st == 0 and need == 6 * nmembers
    for k, (m, row) in enumerate(zip(members, rows)):
        assert (row["status"], row["extra_len"], row["extra_off"], row["flg"], row["text_off"]) == (0, 6, m[0] + 12, 4, 6 * k)
        assert text[6 * k:6 * k + 6] == b"BC\x02\x00" + (m[1] - 1).to_bytes(2, "little")
