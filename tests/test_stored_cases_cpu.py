"""The crafted stored blocks (tests/stored_cases.py) without a GPU: first the cases themselves against three readers that are
no part of the product -- CPython's zlib, the oracle (oracle/inflate_oracle.c) and the block parser of tests/deflate_parse.py --
and that every family stands on the edges it was built for; then the product's host token decoder (inflate_host.cpp:328-364)
against the oracle: status, message and the token replay on every valid case, every bad NLEN and every cut."""
import importlib
import zlib

import pytest

import deflate_parse
import inflate_util
import stored_cases as sc
from test_inflate_dynamic_cpu import _replay

STARVED = "input ended before the final block"
BAD_LEN = "invalid stored block lengths"


def _inf():
    importlib.import_module("zlib-ng_amd")
    return importlib.import_module("zlib-ng_amd.inflate")


def _oracle(stream, history, cap):
    return inflate_util.oracle_inflate_dict(stream, history, cap) if history else inflate_util.oracle_inflate(stream, cap)


@pytest.mark.parametrize("family", sc.VALID)
def test_valid_cases_are_what_zlib_the_oracle_and_the_parser_read(family):
    for c in sc.cases(family):
        z = zlib.decompressobj(-15, zdict=c.history) if c.history else zlib.decompressobj(-15)
        assert z.decompress(c.stream) == c.plain and z.eof and not z.unused_data, c.name
        got = _oracle(c.stream, c.history, len(c.plain))
        assert got == (1, "", c.plain, len(c.stream)), (c.name, got[:2], got[3])
        p = deflate_parse.parse(c.stream, c.history)
        found = [b for b in p.blocks if b.btype == deflate_parse.STORED]
        assert p.data == c.plain and len(found) == len(c.stored) >= 1, c.name
        for b, s in zip(found, c.stored):
            assert (b.start, b.start >> 3, b.header_end >> 3, b.out_start, b.nbytes) == (s.start_bit, s.hdr_byte, s.in_at, s.out_at, s.length), c.name
            assert c.stream[s.in_at:s.in_at + s.length] == c.plain[s.out_at:s.out_at + s.length]


def test_large_streams_are_what_zlib_reads():
    for args in ((True,), (False,), (True, 0, False), (True, 40)):
        big = sc.large_stream(*args)
        z = zlib.decompressobj(-15, zdict=big.history) if big.history else zlib.decompressobj(-15)
        assert z.decompress(big.comp) == big.plain and z.eof and not z.unused_data
        status, blocks = inflate_util.oracle_block_starts(big.comp, len(big.plain)) if not big.history else (1, None)
        assert status == 1 and (blocks is None or len(blocks) == big.blocks)
        if len(args) < 2 or not args[1]:
            assert len(big.comp) >= (128 << 10) and big.groups >= len(sc.LENS)
            assert {s.length for s in big.stored} == set(sc.LENS) and {s.start_bit % 8 for s in big.stored} == set(range(8))


def test_every_family_reaches_its_edge():
    ln = sc.cases("len")
    assert {(c.meta["L"], c.meta["P"], c.meta["final"]) for c in ln} == {(L, P, f) for L in sc.LENS for P in sc.FRONT for f in (True, False)}
    assert {64, 65} <= {c.stored[0].out_at for c in ln}      # P = 64 and P = 65: the stored bytes begin there
    bit = sc.cases("bit")
    assert {c.stored[0].start_bit % 8 for c in bit} == set(range(8))
    assert {(c.stored[0].start_bit % 8, c.meta["pad"], c.meta["L"]) for c in bit} == {(o, p, L) for o in range(8) for p in sc.PADS for L in sc.BIT_LENS}
    seen = set()
    for c in bit + ln + sc.cases("after") + sc.cases("window"):
        for s in c.stored:
            first = (s.start_bit + 3) % 8                     # the pad: from the bit behind BTYPE to the end of that byte
            if first:
                pad = c.stream[(s.start_bit + 3) >> 3] >> first
                seen.add((s.pad, pad == 0, pad == (0xff >> first)))
                assert pad == {"zeros": 0, "ones": 0xff, "alt": 0x55}[s.pad] & (0xff >> first), c.name
    assert {p for p, _, _ in seen} == set(sc.PADS) and ("ones", False, True) in seen and ("alt", False, False) in seen
    win = sc.cases("window")
    at = set()
    for c in win:
        s = c.stored[-1]
        seek = c.stored[0].in_at + c.stored[0].length if len(c.stored) == 2 else 0       # the end of the stored block in front
        assert (len(c.stored) == 2) == (c.meta["base"] == "stored7") and (len(c.stored) == 1 or c.stored[0].length == 7)
        assert all(t < 144 for t in c.plain[(7 if seek else 0):s.out_at])                 # placed with 8-bit literals
        at.add((c.meta["base"], s.in_at - 4 - seek))
    assert at == {(b, a) for b in ("start", "stored7") for a in sc.WINDOW_AT}
    have = set()
    for c in sc.cases("after"):
        last = deflate_parse.parse(c.stream, c.history).blocks[-1]
        assert last.final and [m[1:3] for m in last.matches] == [tuple(x) for x in c.meta["copies"]], c.name
        assert c.stored[0].out_at == c.meta["Q"] and c.stored[0].length == c.meta["L"]
        if c.meta["form"] == 1:
            have.add((c.meta["Q"], c.meta["L"]) + last.matches[0][1:3])
        elif c.meta["form"] == 2:
            assert last.matches[0][2] >= 3839 and last.matches[1][2] < 3838
        else:
            assert len(c.history) == 300 and last.matches[0][2] - c.meta["Q"] - c.meta["L"] in (1, 300)
    want = {(Q, L, n, D) for Q in sc.AFTER_FRONT for L in sc.AFTER_LENS for n in (3, 258) for D in sc.after_distances(L, Q)}
    assert have == want and {3837, 3838, 3839, 3840, 4095, 4096, 4097, 32768} <= {w[3] for w in want}
    assert {f for f in (c.meta["form"] for c in sc.cases("after"))} == {1, 2, 3}
    chains = {c.name: c for c in sc.cases("chain")}
    assert [s.length for s in chains["chain/empty"].stored] == [0] and [s.length for s in chains["chain/empty-last"].stored] == [5, 0]
    assert [s.length for s in chains["chain/walk"].stored] == list(sc.LENS) and len(chains["chain/zeros"].stored) == 301
    total = sc.totals()
    assert sum(n for f, (n, _) in total.items() if f != "room") < 3000 and sum(b for _, b in total.values()) < (24 << 20), total


def test_bad_nlen_is_refused_alike_by_zlib_and_the_oracle():
    cases = sc.cases("nlen")
    seen = set()
    for c in cases:
        assert len(c.plain) == 40
        assert inflate_util.oracle_inflate(c.stream, 4096)[:3] == (-3, BAD_LEN, c.plain), c.name
        with pytest.raises(zlib.error, match=BAD_LEN):
            zlib.decompressobj(-15).decompress(c.stream)
        seen.add((c.meta["off"], c.meta["L"], c.meta["len"] ^ c.meta["nlen"] ^ 0xffff))
    for off in (0, 3):
        assert {c.stored[0].start_bit % 8 for c in cases if c.meta["off"] == off} == {off}
        for L in (0, 5):
            assert {(off, L, 1 << k) for k in range(16)} <= seen and (off, L, 0xffff) in seen
    assert {(c.meta["len"], c.meta["nlen"]) for c in cases} >= {(0, 0), (0xffff, 0xffff), (5, 5)}


def test_every_cut_has_an_exact_answer():
    cuts = sc.cases("cuts")
    sources = {c.name: c for f in ("bit", "len", "chain") for c in sc.cases(f)}
    for c in cuts:
        src = sources[c.meta["of"]]
        cut = c.meta["cut"]
        assert src.stored[0].hdr_byte < cut < len(src.stream) and c.stream == src.stream[:cut]
        got = inflate_util.oracle_inflate(c.stream, c.meta["cap"])
        assert got[:3] == (-5, STARVED, c.plain), (c.name, got[:2], len(got[2]), len(c.plain))    # none is left undecided
        assert src.plain.startswith(c.plain) and len(c.plain) >= src.stored[0].out_at
        # room for exactly the bytes that are there: still the input that ended, not the room
        assert inflate_util.oracle_inflate(c.stream, len(c.plain))[:3] == (-5, STARVED, c.plain), c.name
    used = {c.meta["of"] for c in cuts}
    assert used == {c.name for c in sc.cases("bit")} | {c.name for c in sc.cases("len") if c.meta["L"] in sc.CUT_LENS} | \
        {"chain/" + n for n in sc.SHORT_CHAINS}
    # every cut there is for a short payload; of a long one the listed ones
    for name in ("bit/3/ones/17", "len/17/64/final", "chain/0005"):
        s = sources[name]
        assert {c.meta["cut"] for c in cuts if c.meta["of"] == name} == set(range(s.stored[0].hdr_byte + 1, len(s.stream)))
    s = sources["len/3073/65/more"]
    inside = {c.meta["cut"] - s.stored[0].in_at for c in cuts if c.meta["of"] == s.name and c.meta["cut"] > s.stored[0].in_at}
    assert inside == set(sc.PAYLOAD_CUTS) | {3072, 3073}     # (3073: the payload whole, the block behind it missing)


def test_room_runs_by_the_oracle():
    runs = sc.room_runs()
    for r in runs:
        c = r.case
        st, msg, out, used = _oracle(c.stream, c.history, r.cap)
        if r.exact:
            assert (st, msg, out, used) == (1, "", c.plain, len(c.stream)), (c.name, r.cap, st, msg)
        else:
            assert r.cap < len(c.plain) and (st, msg) == (-5, "output buffer full") and c.plain.startswith(out), (c.name, r.cap, st, msg)
    ln = [r for r in runs if r.kind == "len"]
    for c in sc.cases("len"):
        L, P = c.meta["L"], c.meta["P"]
        if L:
            assert {r.cap for r in ln if r.case is c} == {0, 1, P, P + 1, P + L - 1, P + L}
    assert sum(1 for r in ln if r.exact) == sum(1 for c in sc.cases("len") if c.meta["L"] and c.meta["final"])
    tails = [r for r in runs if r.kind == "tail"]
    assert tails and all(r.exact and not r.case.stored[0].length == 0 for r in tails) and {r.case.meta["tail"] for r in tails} == {"stored", "eob"}
    assert all(r.case.meta["Q"] + r.case.meta["L"] < r.cap < len(r.case.plain) - 3 for r in runs if r.kind == "after")


def test_host_decoder_on_every_family():
    inf = _inf()
    for c in sc.valid_cases():
        h = inf.decode_tokens(c.stream, window_len=len(c.history))
        assert (h.status, h.msg, h.in_used, h.out_len) == (1, "", len(c.stream), len(c.plain)), (c.name, h.status, h.msg)
        assert _replay(h, c.history) == c.plain, c.name
    for c in sc.cases("nlen"):
        ost, omsg, oout, oused = inflate_util.oracle_inflate(c.stream, 4096)
        h = inf.decode_tokens(c.stream)
        # (not the input used: at a fault the oracle reports the bytes it pulled, the decoder where the fault's field begins)
        assert (h.status, h.msg) == (ost, omsg) and _replay(h) == oout == c.plain, (c.name, h.status, h.msg)
    for c in sc.cases("cuts"):
        ost, omsg, oout, oused = inflate_util.oracle_inflate(c.stream, c.meta["cap"])
        h = inf.decode_tokens(c.stream)
        assert (h.status, h.msg) == (ost, omsg) == (-5, STARVED), (c.name, h.status, h.msg)
        assert _replay(h) == oout == c.plain and h.out_len == len(oout), c.name
