"""The crafted dynamic-Huffman cases (tests/dynamic_cases.py) without a GPU: first the cases themselves against two inflaters
that are no part of the product -- CPython's zlib and the oracle (oracle/inflate_oracle.c) -- then the product's host token
decoder (inflate_host.cpp: its own bit reader and table builder for inflate.c:814-917 and inftrees.c:32-297) against the
oracle: status, message and input used on every case, every invalid block and every truncation of six small headers with
every value of the last byte; the token replay against the plaintext."""
import importlib
import zlib

import dynamic_cases as dc
import inflate_util


def _inf():
    importlib.import_module("zlib-ng_amd")
    return importlib.import_module("zlib-ng_amd.inflate")


def _replay(dec, history=b""):
    """the bytes a decoded stream's tokens produce behind `history`"""
    out = bytearray(history)
    lit, lp = dec.literals.tobytes(), 0
    for tok in dec.tokens.tolist():
        if tok >> 31:
            ln, dist = ((tok >> 16) & 0xff) + 3, (tok & 0xffff) + 1
            assert dist <= len(out)
            for _ in range(ln):
                out.append(out[-dist])
        else:
            out += lit[lp:lp + tok]
            lp += tok
    assert lp == len(lit)
    return bytes(out[len(history):])


def _zlib(stream, history=b""):
    """(status, message, bytes) of CPython's zlib"""
    z = zlib.decompressobj(-15, zdict=history) if history else zlib.decompressobj(-15)
    try:
        out = z.decompress(stream)
    except zlib.error as e:
        return -3, str(e), None
    return (1 if z.eof else -5), "", out


def test_valid_cases_are_what_zlib_and_the_oracle_decode():
    cases = dc.valid_cases()
    assert len(dc.kinds()) <= 20                          # every kind can have 5 % of a stream's blocks
    for c in cases:
        assert _zlib(c.stream, c.history) == (1, "", c.plain), c.name
        got = inflate_util.oracle_inflate_dict(c.stream, c.history, len(c.plain) + 8) if c.needs else \
            inflate_util.oracle_inflate(c.stream, len(c.plain) + 8)
        assert got == (1, "", c.plain, len(c.stream)), (c.name, got[:2], got[3])
    # what the cases are for: codes of every length, on both sides of every root
    lens = set()
    for name, (lit, dist) in dc._SETS.items():
        lens |= set(lit) | set(dist)
    assert lens >= set(range(16))


def test_invalid_cases_are_refused_alike_by_zlib_and_the_oracle():
    inv = dc.invalid_cases()
    assert len(inv) >= 48
    for x in inv:
        st, msg, _ = _zlib(x.stream)
        assert x.expect[0] == st == -3 and msg.endswith(x.expect[1]) and x.expect[1], (x.name, msg, x.expect[:2])
    assert len({x.expect[1] for x in inv}) >= 9           # the messages of inflate.c:808-917 and of the two code errors


def test_the_sweep_is_mostly_decided():
    """both sides out of input or room says nothing: that share of the sweep, by the oracle alone"""
    sweep = dc.truncation_sweep()
    undecided = sum(1 for _, e in sweep if e[0] == -5)
    assert len(sweep) >= 6 * 20 * 256 and undecided < 0.6 * len(sweep), (undecided, len(sweep))
    assert not any(x.expect[0] == -5 for x in dc.invalid_cases())


def test_host_decoder_on_every_case():
    inf = _inf()
    for c in dc.valid_cases():
        h = inf.decode_tokens(c.stream, window_len=c.needs)
        assert (h.status, h.msg, h.in_used, h.out_len) == (1, "", len(c.stream), len(c.plain)), (c.name, h.status, h.msg)
        assert _replay(h, c.history) == c.plain, c.name
    for x in dc.invalid_cases():
        h = inf.decode_tokens(x.stream)
        assert (h.status, h.msg, h.in_used) == (x.expect[0], x.expect[1], x.expect[3]), (x.name, h.status, h.msg, h.in_used, x.expect)


def test_host_decoder_on_the_truncation_sweep():
    inf = _inf()
    differ = []
    for s, (ost, omsg, oout, oused) in dc.truncation_sweep():
        h = inf.decode_tokens(s)
        if (h.status, h.msg, h.in_used) != (ost, omsg, oused) or (ost == 1 and _replay(h) != oout):
            differ.append((s.hex(), (h.status, h.msg, h.in_used), (ost, omsg, oused)))
    assert not differ, (len(differ), differ[:5])


def test_host_threads_on_a_stream_of_crafted_blocks():
    """block follows block at any bit offset, 640 KiB and more of them: the threaded decode (inflate_threads.cpp, with the
    host's own block-start finder) cuts the stream, and has to give the sequential answer"""
    inf = _inf()
    big = dc.large_stream(False, min_bytes=640 << 10)
    st, _, plain = _zlib(big.comp)
    assert st == 1 and len(big.comp) >= (512 << 10) and min(big.share.values()) >= 0.05
    status, blocks = inflate_util.oracle_block_starts(big.comp, len(plain))
    assert status == 1 and len(blocks) == big.total       # the builder's own count of its blocks
    one = inf.decode_tokens(big.comp)
    four = inf.decode_tokens(big.comp, nthreads=4)
    for h in (one, four):
        assert (h.status, h.msg, h.in_used, h.out_len) == (1, "", len(big.comp), len(plain))
    assert _replay(four) == plain
    # an invalid block deep in such a stream: the same refusal from one thread and from four
    for name in ("dist-over", "no-eob", "dist-unused-code", "16-overrun"):
        bad = dc.large_stream(True, bad=name).comp
        ost, omsg, _, oused = inflate_util.oracle_inflate(bad, cap=4 << 20)
        assert ost == -3
        for n in (1, 4):
            h = inf.decode_tokens(bad, nthreads=n)
            assert (h.status, h.msg, h.in_used) == (ost, omsg, oused), (name, n, h.status, h.msg, h.in_used, omsg, oused)
