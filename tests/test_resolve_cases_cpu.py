"""The crafted token streams of tests/resolve_cases.py, checked without a GPU: every case keeps the device stage's contract
and the checker refuses a violation of each rule; replay() agrees with CPython's zlib on the same token lists written as
fixed-Huffman streams (tests/deflate_craft.py); the host decoder turns those streams into tokens of the same format, whose
replay is the plaintext and whose segments keep the contract; the inputs have the properties the GPU tests count on."""
import importlib
import zlib

import numpy as np
import pytest

import resolve_cases as rc

CTX = rc.CTX


def _all_streams():
    out = list(rc.k1_streams())
    for policy in ("decoder", "placed"):
        for wl in (0, CTX):
            out += [rc.alive_case(policy, wl, n) for n in rc.ALIVE_NSEGS]
        out += rc.alignment_cases(policy)
    for wl in rc.WINDOW_LENS:
        out += rc.window_streams(wl)
        out.append(rc.window_alive(wl))
    return out + rc.batch_streams()


@pytest.fixture(scope="module")
def streams():
    return _all_streams()


@pytest.fixture(scope="module")
def encoded(streams):
    """[(stream, fixed-Huffman bytes)]: one of every stream; of the alive family the largest of each kind (the others are
    its prefixes)"""
    seen, out = set(), []
    for s in sorted(streams, key=lambda s: -s.out_len):
        kind = s.name.rsplit("/nsegs", 1)[0] if s.name.startswith("alive/") else s.name
        if kind not in seen:
            seen.add(kind)
            out.append((s, rc.fixed_stream(s)))
    return out


def test_every_case_keeps_the_contract(streams):
    assert len(streams) >= 100
    for s in streams:
        rc.check_contract(s)
        sizes = np.diff(s.seg_bounds())
        assert s.out_len < (7 << 20) and ((sizes[:-1] >= CTX) & (sizes[:-1] <= CTX + 257)).all(), s.name


def _tiny():
    rng = np.random.default_rng(1)
    b = rc.Builder("decoder")
    b.fill(rng, 40000)
    b.match(100, CTX)
    b.fill(rng, 10)
    return b.finish("tiny")


def _broken(change):
    s = _tiny()
    tokens, literals, segs = s.tokens.copy(), s.literals.copy(), s.segs.copy()
    tokens, literals, segs = change(tokens, literals, segs) or (tokens, literals, segs)
    return rc.Stream("broken", tokens, literals, segs)


def _set(arr, k, v):
    arr[k] = v


@pytest.mark.parametrize("rule,change", [
    ("segment size", lambda t, l, s: (_set(s, 3, 1), _set(s, 4, CTX - 1), _set(s, 5, CTX - 1),
                                      _set(t, 0, CTX - 1), _set(t, 1, int(t[1]) + 1))[0]),       # first segment one byte short
    ("segment size", lambda t, l, s: (np.array([CTX + 258, 10], dtype=np.uint32), np.zeros(CTX + 268, dtype=np.uint8),
                                      np.array([0, 0, 0, 1, CTX + 258, CTX + 258, 2, CTX + 268, CTX + 268], dtype=np.uint64))),
    ("encoding", lambda t, l, s: _set(t, 2, int(t[2]) | (1 << 24))),                               # a bit between length and flag
    ("encoding", lambda t, l, s: (np.concatenate((t, np.zeros(1, dtype=np.uint32))), l,
                                  np.concatenate((s[:-3], np.array([t.size + 1, s[-2], s[-1]], dtype=np.uint64))))),
    ("distance above 32768", lambda t, l, s: _set(t, 2, rc.MATCH | (97 << 16) | CTX)),             # 32769
    ("distance too far back", lambda t, l, s: (np.concatenate((np.array([rc.tok_match(3, 1)], dtype=np.uint32), t)), l,
                                               np.array([0, 0, 0, 2, CTX + 3, CTX, t.size + 1, s[-2] + 3, s[-1]], dtype=np.uint64))),
    ("literal total", lambda t, l, s: (t, np.concatenate((l, np.zeros(1, dtype=np.uint8))), s)),
    ("segs", lambda t, l, s: _set(s, 5, int(s[5]) - 1)),                                           # first literal of segment 1
    ("segs", lambda t, l, s: _set(s, -2, int(s[-2]) + 1)),                                         # the terminal triple
])
def test_the_checker_refuses_a_violation_of_each_rule(rule, change):
    rc.check_contract(_tiny())
    with pytest.raises(rc.ContractError, match="^" + rule):
        rc.check_contract(_broken(change))


def test_a_distance_within_the_window_needs_the_window():
    b = rc.Builder("decoder", window=b"x" * 5)
    b.match(3, 5)
    s = b.finish("w")
    rc.check_contract(s)
    with pytest.raises(rc.ContractError, match="^distance too far back"):
        rc.check_contract(s, window_len=4)


def _inflate(comp, window):
    d = zlib.decompressobj(-15, zdict=window) if window else zlib.decompressobj(-15)
    out = d.decompress(comp)
    assert d.eof and not d.unused_data
    return out


def test_replay_agrees_with_cpython(encoded, streams):
    for s, comp in encoded:
        assert _inflate(comp, s.window) == s.expected(), s.name
    done = {s.name for s, _ in encoded}
    full = {s.name.rsplit("/nsegs", 1)[0]: s for s, _ in encoded if s.name.startswith("alive/")}
    for s in streams:                                             # the prefixes: the same tokens, so the same bytes, cut
        if s.name not in done:
            whole = full[s.name.rsplit("/nsegs", 1)[0]]
            assert (s.tokens == whole.tokens[:s.tokens.size]).all() and s.expected() == whole.expected()[:s.out_len], s.name


def test_the_host_decoder_writes_the_same_token_format(encoded):
    importlib.import_module("zlib-ng_amd")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    for s, comp in encoded:
        dec = inf.decode_tokens(comp, window_len=len(s.window))
        assert dec.status == 1 and dec.out_len == s.out_len and dec.in_used == len(comp), (s.name, dec.status, dec.msg)
        assert rc.replay(dec.tokens, dec.literals, s.window) == s.expected(), s.name
        rc.check_contract(rc.Stream(s.name + "/decoded", dec.tokens, dec.literals, dec.segs, s.window))


@pytest.mark.parametrize("behind", ["literals", "stored block", "nothing"])
def test_the_decoder_ends_a_segment_behind_the_match_that_fills_it(behind):
    """a match of 258 that begins at byte 32767 of a segment: the segment holds 33025 bytes, whatever follows -- not the
    literal behind the match as well, nor a whole stored block (include/zng_rocm.h: fewer than 32 KiB + 258)"""
    import deflate_craft as craft
    importlib.import_module("zlib-ng_amd")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    rng = np.random.default_rng(33026)
    toks = [("L", int(v)) for v in rng.integers(0, 256, size=CTX - 1)] + [("M", 258, 100)]
    bits = craft.Bits()
    if behind == "literals":
        toks += [("L", int(v)) for v in rng.integers(0, 256, size=40000)]
    craft.fixed_block(bits, toks, behind != "stored block")
    if behind == "stored block":
        craft.stored_block(bits, bytes(rng.integers(0, 256, size=60000, dtype=np.uint8)), True)
    bits.align()
    comp = bytes(bits.out)
    plain = zlib.decompressobj(-15).decompress(comp)
    dec = inf.decode_tokens(comp)
    assert dec.status == 1 and rc.replay(dec.tokens, dec.literals) == plain
    sizes = np.diff(dec.segs.reshape(-1, 3)[:, 1].astype(np.int64))
    assert sizes[0] == CTX + 257 and (sizes[:-1] >= CTX).all() and (sizes < CTX + 258).all(), sizes
    rc.check_contract(rc.Stream(behind, dec.tokens, dec.literals, dec.segs))


@pytest.mark.parametrize("policy", ["decoder", "placed"])
@pytest.mark.parametrize("window_len", [0, CTX])
def test_alive_streams_have_no_period_and_live_references_at_the_borders(policy, window_len):
    full = rc.alive_full(policy, window_len)
    plain = np.frombuffer(full.window + full.expected(), dtype=np.uint8)
    differ = plain[CTX:] != plain[:-CTX]
    assert differ.mean() >= 0.25, differ.mean()
    for n in rc.ALIVE_NSEGS:                                      # ... and so has every stream cut from it
        k = rc.alive_case(policy, window_len, n).out_len + len(full.window)
        if k > CTX:
            assert differ[:k - CTX].mean() >= 0.25, (n, differ[:k - CTX].mean())
    # segments made of matches alone hold nothing but references; those at the group borders are longer than 32768, so
    # that references sit on both sides of the tail border
    tri = full.segs.reshape(-1, 3).astype(np.int64)
    first = 1 if window_len == 0 else 0
    assert (np.diff(tri[first:, 2]) == 0).all()
    sizes = np.diff(tri[:, 1])
    assert (sizes[[63, 64, 65, 127, 128, 129]] > CTX).all(), sizes[[63, 64, 65, 127, 128, 129]]
    if policy == "placed":
        assert set(sizes[:-1].tolist()) == set(rc.PLACED_SIZES)
        assert {int(v - CTX) % 8 for v in sizes[:-1]} >= {0, 1, 7}


def test_the_windowed_alive_streams_have_no_period_either():
    for wl in (257, 32767, CTX):
        s = rc.window_alive(wl)
        plain = np.frombuffer(s.expected(), dtype=np.uint8)
        assert (plain[CTX:] != plain[:-CTX]).mean() >= 0.25, wl
        assert int(s.segs[5]) == 0                                # segment 0 takes no literal: matches into the window alone


def test_the_k1_cases_stand_where_they_say():
    for policy in ("decoder", "placed"):
        s = rc.literal_window_stream(policy)
        tri = s.segs.reshape(-1, 3).astype(np.int64)
        assert {int(v) % 16 for v in tri[:-1, 2]} == set(range(16))
        counts = set(np.diff(tri[:, 0]).tolist())
        assert counts >= {63, 64, 65, 128, 129} and (policy == "placed" or 1 in counts)
        is_match, n, out0, lit0 = rc.token_spans(s.tokens)
        # runs that end on, begin on and cross a multiple of 1024 literals counted from their segment's first
        seg_of = np.searchsorted(tri[:, 0], np.arange(s.tokens.size), side="right") - 1
        rel0 = lit0[:-1] - tri[seg_of, 2]
        runs = ~is_match
        assert (runs & (rel0 > 0) & (rel0 % 1024 == 0)).any()
        assert (runs & ((rel0 + n) % 1024 == 0)).any()
        assert (runs & (rel0 % 1024 != 0) & (rel0 // 1024 != (rel0 + n - 1) // 1024)).any()
    single = rc.literal_window_stream("decoder")
    tri = single.segs.reshape(-1, 3).astype(np.int64)
    one = np.flatnonzero(np.diff(tri[:, 0]) == 1)
    assert any(int(single.tokens[tri[k, 0]]) == CTX for k in one)                  # a segment that is one 32768-literal token
    for k, s in enumerate(rc.last_literals_streams(), 1):
        assert int(s.tokens[-1]) == k and s.nsegs == 2 and s.literals.size == int(s.segs[-1])
    names = [m[0] for m in rc.flush_mark_stream("decoder").marks]
    assert len(names) == len(set(names)) and len(names) > 300
    for F in (2048, 4096, 6144):
        for tag in ("far_len258_straddles", "far_len3_from_F-1", "run_len65_src_F-1", "overlap_dist257_len258_op_F+0",
                    "overlap_dist2_len3_op_F+1", "far_len64_at_mark_ends_at"):
            assert "F%d_%s" % (F, tag) in names, (F, tag)
