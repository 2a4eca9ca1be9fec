"""CPU: the test infrastructure of the block-emitter tests checked on its own -- the DEFLATE block parser (deflate_parse.py)
against CPython's zlib and against the crafted streams of dynamic_cases.py, the Huffman cost model (huffman_model.py) against
brute force and against CPython's own blocks, and every crafted input of emitter_cases.py: the condition it was built for
holds, and the reference (CPython's zlib, same strategy) stays inside every condition the GPU tests assert of the product."""
import itertools
import random
import time
import zlib

import pytest

import deflate_craft as craft
import deflate_parse as dp
import dynamic_cases as dc
import emitter_cases as ec
import huffman_model as hm
import synth

STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)


def _zlib(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush()


def _inputs():
    return {"silesia": synth.silesia_like(256 << 10).tobytes(), "empty": b"", "one": b"z", "zeros": bytes(70000)}


def check_tiling(p, comp):
    """block follows block bit by bit from bit 0 to the stream's last byte, and byte by byte through the plaintext"""
    assert p.blocks[0].start == 0 and p.blocks[0].out_start == 0
    for a, b in zip(p.blocks, p.blocks[1:]):
        assert a.end == b.start and a.out_end == b.out_start and not a.final
    assert p.blocks[-1].final and p.blocks[-1].out_end == len(p.data)
    assert (p.end_bit + 7) // 8 == len(comp)
    for b in p.blocks:
        assert b.start < b.header_end <= b.end and b.out_start <= b.out_end


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("level", [1, 6, 9])
def test_parser_reads_cpython(level, strategy):
    for name, data in _inputs().items():
        comp = _zlib(data, level, strategy)
        t0 = time.time()
        p = dp.parse(comp)
        took = time.time() - t0
        assert took < 3.0, (name, took)                       # 256 KiB of tokens in about a second
        assert p.data == data, name
        assert craft.replay([t for b in p.blocks for t in b.tokens]) == data, name
        check_tiling(p, comp)
        for b in p.blocks:
            assert p.bytes_of(b) == data[b.out_start:b.out_end]
            if b.btype == dp.STORED:
                continue
            # the histograms are the tokens', the end-of-block counted once
            toks = b.tokens
            assert sum(b.lit_hist) == len(toks) + 1 and b.lit_hist[256] == 1
            assert sum(b.dist_hist) == sum(1 for t in toks if t[0] == "M") == len(b.matches)
            assert sum(b.lit_hist[:256]) == sum(1 for t in toks if t[0] == "L")
            if strategy == zlib.Z_FIXED:
                assert b.btype == dp.STATIC
            if strategy == zlib.Z_HUFFMAN_ONLY:
                assert not b.matches
            if strategy == zlib.Z_RLE:
                assert all(m[2] == 1 for m in b.matches)
            if b.btype == dp.DYNAMIC:
                assert len(b.lit_lens) == 286 and len(b.dist_lens) == 30 and len(b.cl_lens) == 19
                assert sum(b.cl_hist) == len(b.cl_syms)
                assert all(b.lit_lens[s] for s, f in enumerate(b.lit_hist) if f)
                assert all(b.dist_lens[s] for s, f in enumerate(b.dist_hist) if f)


def _norm(tokens):
    out = []
    for t in tokens:
        if t[0] == "S" and t[1] < 256:
            out.append(("L", t[1]))
        elif t[0] == "S":
            out.append(("M", craft._LEN_BASE[t[1] - 257] + t[2], craft._DIST_BASE[t[3]] + t[4]))
        else:
            out.append(tuple(t))
    return out


_CL_LENS = {                                                   # the cases that do not use the default code-length code
    "lit-hclen5/plain": dc.sparse_lens(19, {0: 1, 8: 1}), "lit-hclen5/16": dc.sparse_lens(19, {0: 2, 8: 1, 16: 2}),
    "hdr-cl/7bit": dc.sparse_lens(19, dict(zip([7, 6, 18, 3, 0, 16, 17, 5], [1, 2, 3, 4, 5, 6, 7, 7]))),
    "hdr-cl/two-1bit": dc.sparse_lens(19, {0: 1, 1: 1}),
}


def _expand(cl_syms):
    out = []
    for s in cl_syms:
        if isinstance(s, tuple):
            out += [out[-1] if s[0] == 16 else 0] * s[1]
        else:
            out.append(s)
    return out


def test_parser_reads_crafted_blocks():
    """every well-formed case of dynamic_cases.py: the lengths, HLIT / HDIST / HCLEN and the tokens it was built from"""
    seen = 0
    for c in dc.valid_cases():
        p = dp.parse(c.stream, history=c.history, strict=False)
        assert p.data == c.plain, c.name
        assert [t for b in p.blocks for t in b.tokens] == _norm(c.tokens), c.name
        check_tiling(p, c.stream)
        for b in p.blocks:
            assert b.btype == dp.DYNAMIC
            assert _expand(b.cl_syms) == b.lit_lens[:b.hlit] + b.dist_lens[:b.hdist], c.name
        if c.name not in dc._SETS:
            continue
        lit, dist = dc._SETS[c.name]
        b = p.blocks[0]
        assert (b.hlit, b.hdist) == (len(lit), len(dist)), c.name
        assert b.lit_lens[:b.hlit] == list(lit) and b.dist_lens[:b.hdist] == list(dist), c.name
        assert not any(b.lit_lens[b.hlit:]) and not any(b.dist_lens[b.hdist:])
        cl = _CL_LENS.get(c.name, craft.flat_lens(19))
        assert b.cl_lens == cl, c.name
        assert b.hclen == max([4] + [k + 1 for k in range(19) if cl[dp.CL_ORDER[k]]]) or c.name.startswith("lit-hclen5"), c.name
        if c.name.startswith("lit-hclen5"):
            assert b.hclen == 5
        # the parser's own verdict on each set is the Kraft sum of the lengths the case was built from
        assert b.states["lit"] == dp.code_state(lit) and b.states["dist"] == dp.code_state(dist), c.name
        seen += 1
    assert seen > 150
    # the code-length symbols as sent: one pair of sets written in four ways
    lit, dist = dc._v6_sets()
    for style in ("plain", "greedy", "max", "cross"):
        c = next(x for x in dc.valid_cases() if x.name == "hdr-rle/" + style)
        assert dp.parse(c.stream, strict=False).blocks[0].cl_syms == craft.rle(lit + dist, style, border=len(lit)), style
    # strict: an incomplete literal/length set is refused, the distance set may have one code of one bit or none
    empty = next(x for x in dc.valid_cases() if x.name == "lit-empty")
    with pytest.raises(dp.ParseError):
        dp.parse(empty.stream)
    for name in ("dist-none", "dist-one/0", "dist-one/4", "dist-two"):
        c = next(x for x in dc.valid_cases() if x.name == name)
        assert dp.parse(c.stream).data == c.plain


def test_parser_refuses_bad_code_sets():
    small, d2 = dc.sparse_lens(259, dc._SMALL), [1, 1]
    toks = dc._text(6)
    for lit, dist, kw in ((dc.sparse_lens(259, {97: 1, 98: 2, 99: 3, 256: 3, 257: 5}), d2, {}),           # over-subscribed
                          (dc.sparse_lens(259, {97: 1, 98: 2, 99: 3, 256: 4}), d2, {}),                   # incomplete
                          (small, [1, 1, 2], {}), (small, [2, 2], {}), (small, [2], {}),
                          (small, d2, dict(cl_lens=dc.sparse_lens(19, {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 5, 18: 6}))),
                          (small, d2, dict(cl_lens=dc.sparse_lens(19, {0: 1, 1: 2, 2: 2, 3: 3, 4: 3, 5: 3, 18: 3})))):
        b = craft.Bits()
        craft.dynamic_block(b, toks, True, lit, dist, **kw)
        b.align()
        with pytest.raises(dp.ParseError):
            dp.parse(bytes(b.out))


# ---- the model ----------------------------------------------------------------------------------------------------------
def test_limited_optimum_is_brute_force():
    rng = random.Random(7)
    shapes = [[1, 1, 2, 3, 5, 8, 13], [1, 1, 3, 5, 9, 15, 25], [5, 5, 5, 5], [1, 100], [7], [1, 2, 4, 8, 16, 32, 64], [3, 3, 3, 3, 3, 3, 3]]
    shapes += [[rng.choice([1, 2, 3, 5, 9, 30, 100, 1000]) for _ in range(rng.randint(2, 7))] for _ in range(150)]
    for f in shapes:
        for maxbits in (2, 3, 4):
            if len(f) > 1 << maxbits:
                with pytest.raises(ValueError):
                    hm.limited_optimum(f, maxbits)
                continue
            got = hm.limited_optimum(f, maxbits)
            assert got == hm.brute_force_limited(f, maxbits), (f, maxbits)
            assert got >= hm.optimal_cost(f)
            assert (got == hm.optimal_cost(f)) == (hm.min_max_depth(f) <= maxbits), (f, maxbits)


def test_limit_not_hit_means_unrestricted_optimum():
    rng = random.Random(8)
    for _ in range(300):
        f = [rng.choice([0, 0, 1, 1, 2, 3, 7, 20, 90, 400, 5000]) for _ in range(rng.randint(2, 40))]
        for maxbits in (7, 15):
            if hm.min_max_depth(f) <= maxbits:
                assert hm.limited_optimum(f, maxbits) == hm.optimal_cost(f), f
            else:
                assert hm.limited_optimum(f, maxbits) > hm.optimal_cost(f), f
    assert hm.min_max_depth(ec.series(18)) == 17 and hm.min_max_depth([1] + ec.series(18)) == 18
    # ties: 1 1 2 2 has an optimal chain (3 3 2 1) and an optimal flat code (2 2 2 2); the precondition is the flat one's depth,
    # and a limit the flat code meets costs nothing
    assert hm.min_max_depth([1, 1, 2, 2]) == 2 and hm.limited_optimum([1, 1, 2, 2], 2) == hm.optimal_cost([1, 1, 2, 2]) == 12
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    for limit in (19, 20, 21):                                # a plain Fibonacci series: one tie, the chain stays
        assert (hm.limited_optimum(fib, limit) == hm.optimal_cost(fib)) == (limit >= hm.min_max_depth(fib) == 21)
    assert hm.optimal_cost([]) == 0 and hm.optimal_cost([0, 9]) == 9 and hm.min_max_depth([0, 9]) == 1


def test_block_sizes():
    lit = [0] * 286
    lit[65], lit[200], lit[256], lit[257], lit[270], lit[285] = 10, 3, 1, 2, 1, 1
    dist = [0] * 30
    dist[0], dist[4], dist[29] = 2, 1, 1
    bits = 3 + 10 * 8 + 3 * 9 + 7 + 2 * 7 + (7 + 2) + 8 + 4 * 5 + 1 + 13
    assert hm.static_lenb(lit, dist) == (bits + 7) // 8
    assert [hm.stored_lenb(n) for n in (0, 1, 65535, 65536, 131070, 131071)] == [5, 6, 65540, 65546, 131080, 131086]
    ll, dl = [0] * 286, [0] * 30
    for s, n in ((65, 1), (200, 3), (256, 5), (257, 4), (270, 5), (285, 3)):
        ll[s] = n
    dl[0], dl[4], dl[29] = 1, 2, 2
    bits = 100 + 10 + 9 + 5 + 8 + (5 + 2) + 3 + 2 + (2 + 1) + (2 + 13)
    assert hm.dyn_lenb(100, lit, dist, ll, dl) == (bits + 7) // 8


def _dynamic_blocks(comp):
    return [b for b in dp.parse(comp).blocks if b.btype == dp.DYNAMIC]


def test_cpython_blocks_are_optimal_below_the_limit():
    """wherever the depth precondition says no optimal code breaks the limit, CPython's code costs exactly the optimum"""
    checked = 0
    for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
        for data in (synth.silesia_like(256 << 10).tobytes(), synth.silesia_like(200 << 10, seed=9, seg_bytes=40 << 10).tobytes()):
            for b in _dynamic_blocks(_zlib(data, 6, strategy)):
                for hist, lens, limit in ((b.lit_hist, b.lit_lens, 15), (b.dist_hist, b.dist_lens, 15), (b.cl_hist, b.cl_lens, 7)):
                    if hm.min_max_depth(hist) <= limit and sum(1 for f in hist if f) >= 2:
                        assert hm.body_cost(hist, lens) == hm.optimal_cost(hist)
                        checked += 1
    assert checked > 30


# ---- the crafted inputs -------------------------------------------------------------------------------------------------
def _ref_blocks(c):
    comp = _zlib(c.data, c.level, c.strategy, mem=9)
    p = dp.parse(comp)
    assert p.data == c.data and zlib.decompress(comp, -15) == c.data
    return p.blocks


def _sets(b):
    return {"lit": (b.lit_hist, b.lit_lens, 15), "dist": (b.dist_hist, b.dist_lens, 15), "cl": (b.cl_hist, b.cl_lens, 7)}


@pytest.mark.parametrize("case", ec.cases(), ids=lambda c: c.name)
def test_crafted_input(case):
    """the generator's own histogram meets the condition the case was built for; CPython round-trips the input and, where the
    case is one block for it, shows the same histogram and stays inside what the GPU tests assert of the product"""
    c = case
    blocks = _ref_blocks(c)
    if c.hist is not None:
        n = [0] * 256
        for v in c.data:
            n[v] += 1
        assert n == c.hist[:256] and c.hist[256] == 1 and not any(c.hist[257:])
    intended = {"lit": c.hist, "cl": c.cl_hist, "dist": c.extra.get("dist_hist")}
    for which, limit in c.deep.items():
        assert hm.min_max_depth(intended[which]) > limit, (which, hm.min_max_depth(intended[which]))
    for which, limit in c.exact.items():
        assert hm.min_max_depth(intended[which]) == limit, (which, hm.min_max_depth(intended[which]))
    if not c.single:
        return
    want = c.extra.get("btype", dp.DYNAMIC)
    if "dyn_lenb" in c.extra and len(c.data) + 4 <= min(c.extra["dyn_lenb"], c.extra["static_lenb"]):
        want = dp.STORED                                       # zlib counts a stored block's header as 4 bytes (trees.c:672): it
    assert len(blocks) == 1 and blocks[0].btype == want        # goes on in the byte before; the product's blocks start on a byte
    b = blocks[0]
    if b.btype == dp.STORED:
        return
    assert b.lit_hist == c.hist
    if b.btype == dp.STATIC:                                   # dyn_tie: static is not larger than the dynamic block would be
        assert (b.end - b.start + 7) // 8 == c.extra["static_lenb"] <= c.extra["dyn_lenb"]
        return
    if c.cl_hist:
        assert b.cl_hist == c.cl_hist
    if "lit_lens" in c.extra:                                  # exact powers of two: these and no other lengths are optimal
        assert b.lit_lens[:257] == c.extra["lit_lens"]
    for which, (hist, lens, limit) in _sets(b).items():
        if which == "dist":
            continue
        cost, best = hm.body_cost(hist, lens), hm.limited_optimum(hist, limit)
        assert max(lens) <= limit and cost >= best
        if hm.min_max_depth(hist) <= limit:
            assert cost == hm.optimal_cost(hist), which
        else:
            assert which in c.deep and cost <= best * 1.005, (which, cost, best)
    size = hm.dyn_lenb(b.header_bits, b.lit_hist, b.dist_hist, b.lit_lens, b.dist_lens)
    assert size == (b.end - b.start + 7) // 8
    if "dyn_lenb" in c.extra:                                  # the size predicted without an encoder
        assert b.header_bits == ec.predicted_header_bits(b.lit_lens[:257], [1, 1])
        assert size == c.extra["dyn_lenb"] < c.extra["static_lenb"]


def test_crafted_inputs_cover_what_they_claim():
    names = [c.name for c in ec.cases()]
    for want in ("lit_deep", "lit_deep/block", "lit_exact15", "cl_deep", "cl_exact7", "dist_deep", "dist_one", "dist_all", "len_258",
                 "rle_header/a", "rle_header/b", "rle_header/c", "rle_header/cross", "blocks_differ", "mixed/default"):
        assert want in names
    assert [c.extra["k"] for c in ec.cases() if c.name.startswith("fixed_tie/")] == list(range(20, 34))
    assert [c.extra["k"] for c in ec.cases() if c.name.startswith("stored_tie/")] == list(range(20, 34))
    # dyn_tie: static smaller, the tie, dynamic smaller -- and stored larger than both throughout
    ties = [c.extra for c in ec.cases() if c.name.startswith("dyn_tie/")]
    assert all(x["stored_lenb"] > min(x["static_lenb"], x["dyn_lenb"]) for x in ties)
    assert {(x["static_lenb"] > x["dyn_lenb"]) - (x["static_lenb"] < x["dyn_lenb"]) for x in ties} == {-1, 0, 1}
    assert all(x["btype"] == (dp.DYNAMIC if x["dyn_lenb"] < x["static_lenb"] else dp.STATIC) for x in ties)
    # rle_header: the runs the case names are in its length sequence
    runs = lambda seq: [(v, len(list(g))) for v, g in itertools.groupby(seq)]
    a = runs(ec.by_name("rle_header/a").extra["lit_lens"])
    assert {n for v, n in a if v == 0} >= {2, 3, 10, 11, 138} and {n for v, n in a if v} >= {3, 4, 7, 8, 13}
    assert a[-2] == (0, 47) and a[-1][0] == 10                # zeros up to byte 255, the end-of-block behind them
    assert (0, 139) in runs(ec.by_name("rle_header/b").extra["lit_lens"])
    assert (0, 149) in runs(ec.by_name("rle_header/c").extra["lit_lens"])
    # blocks_differ: neighbours inside a segment share no byte value
    c = ec.by_name("blocks_differ")
    al = c.extra["alphabets"]
    assert len(c.data) == 200 << 10 and len(al) == 5
    for (lo0, hi0, a0, b0), (lo1, hi1, a1, b1) in zip(al, al[1:]):
        assert hi0 == lo1
        if lo1 % ec.SEGMENT:
            assert b0 <= a1 or b1 <= a0
    for lo, hi, a0, b0 in al:
        assert all(a0 <= v < b0 for v in c.data[lo:hi])
    # fixed_tie: no byte twice, k of them above 143
    for c in ec.cases():
        if c.name.startswith(("fixed_tie/", "stored_tie/")):
            assert len(set(c.data)) == len(c.data) == c.extra["n"] and sum(v >= 144 for v in c.data) == c.extra["k"]
            lit = [0] * 286
            for v in c.data:
                lit[v] = 1
            lit[256] = 1
            assert hm.static_lenb(lit, [0] * 30) == (10 + 8 * c.extra["n"] + c.extra["k"] + 7) // 8
