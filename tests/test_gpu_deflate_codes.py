"""GPU: what the block emitter (emit_dynamic_kernel, deflate_dyn.hip) writes, judged by what a right answer IS and not only
by whether it decodes.  Every crafted input of emitter_cases.py goes through deflate_dev on its own and, with all the others
of its strategy, as one ragged batch through zng_rocm_deflate_strategy_streams_dev (every stream's first block then has no
histogram before it while the batch shares the histogram scratch).  Each output is read back by CPython's zlib and by the
product's inflater, taken apart by tests/deflate_parse.py, and every block is held against tests/huffman_model.py:

  codes    the three code sets of a dynamic block are complete, within 15 / 15 / 7 bits, cover every symbol that occurs and
           no other, and HLIT / HDIST / HCLEN are the smallest that cover them;
  optimum  where no optimal code needs more than the limit (min_max_depth <= limit), the block's own histogram costs exactly
           the Huffman optimum -- costs are compared, never lengths: ties may fall either way;
  limit    where every optimal code breaks the limit (lit_deep, cl_deep, dist_deep: asserted on the parsed block, never
           skipped), the cost lies between the exact length-limited optimum (package-merge) and that optimum x (1 + MARGIN);
  choice   stored if not larger, else static if not larger than dynamic (trees.c:660-719), from the exact sizes of the parsed
           block; no block is larger than the smaller of its static and stored forms.

MARGIN.  Halving all frequencies until the tree fits costs more than zlib's redistribution of the overflowing leaves
(gen_bitlen), so the bound is the optimum's, not zlib's.  Measured (cost in bits: unrestricted optimum / length-limited
optimum / CPython's zlib on the same histogram / the product):
    lit_deep        35227 / 35236 / 35240 / 35299     + 0.179 % over the limited optimum
    lit_deep/block  148254 / 148299 / (two blocks) / 148534     + 0.158 %
    cl_deep         509 / 513 / 513 / 513             + 0
    dist_deep       21705 / 21708 / (its matcher parses otherwise) / 21715     + 0.032 %
The worst excess, 0.179 %, rounded up to the next half percent: MARGIN = 0.5 %."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import deflate_parse as dp
import emitter_cases as ec
import huffman_model as hm
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu

MARGIN = 0.005
LIMITS = {"lit": 15, "dist": 15, "cl": 7}
PATHS = ("one", "batch")


class Outputs:
    def __init__(self):
        zr = product()
        zr.init()
        self.dfl = importlib.import_module("zlib-ng_amd.deflate")
        self.inf = importlib.import_module("zlib-ng_amd.inflate")
        self.lib = zr.rocm.lib()
        self.comp, self._parsed = {}, {}
        torch = torch_mod()
        cases = ec.cases()
        for c in cases:
            src = torch.from_numpy(np.frombuffer(c.data + bytes(16), dtype=np.uint8).copy()).cuda()
            dst, n = self.dfl.deflate_dev(src, level=c.level, length=len(c.data), strategy=c.strategy)
            assert n <= self.dfl.deflate_bound(len(c.data))
            self.comp[c.name, "one"] = dst[:n].cpu().numpy().tobytes()
        for key in sorted({(c.level, c.strategy) for c in cases}):
            group = [c for c in cases if (c.level, c.strategy) == key]
            offs, buf = [], bytearray()
            for c in group:
                offs.append(len(buf))
                buf += c.data + bytes(-len(c.data) % 16)
            src = torch.from_numpy(np.frombuffer(bytes(buf) + bytes(16), dtype=np.uint8).copy()).cuda()
            b = self.dfl.StreamsBatch(src, offs, [len(c.data) for c in group])
            rc = self.lib.zng_rocm_deflate_strategy_streams_dev(key[0], key[1], C.byref(b.jobs), b.n, C.byref(b.out_lens), None)
            assert rc == 0, key
            for i, c in enumerate(group):
                self.comp[c.name, "batch"] = b.compressed(i)

    def parsed(self, name, path):
        if (name, path) not in self._parsed:
            self._parsed[name, path] = dp.parse(self.comp[name, path])          # strict: an incomplete set is an error
        return self._parsed[name, path]


@pytest.fixture(scope="module")
def outs():
    return Outputs()


def _params():
    return [pytest.param(c, p, id="%s-%s" % (c.name, p)) for c in ec.cases() for p in PATHS]


def _sets(b):
    return {"lit": (b.lit_hist, b.lit_lens), "dist": (b.dist_hist, b.dist_lens), "cl": (b.cl_hist, b.cl_lens)}


@pytest.mark.parametrize("case,path", _params())
def test_round_trip(outs, case, path):
    comp = outs.comp[case.name, path]
    d = zlib.decompressobj(-15)
    assert d.decompress(comp) == case.data and d.eof and d.unused_data == b""
    dec = outs.inf.decode_tokens(comp)
    assert dec.status == 1
    assert outs.inf.resolve_dev(dec).cpu().numpy().tobytes() == case.data
    p = outs.parsed(case.name, path)
    assert p.data == case.data and (p.end_bit + 7) // 8 == len(comp)
    if case.strategy == ec.Z_HUFFMAN_ONLY:
        assert not any(b.matches for b in p.blocks)
    if case.strategy == ec.Z_FIXED:
        assert all(b.btype != dp.DYNAMIC for b in p.blocks)


@pytest.mark.parametrize("case,path", _params())
def test_code_sets(outs, case, path):
    """complete, within the limits, a code for every symbol that occurs and for no other, the smallest HLIT / HDIST / HCLEN"""
    for b in dp.data_blocks(outs.parsed(case.name, path)):
        if b.btype != dp.DYNAMIC:
            continue
        assert b.states == {"cl": "complete", "lit": "complete", "dist": "complete"}
        for which, (hist, lens) in _sets(b).items():
            assert max(lens) <= LIMITS[which], which
            used = [s for s, f in enumerate(hist) if f]
            coded = [s for s, n in enumerate(lens) if n]
            assert set(used) <= set(coded), which
            # a set with fewer than two symbols gets a second code (the first symbol that has none), as zlib forces it
            forced = [s for s in range(len(lens)) if s not in used][:max(0, 2 - len(used))]
            assert coded == sorted(used + forced), (which, used, coded)
        assert b.hlit == max([257] + [s + 1 for s in range(286) if b.lit_lens[s]])
        assert b.hdist == max([1] + [s + 1 for s in range(30) if b.dist_lens[s]])
        assert b.hclen == max([4] + [k + 1 for k in range(19) if b.cl_lens[dp.CL_ORDER[k]]])


@pytest.mark.parametrize("case,path", _params())
def test_optimal_below_the_limit(outs, case, path):
    """where the limit cannot bind, sum f * len over the block's own histogram is the Huffman optimum, exactly"""
    checked = 0
    for b in dp.data_blocks(outs.parsed(case.name, path)):
        if b.btype != dp.DYNAMIC:
            continue
        for which, (hist, lens) in _sets(b).items():
            if hm.min_max_depth(hist) <= LIMITS[which]:
                assert hm.body_cost(hist, lens) == hm.optimal_cost(hist), (which, b.out_start)
                checked += 1
    if "k" not in case.extra and case.extra.get("btype", dp.DYNAMIC) == dp.DYNAMIC:
        assert checked, "the case has no dynamic block"


def _deep_block(p, case, which):
    """the block the case was built for: the one whose histogram is deepest"""
    blocks = [b for b in dp.data_blocks(p) if b.btype == dp.DYNAMIC]
    assert blocks, "no dynamic block"
    return max(blocks, key=lambda b: hm.min_max_depth(_sets(b)[which][0]))


_DEEP = [pytest.param(c, w, p, id="%s-%s-%s" % (c.name, w, p)) for c in ec.cases() for w in c.deep for p in PATHS]
_EXACT = [pytest.param(c, w, p, id="%s-%s-%s" % (c.name, w, p)) for c in ec.cases() for w in c.exact for p in PATHS]


@pytest.mark.parametrize("case,which,path", _DEEP)
def test_cost_above_the_limit(outs, case, which, path):
    """every optimal code of this histogram is deeper than the limit -- asserted on the parsed block --, so the depth-limit
    loop ran: the code costs no less than the length-limited optimum and at most MARGIN more.
    dist_deep: the matcher decides the tokens; the distance histogram it gave and the costs are in DESIGN.md 3.6.1."""
    b = _deep_block(outs.parsed(case.name, path), case, which)
    hist, lens = _sets(b)[which]
    limit = case.deep[which]
    depth = hm.min_max_depth(hist)
    cost, best, free = hm.body_cost(hist, lens), hm.limited_optimum(hist, limit), hm.optimal_cost(hist)
    ref = None
    if case.single:                                            # CPython's zlib on the same histogram
        c = zlib.compressobj(case.level, zlib.DEFLATED, -15, 9, case.strategy)
        rb = dp.parse(c.compress(case.data) + c.flush()).blocks
        assert len(rb) == 1 and _sets(rb[0])[which][0] == hist, "the reference block has another histogram"
        ref = hm.body_cost(hist, _sets(rb[0])[which][1])
    print("%s %s %s: depth %d, optimum %d, limited optimum %d, zlib %s, product %d (+%.3f %%)%s"
          % (case.name, which, path, depth, free, best, ref, cost, 100.0 * (cost - best) / best,
             " hist %s" % hist if which == "dist" else ""))
    assert depth > limit, "the case does not reach the depth limit"
    assert max(lens) <= limit
    assert best > free and cost >= best, "the model's optimum is not one"
    assert cost <= best * (1 + MARGIN), (cost, best)
    if which == "lit" and case.hist:
        assert hist == case.hist
    if which == "cl" and case.cl_hist:
        assert hist == case.cl_hist


@pytest.mark.parametrize("case,which,path", _EXACT)
def test_cost_at_the_limit(outs, case, which, path):
    """depth exactly at the limit: nothing may be halved, the cost is the unrestricted optimum"""
    blocks = dp.data_blocks(outs.parsed(case.name, path))
    assert len(blocks) == 1 and blocks[0].btype == dp.DYNAMIC
    hist, lens = _sets(blocks[0])[which]
    assert hist == (case.hist if which == "lit" else case.cl_hist)
    assert hm.min_max_depth(hist) == case.exact[which] == max(lens)
    assert hm.body_cost(hist, lens) == hm.optimal_cost(hist) == hm.limited_optimum(hist, case.exact[which])


def _literal_hist(data):
    h = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=286).tolist()
    h[256] = 1
    return h


@pytest.mark.parametrize("case,path", _params())
def test_block_type_choice(outs, case, path):
    """stored if not larger, else static if not larger than dynamic -- ties go to the simpler block.  A stored block carries no
    tokens; its static size is computed for its bytes as literals, which is exact where the strategy or the input allows no
    match (Z_HUFFMAN_ONLY, fixed_tie) and an upper bound of the matcher's tokens' size elsewhere."""
    comp = outs.comp[case.name, path]
    p = outs.parsed(case.name, path)
    data_blocks = dp.data_blocks(p)
    for b in data_blocks:
        size = (b.end - b.start + 7) // 8
        stored = hm.stored_lenb(b.nbytes)
        if b.btype == dp.STORED:
            static = hm.static_lenb(_literal_hist(p.bytes_of(b)), [0] * 30)
            assert size == stored and stored <= static, (b.out_start, stored, static)
            continue
        static = hm.static_lenb(b.lit_hist, b.dist_hist)
        if b.btype == dp.DYNAMIC:
            dyn = hm.dyn_lenb(b.header_bits, b.lit_hist, b.dist_hist, b.lit_lens, b.dist_lens)
            assert size == dyn and dyn < static and dyn < stored, (b.out_start, dyn, static, stored)
        else:
            assert size == static and static < stored, (b.out_start, static, stored)
        assert size <= min(static, stored)
    # with what the design adds behind it -- the empty stored block that byte-aligns it, the final block; counted from the
    # parsed stream -- no block takes more room than the smaller of its static and stored forms
    starts = [b.start for b in data_blocks] + [8 * len(comp)]
    for b, nxt in zip(data_blocks, starts[1:]):
        added = nxt - b.end
        assert added <= 3 + 7 + 32 + 10 + 7
        assert nxt - b.start <= 8 * min(hm.static_lenb(_literal_hist(p.bytes_of(b)), [0] * 30) if b.btype == dp.STORED
                                        else hm.static_lenb(b.lit_hist, b.dist_hist), hm.stored_lenb(b.nbytes)) + 8 * ((added + 7) // 8)
    if "k" in case.extra:                                      # fixed_tie (Z_FIXED) and stored_tie: n distinct bytes, no match,
        assert len(data_blocks) == 1                           # and a dynamic block is out of reach -- decidable both ways
        lit = _literal_hist(case.data)
        want = dp.STORED if hm.stored_lenb(len(case.data)) <= hm.static_lenb(lit, [0] * 30) else dp.STATIC
        assert data_blocks[0].btype == want, (case.name, hm.stored_lenb(len(case.data)), hm.static_lenb(lit, [0] * 30))
        # static is ceil((10 + 8 n + k) / 8) bytes, stored n + 5: k = 22 static, k = 23 the tie, stored from there on
        assert want == (dp.STATIC if case.extra["k"] <= 22 else dp.STORED)
    if "btype" in case.extra:                                  # dyn_tie: all three sizes are known without the product
        assert len(data_blocks) == 1 and data_blocks[0].btype == case.extra["btype"], case.extra
        b = data_blocks[0]
        assert (b.end - b.start + 7) // 8 == case.extra["dyn_lenb" if b.btype == dp.DYNAMIC else "static_lenb"]


@pytest.mark.parametrize("path", PATHS)
def test_mixed_has_every_block_type(outs, path):
    types = {b.btype for b in dp.data_blocks(outs.parsed("mixed/default", path))}
    assert dp.STORED in types and dp.DYNAMIC in types
    assert {b.btype for b in dp.data_blocks(outs.parsed("fixed_tie/22", path))} == {dp.STATIC}


@pytest.mark.parametrize("path", PATHS)
def test_crafted_edges_are_reached(outs, path):
    """the matcher and the front ends did produce what each edge case was built for"""
    def only(name):
        blocks = [b for b in dp.data_blocks(outs.parsed(name, path)) if b.btype == dp.DYNAMIC]
        assert len(blocks) == 1, name
        return blocks[0]
    b = only("dist_one")                                       # one distance code: a second one is forced, one bit each
    assert [s for s, f in enumerate(b.dist_hist) if f] == [10]
    assert [(s, n) for s, n in enumerate(b.dist_lens) if n] == [(0, 1), (10, 1)] and b.hdist == 11
    b = only("dist_all")
    assert b.dist_hist[0] and b.dist_hist[29] and b.hdist == 30
    b = only("len_258")
    assert b.lit_hist[285] and b.hlit == 286 and [s for s, f in enumerate(b.dist_hist) if f] == [0]
    for name in ("lit_deep", "rle_header/a", "rle_header/b", "rle_header/c", "rle_header/cross"):      # literals only
        b = only(name)
        assert b.hlit == 257 and b.hdist == 2 and b.dist_lens[:2] == [1, 1] and not b.matches
        c = ec.by_name(name)
        if "lit_lens" in c.extra:                              # exact powers of two: no other lengths are optimal
            assert b.lit_lens[:257] == c.extra["lit_lens"], name
    syms = lambda name: only(name).cl_syms
    a = syms("rle_header/a")
    for want in ((17, 3), (17, 10), (18, 11), (18, 138), (16, 3), (16, 4), (16, 6), (18, 47)):
        assert want in a, want
    assert [0, 0] == [s for s in a if s == 0]                  # the run of two zeros: two single zeros, no other
    assert (18, 138) in syms("rle_header/b") and 0 in syms("rle_header/b")
    assert [(18, 138), (18, 11)] == [s for s in syms("rle_header/c") if isinstance(s, tuple)][:2]
    assert syms("rle_header/cross")[-3:] == [1, 1, 1]          # end-of-block, then both distance lengths


@pytest.mark.parametrize("path", PATHS)
def test_blocks_differ(outs, path):
    """every block's lengths are non-zero on its own alphabet only: a block's histogram is the difference of two cumulative
    snapshots, and the first block of a segment has nothing to subtract"""
    case = ec.by_name("blocks_differ")
    blocks = dp.data_blocks(outs.parsed(case.name, path))
    assert [(b.out_start, b.out_end) for b in blocks] == [(lo, hi) for lo, hi, _, _ in case.extra["alphabets"]]
    for b, (lo, hi, a0, b0) in zip(blocks, case.extra["alphabets"]):
        assert b.btype == dp.DYNAMIC
        coded = [s for s, n in enumerate(b.lit_lens) if n]
        assert coded == sorted(set(case.data[lo:hi])) + [256]
        assert all(a0 <= s < b0 for s in coded[:-1])
        assert hm.body_cost(b.lit_hist, b.lit_lens) == hm.optimal_cost(b.lit_hist)
