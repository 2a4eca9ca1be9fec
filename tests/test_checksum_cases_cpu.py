"""No GPU: the crafted checksum cases (tests/checksum_cases.py) reach what they claim to reach.

  * the model's constants are the ones in context.h, gf2.h, checksum_kernel.h and checksum.hip;
  * for 256, 304, 64 and 8 CUs the families together reach every class of stream_body's control flow, each assertion naming the
    class it misses;
  * the references agree with one another: CPython's zlib, the project's oracle, the reference's own crc32_braid where
    oracle/_ref is built, and the closed form for constant fills;
  * for contrast, the sizes of test_gpu_checksums.py's structured inputs and of its largest fold_copy_dev case reach no mid-stream
    reduction and no pipelined group of the copy pass on a 256-CU device."""
import os
import re
import zlib

import pytest

import checksum_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib-ng_amd", "csrc")
CU_COUNTS = (256, 304, 64, 8)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(text, pattern):
    m = re.search(pattern, text)
    assert m, "pattern %r not found: the model's constants cannot be held to the source" % pattern
    return tuple(int(g, 0) for g in m.groups()) if m.re.groups > 1 else int(m.group(1), 0)


def test_model_constants_are_the_kernels():
    ctx, ker, host, gf2 = _src("context.h"), _src("checksum_kernel.h"), _src("checksum.hip"), _src("gf2.h")
    assert _int(ctx, r"constexpr int kWgThreads\s*=\s*(\d+);") == cc.LANES
    assert _int(ctx, r"constexpr int kPieceBytes\s*=\s*(\d+);") == cc.PIECE
    assert re.search(r"constexpr int kUnitBytes\s*=\s*kWgThreads \* kPieceBytes;", ctx)
    assert cc.UNIT == cc.LANES * cc.PIECE == 16384
    assert _int(ctx, r"constexpr int kMaxGroups\s*=\s*(\d+);") == cc.MAX_GROUPS
    assert _int(gf2, r"constexpr uint32_t kAdlerBase\s*=\s*(\d+)u;") == cc.BASE
    assert _int(ker, r"constexpr int BATCH_MAX\s*=\s*(\d+);") == cc.BATCH_MAX
    assert _int(ker, r"constexpr int kRowsPerBuffer\s*=\s*(\d+), kRowsPerBufferCopy\s*=\s*(\d+);") == (cc.ROWS, cc.ROWS_COPY)
    assert re.search(r"int UNROLL = COPY \? kRowsPerBufferCopy : kRowsPerBuffer>", ker)
    assert re.search(r"stream_body<DO_ADLER, DO_CRC, false, V, false, kRowsPerBuffer>\(messages\[blockIdx\.y\]", ker)
    # the many-message rule: the overestimate of a message's units, one workgroup per 1024 of them, at most 16
    assert re.search(r"\(jobs\[i\]\.len \+ 15 \+ kUnitBytes\) / kUnitBytes", host)
    assert _int(host, r"size_t G = \(max_units \+ (\d+)\) / (\d+);") == (cc.BATCH_G_UNITS - 1, cc.BATCH_G_UNITS)
    assert _int(host, r"if \(G > (\d+)\) G = (\d+);") == (cc.BATCH_G_CAP, cc.BATCH_G_CAP)
    # pick_groups and the cut, as restated
    assert re.search(r"long long g = c->cus - g_reserved_cus\.load", host) and re.search(r"if \(nunits < g\) g = nunits > 0 \? nunits : 1;", host)
    assert re.search(r"sa\.nunits = \(sa\.body \+ kUnitBytes - 1\) / kUnitBytes;", host)
    # the product's variant requests neither the second buffer early (b_requested stays false: one set of ping-pong exits)
    variant = re.search(r"constexpr int kCrcVariant = ([^;]+);", ker).group(1)
    assert "kVarBothBuffers" not in variant


def test_model_on_hand_worked_geometries():
    # 5 units in one workgroup at phase 9, 15 bytes behind: the head unit, four pipelined groups
    g = cc.geometry(cc.length_for(5, 9, 15), 9, 1, 1)
    assert (g.head, g.tail, g.body, g.nunits, g.tail_lo) == (9, 15, 5 * cc.UNIT, 5, 0)
    assert g.wgs == (cc.Workgroup(5, True, 4, 0, "even >= 4", 0, 5, 0, 1),)
    # the copy pass over 245 units: 1 + 60 * 4 = 241 reduced mid-stream, one group of four behind it
    (w,) = cc.geometry(245 * cc.UNIT, 0, 1, 4).wgs
    assert (w.groups, w.leftover, w.folds, w.deepest) == (61, 0, 1, 241)
    # 7 units over 3 workgroups: 3 + 2 + 2, the first holds the head unit
    g = cc.geometry(7 * cc.UNIT + 3, 0, 3, 1)
    assert [(w.units, w.head_unit, w.groups, w.k_after) for w in g.wgs] == [(3, True, 2, 4), (2, False, 2, 2), (2, False, 2, 0)]
    # a message inside one granule: no body, the tail bytes begin at the phase
    assert cc.cut(5, 3) == (3, 8, 0, 0, 3) and cc.cut(0, 7) == (7, 0, 0, 0, 0)
    assert cc.groups_for(256, 4, 5000) == 252 and cc.groups_for(256, 255, 5000) == 1 and cc.groups_for(256, 0, 3) == 3
    assert cc.groups_for(256, 0, 0) == 1 and cc.groups_for(2000, 0, 5000) == 1024
    assert cc.batch_groups(0) == 1 and cc.batch_groups(1024 * cc.UNIT - 16) == 1 and cc.batch_groups(1024 * cc.UNIT - 15) == 2
    assert cc.batch_groups(1 << 34) == 16
    # the smallest all-0xFF batch whose SR no longer fits 32 bits lies between the mid-stream limit and the deep case
    first = next(b for b in range(1, 4096) if 4080 * b * (b - 1) // 2 >= 1 << 32)
    assert first == 1452 and cc.BATCH_MAX < first <= cc.DEEP_FF_UNITS


def _need(reached, wanted, what, cus):
    for cls in wanted:
        assert cls in reached, "%s: no case reaches %r at %d CUs" % (what, cls, cus)


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_families_reach_every_class(cus):
    read, copy = set(), set()
    for family, build in cc.FAMILIES:
        cases = build(cus)
        assert len({c.name for c in cases}) == len(cases), family
        for c in cases:
            assert 0 <= c.reserved < cus and 0 <= c.phase < 16 and c.n >= 0, c
            geo = cc.case_geometry(c, cus)
            reached = copy if c.copy else read
            if geo.nunits == 0 and c.n > 0:
                reached.add("no units, tail bytes")
            if geo.nunits > 0 and 1 <= geo.head <= 15:
                reached.add("head 1..15 in the piece at offset 0")
            for w in geo.wgs:
                reached.update({("exit", w.exit), ("groups", min(w.groups, 5)), ("leftover", w.leftover), ("folds", min(w.folds, 2)),
                                ("deepest", w.deepest), ("digits", w.digits)})
                if w.head_unit and w.units == 1:
                    reached.add("head unit alone")
                if w.units == 0:
                    reached.add("empty unit range")
    many_G = set()
    many = set()
    for name, idx in cc.many_calls():
        G, geos = cc.many_geometry(idx)
        many_G.add(G)
        for i, geo in zip(idx, geos):
            if G > geo.nunits:
                many.add("G above the message's units")
            if G > 1 and cc.many_messages()[i].n == 0:
                many.add("empty message beside G > 1")
            for w in geo.wgs:                                  # the many-message pass is the read-only kernel
                read.update({("exit", w.exit), ("folds", min(w.folds, 2)), ("deepest", w.deepest), ("digits", w.digits)})
                if w.units == 0:
                    read.add("empty unit range")
                if w.head_unit and w.units == 1:
                    read.add("head unit alone")
    _need(read, ["head unit alone", "empty unit range", ("deepest", 240), ("digits", 1), ("digits", 2)]
          + [("exit", e) for e in ("groups 0", "groups 1", "groups 2", "odd >= 3", "even >= 4")]
          + [("folds", f) for f in (0, 1, 2)], "read-only pass", cus)
    _need(copy, ["no units, tail bytes", "head 1..15 in the piece at offset 0", ("deepest", 240), ("deepest", 241)]
          + [("groups", g) for g in range(6)] + [("leftover", v) for v in range(4)] + [("folds", f) for f in (0, 1, 2)]
          + [("exit", e) for e in ("groups 0", "groups 1", "groups 2", "odd >= 3", "even >= 4")], "copy pass", cus)
    _need(many_G, [1, 2, 16], "many-message G", cus)
    _need(many, ["G above the message's units", "empty message beside G > 1"], "many-message pass", cus)


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_family_sizes_are_what_the_names_say(cus):
    G = max(cus - 4, 1)
    big = [c for c in cc.sweep_cases(cus) if "second unit_pow digit" in c.name]
    assert len(big) == 2
    for c in big:
        geo = cc.case_geometry(c, cus)
        assert geo.G == G and geo.wgs[0].k_after >= 1024 and geo.wgs[0].digits == 2 and geo.wgs[-1].digits == 1, cc.describe(geo)
        assert cc.geometry(c.n - cc.UNIT, c.phase, G, 1).wgs[0].k_after < 1024       # and no unit to spare
        assert c.n + c.phase <= cc.POOL_BYTES
    for c in cc.one_workgroup_read_cases(cus) + cc.one_workgroup_copy_cases(cus):
        geo = cc.case_geometry(c, cus)
        assert geo.G == 1 and len(geo.wgs) == 1, (c.name, cc.describe(geo))
        assert " units " not in c.name or " units %d " % geo.nunits in c.name, (c.name, cc.describe(geo))
    deep = [cc.case_geometry(c, cus) for c in cc.one_workgroup_read_cases(cus) if c.fill == ("ff",) and "units %d " % cc.DEEP_FF_UNITS in c.name]
    assert len(deep) == 6 and all(g.wgs[0].units == cc.DEEP_FF_UNITS and g.wgs[0].folds == 6 and g.wgs[0].deepest == 240 for g in deep)
    for c in cc.impulse_cases(cus):
        geo = cc.case_geometry(c, cus)
        assert (geo.nunits, geo.tail, geo.head) == (6, 15, 0) and geo.G in (1, 3)
    msgs = cc.many_messages()
    assert len({m.phase for m in msgs}) == len(msgs) and all(m.offset % 16 == m.phase for m in msgs)
    assert all(a.offset + a.n <= b.offset for a, b in zip(msgs, msgs[1:]))
    assert [cc.cut(m.n, m.phase)[3] for m in msgs] == [0, 0, 1, 1, 1024, 1025, 16 * 1024 + 1]       # 15 bytes at phase 1: one masked piece
    assert cc.many_random_bytes()[0] <= cc.POOL_BYTES
    assert [cc.many_geometry(idx)[0] for _, idx in cc.many_calls()] == [16, 2, 1]
    one = cc.geometry(cc.DESCRIPTOR_BYTES, 0, 1, cc.ROWS).wgs[0]
    assert (one.units, one.folds, one.deepest) == (512, 2, 240)


def test_references_agree(oracle, refcrc):
    """zlib, the oracle and the closed form on every distinct message of the 256-CU and 8-CU cases (all are below 32 MiB)"""
    seen = set()
    for cus in (256, 8):
        for family, build in cc.FAMILIES:
            for c in build(cus):
                key = (c.fill, c.n, c.phase if c.fill[0] == "random" else 0, c.adler_seed, c.crc_seed)
                if key in seen:
                    continue
                seen.add(key)
                assert c.n < (32 << 20)
                data = cc.message(c)
                assert data.size == c.n
                ptr = data.ctypes.data if c.n else cc.pool().ctypes.data       # a null buffer asks for the initial value
                want = (zlib.adler32(data, c.adler_seed), zlib.crc32(data, c.crc_seed))
                assert cc.reference(c) == want, c.name
                assert (oracle.oracle_adler32(c.adler_seed, ptr, c.n), oracle.oracle_crc32_braid(c.crc_seed, ptr, c.n)) == want, c.name
                if refcrc is not None and c.n:
                    assert refcrc(c.crc_seed, ptr, c.n) == want[1], c.name
                if c.fill[0] == "ff":
                    assert cc.adler_constant(0xFF, c.n, c.adler_seed) == want[0], c.name
    for m in cc.many_messages()[:-1]:
        data = cc.pool()[m.offset:m.offset + m.n]
        ptr = data.ctypes.data if m.n else cc.pool().ctypes.data
        assert cc.many_reference(m) == (oracle.oracle_adler32(m.adler_seed, ptr, m.n), oracle.oracle_crc32_braid(m.crc_seed, ptr, m.n)), m.name


def test_closed_form_on_the_long_message():
    """above 32 MiB: the closed form against zlib once, on the 256 MiB + 16 KiB of 0xFF of the many-message family"""
    m = cc.many_messages()[-1]
    assert m.fill == "ff" and m.n > (256 << 20)
    assert cc.many_reference(m)[0] == zlib.adler32(b"\xff" * m.n, m.adler_seed)
    for v, n, seed in ((0, 5, 1), (0x80, 70000, 0xfff0fff0), (0xFF, 65521 * 3 + 1, 0xffffffff), (7, 0, 0x12345678)):
        assert cc.adler_constant(v, n, seed) == zlib.adler32(bytes([v]) * n, seed)


def test_existing_sizes_reach_no_fold_and_no_copy_pipeline():
    """what test_gpu_checksums.py's inputs do on a 256-CU device, by the same model: the reason for the crafted cases"""
    cus = 256
    n = 16384 * 520 + 123                                       # test_dev_structured_inputs: all-zero, all-0xFF, ramp
    geo = cc.geometry(n, 0, cc.groups_for(cus, 0, cc.cut(n, 0)[3]), cc.ROWS)
    assert geo.nunits == 521 and geo.G == cus
    assert {w.units for w in geo.wgs} == {2, 3} and max(w.groups for w in geo.wgs) == 3
    assert all(w.folds == 0 and w.deepest <= 3 and w.digits == 1 for w in geo.wgs), cc.describe(geo)
    for n, phase in ((16384 * 70 + 900, 9), (16384 * 64, 0), (40000, 15), (16384 * 520 + 123, 0)):      # test_fold_copy_dev's, and the above
        geo = cc.geometry(n, phase, cc.groups_for(cus, 0, cc.cut(n, phase)[3]), cc.ROWS_COPY)
        assert all(w.groups == 0 and w.folds == 0 for w in geo.wgs), cc.describe(geo)
    n = 16 << 20                                                # the host slots' staging chunk through the copy kernel
    geo = cc.geometry(n, 0, cc.groups_for(cus, 0, cc.cut(n, 0)[3]), cc.ROWS_COPY)
    assert {w.groups for w in geo.wgs} <= {0, 1} and all(w.folds == 0 for w in geo.wgs), cc.describe(geo)
