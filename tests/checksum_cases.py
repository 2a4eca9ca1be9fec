"""Crafted messages for the streaming checksum pass (test infrastructure, no GPU and no torch): a model of the pass's geometry,
the case families built on it, and references that owe nothing to the code under test.

checksum_kernel.h's stream_body decides what it does from the number of 16 KiB units its workgroup owns, not from the message's
length: with one workgroup per CU a message needs hundreds of MiB before a workgroup pipelines, folds its Adler sums mid-stream or
weighs its CRC over more than 1023 units.  zng_rocm_reserve_cus(CUs - G) runs the single-message pass in G workgroups, so the
same control flow is reached with a few hundred KiB.  The model restates
  launch_checksum's cut            (checksum.hip: a0, tail_base, body, nunits, head, tail),
  pick_groups                      (checksum.hip: workgroups of one message),
  zng_rocm_checksums_dev's G rule  (checksum.hip: workgroups of every message of a many-message call),
  stream_body's q / r split, its head unit, pipelined groups, ping-pong exits, leftover loop and Adler batches,
and tests/test_checksum_cases_cpu.py holds its constants to the headers and proves that the families below reach every class of
that control flow for several CU counts.

A case: name, which (1 Adler-32, 2 CRC-32, 3 both), copy (fold_copy_dev), reserved (the argument of zng_rocm_reserve_cus), n and
phase (the message's length and its address mod 16), fill, the two seeds, and for copies dst_shift (the destination lies at the
same phase, that many bytes further on).  Fills: ("random",) the bytes at `phase` of one seeded pool, ("ff",), ("ff_hole", at) 0xFF
with one 0x00, ("ramp",) i % 251, ("impulse", at, value) zeros with one byte."""
import collections
import functools
import zlib

import numpy as np

UNIT = 16384                 # kUnitBytes: what one workgroup consumes per step
PIECE = 16                   # kPieceBytes: one dwordx4 per lane
LANES = 1024                 # kWgThreads
BATCH_MAX = 240              # units a lane sums before the mid-stream Adler reduction
ROWS, ROWS_COPY = 1, 4       # kRowsPerBuffer, kRowsPerBufferCopy: units per register buffer (UNROLL)
MAX_GROUPS = 1024            # kMaxGroups
BATCH_G_CAP = 16             # zng_rocm_checksums_dev: workgroups per message at most
BATCH_G_UNITS = 1024         # ... one per this many units
BASE = 65521                 # kAdlerBase

SEEDS = ((1, 0), (0xffffffff, 0xffffffff), (0xfff0fff0, 0x00000001))

Case = collections.namedtuple("Case", "name which copy reserved n phase fill adler_seed crc_seed dst_shift", defaults=(0,))
Workgroup = collections.namedtuple("Workgroup", "units head_unit groups leftover exit folds deepest k_after digits")
Geometry = collections.namedtuple("Geometry", "head tail body nunits tail_lo G unroll wgs")


# ---- the model -----------------------------------------------------------------------------------------------------------------
def cut(n, phase):
    """launch_checksum's cut of [phase, phase + n) on 16-byte granules, addresses relative to the granule of the first byte:
    (head, tail, body, nunits, tail_lo)"""
    a0, tail_base = 0, (phase + n) & ~15
    body = tail_base - a0
    nunits = (body + UNIT - 1) // UNIT
    head, tail = phase, phase + n - tail_base
    tail_lo = head if body == 0 else 0
    if n == 0:
        tail_lo = tail = 0
    return head, tail, body, nunits, tail_lo


def groups_for(cus, reserved, nunits):
    """pick_groups: workgroups of a single-message pass"""
    g = cus - reserved
    g = max(g, 1)
    g = min(g, MAX_GROUPS)
    if nunits < g:
        g = nunits if nunits > 0 else 1
    return g


def batch_groups(max_len):
    """zng_rocm_checksums_dev: workgroups of EVERY message of a call whose longest message has max_len bytes"""
    max_units = max(1, (max_len + 15 + UNIT) // UNIT)
    return min((max_units + BATCH_G_UNITS - 1) // BATCH_G_UNITS, BATCH_G_CAP)


def exit_class(groups):
    """which way a workgroup leaves the ping-pong loop"""
    if groups <= 2:
        return "groups %d" % groups
    return "odd >= 3" if groups & 1 else "even >= 4"


def geometry(n, phase, G_asked, unroll):
    """what each of G_asked workgroups of stream_body does with the message"""
    head, tail, body, nunits, tail_lo = cut(n, phase)
    q, r = divmod(nunits, G_asked)
    wgs = []
    for g in range(G_asked):
        u_lo = g * q + min(g, r)
        u_hi = u_lo + q + (1 if g < r else 0)
        units = u_hi - u_lo
        head_unit = units > 0 and u_lo == 0
        groups = (units - head_unit) // unroll
        leftover = units - head_unit - groups * unroll
        batch, folds, deepest = int(head_unit), 0, 0
        for _ in range(groups):                       # retire(): the mid-stream reduction
            batch += unroll
            if batch >= BATCH_MAX:
                deepest, folds, batch = max(deepest, batch), folds + 1, 0
        batch += leftover
        deepest = max(deepest, batch)                 # the reduction behind the last unit
        k_after = nunits - u_hi
        wgs.append(Workgroup(units, bool(head_unit), groups, leftover, exit_class(groups), folds, deepest, k_after,
                             2 if k_after >= 1024 else 1))
    return Geometry(head, tail, body, nunits, tail_lo, G_asked, unroll, tuple(wgs))


def case_geometry(case, cus):
    """the single-message pass of a case; no workgroups where the streaming kernel is not launched (a body of no units)"""
    nunits = cut(case.n, case.phase)[3]
    geo = geometry(case.n, case.phase, groups_for(cus, case.reserved, nunits), ROWS_COPY if case.copy else ROWS)
    return geo if nunits else geo._replace(wgs=())


def describe(geo):
    """the geometry in one line, for assertion messages"""
    kinds = collections.Counter((w.units, w.head_unit, w.groups, w.leftover, w.folds, w.deepest, w.digits) for w in geo.wgs)
    return "head %d tail %d units %d G %d unroll %d: %s" % (
        geo.head, geo.tail, geo.nunits, geo.G, geo.unroll,
        "; ".join("%dx(units %d head %d groups %d left %d folds %d deepest %d digits %d)" % ((c,) + k) for k, c in sorted(kinds.items())))


def length_for(units, phase, tail, partial=0):
    """the length that makes a message at `phase` `units` units long with `tail` bytes behind them; partial: 16-byte pieces
    missing from the first unit"""
    assert units >= 1 and 0 <= tail < 16 and 0 <= partial < LANES
    return units * UNIT - partial * PIECE - phase + tail


# ---- the bytes -----------------------------------------------------------------------------------------------------------------
POOL_UNITS = 2080            # the random messages of the many-message family, back to back: 1 + 1024 + 1025 units and change
POOL_BYTES = POOL_UNITS * UNIT + 64


@functools.lru_cache(maxsize=None)
def pool():
    """the random bytes every ("random",) case reads at its phase"""
    return np.random.default_rng(0xC5EC).integers(0, 256, size=POOL_BYTES, dtype=np.uint8)


def message(case):
    """the case's bytes (uint8 array of n; a view for random fills)"""
    kind = case.fill[0]
    if kind == "random":
        assert case.phase + case.n <= POOL_BYTES
        return pool()[case.phase:case.phase + case.n]
    if kind == "ramp":
        return (np.arange(case.n) % 251).astype(np.uint8)
    arr = np.full(case.n, 0xFF if kind in ("ff", "ff_hole") else 0, dtype=np.uint8)
    if kind == "ff_hole":
        arr[case.fill[1]] = 0
    elif kind == "impulse":
        arr[case.fill[1]] = case.fill[2]
    else:
        assert kind == "ff", kind
    return arr


# ---- the references ------------------------------------------------------------------------------------------------------------
def adler_constant(v, n, seed):
    """Adler-32 of n bytes of value v behind `seed`, in exact integers: the seed's halves are masked, not reduced
    (adler32_c.c:16-17), A = s1 + v n, B = s2 + n s1 + v n (n + 1) / 2, both mod 65521"""
    s1, s2 = seed & 0xffff, (seed >> 16) & 0xffff
    a = (s1 + v * n) % BASE
    b = (s2 + n * s1 + v * n * (n + 1) // 2) % BASE
    return (b << 16) | a


@functools.lru_cache(maxsize=None)
def _ff_bytes(n):
    return b"\xff" * n


@functools.lru_cache(maxsize=None)
def _crc_ff(n, seed):
    return zlib.crc32(_ff_bytes(n), seed)


_refs = {}


def reference(case):
    """(adler32, crc32) of the case from CPython's zlib; the Adler-32 of constant fills from the closed form"""
    key = (case.fill, case.n, case.phase if case.fill[0] == "random" else 0, case.adler_seed, case.crc_seed)
    if key not in _refs:
        if case.fill[0] == "ff":
            _refs[key] = (adler_constant(0xFF, case.n, case.adler_seed), _crc_ff(case.n, case.crc_seed))
        else:
            data = message(case)
            _refs[key] = (zlib.adler32(data, case.adler_seed), zlib.crc32(data, case.crc_seed))
    return _refs[key]


# ---- the families --------------------------------------------------------------------------------------------------------------
ONE_WG_UNITS = (1, 2, 3, 4, 5, 6, 239, 240, 241, 242, 479, 480, 481)
ONE_WG_FF_UNITS = (240, 241, 481)
DEEP_FF_UNITS = 1536         # 4080 B (B - 1) / 2 >= 2^32 from B = 1452 units of 0xFF: one unreduced batch overflows SR
# the copy pass: groups 0..6 with leftovers 0 and 1 (the first 11), leftovers 2 and 3 at groups 0 and 1 (3, 4, 7, 8), batches of
# 240 and 241, no, one and two mid-stream reductions
ONE_WG_COPY_UNITS = (1, 2, 5, 6, 9, 10, 13, 14, 17, 21, 25, 240, 241, 244, 245, 481, 3, 4, 7, 8)
ONE_WG_COPY_FF_UNITS = (241, 481)


def one_workgroup_read_cases(cus):
    """the read-only pass (one unit per register buffer) in ONE workgroup"""
    out, res, i = [], cus - 1, 0
    for units in ONE_WG_UNITS:
        for phase in (0, 9):
            for tail in (0, 15):
                for which in (1, 2, 3):
                    sa, sc = SEEDS[i % 3]
                    i += 1
                    out.append(Case("read1 random units %d phase %d tail %d which %d" % (units, phase, tail, which), which, False, res,
                                    length_for(units, phase, tail), phase, ("random",), sa, sc))
    for units in ONE_WG_FF_UNITS:
        for phase in (0, 9):
            for tail in (0, 15):
                for sa, sc in SEEDS:
                    out.append(Case("read1 ff units %d phase %d tail %d seeds %#x %#x" % (units, phase, tail, sa, sc), 3, False, res,
                                    length_for(units, phase, tail), phase, ("ff",), sa, sc))
    for phase, tail in ((0, 0), (9, 15)):
        for which, (sa, sc) in zip((3, 1, 3), SEEDS):
            out.append(Case("read1 ff units %d phase %d tail %d which %d seeds %#x %#x" % (DEEP_FF_UNITS, phase, tail, which, sa, sc),
                            which, False, res, length_for(DEEP_FF_UNITS, phase, tail), phase, ("ff",), sa, sc))
    # maximal bytes with one hole, and the ramp, through a batch of 240 and the unit behind it
    n = length_for(241, 9, 15)
    for at in (0, 7, 120 * UNIT + 16 * 63 + 15, 239 * UNIT + 5, 240 * UNIT - 9, n - 1):
        out.append(Case("read1 ff_hole at %d" % at, 3, False, res, n, 9, ("ff_hole", at), *SEEDS[1]))
    for phase in (0, 9):
        out.append(Case("read1 ramp phase %d" % phase, 3, False, res, length_for(241, phase, 15), phase, ("ramp",), *SEEDS[2]))
    return out


def one_workgroup_copy_cases(cus):
    """the copying pass (four units per register buffer) in ONE workgroup"""
    out, res, i = [], cus - 1, 0
    for units in ONE_WG_COPY_UNITS:
        for phase in (0, 1, 15):
            for which in (1, 2, 3):
                sa, sc = SEEDS[i % 3]
                tail, shift = (0, 15, 7)[(i // 3) % 3], (16, 32)[i % 2]
                i += 1
                out.append(Case("copy1 random units %d phase %d tail %d which %d" % (units, phase, tail, which), which, True, res,
                                length_for(units, phase, tail), phase, ("random",), sa, sc, shift))
    for units in ONE_WG_COPY_FF_UNITS:
        for phase in (0, 1, 15):
            for which, (sa, sc) in zip((1, 2, 3), SEEDS):
                out.append(Case("copy1 ff units %d phase %d which %d" % (units, phase, which), which, True, res,
                                length_for(units, phase, 15), phase, ("ff",), sa, sc, 16 if phase else 32))
    return out


def copy_edge_lengths(phase):
    """0..48, and the lengths that put the message's end, or its length, one byte either side of the first unit's end"""
    edge = {16383, 16384, 16385}
    return sorted(set(range(49)) | edge | {n + phase for n in edge} | {n - phase for n in edge})


def copy_edge_cases(cus):
    """short copies at every phase, every CU in use: the head mask, the tail bytes, a body of no units"""
    out = []
    for phase in range(16):
        for n in copy_edge_lengths(phase):
            for which in (1, 2, 3):
                sa, sc = SEEDS[(n + phase + which) % 3]
                out.append(Case("copy edge n %d phase %d which %d" % (n, phase, which), which, True, 0, n, phase, ("random",), sa, sc, 64))
    return out


def sweep_groups(cus):
    return sorted({g for g in (1, 2, 3, 7, cus - 4, cus - 1, cus) if 1 <= g <= cus})


def second_digit_units(G):
    """the fewest units at which the first of G workgroups has 1024 or more units behind its own"""
    nunits = 1025
    while nunits - (nunits + G - 1) // G < 1024:
        nunits += 1
    return nunits


def sweep_cases(cus):
    """workgroup counts other than min(CUs, units), around the unit counts where the q / r split changes; the first unit partial"""
    out, i = [], 0
    for G in sweep_groups(cus):
        for units in sorted({u for u in (G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G + 2) if u > 0}):
            for phase in (0, 5):
                for which in (3, 2):
                    sa, sc = SEEDS[i % 3]
                    i += 1
                    out.append(Case("sweep G %d units %d phase %d which %d" % (G, units, phase, which), which, False, cus - G,
                                    length_for(units, phase, 7, partial=613), phase, ("random",), sa, sc))
    G = max(cus - 4, 1)
    units = second_digit_units(G)
    for which, phase in ((3, 5), (2, 0)):
        out.append(Case("sweep G %d units %d phase %d which %d (second unit_pow digit)" % (G, units, phase, which), which, False,
                        cus - G, length_for(units, phase, 7, partial=613), phase, ("random",), *SEEDS[which % 3]))
    return out


IMPULSE_UNITS = 6


def impulse_positions():
    """(what, offset) of the single 0x80 byte in a message of 6 units and a 15-byte tail at phase 0"""
    n = length_for(IMPULSE_UNITS, 0, 15)
    pos = [("first byte of the message", 0), ("last byte of the message", n - 1), ("first byte of the tail", IMPULSE_UNITS * UNIT)]
    for unit in (0, IMPULSE_UNITS - 1):
        for lane in (0, 63, 64, 1023):
            at = unit * UNIT + lane * PIECE
            pos.append(("first byte of lane %d of unit %d" % (lane, unit), at))
            pos.append(("last byte of lane %d of unit %d" % (lane, unit), at + PIECE - 1))
    seen, out = set(), []
    for what, at in pos:
        if at not in seen:
            seen.add(at)
            out.append((what, at))
    return out


def impulse_cases(cus):
    """one 0x80 among zeros: a wrong CRC weight shows in the case that names its lane, unit or workgroup"""
    out, n = [], length_for(IMPULSE_UNITS, 0, 15)
    for G in (1, 3):
        if G > cus:
            continue
        for what, at in impulse_positions():
            for which in (2, 3):
                out.append(Case("impulse G %d which %d: %s (offset %d)" % (G, which, what, at), which, False, cus - G, n, 0,
                                ("impulse", at, 0x80), 1, 0))
    return out


# many messages in one call: the random ones lie in the pool in this order, each at its own phase; the long one is constant fill
# behind them, built on the device
MANY_BIG_UNITS = 16 * 1024 + 1
Message = collections.namedtuple("Message", "name n phase fill offset adler_seed crc_seed")


def many_messages():
    """the messages of the many-message family with their offsets in one buffer (each offset's low four bits are the phase); the
    last one is the 256 MiB + 16 KiB of 0xFF that takes G to its cap"""
    spec = [("empty", 0, 3, "random"), ("1 byte", 1, 6, "random"), ("15 bytes", 15, 1, "random"),
            ("1 unit", length_for(1, 4, 4), 4, "random"), ("1024 units", length_for(1024, 11, 2), 11, "random"),
            ("1025 units", length_for(1025, 13, 9), 13, "random"), ("%d units of 0xFF" % MANY_BIG_UNITS, length_for(MANY_BIG_UNITS, 5, 11), 5, "ff")]
    out, at = [], 0
    for i, (name, n, phase, fill) in enumerate(spec):
        at = (at + 15) // 16 * 16 + 16 + phase
        sa, sc = SEEDS[i % 3]
        out.append(Message(name, n, phase, fill, at, sa, sc))
        at += n
    return out


def many_calls():
    """(name, indices into many_messages()) of the family's calls: G at its cap, G = 2 without the long message, G = 1"""
    return (("all", (0, 1, 2, 3, 4, 5, 6)), ("without the long one", (0, 1, 2, 3, 4, 5)), ("short ones", (0, 1, 2, 3)))


def many_random_bytes():
    """bytes of the buffer in front of the long message (the pool), and the buffer's whole length"""
    msgs = many_messages()
    return msgs[-1].offset - msgs[-1].phase, msgs[-1].offset + msgs[-1].n + 64


def many_reference(msg):
    if msg.fill == "ff":
        return adler_constant(0xFF, msg.n, msg.adler_seed), _crc_ff(msg.n, msg.crc_seed)
    data = pool()[msg.offset:msg.offset + msg.n]
    return zlib.adler32(data, msg.adler_seed), zlib.crc32(data, msg.crc_seed)


def many_geometry(indices):
    """G of a call and the geometry of each of its messages"""
    msgs = [many_messages()[i] for i in indices]
    G = batch_groups(max(m.n for m in msgs))
    return G, [geometry(m.n, m.phase, G, ROWS) for m in msgs]


# device-built descriptors (fill_check_descriptor): one workgroup whatever the length
DESCRIPTOR_BYTES = 8 << 20

FAMILIES = (("one workgroup, read-only", one_workgroup_read_cases), ("one workgroup, copy", one_workgroup_copy_cases),
            ("copy edges", copy_edge_cases), ("workgroup-count sweep", sweep_cases), ("CRC impulses", impulse_cases))
