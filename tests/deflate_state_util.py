"""Builders for deflate_state-shaped test inputs (host numpy + oracle view, device view)."""
import ctypes as C

import numpy as np

import oracle_lib

W_BITS = 15
W_SIZE = 1 << W_BITS
PAD = 512   # readable bytes past 2*w_size (the reference pads the window for compare overreads)

LEVEL_PARAMS = {   # deflate.c:142-168 configuration_table {good, lazy, nice, chain}
    1: (0, 0, 0, 0), 2: (4, 4, 8, 4), 3: (4, 6, 16, 6), 4: (4, 12, 32, 24), 5: (8, 16, 32, 32),
    6: (8, 16, 128, 128), 7: (8, 32, 128, 256), 8: (32, 128, 258, 1024), 9: (32, 258, 258, 4096),
}


def texty(n, seed, alphabet=24, words=400):
    """compressible pseudo-text: Zipf-ish draws from a small dictionary of random words"""
    rng = np.random.default_rng(seed)
    vocab = [bytes(rng.integers(97, 97 + alphabet, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(words)]
    ranks = rng.zipf(1.3, size=n // 3 + 16) % words
    out = bytearray()
    for r in ranks:
        out += vocab[r] + b" "
        if len(out) >= n:
            break
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


class HostState:
    """numpy-backed window/prev/head + the oracle's struct over them"""

    def __init__(self, data, w_size=W_SIZE):
        self.w_size = w_size
        self.window = np.zeros(2 * w_size + PAD, dtype=np.uint8)
        n = min(len(data), 2 * w_size)
        self.window[:n] = data[:n]
        self.filled = n
        self.prev = np.zeros(w_size, dtype=np.uint16)
        self.head = np.zeros(65536, dtype=np.uint16)
        self.st = oracle_lib.DeflateState()
        self.st.w_size = w_size
        self.st.w_bits = int(np.log2(w_size))
        self.st.w_mask = w_size - 1
        self.st.window_size = 2 * w_size
        self.st.window = self.window.ctypes.data
        self.st.prev = self.prev.ctypes.data
        self.st.head = self.head.ctypes.data

    def set_level(self, level):
        good, lazy, nice, chain = LEVEL_PARAMS[level]
        self.st.level = level
        self.st.good_match = good
        self.st.nice_match = nice
        self.st.max_chain_length = chain

    def ref(self):
        return C.byref(self.st)


# ---- in-contract states: tables as fill_window / deflate leave them -------------------------------------------
MIN_LOOKAHEAD = 262
WINDOW_SIZES = (512, 4096, 32768)
LOOKAHEADS = (1, 2, 3, 6, 258, 259, 262)
DATA_KINDS = ("texty3", "texty24", "zeros", "run1", "run2", "run3", "run4")


def stream_data(kind, n, seed=0):
    """n bytes of one of DATA_KINDS: texty with alphabet 3 / 24, all zero, or a run of period 1..4"""
    if kind == "texty3":
        return texty(n, 7000 + seed, alphabet=3, words=40)
    if kind == "texty24":
        return texty(n, 7100 + seed, alphabet=24, words=400)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    period = int(kind[3:])
    unit = np.frombuffer(b"qrst"[:period], dtype=np.uint8)
    return np.tile(unit, n // period + 1)[:n].copy()


def hash_at(window, pos, roll):
    """head[] slot of the string at `pos`: multiplicative hash of 4 bytes, or the rolling key of 3 (level 9)"""
    if roll:
        return ((int(window[pos]) << 10) ^ (int(window[pos + 1]) << 5) ^ int(window[pos + 2])) & 32767
    return ((int.from_bytes(window[pos:pos + 4].tobytes(), "little") * 2654435761) & 0xffffffff) >> 16


def phase_strstarts(w_size, per_phase, rng):
    """strstart values of the three phases, each ascending:
    0: below MAX_DIST (limit == 0), w_size - MIN_LOOKAHEAD itself included;
    1: in (w_size, 2*w_size - 262] before a slide (limit > 0), window_size - MIN_LOOKAHEAD itself included;
    2: after one slide at window_size - MIN_LOOKAHEAD, up to that value again (limit 0 and > 0)."""
    max_dist, top = w_size - MIN_LOOKAHEAD, 2 * w_size - MIN_LOOKAHEAD
    p0 = sorted(set(rng.integers(4, max_dist, size=per_phase - 1).tolist()) | {max_dist})
    p1 = sorted(set(rng.integers(w_size + 1, top, size=per_phase - 1).tolist()) | {top})
    p2 = sorted(set(rng.integers(max_dist + 1, top, size=per_phase - 1).tolist()) | {top})
    return p0, p1, p2


def _snapshot(hs, strstart, phase):
    """a HostState of its own head/prev copies that shares hs's window"""
    snap = HostState(np.zeros(0, dtype=np.uint8), w_size=hs.w_size)
    snap.window = hs.window
    snap.st.window = hs.window.ctypes.data
    snap.head[:] = hs.head
    snap.prev[:] = hs.prev
    snap.st.ins_h = hs.st.ins_h
    snap.st.strstart = strstart
    snap.strstart, snap.phase = strstart, phase
    return snap


def in_contract_snapshots(lib, prefix, kind, w_size, roll, per_phase=8, seed=0):
    """State snapshots made the way fill_window and deflate make them, by `lib`'s <prefix>insert_string(_roll) and
    <prefix>slide_hash: the window is filled, positions 0 .. strstart-1 are inserted with the hash family (roll: the
    rolling hash of level 9), so no table entry is >= strstart; after phase 1 the upper half moves down, slide_hash
    runs and insertion goes on.  Returns a list of HostState, each with .strstart and .phase, tables of its own and
    the window of its phase shared."""
    insert = getattr(lib, prefix + ("insert_string_roll" if roll else "insert_string"))
    slide = getattr(lib, prefix + "slide_hash")
    data = stream_data(kind, 3 * w_size, seed)
    rng = np.random.default_rng(w_size + 17 * seed + (1 if roll else 0))
    p0, p1, p2 = phase_strstarts(w_size, per_phase, rng)
    hs = HostState(data, w_size=w_size)
    snaps, pos = [], 0
    for phase, starts in ((0, p0), (1, p1)):
        for s in starts:
            insert(hs.ref(), pos, s - pos)
            pos = s
            snaps.append(_snapshot(hs, s, phase))
    assert pos == 2 * w_size - MIN_LOOKAHEAD
    after = HostState(np.concatenate([data[w_size:2 * w_size], data[2 * w_size:3 * w_size]]), w_size=w_size)
    after.head[:] = hs.head
    after.prev[:] = hs.prev
    after.st.ins_h = hs.st.ins_h
    slide(after.ref())
    pos -= w_size
    for s in p2:
        insert(after.ref(), pos, s - pos)
        pos = s
        snaps.append(_snapshot(after, s, 2))
    return snaps


def cur_match_candidates(snap, kind, roll):
    """(cur_match, in_contract) pairs for a snapshot: head[hash] of the string at strstart when deflate would search it
    (non-zero, within MAX_DIST), strstart - 1 on runs, and one value >= strstart"""
    s = snap.strstart
    out = []
    cur = int(snap.head[hash_at(snap.window, s, roll)])
    assert cur < s
    if cur != 0 and s - cur <= snap.w_size - MIN_LOOKAHEAD:
        out.append(cur)
    if kind in ("zeros", "run1", "run2", "run3", "run4") and s - 1 not in out:
        out.append(s - 1)
    out.append(s if s & 1 else s + 7)
    return out


def match_param_sets(level):
    """every (prev_length, lookahead) pair of the level: {0, 2, 3, 4, good-1, good, nice-1, nice, 257, 258} x LOOKAHEADS
    (level 1 has no matcher parameters of its own in the table and takes level 2's)"""
    good, _, nice, _ = LEVEL_PARAMS[max(level, 2)]
    return [(p, la) for p in sorted({0, 2, 3, 4, good - 1, good, nice - 1, nice, 257, 258}) for la in LOOKAHEADS]


def set_match_level(hs, level):
    """matcher parameters of `level` in hs.st (level 1: level 2's parameters with s->level 1)"""
    hs.set_level(max(level, 2))
    hs.st.level = level


def match_call(fn, hs, cur, prev_length, lookahead):
    """one longest_match(_slow) call of `fn` on hs at hs.strstart: (length, match_start afterwards)"""
    st = hs.st
    st.strstart, st.prev_length, st.lookahead, st.match_start = hs.strstart, prev_length, lookahead, 0x123456
    return fn(hs.ref(), cur), st.match_start


# ---- the states of the two older GPU match tests (tables filled to the end of the slab, queries anywhere) ------
def shared_slab_cases(lib, prefix, level):
    """test_gpu_deflate_prims.test_longest_match's state and queries: (hs, [(strstart, cur, prev_length, lookahead)])"""
    hs = HostState(texty(64000, 100 + level, alphabet=5, words=50))
    hs.set_level(level if level > 1 else 2)
    hs.st.level = level
    getattr(lib, prefix + "insert_string")(hs.ref(), 0, 63000)
    rng = np.random.default_rng(level)
    cases = []
    for strstart in rng.integers(300, 62000, size=400).tolist():
        cur = int(hs.prev[strstart & hs.st.w_mask])
        if cur == 0 or cur >= strstart or strstart - cur > W_SIZE - 262:
            continue
        for prev_length, lookahead in ((0, 400), (3, 400), (12, 400), (0, 6), (5, 262)):
            cases.append((strstart, cur, prev_length, lookahead))
    return hs, cases


def shared_slab_cases_slow(lib, prefix, level):
    """test_gpu_match_slow.test_longest_match_slow's state and queries"""
    hs = HostState(texty(32000, 500 + level, alphabet=5, words=50))
    hs.set_level(level)
    getattr(lib, prefix + ("insert_string_roll" if level == 9 else "insert_string"))(hs.ref(), 0, 31700)
    rng = np.random.default_rng(level)
    cases = []
    for strstart in rng.integers(300, 31000, size=700).tolist():
        cur = int(hs.prev[strstart & hs.st.w_mask])
        if cur == 0 or cur >= strstart or strstart - cur > W_SIZE - 262:
            continue
        for prev_length, lookahead in ((0, 400), (3, 400), (5, 400), (12, 400), (30, 400), (4, 7), (6, 262)):
            cases.append((strstart, cur, prev_length, lookahead))
    return hs, cases


# ---- chains that end exactly at `limit` -------------------------------------------------------------------
LIMIT_EDGE_MATCH = 40


def limit_edge_state(lib, prefix, w_size, roll, at_zero, probe_miss):
    """An in-contract state whose chain for the string at strstart is  strstart-3 -> [m2 ->] q  with q == limit exactly
    (at_zero: q == limit == 0, else limit > 0).  strstart-3 matches 4 bytes (and ends beyond strstart, so the slow
    matcher does not re-anchor), m2 (only with probe_miss) shares those 4 bytes and fails the byte-pair probe, and q
    matches LIMIT_EDGE_MATCH bytes.  match_tpl.h stops a chain at `cur_match <= limit`, so the answer is (4, strstart-3);
    a matcher that steps on `>= limit` answers LIMIT_EDGE_MATCH, from the probe loop's step with probe_miss and from
    the step after a compare without.  Returns a HostState with .strstart, .phase and .cur (the chain head)."""
    max_dist = w_size - MIN_LOOKAHEAD
    s = max_dist - 7 if at_zero else w_size + 100
    q = 0 if at_zero else s - max_dist
    x = np.frombuffer(b"abcaz" + bytes(range(32, 32 + LIMIT_EDGE_MATCH - 5)), dtype=np.uint8)
    want_chain = [s - 3] + ([q + 60] if probe_miss else []) + [q]
    for attempt in range(16):               # a filler string may hash into this chain: take the first filler where none does
        rng = np.random.default_rng(16 * (3 * w_size + 2 * at_zero + probe_miss) + attempt)
        data = rng.integers(128, 256, size=2 * w_size, dtype=np.uint8)      # filler shares no byte with the strings
        data[q:q + x.size] = x
        data[s:s + x.size] = x
        data[s + x.size] = 1                                                # the two copies end here
        data[s - 3:s] = x[:3]
        if probe_miss:
            data[q + 60:q + 65] = np.frombuffer(b"abcaQ", dtype=np.uint8)
        hs = HostState(data, w_size=w_size)
        getattr(lib, prefix + ("insert_string_roll" if roll else "insert_string"))(hs.ref(), 0, s)
        snap = _snapshot(hs, s, 1 - at_zero)
        snap.cur = int(hs.head[hash_at(hs.window, s, roll)])
        chain = [snap.cur]
        while chain[-1] > q and len(chain) < 8:
            chain.append(int(hs.prev[chain[-1] & hs.st.w_mask]))
        if chain == want_chain:
            return snap
    raise AssertionError("no filler without a stray chain member", w_size, roll, at_zero, probe_miss)


def limit_edge_states(lib, prefix, roll):
    return [limit_edge_state(lib, prefix, w, roll, z, m) for w in WINDOW_SIZES for z in (0, 1) for m in (0, 1)]
