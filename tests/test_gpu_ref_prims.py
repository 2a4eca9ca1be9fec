"""GPU parity against the reference's own compiled primitives (oracle/_ref/libzng_ref_prims.so: the reference built
with NO_UNALIGNED behind oracle/ref_shim.c), at the shapes the older GPU tests leave out: in-contract states at three
window sizes before and after a slide, every level, prev_length / lookahead at their edges, tables that evolve on the
device only, and the long-copy and memmove-order routes of chunkmemset_safe_dev.  Bit-exact throughout."""
import numpy as np
import pytest

import oracle_lib
from deflate_state_util import (DATA_KINDS, LOOKAHEADS, MIN_LOOKAHEAD, WINDOW_SIZES, HostState,
                                cur_match_candidates, hash_at, in_contract_snapshots, limit_edge_states, match_call,
                                match_param_sets, set_match_level, stream_data)
from gpu_common import product, to_dev, torch_mod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zr():
    m = product()
    m.init()
    return m


@pytest.fixture(scope="module")
def ref():
    return oracle_lib.load_ref_prims()


def _u16_dev(arr):
    return torch_mod().from_numpy(np.ascontiguousarray(arr).view(np.int16)).cuda()


def _view(zr, window, prev, head, hs):
    """zng_rocm_deflate_view over device slabs with hs.st's scalars"""
    v = zr.rocm.DeflateView()
    v.window, v.prev, v.head = window.data_ptr(), prev.data_ptr(), head.data_ptr()
    for f in ("w_size", "w_mask", "lookahead", "strstart", "match_start", "prev_length", "max_chain_length",
              "good_match", "nice_match", "level"):
        setattr(v, f, getattr(hs.st, f))
    return v


def _launch_match(zr, slow, views, curs):
    torch = torch_mod()
    d_views = zr.rocm.views_to_device(views)
    d_cur = _u16_dev(np.array(curs, dtype=np.uint16))
    lens = torch.zeros(len(views), dtype=torch.int32, device="cuda")
    starts = torch.zeros(len(views), dtype=torch.int32, device="cuda")
    if slow:
        zr.rocm._check(zr.rocm.lib().zng_rocm_longest_match_slow_dev(
            zr.rocm._dev_ptr(d_views), len(views), zr.rocm._dev_ptr(d_cur), zr.rocm._dev_ptr(lens),
            zr.rocm._dev_ptr(starts), zr.rocm._stream_ptr(None)), "zng_rocm_longest_match_slow_dev")
    else:
        zr.rocm.longest_match_dev(d_views, len(views), d_cur, lens, starts)
    return list(zip(lens.cpu().tolist(), starts.cpu().tolist()))


def _queries(ref, zr, snap, dev, kind, roll, slow, rng, views, curs, wants, labels):
    """a sample of the (level, cur_match, prev_length, lookahead) space on one snapshot: reference result + device view"""
    window, prev, head = dev
    name = "longest_match_slow" if slow else "longest_match"
    fn = getattr(ref, "ref_" + name)
    levels = (9,) if roll else ((7, 8) if slow else range(1, 9))
    per_cur = {(False, False): 2, (False, True): 5, (True, False): 6, (True, True): 8}[(roll, slow)]
    for level in levels:
        set_match_level(snap, level)
        params = match_param_sets(level)
        for cur in cur_match_candidates(snap, kind, roll):
            for k in rng.choice(len(params), size=per_cur, replace=False).tolist():
                p, la = params[k]
                wants.append(match_call(fn, snap, cur, p, la))
                views.append(_view(zr, window, prev, head, snap))
                views[-1].match_start = 0x123456
                curs.append(cur)
                labels.append((name, kind, roll, snap.phase, snap.strstart, level, cur, p, la))


@pytest.mark.parametrize("w_size", WINDOW_SIZES)
def test_match_kernels_in_contract(zr, ref, w_size):
    """longest_match_dev (levels 1-9) and longest_match_slow_dev (levels 7-9) on 24 snapshots per data kind and hash
    family: strstart below MAX_DIST, in (w_size, 2*w_size - 262] with window_size - MIN_LOOKAHEAD itself, and after a
    slide; (length, match_start) lists equal the reference's."""
    rng = np.random.default_rng(w_size)
    batches = {False: ([], [], [], []), True: ([], [], [], [])}          # slow -> views, curs, wants, labels
    keep = []
    for kind in DATA_KINDS:
        for roll in (False, True):
            snaps = in_contract_snapshots(ref, "ref_", kind, w_size, roll, per_phase=8)
            assert len(snaps) >= 20 and {s.phase for s in snaps} == {0, 1, 2}
            assert any(s.strstart == 2 * w_size - MIN_LOOKAHEAD and s.phase == 1 for s in snaps)
            windows = {}
            for s in snaps:
                if id(s.window) not in windows:
                    windows[id(s.window)] = to_dev(s.window)
            d_head = _u16_dev(np.stack([s.head for s in snaps]))
            d_prev = _u16_dev(np.stack([s.prev for s in snaps]))
            keep.append((windows, d_head, d_prev))
            for i, s in enumerate(snaps):
                dev = (windows[id(s.window)], d_prev[i], d_head[i])
                for slow in (False, True):
                    _queries(ref, zr, s, dev, kind, roll, slow, rng, *batches[slow])
    for slow in (False, True):
        views, curs, wants, labels = batches[slow]
        assert len(views) > 2000
        assert {l[7] for l in labels} >= {0, 2, 3, 4, 257, 258} and {l[8] for l in labels} == set(LOOKAHEADS)
        got = _launch_match(zr, slow, views, curs)
        bad = [i for i in range(len(wants)) if got[i] != wants[i]]
        assert not bad, (len(bad), [(labels[i], got[i], wants[i]) for i in bad[:5]])


def test_chain_ends_at_limit(zr, ref):
    """Chains whose next member lies exactly at `limit` (limit 0 and > 0, three window sizes, both hash families): the
    chain stops there, at the probe loop's step and at the step after a compare, in both matchers.  The reference
    answers (4, strstart - 3); a `>= limit` step would take the 40-byte match at `limit`."""
    batches = {False: ([], [], []), True: ([], [], [])}
    keep = []
    for roll in (False, True):
        for snap in limit_edge_states(ref, "ref_", roll):
            dev = (to_dev(snap.window), _u16_dev(snap.prev), _u16_dev(snap.head))
            keep.append(dev)
            for slow, levels in ((False, (9,) if roll else range(1, 9)), (True, (9,) if roll else (7, 8))):
                fn = ref.ref_longest_match_slow if slow else ref.ref_longest_match
                views, curs, wants = batches[slow]
                for level in levels:
                    set_match_level(snap, level)
                    for p, la in ((0, 262), (2, 258), (0, 41)):
                        wants.append(match_call(fn, snap, snap.cur, p, la))
                        assert wants[-1] == (4, snap.strstart - 3)
                        views.append(_view(zr, *dev, snap))
                        views[-1].match_start = 0x123456
                        curs.append(snap.cur)
    for slow in (False, True):
        views, curs, wants = batches[slow]
        assert _launch_match(zr, slow, views, curs) == wants, slow


def _tables_equal(d_head, d_prev, hs):
    head = d_head.cpu().numpy().view(np.uint16)
    prev = d_prev.cpu().numpy().view(np.uint16)
    return (head == hs.head).all() and (prev == hs.prev).all()


@pytest.mark.parametrize("roll,w_size", [(False, 32768), (True, 32768), (False, 512), (True, 4096)])
def test_device_evolved_tables(zr, ref, roll, w_size):
    """insert_string(_roll)_dev, slide_hash_dev with the window moved on the device, insert again, then the match
    kernels: head and prev never come from the host after the first (zeroed) upload.  After every step head, prev and
    ins_h equal the reference's doing the same on the CPU, and so do the matches."""
    torch = torch_mod()
    data = stream_data("texty3", 3 * w_size, seed=5 if roll else 4)
    hs = HostState(data, w_size=w_size)
    hs.st.ins_h = 0x2a5
    d_window = to_dev(hs.window)
    d_head, d_prev = _u16_dev(hs.head), _u16_dev(hs.prev)
    d_ins_h = torch.from_numpy(np.array([hs.st.ins_h], dtype=np.uint32).view(np.int32)).cuda()
    d_views = zr.rocm.views_to_device([_view(zr, d_window, d_prev, d_head, hs)])
    ref_insert = ref.ref_insert_string_roll if roll else ref.ref_insert_string

    def insert(start, count):
        strs = torch.full((1,), start, dtype=torch.int32, device="cuda")
        cnts = torch.full((1,), count, dtype=torch.int32, device="cuda")
        if roll:
            zr.rocm.insert_string_roll_dev(d_views, 1, strs, cnts, d_ins_h)
        else:
            zr.rocm.insert_string_dev(d_views, 1, strs, cnts)
        ref_insert(hs.ref(), start, count)
        assert _tables_equal(d_head, d_prev, hs), ("insert", start, count)
        if roll:
            assert int(d_ins_h.cpu().numpy().view(np.uint32)[0]) == hs.st.ins_h, ("ins_h", start, count)

    def matches(strstart):
        hs.strstart = strstart
        cur = int(hs.head[hash_at(hs.window, strstart, roll)])
        curs_here = [c for c in (cur, int(hs.prev[cur & hs.st.w_mask])) if 0 < c and strstart - c <= w_size - MIN_LOOKAHEAD]
        curs_here.append(strstart + 1)
        for slow, levels in ((False, (9,) if roll else range(1, 9)), (True, (9,) if roll else (7, 8))):
            fn = ref.ref_longest_match_slow if slow else ref.ref_longest_match
            views, curs, wants = [], [], []
            for level in levels:
                set_match_level(hs, level)
                for c in curs_here:
                    for p, la in match_param_sets(level):
                        wants.append(match_call(fn, hs, c, p, la))
                        views.append(_view(zr, d_window, d_prev, d_head, hs))
                        views[-1].match_start = 0x123456
                        curs.append(c)
            assert _launch_match(zr, slow, views, curs) == wants, (slow, strstart)

    top = 2 * w_size - MIN_LOOKAHEAD
    insert(0, w_size - 300)
    matches(w_size - 300)                                       # limit == 0
    insert(w_size - 300, top - (w_size - 300))
    matches(top)                                                # limit > 0 at window_size - MIN_LOOKAHEAD
    # fill_window's slide: upper half down, new data behind it, every table entry down by w_size
    d_window[:w_size] = d_window[w_size:2 * w_size].clone()
    d_window[w_size:2 * w_size] = to_dev(data[2 * w_size:3 * w_size])
    hs.window[:w_size] = hs.window[w_size:2 * w_size].copy()
    hs.window[w_size:2 * w_size] = data[2 * w_size:3 * w_size]
    zr.rocm.slide_hash_dev(d_views, 1)
    ref.ref_slide_hash(hs.ref())
    assert _tables_equal(d_head, d_prev, hs), "slide_hash"
    matches(top - w_size)                                       # straight after the slide
    insert(top - w_size, w_size // 2 + 77)
    matches(top - w_size + w_size // 2 + 77)                    # limit > 0 over slid and new entries


# ---- chunkmemset_safe_dev: the long-copy route and the memmove-order route -----------------------------------
LONG_LENS = (2047, 2048, 2049, 4101, 70000)                      # around kLongCopy = 2048
AHEADS = (1, 15, 16, 17, 255, 256, 257, 300)
BATCHES = (1, 47, 48, 49, 48 * 64 + 1)                           # kCopiesPerWave = 48 edges


def _copy_plan():
    """(dist, len, left): dist > 0 = from behind out, dist < 0 = from ahead of out"""
    rng = np.random.default_rng(77)
    plan = []
    for ln in LONG_LENS:                                           # long copies: pattern, plain, ahead
        for dist in (1, 3, 16, 17, 255, 2049, ln + 5):
            plan.append((dist, ln, ln + int(rng.integers(0, 40))))
        for ahead in AHEADS + (ln, ln + 9):
            plan.append((-ahead, ln, ln + int(rng.integers(0, 40))))
    ahead_lens = list(range(1, 40)) + [255, 256, 257, 258, 271, 272, 273, 511, 512, 513, 767, 768, 769, 1000, 2048,
                                       2049, 4095, 4096, 4097, 5000]
    for ahead in AHEADS:                                           # many 256-byte rounds in memmove order
        for ln in ahead_lens + rng.integers(1, 5001, size=12).tolist():
            plan.append((-ahead, ln, ln + int(rng.integers(0, 40))))
    plan += [(7, 100, 60), (1, 258, 1), (300, 258, 200), (-5, 100, 60), (-16, 600, 599),      # left < len, both routes
             (5, 4000, 3000), (-17, 70000, 2049), (9, 70000, 2048), (3, 3000, 100), (-300, 5000, 301),
             (-1, 5000, 4999), (40, 2049, 2048), (-256, 2049, 0), (11, 0, 50)]
    while len(plan) < BATCHES[-1]:                                 # the inflate caller's mix around them
        plan.append((int(rng.integers(1, 600)), int(rng.integers(3, 259)), 258 + int(rng.integers(0, 40))))
    order = rng.permutation(len(plan)).tolist()
    plan = [plan[i] for i in order]
    plan.insert(0, (-17, 1000, 1003))                              # a batch of one: the list route alone
    plan[BATCHES[-1] - 1] = (-255, 4101, 4101)                     # the last wave's only copy
    return plan[:BATCHES[-1]]


def _copy_batch(ref):
    """the plan laid out in one buffer, each copy in a region of its own, and the reference's bytes of each copy's
    contractual range [out, out + min(len, left))"""
    rng = np.random.default_rng(78)
    plan = _copy_plan()
    gap = 96
    out_off = np.zeros(len(plan), dtype=np.uint64)
    from_off = np.zeros(len(plan), dtype=np.uint64)
    at = 0
    for i, (dist, ln, left) in enumerate(plan):
        lo = at + gap                                              # first byte the copy may touch
        out = lo + max(dist, 0)
        out += (i * 7 - out) % 16                                  # out walks through every 16-byte phase
        out_off[i], from_off[i] = out, out - dist
        at = out + max(-dist, 0) + max(ln, left) + gap
    size = at + 256
    base = rng.integers(0, 256, size=size, dtype=np.uint8)
    ln_a = np.array([p[1] for p in plan], dtype=np.uint32)
    left_a = np.array([p[2] for p in plan], dtype=np.uint32)
    n_a = np.minimum(ln_a, left_a)
    assert (from_off.astype(np.int64) >= gap).all() and (np.maximum(out_off, from_off) + n_a + gap <= size).all()
    listed = (n_a > 2048) | ((from_off > out_off) & (from_off - out_off < n_a))
    for sel in (listed, ~listed):
        assert {int(o) & 15 for o in out_off[sel]} == set(range(16)) == {int(f) & 15 for f in from_off[sel]}
    assert listed[0] and listed[-1] and 200 < int(listed.sum()) < len(plan) - 2000

    results = []                                                   # the reference's bytes of each contractual range
    for i, (dist, ln, left) in enumerate(plan):
        lo = int(min(out_off[i], from_off[i])) - gap
        hi = int(max(out_off[i], from_off[i])) + max(ln, left) + gap
        region = base[lo:hi].copy()
        o, f = int(out_off[i]) - lo, int(from_off[i]) - lo
        end = ref.ref_chunkmemset_safe(region.ctypes.data + o, region.ctypes.data + f, ln, left)
        assert end == region.ctypes.data + o + int(n_a[i])
        results.append(region[o:o + int(n_a[i])].copy())

    return base, out_off, from_off, ln_a, left_a, n_a, results


def test_chunkmemset_safe_long_and_ahead(zr, ref):
    """One mixed batch, cut at 1, 47, 48, 49 and 48*64+1 copies.  Inside each copy's contractual range
    [out, out + min(len, left)) the bytes equal the reference's (run on a copy: its chunk stores may pass out + len);
    every other byte of the buffer is unchanged."""
    torch = torch_mod()
    base, out_off, from_off, ln_a, left_a, n_a, results = _copy_batch(ref)
    gap, plan = 96, _copy_plan()
    for count in BATCHES:
        expected = base.copy()
        for i in range(count):
            expected[int(out_off[i]):int(out_off[i]) + int(n_a[i])] = results[i]
        d_base = to_dev(base)
        zr.rocm.chunkmemset_safe_dev(d_base, torch.from_numpy(out_off[:count].view(np.int64).copy()).cuda(),
                                     torch.from_numpy(from_off[:count].view(np.int64).copy()).cuda(),
                                     torch.from_numpy(ln_a[:count].view(np.int32).copy()).cuda(),
                                     torch.from_numpy(left_a[:count].view(np.int32).copy()).cuda())
        got = d_base.cpu().numpy()
        bad = np.nonzero(got != expected)[0]
        if bad.size:
            k = int(np.searchsorted(out_off.astype(np.int64) - gap, int(bad[0]), side="right")) - 1
            raise AssertionError((count, bad.size, int(bad[0]), k, plan[k], int(out_off[k]), int(from_off[k])))
