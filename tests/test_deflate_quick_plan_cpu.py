"""CPU checks of the rules that hold ONE stream of the level-1 class kernels to the whole range the calls accept:
zlib-ng_amd/csrc/deflate_quick_plan.h through a small C++ driver (tests/c/deflate_quick_plan_driver.cpp) built here with g++.

  the flush rule   the kernel's bit cursor wraps at 2^32 bits (512 MiB of output), up to seven times below the bound of the largest
                   stream.  The rule is walked batch by batch against a model in Python's integers, where nothing wraps: the words
                   every flush writes, the words pending in the ring (always below kRingWords) and the stream's final byte count
                   -- at the start of a stream, across every multiple of 2^32 bits, and up to the last bit of the largest stream.
                   The rule this one replaced (`cursor >> 5` against the words written, in 32 bits) is restated below and writes
                   more than 2^31 words at the first flush behind the first wrap.
  the Adler fold   a lane's sums in closed form for runs of one byte value, folded by the driver as the kernel folds them, against
                   Adler-32 from its definition.  The order this one replaced (add a wave's 64 lanes modulo 2^64, reduce
                   afterwards) is restated below and is wrong at 768 MiB of 0xff.
  the job check    the largest in_len and one more, dict_len, flags, alignment, out_cap: through both entry points' forms.
Every expected value is worked out here from the definitions or comes from CPython's zlib."""
import os
import random
import subprocess
import tempfile
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -3
BASE = 65521
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "deflate_quick_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-O1",
                               "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"),
                               os.path.join(ROOT, "tests", "c", "deflate_quick_plan_driver.cpp"), "-o", exe])

        def run(*args, stdin=""):
            out = subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (args, out.returncode, out.stderr)
            return out.stdout.splitlines()
        yield run


@pytest.fixture(scope="module")
def consts(driver):
    ring, flush, batch_bits, max_in, max_hist = (int(v) for v in driver("consts")[0].split())
    return {"ring": ring, "flush": flush, "batch_bits": batch_bits, "max_in": max_in, "max_hist": max_hist}


def bound(n):
    """zng_rocm_deflate_quick_bound: 3 header bits, 9 bits per byte, 7 EOB bits, the sync-flush marker; 16-byte steps"""
    return (n + ((n + 7) >> 3) + 13 + 15) & ~15


# ---- the bound and the largest stream ------------------------------------------------------------------------------------------
def test_largest_stream_is_the_last_whose_bound_fits_32_bits(driver, consts):
    n = consts["max_in"]
    assert n == 3817748681 and consts["max_hist"] == 32768 and consts["batch_bits"] == 256 * 9
    assert bound(n) <= M32 < bound(n + 1)
    for v in (0, 1, 7, 8, 9, 4096 + 3, (40 << 20) + 3, 1 << 31, n, n + 1, M32):
        assert int(driver("bound", v)[0]) == bound(v), v
    assert 3 + 9 * n + 7 + 3 < 8 << 32                      # the cursor wraps seven times at the most


# ---- the flush rule ------------------------------------------------------------------------------------------------------------
def model_walk(cursor, flushed, steps, sync, ring, keep):
    """the same bookkeeping in unbounded integers: per batch the words its flush writes; then flush(1) and the stream's length"""
    counts = []
    for bits in steps:
        pend = cursor // 32 - flushed
        cnt = pend & ~31 if pend >= keep else 0
        counts.append(cnt)
        flushed += cnt
        cursor += bits                                      # place: the ring holds words flushed .. cursor // 32
        assert cursor // 32 - flushed < ring, (cursor, flushed)
    last = cursor // 32 - flushed
    flushed += last
    total_bits = cursor + 7 + (3 if sync else 0)            # EOB; the header of the empty stored block
    return counts, last, flushed, (total_bits + 7) // 8 + (4 if sync else 0)


def parent_flush_words(cursor32, flushed, keep):
    """the rule before this one, in the kernel's 32-bit registers: `full = cursor >> 5; if (full - flushed >= keep_below)
    cnt = keep_below > 1 ? (full - flushed) & ~31u : full - flushed`"""
    diff = ((cursor32 >> 5) - flushed) & M32
    if diff < keep:
        return 0
    return diff & ~31 & M32 if keep > 1 else diff


def check_walk(driver, consts, cursor, pending, steps, sync):
    ring, keep = consts["ring"], consts["flush"]
    flushed = cursor // 32 - pending
    got = driver("walk", cursor, flushed, int(sync), stdin="\n".join(str(s) for s in steps) + "\n")
    counts, last, words, total = model_walk(cursor, flushed, steps, sync, ring, keep)
    assert [int(v) for v in got[:-1]] == counts, (cursor, pending)
    end = cursor + sum(steps)
    g_last, g_word, g_spill, g_first, g_nbytes, g_bytes = (int(v) for v in got[-1].split())
    assert (g_last, g_word) == (last, words) and words == end // 32, (cursor, pending)
    # (byte counts are 32 bits wide as the row is: equal to the model's for every stream, whose length is below its bound)
    assert g_bytes == total & M32 and (g_first + g_nbytes + (4 if sync else 0)) & M32 == g_bytes, (cursor, pending, got[-1])
    assert g_first == (4 * (words + g_spill)) & M32 and g_spill == (1 if end % 32 + 7 >= 32 else 0)
    return counts, total


def step_patterns(batch_bits, count, seed):
    rng = random.Random(seed)
    yield [batch_bits] * count                              # 256 nine-bit literals in every batch
    yield [rng.randint(0, batch_bits) for _ in range(count)]
    yield [rng.choice((0, 1, 31, 32, 33, 2048, batch_bits - 1, batch_bits)) for _ in range(count)]
    yield [rng.randint(0, 40) for _ in range(count)]        # long matches: a flush every hundred batches


def test_flush_rule_from_the_start_of_a_stream(driver, consts):
    for k, steps in enumerate(step_patterns(consts["batch_bits"], 6000, 1)):
        counts, total = check_walk(driver, consts, 3, 0, steps, sync=bool(k & 1))
        assert sum(counts) > 0 and total < 1 << 24


@pytest.mark.parametrize("wrap", range(1, 9))
def test_flush_rule_across_every_multiple_of_2_32_bits(driver, consts, wrap):
    """The bound of the largest stream is 8 * 2^32 bits less 128: a stream can cross the multiples 1..7, and the walk up to the
    last bit of the largest stream (below) ends in front of the eighth.  The eighth is walked all the same: the words every
    flush writes are right there too; only the byte count no longer fits the row's 32 bits."""
    bb = consts["batch_bits"]
    assert 8 * bound(consts["max_in"]) == (8 << 32) - 128
    for k, steps in enumerate(step_patterns(bb, 6000, 10 + wrap)):
        before = sum(steps) // 2                            # the multiple is crossed in the middle of the walk
        for pending in (0, 31, consts["flush"] - 1):
            cursor = (wrap << 32) - before - 32 * pending + 5
            assert cursor < wrap << 32 < cursor + sum(steps)
            check_walk(driver, consts, cursor, pending, steps, sync=bool(k & 1))
    # ... and landing on the multiple itself, one bit either side, with the end of the stream right there
    for delta in (-33, -32, -8, -7, -1, 0, 1, 24, 25, 26, 31, 32):
        for sync in (False, True):
            check_walk(driver, consts, (wrap << 32) - bb + delta, 100, [bb], sync)


def test_flush_rule_up_to_the_last_bit_of_the_largest_stream(driver, consts):
    n, bb = consts["max_in"], consts["batch_bits"]
    last = 3 + 9 * n                                        # every byte a nine-bit literal
    for k, steps in enumerate(step_patterns(bb, 6000, 99)):
        for sync in (False, True):
            total = check_walk(driver, consts, last - sum(steps), 17, steps, sync)[1]
            assert total <= bound(n) <= M32, (k, sync, total)


def test_the_rule_before_this_one_runs_away_behind_the_wrap(driver, consts):
    """the counter-example: 2000 bits in front of 2^32, one batch of 256 nine-bit literals"""
    keep, bb = consts["flush"], consts["batch_bits"]
    before = (1 << 32) - 2000
    for pending in (0, 100, keep - 1):
        flushed = before // 32 - pending
        after = before + bb
        want = ((after // 32 - flushed) & ~31) if after // 32 - flushed >= keep else 0
        old = parent_flush_words(after & M32, flushed, keep)
        assert old > 1 << 31, (pending, old)                # ... words stored behind out + 4 * flushed
        got = driver("walk", before, flushed, 0, stdin="%d\n0\n" % bb)
        assert int(got[0]) == 0 and int(got[1]) == want, (pending, got)
    for pend in (0, 31, keep - 1, keep, keep + 31, 200, 231):      # in front of the wrap both rules agree
        cursor = (1 << 31) + 5
        want = pend & ~31 if pend >= keep else 0
        assert parent_flush_words(cursor, cursor // 32 - pend, keep) == want
        assert int(driver("walk", cursor, cursor // 32 - pend, 0, stdin="0\n")[0]) == want


# ---- the Adler fold ------------------------------------------------------------------------------------------------------------
def lane_sums(v, n, start):
    """deflate_quick_kernel's 256 lanes over a stream of `start` history bytes and n plaintext bytes of value v: position p goes
    to lane p % 256 (batches begin at multiples of 256); accA = sum of byte, accB = sum of (start + n - p) * byte"""
    total = start + n
    out = []
    for t in range(256):
        first = start + (t - start) % 256
        count = (total - 1 - first) // 256 + 1 if first < total else 0
        weights = count * total - (count * first + 256 * count * (count - 1) // 2)
        out.append((v * count, v * weights))
    return out


def adler_by_definition(v, n):
    """A = 1 + sum of bytes, B = sum over i = 1..n of (1 + v * i), both modulo 65521"""
    return ((1 + v * n) % BASE) | (((n + v * n * (n + 1) // 2) % BASE) << 16)


def parent_fold(lanes, n):
    """the order before this one: a wave's 64 lanes added modulo 2^64, reduced afterwards"""
    a = sum(sum(x[0] for x in lanes[64 * w:64 * w + 64]) % (1 << 64) % BASE for w in range(4)) % BASE
    b = sum(sum(x[1] for x in lanes[64 * w:64 * w + 64]) % (1 << 64) % BASE for w in range(4)) % BASE
    return ((1 + a) % BASE) | (((n + b) % BASE) << 16)


def fold(driver, lanes, n):
    assert all(a <= M64 and b <= M64 for a, b in lanes)     # a lane's own sums fit its 64 bits: the kernel's registers hold these
    return int(driver("adler", n, stdin="".join("%d %d\n" % ab for ab in lanes))[0])


@pytest.mark.parametrize("v", (1, 128, 255))
def test_adler_fold_is_adler32(driver, consts, v):
    sizes = (1, 255, 256, 257, 726 << 20, 1 << 30, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, consts["max_in"])
    for n in sizes:
        want = adler_by_definition(v, n)
        if n <= 257:
            assert want == zlib.adler32(bytes([v]) * n)
        for start in (0, 1, 32768):
            lanes = lane_sums(v, n, start)
            assert sum(a for a, _ in lanes) == v * n
            assert fold(driver, lanes, n) == want, (v, n, start)


def test_closed_forms_against_zlib(driver):
    """the two closed forms above, checked where the bytes can be written out"""
    for v, n, start in ((255, 1 << 18, 0), (128, (1 << 18) + 77, 1), (1, 70000, 32768), (200, 513, 300)):
        data = bytes([v]) * n
        assert adler_by_definition(v, n) == zlib.adler32(data)
        lanes = lane_sums(v, n, start)
        for t in (0, 1, 44, 255):
            ps = [p for p in range(start, start + n) if p % 256 == t]
            assert lanes[t] == (v * len(ps), v * sum(start + n - p for p in ps))
        assert fold(driver, lanes, n) == zlib.adler32(data)


def test_the_order_before_this_one_is_wrong_at_768_mib_of_ff(driver):
    n = 768 << 20
    lanes = lane_sums(255, n, 0)
    for w in range(4):
        assert sum(b for _, b in lanes[64 * w:64 * w + 64]) >= 1 << 64
    want = adler_by_definition(255, n)
    assert parent_fold(lanes, n) != want
    assert fold(driver, lanes, n) == want
    small = lane_sums(255, 40 << 20, 0)                     # below the edge both orders agree
    assert parent_fold(small, 40 << 20) == adler_by_definition(255, 40 << 20) == fold(driver, small, 40 << 20)


# ---- the job check -------------------------------------------------------------------------------------------------------------
def job(driver, form, in_len, out_cap=None, dict_len=0, flags=0, window=0, inp=0x1000, out=0x2000):
    cap = min(bound(in_len), M32) if out_cap is None else out_cap
    return int(driver("job", form, inp, out, in_len, cap, dict_len, flags, window if form else 0)[0])


@pytest.mark.parametrize("form", (0, 1))
def test_job_check(driver, consts, form):
    n, hist = consts["max_in"], consts["max_hist"]
    w = {"window": hist}
    assert job(driver, form, n, **w) == 0
    assert job(driver, form, n + 1, **w) == EINVAL          # out_cap = 0xffffffff: the bound itself has no 32-bit form
    assert job(driver, form, M32, **w) == EINVAL
    for small in (0, 1, 4096 + 3, 1 << 20):
        assert job(driver, form, small, **w) == 0
        assert job(driver, form, small, out_cap=bound(small) - 1, **w) == EINVAL
    assert job(driver, form, n, out_cap=bound(n) - 1, **w) == EINVAL
    # history: a job's own dict_len up to 32768; with a dictionary object none of its own, and the object's window up to 32768
    assert job(driver, form, 1000, dict_len=hist, **w) == (EINVAL if form else 0)
    assert job(driver, form, 1000, dict_len=hist + 1, **w) == EINVAL
    assert job(driver, form, n, dict_len=hist, **w) == (EINVAL if form else 0)
    if form:
        assert job(driver, form, 1000, window=0) == 0 and job(driver, form, 1000, window=hist + 1) == EINVAL
    else:
        assert job(driver, form, 0, dict_len=5, inp=0) == EINVAL
    for flags in (1, 2, 3):
        assert job(driver, form, 1000, flags=flags, **w) == 0
    for flags in (4, 8, 0x80000000, 0xffffffff, 5):
        assert job(driver, form, 1000, flags=flags, **w) == EINVAL
    for out in (0x2001, 0x2002, 0x2003, 0):
        assert job(driver, form, 1000, out=out, **w) == EINVAL
    assert job(driver, form, 1000, inp=0x1003, out=0x2004, **w) == 0      # `in` has any alignment
    assert job(driver, form, 1000, inp=0, **w) == EINVAL and job(driver, form, 0, inp=0, **w) == 0


def test_self_check(driver):
    assert driver("self") == ["self ok"]
