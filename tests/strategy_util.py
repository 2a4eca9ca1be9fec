"""zlib's deflate strategies on the device (deflate_rle.h, emit_dynamic_kernel<true>): the Z_RLE parse restated in Python,
and the token stream of a raw deflate stream as a list, for the strategy tests (test infrastructure)."""
import numpy as np

Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 1, 2, 3, 4


def rle_parse(data, start=0, end=None):
    """the greedy parse of deflate_rle.c over positions [start, end) of `data` (bytes in front of `start` are history):
    p is a match iff data[p-1] == data[p] == data[p+1] == data[p+2] and p + 3 <= end, of distance 1 and of the length of
    the run of data[p-1] from p on, at most 258 and not past `end`; otherwise a literal.
    Returns [('l', byte) | ('m', length, 1), ...]."""
    end = len(data) if end is None else end
    out, p = [], start
    while p < end:
        if p > 0 and p + 3 <= end and data[p - 1] == data[p] == data[p + 1] == data[p + 2]:
            v, n = data[p - 1], 3
            while n < 258 and p + n < end and data[p + n] == v:
                n += 1
            out.append(('m', n, 1))
            p += n
        else:
            out.append(('l', data[p]))
            p += 1
    return out


def rle_closed_form(data, start=0, end=None):
    """the same parse in the form deflate_rle.h computes it, every position at once: (token starts, match starts) as
    boolean arrays over [start, end)"""
    end = len(data) if end is None else end
    d = np.frombuffer(bytes(data), dtype=np.uint8)
    pos = np.arange(start, end + 2, dtype=np.int64)
    brk = np.ones(pos.size, dtype=bool)                   # a break: differs from the byte before, position 0, past the end
    inner = (pos >= 1) & (pos < end)
    q = pos[inner]
    brk[inner] = d[q] != d[q - 1]
    # o = (last break at or before p) + 1, or `start` when there is none in [start, p]
    last = np.where(brk, pos + 1, start)
    o = np.maximum.accumulate(last)
    n = end - start
    b, b1, b2 = brk[:n], brk[1:n + 1], brk[2:n + 2]
    ob = np.concatenate(([start], o[:n - 1])) if n else o[:0]   # o of p = last break BEFORE p, + 1
    j = (pos[:n] - ob) % 258
    tok = b | (~b & ((j == 0) | ((j == 1) & b1)))
    mat = ~b & (j == 0) & ~b1 & ~b2
    return tok, mat


def tokens_of(raw, window_len=0):
    """the token stream of a raw deflate stream, literal runs expanded: [('l', byte) | ('m', length, distance), ...]"""
    import importlib
    inflate = importlib.import_module("zlib-ng_amd.inflate")
    ds = inflate.DecodedStream(raw, window_len)
    assert ds.status == 1, (ds.status, ds.msg)
    out, li = [], 0
    for t in ds.tokens.tolist():
        if t & 0x80000000:
            out.append(('m', ((t >> 16) & 0xff) + 3, (t & 0xffff) + 1))
        else:
            out.extend(('l', int(c)) for c in ds.literals[li:li + t])
            li += t
    return out


def run_heavy(n, seed):
    """runs of every length 1..600 between short stretches of random bytes"""
    rng = np.random.default_rng(seed)
    parts, size = [], 0
    while size < n:
        if rng.random() < 0.5:
            k = int(rng.integers(1, 601))
            parts.append(np.full(k, rng.integers(0, 4), dtype=np.uint8))
        else:
            k = int(rng.integers(1, 24))
            parts.append(rng.integers(0, 4, k, dtype=np.uint8))
        size += k
    return np.concatenate(parts)[:n].tobytes()
