"""What a right answer of the block emitter is, written without looking at it (test infrastructure): the cost of an optimal
Huffman code, whether every optimal code must break a length limit, the exact optimum under a limit, and the three block
sizes zng_tr_flush_block compares (trees.c:660-719).  Costs are unique where lengths are not, so tests compare costs.
Extra bits are RFC 1951's tables (deflate_parse.py)."""
import heapq

from deflate_parse import DIST_EXTRA, LEN_EXTRA, STATIC_LIT_LENS


def _used(freq):
    return [f for f in freq if f]


def optimal_cost(freq):
    """sum of f * len over any Huffman code of the symbols with f > 0 (a lone symbol gets one bit, as deflate sends it)"""
    h = _used(freq)
    if len(h) < 2:
        return sum(h)
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        w = heapq.heappop(h) + heapq.heappop(h)
        cost += w
        heapq.heappush(h, w)
    return cost


def min_max_depth(freq):
    """the longest code of the minimum-variance Huffman code: among equal weights the shallower subtree is merged first,
    which makes the deepest leaf as shallow as any optimal code can have it.  Above a limit, every optimal code breaks it."""
    h = [(f, 0) for f in _used(freq)]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    while len(h) > 1:
        (w0, d0), (w1, d1) = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (w0 + w1, max(d0, d1) + 1))
    return h[0][1]


def limited_optimum(freq, maxbits):
    """the least sum of f * len over prefix codes with every len <= maxbits: package-merge (Larmore and Hirschberg 1990).
    A leaf appears once per level; the cheapest 2n - 2 items of the last level's list are the code, and an item's weight
    counts one bit for every leaf inside it."""
    leaves = sorted(_used(freq))
    n = len(leaves)
    if n < 2:
        return sum(leaves)
    if n > 1 << maxbits:
        raise ValueError("%d symbols do not fit %d bits" % (n, maxbits))
    cur = leaves
    for _ in range(maxbits - 1):
        packages = [cur[i] + cur[i + 1] for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + packages)
    return sum(cur[:2 * n - 2])


def _extra_bits(lit_hist, dist_hist):
    return (sum(f * LEN_EXTRA[s - 257] for s, f in enumerate(lit_hist) if f and s > 256) +
            sum(f * DIST_EXTRA[d] for d, f in enumerate(dist_hist) if f))


def body_cost(hist, lens):
    return sum(f * lens[s] for s, f in enumerate(hist) if f)


def static_lenb(lit_hist, dist_hist):
    """bytes of the block under the static codes: 3 header bits, 7 / 8 / 9-bit literal/length codes, 5-bit distance codes"""
    bits = 3 + body_cost(lit_hist, STATIC_LIT_LENS) + 5 * sum(dist_hist) + _extra_bits(lit_hist, dist_hist)
    return (bits + 7) >> 3


def stored_lenb(nbytes):
    """bytes of the same data in stored blocks: 5 bytes of header in front of every 65535 (an empty block has one too)"""
    return nbytes + 5 * max(1, -(-nbytes // 65535))


def dyn_lenb(header_bits, lit_hist, dist_hist, lit_lens, dist_lens):
    """bytes of the dynamic block: header_bits from the block's first bit to the last bit of its code lengths"""
    bits = header_bits + body_cost(lit_hist, lit_lens) + body_cost(dist_hist, dist_lens) + _extra_bits(lit_hist, dist_hist)
    return (bits + 7) >> 3


def brute_force_limited(freq, maxbits):
    """the same optimum by trying every assignment of lengths 1..maxbits (small alphabets only)"""
    f = _used(freq)
    if len(f) < 2:
        return sum(f)
    best = [None]

    def go(i, kraft, cost):
        if best[0] is not None and cost >= best[0]:
            return
        if i == len(f):
            best[0] = cost
            return
        for n in range(1, maxbits + 1):
            k = kraft + (1 << (maxbits - n))
            if k <= 1 << maxbits:
                go(i + 1, k, cost + f[i] * n)
    go(0, 0, 0)
    return best[0]
