"""Generate the literal/length code tables of the GPU PNG stream (png.TABLES).

    python tools/png_tables.py            # prints the TABLES literal to paste into render-in-between_amd/png.py

A strip of the stream (png.py) picks the cheapest of K fixed Huffman tables, so no tree is built on the device.  The tables
are fitted to models, not to images: a PNG-filtered byte of photographic content is close to a two-sided geometric
("Laplacian") residual around 0, read as int8, and what differs between strips is its scale and how much of the strip is
runs.  Table 0 is flat (every length <= 9: the worst case the size bound is derived from); the others are the
length-limited Huffman codes of a Laplacian of scale b, each without and with weight on the run lengths, plus one table
for flat graphics (zeros and maximal runs).  Every table is a complete prefix code with lengths 1..15; png.py asserts it.
"""
import heapq
import math
import sys

NSYM = 286
SCALES = (0.6, 1.2, 2.5, 5.0, 10.0, 20.0)
RUN_WEIGHTS = (0.002, 0.08)          # share of the tokens that are matches: without / with weight on the run lengths


def huffman_lengths(freq):
    heap = [(f, i, (i,)) for i, f in enumerate(freq)]
    heapq.heapify(heap)
    lengths = [0] * len(freq)
    tick = len(freq)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for s in a + b:
            lengths[s] += 1
        heapq.heappush(heap, (fa + fb, tick, a + b))
        tick += 1
    return lengths


def limited_lengths(freq, limit):
    """Huffman lengths clamped to `limit`, then repaired to a complete code (Kraft sum exactly 1)."""
    lengths = [min(l, limit) for l in huffman_lengths(freq)]
    target = 1 << limit
    kraft = sum(1 << (limit - l) for l in lengths)
    order = sorted(range(len(freq)), key=lambda s: (freq[s], s))
    while kraft > target:                     # over-subscribed: lengthen the rarest symbol that still can be
        s = next(s for s in order if lengths[s] < limit)
        kraft -= 1 << (limit - lengths[s] - 1)
        lengths[s] += 1
    while kraft < target:                     # room left: shorten the most frequent symbol that fits
        s = next(s for s in reversed(order) if lengths[s] > 1 and kraft + (1 << (limit - lengths[s])) <= target)
        kraft += 1 << (limit - lengths[s])
        lengths[s] -= 1
    assert sum(1 << (limit - l) for l in lengths) == target and min(lengths) >= 1 and max(lengths) <= limit
    return lengths


def length_symbol_weights():
    """Relative weight of the 29 length symbols 257..285 among the matches: short runs decay, the maximal run stands out."""
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    w = [1.0 / (b + 2) for b in base]
    w[0] = 1e-4                               # length 3 never occurs: matches start at 4
    w[28] = 0.25 * sum(w[:28])
    t = sum(w)
    return [x / t for x in w]


def model(scale, run_weight, zero_boost=0.0):
    lit = [math.exp(-min(v, 256 - v) / scale) for v in range(256)]
    t = sum(lit)
    lit = [x / t for x in lit]
    if zero_boost:
        lit = [x * (1 - zero_boost) for x in lit]
        lit[0] += zero_boost
    freq = [(1 - run_weight) * x for x in lit] + [2e-4] + [run_weight * x for x in length_symbol_weights()]
    return [max(f, 1e-7) for f in freq]


def tables():
    flat = [1.0] * 256 + [0.4] * 30
    for v in range(113, 143):                 # the residuals a Laplacian makes rarest take the 9-bit codes with EOB and the lengths
        flat[v] = 0.4
    out = [limited_lengths(flat, 9)]
    for b in SCALES:
        for rw in RUN_WEIGHTS:
            out.append(limited_lengths(model(b, rw, zero_boost=0.15 if rw > 0.01 else 0.0), 15))
    out.append(limited_lengths(model(0.6, 0.45, zero_boost=0.5), 15))      # flat graphics
    return out


def main():
    tabs = tables()
    print("TABLES = np.array([")
    for t in tabs:
        assert len(t) == NSYM
        lines = [", ".join("%d" % v for v in t[i:i + 48]) for i in range(0, NSYM, 48)]
        print("    [" + ",\n     ".join(lines) + "],")
    print("], dtype=np.uint8)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
