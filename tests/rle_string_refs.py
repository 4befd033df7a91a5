"""TEST-ONLY: the compressed RLE string coding of include/detops.h ("Compressed RLE strings") put down literally, step by
step, and its inverse.  The coder is the yardstick of `_rle_cpu.rle_strings` (numpy) and, through that, of
`_C.rle_strings` (HIP); the decoder exists for the tests alone: the product decodes nothing.

Both are restatements of pycocotools' rleToString / rleFrString written from knowledge of that code; pycocotools is not
installed where this project is built and tested, so nobody has run them against it.
"""

# counts -> string, made with `rle_to_string` below (the last one is recalled from public pycocotools examples)
VECTORS = [
    ([16], "`0"),
    ([0, 16], "0`0"),
    ([0, 5, 3], "053"),
    ([15, 16, 17, 1], "?`0a0A"),
    ([3, 1, 2, 1, 1, 40, 1, 1], "3120OW10iN"),
    ([100, 3, 97, 3, 97, 3, 797], "T33Q3000le0"),
    ([1066400], "P]aP1"),
    ([6, 1, 40, 4, 5, 4, 5, 4, 21], "61X13mN000`0"),
]

# the values the seeded masks draw from: both sides of every 5-bit group boundary, and the largest int32
EDGE_VALUES = [0, 1, 15, 16, 17, 511, 512, 16383, 16384, 524287, 524288, 2 ** 24 - 1, 2 ** 24, 2 ** 29 - 1, 2 ** 31 - 1]


def _wrap64(x):
    """a Python int as a signed 64-bit value"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def rle_to_string(counts):
    """the runs of one mask -> its string"""
    out = []
    for i in range(len(counts)):
        x = _wrap64(int(counts[i]))
        if i > 2:
            x = _wrap64(x - int(counts[i - 2]))
        while True:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if ch & 0x10 else (x != 0)
            if more:
                ch |= 0x20
            out.append(ch + 48)
            if not more:
                break
    return bytes(out).decode("ascii")


def rle_from_string(s):
    """a string -> the runs of one mask (rleFrString)"""
    counts = []
    data = s.encode("ascii")
    p = 0
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            ch = data[p] - 48
            x |= (ch & 0x1f) << (5 * k)
            more = bool(ch & 0x20)
            p += 1
            k += 1
            if not more and ch & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def code_length(x):
    """the closed form: the smallest k >= 1 with -2^(5k-1) <= x < 2^(5k-1)"""
    k = 1
    while not -(1 << (5 * k - 1)) <= x < (1 << (5 * k - 1)):
        k += 1
    return k


def seeded_masks(n=2000, seed=20241020):
    """n lists of 1 to 40 int32 runs: EDGE_VALUES and uniform draws of every magnitude"""
    import numpy as np

    rng = np.random.RandomState(seed)
    masks = []
    for _ in range(n):
        m = int(rng.randint(1, 41))
        edge = rng.randint(0, len(EDGE_VALUES), m)
        bits = rng.randint(1, 32, m)
        uniform = (rng.randint(0, 2 ** 31 - 1, m, dtype=np.int64) >> (31 - bits))
        pick = rng.rand(m) < 0.5
        masks.append([int(EDGE_VALUES[e]) if p else int(u) for e, u, p in zip(edge, uniform, pick)])
    return masks
