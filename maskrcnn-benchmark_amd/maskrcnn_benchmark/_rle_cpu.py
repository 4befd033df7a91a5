"""Host implementation of the compressed RLE strings defined in include/detops.h ("Compressed RLE strings"), for CPU
tensors (numpy).

The same formulation as csrc/rle_string.hip: per run of the flat array its index inside its mask, the value to code (the
run, minus the run two before it from the mask's fourth run on) in 64 bits, the value's length in closed form, the 7
candidate 5-bit groups, and one gather of the groups below the length.  Nothing here loops over runs or masks.
"""
import numpy as np

MAX_LEN = 7    # bytes of the difference of two int32 values at most


def deltas(counts, run_offset):
    """counts int32 [total], run_offset int64 [N + 1] -> the values to code, int64 [total]"""
    c = np.ascontiguousarray(counts).astype(np.int64).reshape(-1)
    ro = np.asarray(run_offset, dtype=np.int64).reshape(-1)
    if ro.size < 1 or ro[0] != 0 or ro[-1] != c.size or (np.diff(ro) < 0).any():
        raise ValueError("rle_strings: run_offset must start at 0, not decrease and end at len(counts)")
    k = np.arange(c.size, dtype=np.int64) - np.repeat(ro[:-1], np.diff(ro))     # index of a run inside its mask
    x = c.copy()
    later = np.nonzero(k > 2)[0]
    x[later] -= c[later - 2]
    return x


def code_lengths(x):
    """bytes of every value: the smallest k >= 1 with -2^(5k-1) <= x < 2^(5k-1)"""
    x = np.asarray(x, dtype=np.int64)
    n = np.ones(x.shape, dtype=np.int64)
    for k in range(1, MAX_LEN):
        half = np.int64(1) << (5 * k - 1)
        n += (x >= half) | (x < -half)
    return n


def rle_strings(counts, run_offset):
    """-> (the strings' bytes back to back, uint8 [B]; byte_offset int64 [N + 1]): mask n's string is
    bytes[byte_offset[n]:byte_offset[n + 1]]"""
    x = deltas(counts, run_offset)
    ro = np.asarray(run_offset, dtype=np.int64).reshape(-1)
    n = code_lengths(x)
    b = np.arange(MAX_LEN, dtype=np.int64)
    groups = (x[:, None] >> (5 * b)[None, :]) & 0x1f                 # arithmetic shift: the sign fills in
    groups |= np.where(b[None, :] + 1 < n[:, None], 0x20, 0)        # every byte but a value's last says "more"
    data = (groups + 48)[b[None, :] < n[:, None]].astype(np.uint8)   # row-major: run after run, low group first
    ends = np.concatenate([np.zeros(1, np.int64), np.cumsum(n)])
    return data, ends[ro]


def to_str_list(data, byte_offset):
    """the bytes and offsets of rle_strings -> a list of N str (one decode, then slices)"""
    text = bytes(memoryview(np.ascontiguousarray(data, dtype=np.uint8))).decode("ascii")
    off = np.asarray(byte_offset, dtype=np.int64).tolist()
    return [text[off[i]:off[i + 1]] for i in range(len(off) - 1)]
