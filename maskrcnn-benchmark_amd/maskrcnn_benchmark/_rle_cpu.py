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


BAD_BYTE, TRUNCATED, LONG_VALUE, BAD_RUN, BAD_SUM = 1, 2, 4, 8, 16    # DETOPS_RLE_*


def _mask_sums(per_item, offsets):
    """per_item int64 [n], offsets int64 [N + 1] into it -> the sum of every mask's items (wrapping), [N]"""
    prefix = np.concatenate([np.zeros(1, np.int64), np.cumsum(per_item, dtype=np.int64)])
    return prefix[offsets[1:]] - prefix[offsets[:-1]]


def rle_decode(data, byte_offset, hw=None):
    """The inverse of rle_strings (include/detops.h, "Reading compressed RLE strings"; the same formulation as
    csrc/rle_decode.hip): bytes uint8 [B], byte_offset int64 [N + 1], hw [N, 2] or None -> (counts int32 [total],
    run_offset int64 [N + 1], status int32 [N]).  Nothing here loops over bytes, values or masks."""
    b = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    bo = np.asarray(byte_offset, dtype=np.int64).reshape(-1)
    if bo.size < 1 or bo[0] != 0 or bo[-1] != b.size or (np.diff(bo) < 0).any():
        raise ValueError("rle_string_decode: byte_offset must start at 0, not decrease and end at len(bytes)")
    N, B = bo.size - 1, b.size
    code = (b.astype(np.int64) - 48) & 0xff
    last = np.zeros(B, dtype=bool)
    last[bo[1:][np.diff(bo) > 0] - 1] = True                   # a string's last byte ends a value, whatever it says
    end = ((code & 0x20) == 0) | last
    ends = np.nonzero(end)[0]
    V = ends.size
    length = ends - np.concatenate([np.full(1, -1, np.int64), ends[:-1]])    # a value never crosses two strings
    n = np.minimum(length, MAX_LEN)                            # an overlong value is read from its last MAX_LEN bytes
    x = np.zeros(V, dtype=np.int64)
    for j in range(MAX_LEN):
        p = np.clip(ends - n + 1 + j, 0, max(B - 1, 0))
        x |= np.where(j < n, code[p] & 0x1f, 0) << (5 * j)
    negative = (code[ends] & 0x10) != 0
    x[negative] |= np.int64(-1) << (5 * n[negative])
    ro = np.concatenate([np.zeros(1, np.int64), np.cumsum(end, dtype=np.int64)])[bo]
    per_mask = np.diff(ro)
    k = np.arange(V, dtype=np.int64) - np.repeat(ro[:-1], per_mask)          # index of a run inside its mask
    c = x.copy()
    for cls in ((k & 1) == 1, ((k & 1) == 0) & (k > 0)):       # the two running sums: a plain prefix minus the mask's base
        v = np.where(cls, x, 0)
        prefix = np.concatenate([np.zeros(1, np.int64), np.cumsum(v, dtype=np.int64)])
        c[cls] = (prefix[1:] - np.repeat(prefix[ro[:-1]], per_mask))[cls]
    status = np.zeros(N, dtype=np.int32)
    status[_mask_sums((code > 63).astype(np.int64), bo) != 0] |= BAD_BYTE
    nonempty = np.diff(bo) > 0
    tail = np.zeros(N, dtype=bool)
    tail[nonempty] = (code[bo[1:][nonempty] - 1] & 0x20) != 0
    status[tail] |= TRUNCATED
    status[_mask_sums((length > MAX_LEN).astype(np.int64), ro) != 0] |= LONG_VALUE
    status[_mask_sums(((c < 0) | (c >= 2 ** 31)).astype(np.int64), ro) != 0] |= BAD_RUN
    if hw is not None:
        hw = np.asarray(hw, dtype=np.int64).reshape(N, 2)
        status[_mask_sums(c, ro) != hw[:, 0] * hw[:, 1]] |= BAD_SUM
    return c.astype(np.int32), ro, status


def from_str_list(strings):
    """a list of N str -> (bytes uint8 [B], byte_offset int64 [N + 1]): one encode of the joined strings (a character
    beyond one byte raises UnicodeEncodeError, a ValueError)"""
    lengths = np.fromiter((len(s) for s in strings), dtype=np.int64, count=len(strings))
    data = np.frombuffer("".join(strings).encode("latin-1"), dtype=np.uint8)
    return data, np.concatenate([np.zeros(1, np.int64), np.cumsum(lengths, dtype=np.int64)])


def status_error(status):
    """None, or the ValueError that names the first flagged mask and its status bits"""
    bad = np.nonzero(np.asarray(status))[0]
    if bad.size == 0:
        return None
    from ._abi import RLE_STATUS

    s = int(status[bad[0]])
    names = ", ".join(msg for bit, msg in RLE_STATUS.items() if s & bit)
    return ValueError("rle_string_decode: mask %d is malformed (status %d: %s); %d of %d masks are flagged"
                      % (int(bad[0]), s, names, bad.size, len(status)))


def to_str_list(data, byte_offset):
    """the bytes and offsets of rle_strings -> a list of N str (one decode, then slices)"""
    text = bytes(memoryview(np.ascontiguousarray(data, dtype=np.uint8))).decode("ascii")
    off = np.asarray(byte_offset, dtype=np.int64).tolist()
    return [text[off[i]:off[i + 1]] for i in range(len(off) - 1)]
