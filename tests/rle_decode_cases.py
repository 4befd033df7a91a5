"""TEST-ONLY: the inputs shared by tests/test_rle_decode_cpu.py and tests/test_rle_decode_gpu.py: strings to decode (well
formed and malformed) and planes whose runs go to mask_pack_rle."""
import numpy as np
import torch

import rle_string_refs as R
from maskrcnn_benchmark import _rle_cpu

BAD_BYTE, TRUNCATED, LONG_VALUE, BAD_RUN, BAD_SUM = 1, 2, 4, 8, 16

# (string, (h, w), the bit the case is about, the whole expected status) — every bit by a hand-made string of its own
MALFORMED = [
    ("/", (1, 0), BAD_BYTE, BAD_BYTE | TRUNCATED | BAD_RUN | BAD_SUM),   # 47: below the alphabet (and reads as -1, "more")
    ("p0", (1, 0), BAD_BYTE, BAD_BYTE),                 # 112 = 48 + 64: above it; its low six bits are the value 0
    ("P", (1, 0), TRUNCATED, TRUNCATED),                # the continuation bit and nothing after it
    ("0" + "o" * 7 + "0", (1, 0), LONG_VALUE, LONG_VALUE | BAD_SUM),     # an 8-byte value
    ("00N0", (1, 0), BAD_RUN, BAD_RUN | BAD_SUM),       # N = -2 as run 2
    ("1N3", (1, 2), BAD_RUN, BAD_RUN),                  # [1, -2, 3]: sums to 2 = 1 * 2, still a negative run
    (R.rle_to_string([0, 2 ** 31 - 1, 0, 2 ** 31]), (1, 0), BAD_RUN, BAD_RUN | BAD_SUM),     # run 3 = run 1 + 1 = 2^31
    ("53", (3, 3), BAD_SUM, BAD_SUM),                   # 5 + 3 = 8 of 9 pixels: off by one
    ("", (0, 5), 0, 0),
    ("", (1, 1), BAD_SUM, BAD_SUM),                     # no runs for one pixel
]


def seeded_strings():
    masks = R.seeded_masks()
    return masks, [R.rle_to_string(m) for m in masks]


def long_and_short():
    """one mask of 50,000 values next to masks of 0, 1 and 3 values"""
    rng = np.random.RandomState(11)
    big = rng.randint(0, 3000, 50000).tolist()
    masks = [[], [7], big, [1, 2, 3], []]
    return masks, [R.rle_to_string(m) for m in masks]


def tensors(strings, device="cpu"):
    data, byte_offset = _rle_cpu.from_str_list(strings)
    return torch.from_numpy(data.copy()).to(device), torch.from_numpy(byte_offset).to(device)


def runs_of(plane):
    """the literal run-length coding of one plane: column-major, starting with a 0-run"""
    flat = np.asarray(plane).T.reshape(-1) != 0
    runs, value, n = [], False, 0
    for v in flat.tolist():
        if v != value:
            runs.append(n)
            value, n = v, 0
        n += 1
    runs.append(n)
    return runs


def plane_of(runs, h, w):
    """the literal inverse: pixel (y, x) is set iff position x * h + y lies in an odd-indexed run"""
    flat = np.zeros(h * w, dtype=np.uint8)
    p = 0
    for i, r in enumerate(runs):
        if i & 1:
            flat[p:p + r] = 1
        p += r
    assert p == h * w
    return flat.reshape(w, h).T.copy()


def pack_cases(extra_h=()):
    """-> (planes [list of uint8 H x W], runs [list of lists]): random planes of the word shapes of
    test_evaluation_gpu.plane_groups, 130 x 20 (more than one LDS word per column), all-zero and all-one planes,
    zero-length runs in the middle, one run over several whole columns across a strip boundary; `extra_h`: heights of
    further random planes of 3 columns"""
    rng = np.random.RandomState(5)
    planes = [(rng.rand(h, w) < 0.3).astype(np.uint8) for h, w in ((7, 1), (33, 17), (64, 80), (20, 130), (5, 64), (130, 20))]
    planes += [(rng.rand(h, 3) < 0.5).astype(np.uint8) for h in extra_h]
    runs = [runs_of(p) for p in planes]
    for h, w in ((6, 70), (130, 20)):
        planes += [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)]
        runs += [[h * w], [0, h * w]]
    toggles = [0, 0, 3, 0, 0, 2, 0, 4, 0, 0, 0, 11]           # 4 x 5: zero-length runs that only toggle
    planes.append(plane_of(toggles, 4, 5))
    runs.append(toggles)
    across = [10 * 59 + 3, 10 * 11 - 3, 10 * 150 - 10 * 70]   # 10 x 150: one run from column 59 over the strip boundary at 64
    planes.append(plane_of(across, 10, 150))
    runs.append(across)
    return planes, runs


def run_tensors(runs, device="cpu"):
    counts = torch.tensor([v for r in runs for v in r], dtype=torch.int32)
    run_offset = torch.tensor(np.concatenate([[0], np.cumsum([len(r) for r in runs])]), dtype=torch.int64)
    return counts.to(device), run_offset.to(device)
