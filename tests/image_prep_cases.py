"""Shared by test_image_prep_cpu.py and test_image_prep_gpu.py: the fixture tests/golden/image_prep_reference.npz
(tests/golden/make_golden_image_prep.py: Pillow's own resizes and the torch expressions of ToTensor / Normalize /
to_image_list), loaded once, and the batches the tests build from it."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep_reference.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def cases():
    f = fixture()
    return [(f["c%d_src" % i], f["c%d_resized" % i]) for i in range(int(f["n_cases"]))]


def batches():
    f = fixture()
    return [{k: f["b%d_%s" % (b, k)] for k in ("cases", "flips", "divisible", "mean", "std", "bgr", "batch")}
            for b in range(int(f["n_batches"]))]


def bits(a):
    """float32 array or tensor -> its bit patterns (so that -0.0 != +0.0 and NaNs compare)"""
    a = a.detach().cpu().contiguous().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def raw_batch(items, table, bgr, divisible=0, channels_last=False):
    """items: [(src [h, w, 3] uint8, (oh, ow), flip bits)] -> RawImageBatch"""
    from maskrcnn_benchmark.data.collate_batch import RawImageBatch
    from maskrcnn_benchmark.data.transforms import RawImage

    images = [RawImage(src, (ow, oh), flip) for src, (oh, ow), flip in items]
    return RawImageBatch.pack(images, table, bgr, divisible, channels_last)


def identity_table():
    """table[c][v] = v: the batch shows the resized bytes themselves"""
    return torch.arange(256, dtype=torch.float32).repeat(3, 1).contiguous()


def flipped(img, flip):
    img = img[:, ::-1] if flip & 1 else img
    return img[::-1] if flip & 2 else img
