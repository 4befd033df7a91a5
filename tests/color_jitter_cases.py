"""Shared by test_color_jitter_cpu.py and test_color_jitter_gpu.py: the fixture tests/golden/color_jitter_reference.npz
(tests/golden/make_golden_color_jitter.py: Pillow's own outputs), loaded once, the million-colour sample, and the
batches and records the tests build.  Nothing here imports PIL."""
import functools
import os

import numpy as np
import torch

from maskrcnn_benchmark import _color_jitter_cpu as J

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter_reference.npz")
B, C, S, H = J.BRIGHTNESS, J.CONTRAST, J.SATURATION, J.HUE
# the sample's blue values: the ends, the middle, and their neighbours among sixteen
BLUES = (0, 1, 2, 31, 64, 90, 100, 127, 128, 129, 177, 200, 222, 253, 254, 255)
FOUR_STEPS = [(S, 1.6), (C, 0.7), (H, 37), (B, 1.3)]               # hue not last, contrast in the middle


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_cases():
    """[(source [h, w, 3], record [8], Pillow's output [h, w, 3])]"""
    f = fixture()
    out = []
    for c, (i, rec) in enumerate(zip(f["case_image"].tolist(), f["case_record"])):
        src = f["image_%d" % i]
        lo, hi = f["expected_offset"][c:c + 2]
        out.append((src, rec, f["expected"][lo:hi].reshape(src.shape)))
    return out


@functools.lru_cache(maxsize=None)
def colour_sample():
    """[1024, 1024, 3] uint8: every (r, g) with the sixteen blues: greys and every tie of the maximum among them"""
    r, g, b = np.meshgrid(np.arange(256), np.arange(256), np.asarray(BLUES), indexing="ij")
    out = np.stack([r, g, b], axis=-1).astype(np.uint8).reshape(1024, 1024, 3)
    out.setflags(write=False)
    return out


def record(steps):
    """[(code, factor or k)] -> the int32 [8] record"""
    rec = np.zeros(J.FIELDS, dtype=np.int32)
    for i, (code, par) in enumerate(steps):
        rec[i], rec[J.MAX_STEPS + i] = code, (int(par) if code == H else J.factor_bits(par))
    return rec


def steps_of(rec):
    """the record as RawImage.jitter holds it: [(code, factor as a float, or k)]"""
    return [(code, par if code == H else float(J.bits_factor(par))) for code, par in J.steps_of(rec)]


def batch(images, records):
    """-> RawImageBatch of the images [h, w, 3] uint8 with those records (identity table, no resize)"""
    from maskrcnn_benchmark.data.collate_batch import RawImageBatch
    from maskrcnn_benchmark.data.transforms import RawImage

    table = torch.arange(256, dtype=torch.float32).repeat(3, 1).contiguous()
    return RawImageBatch.pack([RawImage(im, jitter=steps_of(rec)) for im, rec in zip(images, records)], table, False)


def views(buf, N):
    """the buffer's offsets [N] int64, geom [N, 5] int32 and jitter [N, 8] int32"""
    return (buf[:N * 8].view(torch.int64), buf[N * 8:N * 28].view(torch.int32).view(N, 5),
            buf[buf.numel() - N * 32:].view(torch.int32).view(N, 8))


def expected_buffer(b):
    """the batch's buffer after the jitter, by the numpy path image by image"""
    out = b.buffer.numpy().copy()
    N = len(b)
    offsets, geom, jitter = (t.numpy() for t in views(b.buffer, N))
    for off, g, rec in zip(offsets.tolist(), geom.tolist(), jitter):
        n = 3 * g[0] * g[1]
        out[off:off + n] = J.jitter_image(out[off:off + n].reshape(g[0], g[1], 3), rec).reshape(-1)
    return out
