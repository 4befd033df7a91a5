"""Host implementation of the batch image preparation defined in include/detops.h (detops_image_batch_u8), for CPU
tensors (numpy): Pillow's bilinear resize of RGB uint8 restated as integer arithmetic, flips, the 256-entry
normalisation table and the zero-padded batch.  The same formulation as csrc/image_prep.hip: per axis and output index a
first tap, a tap count and 22-bit integer coefficients made in fp64; the horizontal pass first, its rounded and clipped
uint8 result the input of the vertical pass; an axis that keeps its size is not resampled.
"""
import numpy as np

PRECISION_BITS = 22            # Pillow: 32 - 8 - 2
GEOM_FIELDS = 5                # per image: source h, w, destination oh, ow, flip bits (1 horizontal, 2 vertical)


def axis_ksize(insize, outsize):
    """the filter's tap budget of one axis: ceil(max(in / out, 1)) * 2 + 1"""
    return int(np.ceil(max(float(insize) / float(outsize), 1.0))) * 2 + 1


def axis_taps(insize, outsize):
    """-> (lo [out], n [out], k [out, ksize]) int32: output index xx sums in[lo + x] * k[x] over x < n (k is 0 beyond n)"""
    insize, outsize = int(insize), int(outsize)
    scale = float(insize) / float(outsize)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(outsize, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / fs
    lo = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    n = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), insize) - lo
    x = np.arange(ksize, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs(((x + lo[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss))
    w = np.where(x < n[:, None], w, 0.0)
    total = np.cumsum(w, axis=1)[:, -1:]              # the sequential sum (np.sum adds pairwise); trailing zeros add nothing
    w = np.where(total != 0.0, w / np.where(total != 0.0, total, 1.0), w)
    k = np.trunc(w * float(1 << PRECISION_BITS) + 0.5).astype(np.int32)
    return lo.astype(np.int32), n.astype(np.int32), k


def _resample(img, axis, outsize):
    """one pass over `axis` (0 or 1) of img [h, w, 3] uint8"""
    insize = img.shape[axis]
    if insize == outsize:
        return img
    lo, n, k = axis_taps(insize, outsize)
    src = img.astype(np.int32)
    shape = [1, 1, 1]
    shape[axis] = outsize
    acc = np.full([outsize if a == axis else s for a, s in enumerate(img.shape)], 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for t in range(k.shape[1]):
        idx = np.minimum(lo + t, insize - 1)          # taps beyond n carry coefficient 0
        acc += np.take(src, idx, axis=axis) * k[:, t].reshape(shape)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_u8(img, oh, ow):
    """img [h, w, 3] uint8 -> [oh, ow, 3] uint8, bit for bit Image.resize((ow, oh), Image.BILINEAR)"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    return _resample(_resample(img, 1, int(ow)), 0, int(oh))


def image_batch(raw, offsets, geom, table, bgr, Hp, Wp):
    """raw [bytes] uint8 (RGB HWC images at byte `offsets` [N]), geom [N, 5] int32, table [3, 256] float32 (the value of
    output channel c for a byte of the source channel it reads: 2 - c with `bgr`, else c) -> float32 [N, 3, Hp, Wp], +0.0
    where no image is"""
    raw, table = np.asarray(raw, dtype=np.uint8).reshape(-1), np.asarray(table, dtype=np.float32)
    geom = np.asarray(geom, dtype=np.int32).reshape(-1, GEOM_FIELDS)
    N = geom.shape[0]
    out = np.zeros((N, 3, int(Hp), int(Wp)), dtype=np.float32)
    for i in range(N):
        h, w, oh, ow, flip = (int(v) for v in geom[i])
        if min(h, w, oh, ow) < 1 or oh > Hp or ow > Wp:
            raise ValueError("image_batch: image %d has sizes %s for a batch of %d x %d" % (i, geom[i].tolist(), Hp, Wp))
        o = int(offsets[i])
        img = resize_u8(raw[o:o + h * w * 3].reshape(h, w, 3), oh, ow)
        if flip & 1:
            img = img[:, ::-1]
        if flip & 2:
            img = img[::-1]
        for c in range(3):
            out[i, c, :oh, :ow] = table[c][img[:, :, 2 - c if bgr else c]]
    return out
