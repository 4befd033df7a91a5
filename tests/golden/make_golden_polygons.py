"""Generate tests/golden/polygons_reference.npz by running the REFERENCE's own polygon structures (build container only;
never runs on the GPU box).

The reference is made importable exactly as in make_golden_masker.py (make_golden_whole_model's `install_reference`; its
pycocotools / cv2 stubs make `PolygonInstance` / `PolygonList` importable).  Only the GEOMETRY is recorded: the reference
rasterises through pycocotools, which is not installed.  The file holds data only.  Per image i:
  i{i}_size (W, H); the raw input as i{i}_numbers (all coordinates, concatenated), i{i}_poly_len (numbers per polygon, some
  below 6) and i{i}_inst_npoly (polygons per instance, in order);
  i{i}_n_kept        instances the list keeps (polygons of fewer than 6 numbers and instances left empty are dropped);
  i{i}_boxes [B, 4] fp32 xyxy and i{i}_box_inst [B] (index into the kept instances);
  i{i}_cr_M{M}       for M in `sizes`: the vertex arrays after crop(box).resize((M, M)), concatenated over the boxes and
                     each box's polygons in order;
  i{i}_flip0 / _flip1  after transpose(FLIP_LEFT_RIGHT / FLIP_TOP_BOTTOM), concatenated over all kept polygons;
  i{i}_resize_to, i{i}_resized       a non-square resize (different ratios per axis);
  i{i}_resize_eq_to, i{i}_resized_eq a resize with equal ratios (the reference's scalar branch);
  i{i}_getitem       lengths after __getitem__ with an int, a slice, a list, an index tensor and a bool tensor (the items
                     are fixed in GETITEMS below; the bool mask keeps the even instances).
The boxes of an image: interior fractional boxes, one clamped at each border, one whose xmin is clamped to W - 1 (wholly
right of the image), one larger than the image, a sub-pixel box and a box disjoint from its instance.

Run:  python tests/golden/make_golden_polygons.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_whole_model as W  # noqa: E402,F401  (installs the reference as `maskrcnn_benchmark`)

from maskrcnn_benchmark.structures.segmentation_mask import (  # noqa: E402
    FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, PolygonList, SegmentationMask)

SIZES = (28, 14, 7)
IMAGES = [(64, 48), (33, 50)]


def getitems(n):
    """the five __getitem__ forms on a list of n instances"""
    return [1, slice(1, n), [0, n - 1], torch.tensor([n - 1, 0, 1]), torch.tensor([k % 2 == 0 for k in range(n)])]


def star(rng, cx, cy, r, k):
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(0.5, 1.0, k) * r
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).astype(np.float32).reshape(-1).tolist()


def make_image(rng, Wd, Ht):
    inst = []
    inst.append([star(rng, 0.4 * Wd, 0.5 * Ht, 0.3 * Ht, 7)])
    inst.append([star(rng, 0.6 * Wd, 0.4 * Ht, 0.25 * Ht, 5), star(rng, 0.65 * Wd, 0.5 * Ht, 0.2 * Ht, 9)])
    inst.append([[1.0, 2.0, 3.0, 4.0]])                                    # too short: the instance is dropped
    inst.append([star(rng, 0.3 * Wd, 0.3 * Ht, 0.2 * Ht, 3), [5.0, 5.0, 6.0, 6.0]])   # its second polygon is dropped
    inst.append([star(rng, 0.5 * Wd, 0.5 * Ht, 0.7 * Ht, 8)])               # leaves the image
    inst.append([[2.0, 3.0, 2.0, 3.0, Wd - 4.0, 3.0, Wd - 4.0, Ht - 5.0, 2.0, Ht - 5.0]])   # a repeated vertex
    return inst


def make_boxes(rng, Wd, Ht, n_kept):
    b = []
    for _ in range(3):
        x1, x2 = sorted(rng.uniform(0, Wd, 2))
        y1, y2 = sorted(rng.uniform(0, Ht, 2))
        b.append((x1, y1, x2 + 0.37, y2 + 0.61))
    b.append((-7.3, 0.2 * Ht, 0.5 * Wd, 0.7 * Ht))            # left border
    b.append((0.2 * Wd, -3.6, 0.8 * Wd, 0.6 * Ht))            # top border
    b.append((0.4 * Wd, 0.3 * Ht, Wd + 9.2, 0.9 * Ht))        # right border
    b.append((0.1 * Wd, 0.5 * Ht, 0.6 * Wd, Ht + 4.4))        # bottom border
    b.append((Wd + 3.0, 5.0, Wd + 10.0, 20.0))                # xmin clamped to W - 1
    b.append((-11.0, -6.5, Wd + 12.5, Ht + 8.0))              # larger than the image
    b.append((0.4 * Wd + 0.3, 0.5 * Ht + 0.2, 0.4 * Wd + 0.4, 0.5 * Ht + 0.3))   # sub-pixel
    b.append((Wd - 3.0, Ht - 3.0, Wd - 1.0, Ht - 1.0))        # disjoint from instance 2 (top left)
    boxes = torch.tensor(b, dtype=torch.float32)
    inst = [k % n_kept for k in range(len(b))]
    inst[-1] = 2
    return boxes, np.array(inst, np.int64)


def flat(polygon_list):
    parts = [p.numpy() for inst in polygon_list for p in inst.polygons]
    return np.concatenate(parts).astype(np.float32) if parts else np.zeros(0, np.float32)


def main():
    rng = np.random.RandomState(20241018)
    out = {"n_images": np.int64(len(IMAGES)), "sizes": np.array(SIZES, np.int64)}
    for i, (Wd, Ht) in enumerate(IMAGES):
        raw = make_image(rng, Wd, Ht)
        plist = PolygonList(raw, (Wd, Ht))
        assert len(SegmentationMask(raw, (Wd, Ht), mode="poly")) == len(plist)
        n = len(plist)
        boxes, box_inst = make_boxes(rng, Wd, Ht, n)
        k = "i%d_" % i
        out[k + "size"] = np.array([Wd, Ht], np.int64)
        out[k + "numbers"] = np.array([v for inst in raw for p in inst for v in p], np.float32)
        out[k + "poly_len"] = np.array([len(p) for inst in raw for p in inst], np.int64)
        out[k + "inst_npoly"] = np.array([len(inst) for inst in raw], np.int64)
        out[k + "n_kept"] = np.int64(n)
        out[k + "boxes"] = boxes.numpy()
        out[k + "box_inst"] = box_inst
        for M in SIZES:
            parts = []
            for b, g in zip(boxes, box_inst):
                r = plist.polygons[int(g)].crop(b).resize((M, M))
                assert r.size == (M, M)
                parts.extend(p.numpy() for p in r.polygons)
            out[k + "cr_M%d" % M] = np.concatenate(parts).astype(np.float32)
        out[k + "flip0"] = flat(plist.transpose(FLIP_LEFT_RIGHT))
        out[k + "flip1"] = flat(plist.transpose(FLIP_TOP_BOTTOM))
        to = (Wd * 2 - 7, Ht + 13)
        out[k + "resize_to"] = np.array(to, np.int64)
        out[k + "resized"] = flat(plist.resize(to))
        to = (Wd * 3, Ht * 3)
        out[k + "resize_eq_to"] = np.array(to, np.int64)
        out[k + "resized_eq"] = flat(plist.resize(to))
        out[k + "getitem"] = np.array([len(plist[item]) for item in getitems(n)], np.int64)
        print("image %d: %d x %d, %d raw instances, %d kept, %d boxes" % (i, Wd, Ht, len(raw), n, len(boxes)))
    out["empty_len"] = np.int64(len(PolygonList([], (10, 10))))
    path = os.path.join(HERE, "polygons_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
