"""Generate tests/golden/masker_reference.npz by running the REFERENCE's own `Masker` (build container only; never runs on
the GPU box).

The reference is made importable exactly as in make_golden_keypoint.py (make_golden_whole_model's `install_reference`).
The file holds data only.  Per batch b (one `Masker` call over several images, one map size M, one threshold):
  b{b}_maps [N, M, M] fp32, b{b}_boxes [N, 4] fp32 xyxy, b{b}_sizes [I, 2] (H, W) per image, b{b}_counts [I] detections
  per image, b{b}_threshold, b{b}_padding;
  b{b}_planes   the reference's masks, every detection's H x W plane flattened, concatenated and np.packbits-packed;
  b{b}_near     the same layout: pixels whose interpolated value (the reference's expand_masks / expand_boxes and
                `interpolate`) lies within NEAR of the threshold — where an fp32 restatement of ATen's resize may
                legitimately land on the other side (threshold < 0, the `value * 255 != 0` mode: within NEAR of 0 and not 0);
  b{b}_expanded the reference's expand_boxes of the batch's boxes (fp32, before the integer conversion).
And: pad_in / pad_out / pad_scale (expand_masks of three maps), empty_shape (the result for an image without detections).

Maps alternate between sigmoid(3 * randn) and a smooth radial blob (no constant maps: a map of 0.5 is all "near").  The
boxes of an image cycle through: the whole image (the expansion leaves it on all four sides), a sub-pixel box (w = h = 1),
a left and a top edge whose expanded value lies in (-1, 0) (truncation and floor differ), a box wider and taller than the
image, and interior boxes at fractional coordinates.  The reference has no defined answer for a box off the image: none
is in the fixture.

Run:  python tests/golden/make_golden_masker.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_whole_model as W  # noqa: E402,F401  (installs the reference as `maskrcnn_benchmark`)

from maskrcnn_benchmark.layers.misc import interpolate  # noqa: E402
from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import Masker, expand_boxes, expand_masks  # noqa: E402
from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402

NEAR = 1e-5
MAX_NEAR_SHARE = 1e-4

# (M, threshold, [(H, W, detections)])
BATCHES = [
    (28, 0.5, [(80, 64, 67), (40, 53, 0), (33, 17, 1), (7, 1, 4), (20, 15, 6), (24, 16, 6)]),
    (14, 0.5, [(50, 53, 10), (30, 16, 6), (9, 15, 5), (12, 17, 5), (5, 1, 3)]),
    (7, 0.3, [(60, 64, 10), (16, 17, 6), (64, 80, 6)]),
    (14, -1.0, [(31, 33, 6), (18, 16, 5)]),
]


def make_map(rng, M, k):
    if k % 2 == 0:
        return torch.sigmoid(3 * torch.from_numpy(rng.randn(M, M))).float()
    y, x = np.mgrid[0:M, 0:M].astype(np.float64)
    cy, cx = rng.uniform(0.3 * M, 0.7 * M, 2)
    r = rng.uniform(0.25 * M, 0.45 * M)
    d = np.sqrt((y - cy) ** 2 + (x - cx) ** 2)
    return torch.from_numpy(1.0 / (1.0 + np.exp((d - r) * rng.uniform(0.5, 2.0)))).float()


def edge_at(target, hi, scale):
    """lower coordinate of a box [lo, hi] whose expanded lower edge is `target`"""
    return (2 * target - hi * (1 - scale)) / (1 + scale)


def make_boxes(rng, H, W_, n, scale):
    kinds = []
    for k in range(n):
        kind = k % 6 if n > 1 else 5
        if kind == 0:
            b = (0, 0, W_ - 1, H - 1)
        elif kind == 1:
            x, y = rng.uniform(0, max(W_ - 1, 0.5)), rng.uniform(0, max(H - 1, 0.5))
            x, y = np.floor(x) + 0.4, np.floor(y) + 0.4
            b = (x, y, x + 0.1, y + 0.1)
        elif kind == 2:
            x2 = rng.uniform(0.4 * W_, 0.9 * W_) + 1
            y1, y2 = sorted(rng.uniform(0, H, 2))
            b = (edge_at(-rng.uniform(0.2, 0.8), x2, scale), y1, x2, y2 + 1)
        elif kind == 3:
            y2 = rng.uniform(0.4 * H, 0.9 * H) + 1
            x1, x2 = sorted(rng.uniform(0, W_, 2))
            b = (x1, edge_at(-rng.uniform(0.2, 0.8), y2, scale), x2 + 1, y2)
        elif kind == 4:
            b = (-rng.uniform(1, 0.5 * W_ + 2), -rng.uniform(1, 0.5 * H + 2), W_ + rng.uniform(1, 0.5 * W_ + 2),
                 H + rng.uniform(1, 0.5 * H + 2))
        else:
            x1, x2 = sorted(rng.uniform(0, W_, 2))
            y1, y2 = sorted(rng.uniform(0, H, 2))
            b = (x1, y1, x2 + 0.5, y2 + 0.5)
        kinds.append(b)
    return torch.tensor(kinds, dtype=torch.float32).reshape(-1, 4)


def near_plane(mask, box, H, W_, threshold, padding):
    """the reference's paste_mask_in_image (inference.py:119-159) up to the interpolated values, then |value - threshold|"""
    padded, scale = expand_masks(mask[None], padding=padding)
    ib = expand_boxes(box[None], scale)[0].to(dtype=torch.int32)
    x1, y1, x2, y2 = (int(v) for v in ib)
    w, h = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
    v = interpolate(padded[0, 0].expand((1, 1, -1, -1)).to(torch.float32), size=(h, w), mode="bilinear", align_corners=False)[0][0]
    near = (v - max(threshold, 0.0)).abs() <= NEAR
    if threshold < 0:
        near &= v != 0
    out = torch.zeros((H, W_), dtype=torch.bool)
    x_0, x_1, y_0, y_1 = max(x1, 0), min(x2 + 1, W_), max(y1, 0), min(y2 + 1, H)
    assert x_1 > x_0 and y_1 > y_0, "the fixture holds no box off the image"
    out[y_0:y_1, x_0:x_1] = near[y_0 - y1:y_1 - y1, x_0 - x1:x_1 - x1]
    return out, (x1, y1)


def main():
    rng = np.random.RandomState(20240607)
    out = {"n_batches": np.int64(len(BATCHES)), "near_tolerance": np.float64(NEAR)}
    padding = 1
    for b, (M, threshold, images) in enumerate(BATCHES):
        scale = float(M + 2 * padding) / M
        maps, boxes, planes, nears = [], [], [], []
        mask_list, box_list = [], []
        k = 0
        trunc_cases = 0
        for (H, W_, n) in images:
            bx = make_boxes(rng, H, W_, n, scale)
            mp = torch.stack([make_map(rng, M, k + j) for j in range(n)]) if n else torch.zeros((0, M, M))
            k += n
            maps.append(mp)
            boxes.append(bx)
            mask_list.append(mp[:, None])
            box_list.append(BoxList(bx, (W_, H), mode="xyxy"))
        results = Masker(threshold=threshold, padding=padding)(mask_list, box_list)
        for (H, W_, n), mp, bx, res in zip(images, maps, boxes, results):
            if n == 0:
                out["empty_shape"] = np.array(res.shape, np.int64)
                continue
            assert tuple(res.shape) == (n, 1, H, W_) and res.dtype == torch.bool
            exp = expand_boxes(bx, scale)
            trunc_cases += int(((exp[:, :2] > -1) & (exp[:, :2] < 0)).any(dim=1).sum())
            for i in range(n):
                near, _ = near_plane(mp[i], bx[i], H, W_, threshold, padding)
                planes.append(res[i, 0].numpy().reshape(-1))
                nears.append(near.numpy().reshape(-1))
        planes, nears = np.concatenate(planes), np.concatenate(nears)
        share = nears.mean()
        print("batch %d: M=%d thr=%g detections=%d pixels=%d ones=%.3f near=%d (%.2e) trunc!=floor boxes=%d"
              % (b, M, threshold, k, planes.size, planes.mean(), nears.sum(), share, trunc_cases))
        assert share <= MAX_NEAR_SHARE, "too many pixels near the threshold: pick another seed"
        assert trunc_cases > 0
        all_boxes = torch.cat(boxes)
        out["b%d_maps" % b] = torch.cat(maps).numpy()
        out["b%d_boxes" % b] = all_boxes.numpy()
        out["b%d_sizes" % b] = np.array([(H, W_) for H, W_, _ in images], np.int64)
        out["b%d_counts" % b] = np.array([n for _, _, n in images], np.int64)
        out["b%d_threshold" % b] = np.float64(threshold)
        out["b%d_padding" % b] = np.int64(padding)
        out["b%d_planes" % b] = np.packbits(planes)
        out["b%d_near" % b] = np.packbits(nears)
        out["b%d_expanded" % b] = expand_boxes(all_boxes, scale).numpy()
    pad_in = torch.from_numpy(out["b1_maps"][:3])[:, None]
    pad_out, pad_scale = expand_masks(pad_in, padding=2)
    out["pad_in"], out["pad_out"], out["pad_scale"] = pad_in.numpy(), pad_out.numpy(), np.float64(pad_scale)
    assert "empty_shape" in out
    path = os.path.join(HERE, "masker_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
