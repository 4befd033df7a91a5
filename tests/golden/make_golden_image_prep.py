"""Generate tests/golden/image_prep_reference.npz with Pillow and torch only (build container only; the GPU tests read the
file and never import PIL).

The reference's data/transforms/transforms.py goes through torchvision, whose resize of a PIL image is
`img.resize((ow, oh), Image.BILINEAR)`; that call is made here directly.  The file holds data only:
  n_cases; per case i: c{i}_src [h, w, 3] uint8 (a smooth gradient plus noise), c{i}_resized [oh, ow, 3] uint8 = Pillow's
                       output (CASES below lists the (h, w) -> (oh, ow) pairs and why each is there);
  n_batches; per batch b: b{b}_cases (case indices), b{b}_flips (bit 0 horizontal, bit 1 vertical), b{b}_divisible
                       (SIZE_DIVISIBILITY), b{b}_mean, b{b}_std, b{b}_bgr (PIXEL_MEAN, PIXEL_STD, TO_BGR255) and b{b}_batch
                       [N, 3, Hp, Wp] float32: the flipped Pillow outputs through ToTensor, Normalize and to_image_list written
                       out as torch expressions.

Run:  python tests/golden/make_golden_image_prep.py
"""
import os

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# (h, w) -> (oh, ow)
CASES = [
    ((37, 53), (61, 88)),      # upscale in both axes
    ((120, 90), (50, 37)),     # downscale in both axes
    ((33, 47), (33, 90)),      # horizontal pass only
    ((47, 33), (90, 33)),      # vertical pass only
    ((5, 7), (1, 1)),          # everything into one pixel
    ((9, 1), (20, 3)),         # a one-pixel-wide source
    ((40, 30), (40, 30)),      # no resize at all
    ((20, 50), (30, 65)),      # output width one past a wave
    ((24, 100), (10, 129)),    # output width one past two waves; down vertically, up horizontally
]

# (cases, flips, SIZE_DIVISIBILITY, PIXEL_MEAN, PIXEL_STD, TO_BGR255)
BATCHES = [
    ((0, 1, 4), (0, 1, 2), 32, (102.9801, 115.9465, 122.7717), (1.0, 1.0, 1.0), True),
    ((2, 3, 5), (3, 0, 1), 0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), False),
    ((6, 7, 8), (0, 3, 2), 32, (102.9801, 115.9465, 122.7717), (57.375, 57.12, 58.395), True),
]


def source(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [255.0 * xx / max(w - 1, 1), 255.0 * yy / max(h - 1, 1), 127.5 + 127.5 * np.sin(0.3 * xx + 0.2 * yy)]
    img = np.stack(planes, axis=2) + rng.normal(0.0, 25.0, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def normalised(img, mean, std, bgr):
    """ToTensor and Normalize of an [h, w, 3] uint8 image"""
    t = torch.from_numpy(np.array(img)).permute(2, 0, 1).to(torch.float32) / 255
    if bgr:
        t = t[[2, 1, 0]] * 255
    mean, std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return (t - mean[:, None, None]) / std[:, None, None]


def main():
    rng = np.random.RandomState(20241)
    out = {"n_cases": np.int64(len(CASES)), "n_batches": np.int64(len(BATCHES))}
    resized = []
    for i, ((h, w), (oh, ow)) in enumerate(CASES):
        src = source(rng, h, w)
        res = np.asarray(Image.fromarray(src, "RGB").resize((ow, oh), Image.BILINEAR))
        assert res.shape == (oh, ow, 3) and res.dtype == np.uint8
        out["c%d_src" % i], out["c%d_resized" % i] = src, res
        resized.append(res)
    for b, (cases, flips, div, mean, std, bgr) in enumerate(BATCHES):
        imgs = []
        for c, f in zip(cases, flips):
            img = resized[c]
            img = img[:, ::-1] if f & 1 else img
            img = img[::-1] if f & 2 else img
            imgs.append(normalised(img, mean, std, bgr))
        H, W = max(t.shape[1] for t in imgs), max(t.shape[2] for t in imgs)
        if div > 0:
            H, W = (H + div - 1) // div * div, (W + div - 1) // div * div
        batch = torch.zeros((len(imgs), 3, H, W), dtype=torch.float32)
        for t, slot in zip(imgs, batch):
            slot[:, :t.shape[1], :t.shape[2]].copy_(t)
        out.update({"b%d_cases" % b: np.asarray(cases, np.int64), "b%d_flips" % b: np.asarray(flips, np.int64),
                    "b%d_divisible" % b: np.int64(div), "b%d_mean" % b: np.asarray(mean, np.float64),
                    "b%d_std" % b: np.asarray(std, np.float64), "b%d_bgr" % b: np.bool_(bgr), "b%d_batch" % b: batch.numpy()})
    path = os.path.join(HERE, "image_prep_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
