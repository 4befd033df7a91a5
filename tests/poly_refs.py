"""Test-only references for the polygon fill (include/detops.h, "Polygon instance masks").

`crossings` / `fill` are the LITERAL restatement of the polygon-to-RLE routine: the point-by-point walk of the upsampled
boundary, exactly as the definition states it.  It has not been checked against pycocotools (not installed here).
`centre_fill` is an independent rule: a pixel is set iff its centre (col + .5, row + .5) lies inside the polygon
(even-odd).  `star_cases` generates the seeded polygons both test files use.
"""
import math

import numpy as np


def crossings(xy, h, w):                       # literal; int() truncates toward zero like C's (int)
    k = len(xy) // 2
    x = [int(5.0 * xy[2 * j] + .5) for j in range(k)]
    x.append(x[0])
    y = [int(5.0 * xy[2 * j + 1] + .5) for j in range(k)]
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(ys if dx == 0 else int(ys + ((ye - ys) / dx) * t + .5))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + ((xe - xs) / dy) * t + .5))
    out = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / 5.0 - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(min(v[j], v[j - 1]))
            yd = (yd + .5) / 5.0 - .5
            yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
            out.append(int(xd) * h + int(math.ceil(yd)))
    return out                                  # positions in COLUMN-major order, 0 .. h*w inclusive


def fill(xy, h, w):
    """one polygon xy = [x0, y0, x1, y1, ...] (floats) -> uint8 [h, w]"""
    xy = [float(a) for a in xy]
    t = np.zeros(h * w + 1, np.uint8)
    for c in crossings(xy, h, w):
        t[c] ^= 1
    return (np.cumsum(t)[:h * w] & 1).astype(np.uint8).reshape(w, h).T     # [h, w]


def fill_instance(polygons, h, w):
    """union of the polygons' fills"""
    out = np.zeros((h, w), np.uint8)
    for p in polygons:
        if len(p) >= 6:
            out |= fill(p, h, w)
    return out


def centre_fill(xy, h, w):
    """even-odd rule at the pixel centres -> uint8 [h, w]"""
    px = np.asarray(xy, np.float64).reshape(-1, 2)
    cx = np.arange(w)[None, :, None] + 0.5
    cy = np.arange(h)[:, None, None] + 0.5
    x0, y0 = px[:, 0][None, None, :], px[:, 1][None, None, :]
    x1, y1 = np.roll(px[:, 0], -1)[None, None, :], np.roll(px[:, 1], -1)[None, None, :]
    straddle = (y0 <= cy) != (y1 <= cy)
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = x0 + (cy - y0) * (x1 - x0) / (y1 - y0)
    return ((straddle & (xi > cx)).sum(axis=2) & 1).astype(np.uint8)


def l1_perimeter(xy):
    px = np.asarray(xy, np.float64).reshape(-1, 2)
    return float(np.abs(px - np.roll(px, -1, axis=0)).sum())


def star_cases(n, seed):
    """n seeded cases (xy float32 flat list, h, w): star polygons of 3-8 vertices, radii 0.2-0.7 of the grid around a
    centre in 0.2-0.8 of it (many leave the grid); grids 5-60 (every third 28 x 28); a fifth with integer vertices"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        if i % 3 == 0:
            h = w = 28
        else:
            h, w = int(rng.randint(5, 61)), int(rng.randint(5, 61))
        k = int(rng.randint(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(0.2, 0.7, k)
        cx, cy = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h
        px = np.stack([cx + rad * w * np.cos(ang), cy + rad * h * np.sin(ang)], axis=1)
        if i % 5 == 4:
            px = np.round(px)
        out.append((px.astype(np.float32).reshape(-1).tolist(), h, w))
    return out


# hand-made shapes: repeated vertices, axis-aligned edges on integers and on x.5, vertices in (-0.1, 0)
SPECIAL_CASES = [
    ([2, 2, 6, 2, 6, 6, 2, 6], 8, 8),
    ([2, 2, 2, 2, 6, 2, 6, 6, 6, 6, 2, 6, 2, 6], 8, 8),
    ([1.5, 1.5, 9.5, 1.5, 9.5, 7.5, 1.5, 7.5], 10, 12),
    ([0, 0, 12, 0, 12, 10, 0, 10], 10, 12),
    ([-0.05, -0.05, 7.3, -0.09, 7.3, 5.2, -0.02, 5.2], 9, 9),
    ([-0.05, 3, 4, -0.05, 8.5, 3, 4, 8.5], 9, 9),
    ([3, 3, 3, 3, 3, 3], 7, 7),
    ([1, 1, 5, 1, 5, 1, 5, 5, 1, 5, 1, 1], 7, 7),
    ([-20.5, -13.25, 40, -7, 33.5, 41, -9, 30], 28, 28),
    ([3.5, -4, 3.5, 40, 20.5, 40, 20.5, -4], 28, 28),
]


def fixture_image(fx, i):
    """image i of tests/golden/polygons_reference.npz -> (raw nested polygon lists, (W, H), boxes [B, 4], box_inst [B])"""
    k = "i%d_" % i
    numbers, at, raw = fx[k + "numbers"], 0, []
    lens = iter(fx[k + "poly_len"].tolist())
    for npoly in fx[k + "inst_npoly"].tolist():
        inst = []
        for _ in range(npoly):
            n = next(lens)
            inst.append(numbers[at:at + n].tolist())
            at += n
        raw.append(inst)
    size = tuple(int(v) for v in fx[k + "size"])
    return raw, size, fx[k + "boxes"], fx[k + "box_inst"]


def slot_target(instance, box, M):
    """the definition's target of one slot: the fill of instance.crop(box).resize((M, M)) (a PolygonInstance of the
    product, whose geometry the fixture pins) on the M x M grid -> uint8 [M, M]"""
    r = instance.crop(box).resize((M, M))
    return fill_instance([p.tolist() for p in r.polygons], M, M)
