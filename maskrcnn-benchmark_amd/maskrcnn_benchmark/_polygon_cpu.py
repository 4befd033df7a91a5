"""Host implementation of the polygon fill defined in include/detops.h, for CPU tensors (numpy).

The same formulation as csrc/polygon.hip: the work item is one (edge, column) pair.  An edge's walk steps across
u = 5c + 2 | 5c + 3 at most once per column c; where it does, the step follows in closed form (x-major edges) or from an
estimate that the literal u(t) corrects (y-major edges).  Crossings clamped to row h are dropped and the prefix parity
is taken per column: a closed polygon crosses a column's boundary an even number of times, so this is the fill of the
definition's running parity through all columns.  Nothing here walks the upsampled boundary point by point.
"""
import numpy as np

COORD_LIMIT = 500000000.0


def _scaled(v):
    """int(5.0 * v + .5): fp64, two roundings, truncation toward zero; NaN and |values| beyond 5e8 saturate"""
    z = 5.0 * np.asarray(v, dtype=np.float64)
    z = z + 0.5
    z = np.where(z > -COORD_LIMIT, np.minimum(z, COORD_LIMIT), -COORD_LIMIT)
    return np.trunc(z).astype(np.int64)


def _walk_point(a, s, t):
    """int(a + s * t + .5)"""
    z = s * t.astype(np.float64)
    z = a.astype(np.float64) + z
    z = z + 0.5
    return np.trunc(z).astype(np.int64)


def fill_polygon(xy, h, w):
    """xy [k, 2] (float32 vertices, k >= 3) -> bool [h, w]"""
    xy = np.asarray(xy)
    out = np.zeros((h, w), dtype=bool)
    if xy.shape[0] < 3 or h <= 0 or w <= 0:
        return out
    x, y = _scaled(xy[:, 0]), _scaled(xy[:, 1])
    xe, ye = np.roll(x, -1), np.roll(y, -1)
    A = 5 * np.arange(w, dtype=np.int64) + 2
    hit = (np.minimum(x, xe)[:, None] <= A[None, :]) & (np.maximum(x, xe)[:, None] > A[None, :])
    e, c = np.nonzero(hit)
    if e.size == 0:
        return out
    xs, ys, xe, ye, A = x[e], y[e], xe[e], ye[e], A[c]
    dx, dy = np.abs(xe - xs), np.abs(ys - ye)
    x_major = dx >= dy
    flip = np.where(x_major, xs > xe, ys > ye)
    xs, xe = np.where(flip, xe, xs), np.where(flip, xs, xe)
    ys, ye = np.where(flip, ye, ys), np.where(flip, ys, ye)
    vm = np.zeros_like(xs)
    m = x_major
    if m.any():
        s = (ye[m] - ys[m]).astype(np.float64) / dx[m].astype(np.float64)
        t = A[m] - xs[m]
        vm[m] = np.minimum(_walk_point(ys[m], s, t), _walk_point(ys[m], s, t + 1))
    m = ~x_major
    if m.any():
        a, b, top, n, col = xs[m], xe[m], ys[m], dy[m], A[m]
        s = (b - a).astype(np.float64) / n.astype(np.float64)
        up = b > a
        tau = (col.astype(np.float64) + 0.5 - a.astype(np.float64)) / s
        t = np.where(up, np.ceil(tau), np.floor(tau) + 1.0)
        t = np.minimum(np.maximum(t, 1.0), n.astype(np.float64)).astype(np.int64)

        def reached(tt):
            u = _walk_point(a, s, tt)
            return np.where(up, u > col, u <= col)

        while True:   # the estimate is off by a step at most: u(t) decides
            back = (t > 1) & reached(t - 1)
            if not back.any():
                break
            t = t - back
        while True:
            fwd = (t < n) & ~reached(t)
            if not fwd.any():
                break
            t = t + fwd
        vm[m] = t - 1 + top
    r = np.where(vm - 2 <= 0, 0, (vm - 2 + 4) // 5)
    keep = r < h
    counts = np.zeros((w, h), dtype=np.int64)
    np.add.at(counts, (c[keep], r[keep]), 1)
    return ((np.cumsum(counts, axis=1) & 1) != 0).T


def fill_instance(verts, poly_offset, p0, p1, h, w, transform=None):
    """union of the fills of polygons [p0, p1) of the packed arrays; transform(xy [k, 2] float32) -> [k, 2] float32"""
    out = np.zeros((h, w), dtype=bool)
    V = verts.shape[0]
    for p in range(p0, p1):
        v0 = min(max(int(poly_offset[p]), 0), V)
        v1 = min(max(int(poly_offset[p + 1]), v0), V)
        xy = verts[v0:v1]
        if transform is not None:
            xy = transform(xy)
        out |= fill_polygon(xy, h, w)
    return out


def crop_resize(box, W, H, M):
    """PolygonInstance.crop(box).resize((M, M)) on fp32 vertices: the window and the quotient in fp64, no rounding of the
    window, fp32(fp32(x - xmin) * fp32(M / (xmax - xmin)))"""
    b0, b1, b2, b3 = (float(v) for v in box)
    xmin = min(max(b0, 0.0), float(W - 1))
    ymin = min(max(b1, 0.0), float(H - 1))
    xmax = max(min(max(b2, 0.0), float(W)), xmin + 1.0)
    ymax = max(min(max(b3, 0.0), float(H)), ymin + 1.0)
    lo = np.array([xmin, ymin], dtype=np.float32)
    f = np.array([M / (xmax - xmin), M / (ymax - ymin)], dtype=np.float64).astype(np.float32)
    return lambda xy: (xy.astype(np.float32) - lo) * f


def polygon_mask_targets(verts, poly_offset, inst_offset, slot_inst, boxes, slot_wh, M):
    """numpy arrays -> [S, M, M] float32"""
    S, G, P = len(slot_inst), len(inst_offset) - 1, len(poly_offset) - 1
    out = np.zeros((S, M, M), dtype=np.float32)
    for s in range(S):
        g = int(slot_inst[s])
        if g < 0 or g >= G:
            continue
        p0 = min(max(int(inst_offset[g]), 0), P)
        p1 = min(max(int(inst_offset[g + 1]), p0), P)
        xf = crop_resize(boxes[s], int(slot_wh[s][0]), int(slot_wh[s][1]), M)
        out[s] = fill_instance(verts, poly_offset, p0, p1, M, M, xf)
    return out


def polygons_to_masks(verts, poly_offset, inst_offset, H, W):
    """numpy arrays -> [G, H, W] uint8"""
    G, P = len(inst_offset) - 1, len(poly_offset) - 1
    out = np.zeros((G, H, W), dtype=np.uint8)
    for g in range(G):
        p0 = min(max(int(inst_offset[g]), 0), P)
        p1 = min(max(int(inst_offset[g + 1]), p0), P)
        out[g] = fill_instance(verts, poly_offset, p0, p1, H, W)
    return out
