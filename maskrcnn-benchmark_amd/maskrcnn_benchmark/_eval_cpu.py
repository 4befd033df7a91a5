"""Host implementation of the detection-evaluation steps defined in include/detops.h ("Detection evaluation"), for CPU
tensors and for the problems csrc/evaluate.hip does not serve (more than MAX_GT ground truths): numpy, the same four
steps with the same arguments — mask_pack, mask_pair_counts, eval_iou, eval_match.

A problem is the detections (score descending, ties in input order) and the ground truths of one (image, category) pair;
dt_offset / gt_offset [P + 1] delimit them in the sorted arrays and iou_offset [P + 1] its D_p x G_p row-major IoU matrix.
"""
import numpy as np

COCO_SEGM, COCO_BBOX, VOC = 0, 1, 2
MAX_GT = 4096    # DETOPS_EVAL_MAX_GT

_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def _popcount(words):
    return int(_POP8[np.ascontiguousarray(words).view(np.uint8)].sum())


def mask_pack(planes):
    """planes: a list of [n_i, H_i, W_i] arrays (non-zero = set) -> (words uint64 [total], word_offset int64 [N],
    hw int32 [N, 2], area int32 [N], extent int32 [N, 4]): rows of ceil(W / 64) words, bit b of word c = pixel 64 c + b;
    extent = first / last non-empty row, first / last non-empty word column, (H, -1, ceil(W / 64), -1) when empty"""
    words, offs, hw, area, extent = [], [], [], [], []
    total = 0
    shifts = np.arange(64, dtype=np.uint64)
    for group in planes:
        group = np.asarray(group)
        n, H, W = group.shape
        WW = (W + 63) // 64
        for k in range(n):
            bits = np.zeros((H, WW * 64), dtype=np.uint64)
            bits[:, :W] = group[k] != 0
            w = (bits.reshape(H, WW, 64) << shifts).sum(axis=2, dtype=np.uint64) if H and WW else np.zeros((H, WW), np.uint64)
            rows, cols = np.nonzero(w.any(axis=1))[0], np.nonzero(w.any(axis=0))[0]
            extent.append((rows[0], rows[-1], cols[0], cols[-1]) if rows.size else (H, -1, WW, -1))
            area.append(int((group[k] != 0).sum()))
            hw.append((H, W))
            offs.append(total)
            words.append(w.reshape(-1))
            total += H * WW
    return (np.concatenate(words) if words else np.zeros((0,), np.uint64), np.array(offs, np.int64).reshape(-1),
            np.array(hw, np.int32).reshape(-1, 2), np.array(area, np.int32).reshape(-1),
            np.array(extent, np.int32).reshape(-1, 4))


def mask_pack_rle(counts, run_offset, hw):
    """mask_pack of the planes that uncompressed RLE describes (detops_mask_pack_rle): counts int32 [total], run_offset
    int64 [N + 1], hw [N, 2].  Runs are column-major and start with a 0-run, so pixel (y, x) is set iff position x * H + y
    lies in an odd-indexed run; zero-length runs only toggle; positions beyond the runs are 0, runs beyond H * W and
    negative runs are ignored.  One plane at a time is laid out on the host."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    ro = np.asarray(run_offset, dtype=np.int64).reshape(-1)
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    if ro.size != hw.shape[0] + 1 or ro[0] != 0 or ro[-1] != c.size or (np.diff(ro) < 0).any():
        raise ValueError("mask_pack_rle: run_offset must hold N + 1 entries, start at 0, not decrease and end at len(counts)")
    planes = []
    for n in range(hw.shape[0]):
        H, W = int(hw[n, 0]), int(hw[n, 1])
        ends = np.minimum(np.cumsum(np.maximum(c[ro[n]:ro[n + 1]], 0)), H * W)
        runs = np.diff(np.concatenate([np.zeros(1, np.int64), ends]))
        flat = np.repeat((np.arange(runs.size) & 1).astype(np.uint8), runs)
        flat = np.concatenate([flat, np.zeros(H * W - flat.size, np.uint8)])
        planes.append(flat.reshape(W, H).T[None])
    return mask_pack(planes)


def _pairs(dt_offset, gt_offset, iou_offset):
    """-> (d, g) index arrays [total_pairs] into the sorted detections / ground truths"""
    P = len(dt_offset) - 1
    total = int(iou_offset[P]) if P >= 0 else 0
    d, g = np.zeros((total,), np.int64), np.zeros((total,), np.int64)
    for p in range(P):
        d0, g0 = int(dt_offset[p]), int(gt_offset[p])
        D, G = int(dt_offset[p + 1]) - d0, int(gt_offset[p + 1]) - g0
        if D > 0 and G > 0:
            o = int(iou_offset[p])
            d[o:o + D * G] = d0 + np.repeat(np.arange(D), G)
            g[o:o + D * G] = g0 + np.tile(np.arange(G), D)
    return d, g


def mask_pair_counts(dt_words, dt_word_offset, dt_hw, dt_extent, gt_words, gt_word_offset, gt_hw, gt_extent, dt_offset,
                     gt_offset, iou_offset):
    """-> counts int32 [total_pairs]: pixels set in both planes of every pair (-1 where the planes differ in size)"""
    d_idx, g_idx = _pairs(dt_offset, gt_offset, iou_offset)
    out = np.zeros((d_idx.size,), np.int32)
    for i, (d, g) in enumerate(zip(d_idx, g_idx)):
        H, W = int(dt_hw[d][0]), int(dt_hw[d][1])
        if H != int(gt_hw[g][0]) or W != int(gt_hw[g][1]):
            out[i] = -1
            continue
        WW = (W + 63) // 64
        r0, r1 = max(int(dt_extent[d][0]), int(gt_extent[g][0])), min(int(dt_extent[d][1]), int(gt_extent[g][1]))
        c0, c1 = max(int(dt_extent[d][2]), int(gt_extent[g][2])), min(int(dt_extent[d][3]), int(gt_extent[g][3]))
        if r0 > r1 or c0 > c1:
            continue
        a = dt_words[int(dt_word_offset[d]):int(dt_word_offset[d]) + H * WW].reshape(H, WW)[r0:r1 + 1, c0:c1 + 1]
        b = gt_words[int(gt_word_offset[g]):int(gt_word_offset[g]) + H * WW].reshape(H, WW)[r0:r1 + 1, c0:c1 + 1]
        out[i] = _popcount(a & b)
    return out


def eval_iou(mode, counts, dt_area, gt_area, dt_boxes, gt_boxes, gt_crowd, dt_offset, gt_offset, iou_offset):
    """-> iou float64 [total_pairs]; a union of 0 gives 0"""
    d, g = _pairs(dt_offset, gt_offset, iou_offset)
    if d.size == 0:
        return np.zeros((0,), np.float64)
    crowd = np.asarray(gt_crowd)[g] != 0 if gt_crowd is not None and mode != VOC else np.zeros(d.shape, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == COCO_SEGM:
            i = np.asarray(counts).astype(np.float64)
            da, ga = np.asarray(dt_area)[d].astype(np.float64), np.asarray(gt_area)[g].astype(np.float64)
            u = np.where(crowd, da, (da + ga) - i)
            return np.where((i > 0) & (u > 0), i / u, 0.0)
        one = np.float32(1)
        db, gb = np.asarray(dt_boxes, np.float32)[d], np.asarray(gt_boxes, np.float32)[g]
        if mode == COCO_BBOX:
            dw, dh = (db[:, 2] - db[:, 0]) + one, (db[:, 3] - db[:, 1]) + one        # BoxList.convert("xywh"), fp32
            gw, gh = (gb[:, 2] - gb[:, 0]) + one, (gb[:, 3] - gb[:, 1]) + one
            dx, dy, gx, gy = (v.astype(np.float64) for v in (db[:, 0], db[:, 1], gb[:, 0], gb[:, 1]))
            dw, dh, gw, gh = (v.astype(np.float64) for v in (dw, dh, gw, gh))
            da, ga = dw * dh, gw * gh
            iw = np.minimum(dx + dw, gx + gw) - np.maximum(dx, gx)
            ih = np.minimum(dy + dh, gy + gh) - np.maximum(dy, gy)
            i = iw * ih
            u = np.where(crowd, da, (da + ga) - i)
            return np.where((iw > 0) & (ih > 0) & (u > 0), i / u, 0.0)
        dx2, dy2, gx2, gy2 = db[:, 2] + one, db[:, 3] + one, gb[:, 2] + one, gb[:, 3] + one   # the evaluation's own + 1
        area_d = ((dx2 - db[:, 0]) + one) * ((dy2 - db[:, 1]) + one)
        area_g = ((gx2 - gb[:, 0]) + one) * ((gy2 - gb[:, 1]) + one)
        w = np.maximum((np.minimum(dx2, gx2) - np.maximum(db[:, 0], gb[:, 0])) + one, np.float32(0))
        h = np.maximum((np.minimum(dy2, gy2) - np.maximum(db[:, 1], gb[:, 1])) + one, np.float32(0))
        inter = w * h
        u = (area_d + area_g) - inter
        assert inter.dtype == np.float32 and u.dtype == np.float32
        return np.where(u != 0, inter / u, np.float32(0)).astype(np.float64)


def _match_coco_problem(iou, dt_area, gt_area, crowd, iou_thrs, area_rngs):
    """iou [D, G] -> dt_match int32 [A, T, D], dt_ignore uint8 [A, T, D], gt_ignore uint8 [A, G].  Per lane (a, t) the
    walk of the definition keeps the last ground truth with the largest IoU >= the threshold among the non-ignored ones
    not yet taken, else among the ignored ones not yet taken (crowds stay available)."""
    D, G = iou.shape
    A, T = area_rngs.shape[0], iou_thrs.shape[0]
    lo, hi = area_rngs[:, 0], area_rngs[:, 1]
    gt_ign = crowd[None, :] | (gt_area[None, :] < lo[:, None]) | (gt_area[None, :] > hi[:, None])       # [A, G]
    ign = np.repeat(gt_ign, T, axis=0)                                                                    # [L, G]
    thr = np.tile(np.minimum(iou_thrs, 1 - 1e-10), A)                                                     # [L]
    L = A * T
    taken = np.zeros((L, G), bool)
    dtm = np.full((L, D), -1, np.int32)
    dti = np.zeros((L, D), np.uint8)
    d_out = (dt_area[None, :] < lo[:, None]) | (dt_area[None, :] > hi[:, None])                           # [A, D]
    d_out = np.repeat(d_out, T, axis=0)
    lanes = np.arange(L)
    for d in range(D):
        m = np.full((L,), -1, np.int64)
        if G:
            free = ~(taken & ~crowd[None, :])
            for group in (~ign, ign):
                v = np.where(free & group, iou[d][None, :], -np.inf)
                last = G - 1 - np.argmax(v[:, ::-1], axis=1)             # the last index of the row maximum
                found = (v[lanes, last] >= thr) & (m < 0)
                m = np.where(found, last, m)
            hit = m >= 0
            taken[lanes[hit], m[hit]] = True
            dti[hit, d] = ign[lanes[hit], m[hit]]
        dtm[:, d] = m
        miss = m < 0
        dti[miss, d] = d_out[miss, d]
    return dtm.reshape(A, T, D), dti.reshape(A, T, D), gt_ign.astype(np.uint8)


def _match_voc_problem(iou, difficult, thresh):
    D, G = iou.shape
    out = np.zeros((D,), np.int8)
    if G == 0:
        return out
    selected = np.zeros((G,), bool)
    for d in range(D):
        g = int(np.argmax(iou[d]))
        if iou[d, g] < thresh:
            continue
        if difficult[g]:
            out[d] = -1
        else:
            out[d] = 0 if selected[g] else 1
        selected[g] = True
    return out


def eval_match(mode, iou, dt_offset, gt_offset, iou_offset, dt_area, gt_area, gt_flag, iou_thrs, area_rngs, only=None):
    """COCO modes -> (dt_match int32 [A, T, D_total], dt_ignore uint8 [A, T, D_total], gt_ignore uint8 [A, G_total]);
    VOC -> match int8 [D_total].  `only`: the problems to compute (the others' outputs stay -1 / 0)."""
    P = len(dt_offset) - 1
    D_total, G_total = int(dt_offset[P]), int(gt_offset[P])
    iou_thrs = np.asarray(iou_thrs, np.float64).reshape(-1)
    gt_flag = np.asarray(gt_flag) != 0
    if mode == VOC:
        out = np.zeros((D_total,), np.int8)
    else:
        area_rngs = np.asarray(area_rngs, np.float64).reshape(-1, 2)
        A, T = area_rngs.shape[0], iou_thrs.shape[0]
        dtm = np.full((A, T, D_total), -1, np.int32)
        dti = np.zeros((A, T, D_total), np.uint8)
        gti = np.zeros((A, G_total), np.uint8)
    for p in (range(P) if only is None else only):
        d0, d1, g0, g1 = int(dt_offset[p]), int(dt_offset[p + 1]), int(gt_offset[p]), int(gt_offset[p + 1])
        o = int(iou_offset[p])
        mat = np.asarray(iou[o:o + (d1 - d0) * (g1 - g0)], np.float64).reshape(d1 - d0, g1 - g0)
        if mode == VOC:
            out[d0:d1] = _match_voc_problem(mat, gt_flag[g0:g1], float(iou_thrs[0]))
        else:
            a, b, c = _match_coco_problem(mat, np.asarray(dt_area[d0:d1], np.float64), np.asarray(gt_area[g0:g1], np.float64),
                                          gt_flag[g0:g1], iou_thrs, area_rngs)
            dtm[:, :, d0:d1], dti[:, :, d0:d1], gti[:, g0:g1] = a, b, c
    return out if mode == VOC else (dtm, dti, gti)


# ------------------------------------------------------------------------------------------------ keypoints (OKS)
OKS_MAX_K = 32   # DETOPS_EVAL_OKS_MAX_K
# the COCO person table (pycocotools' kpt_oks_sigmas), recalled and not checked against it
COCO_PERSON_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def eval_oks(dt_kpts, gt_kpts, gt_boxes, gt_area, sigmas, dt_offset, gt_offset, iou_offset):
    """include/detops.h, "Keypoint evaluation (OKS)": keypoints fp32 [D_total, K, 3] / [G_total, K, 3], gt_boxes fp32 xyxy,
    gt_area and sigmas fp64, everything in sorted (problem) order -> (oks float64 [total_pairs], dt_area float64 [D_total]).
    Vectorised over the pairs; the sum over the keypoints is a loop, one term after the other, as the definition has it."""
    sig = np.asarray(sigmas, np.float64).reshape(-1)
    K = sig.size
    dk = np.asarray(dt_kpts, np.float32).reshape(-1, K, 3)
    gk = np.asarray(gt_kpts, np.float32).reshape(-1, K, 3)
    x, y = dk[:, :, 0], dk[:, :, 1]
    if dk.shape[0]:
        dt_area = (x.max(axis=1).astype(np.float64) - x.min(axis=1).astype(np.float64)) \
            * (y.max(axis=1).astype(np.float64) - y.min(axis=1).astype(np.float64))
    else:
        dt_area = np.zeros((0,), np.float64)
    d, g = _pairs(dt_offset, gt_offset, iou_offset)
    if d.size == 0:
        return np.zeros((0,), np.float64), dt_area
    xd, yd = x[d].astype(np.float64), y[d].astype(np.float64)
    xg, yg = gk[g, :, 0].astype(np.float64), gk[g, :, 1].astype(np.float64)
    visible = gk[g, :, 2] > 0
    k1 = visible.sum(axis=1)
    has = (k1 > 0)[:, None]
    one = np.float32(1)
    gb = np.asarray(gt_boxes, np.float32).reshape(-1, 4)[g]
    bw = ((gb[:, 2] - gb[:, 0]) + one).astype(np.float64)[:, None]        # BoxList.convert("xywh"), fp32
    bh = ((gb[:, 3] - gb[:, 1]) + one).astype(np.float64)[:, None]
    bx, by = gb[:, 0].astype(np.float64)[:, None], gb[:, 1].astype(np.float64)[:, None]
    x0, x1, y0, y1 = bx - bw, bx + 2.0 * bw, by - bh, by + 2.0 * bh
    dx = np.where(has, xd - xg, np.fmax(0.0, x0 - xd) + np.fmax(0.0, xd - x1))
    dy = np.where(has, yd - yg, np.fmax(0.0, y0 - yd) + np.fmax(0.0, yd - y1))
    s2 = 2.0 * sig
    var = s2 * s2
    area = np.asarray(gt_area, np.float64).reshape(-1)[g] + np.spacing(1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = (dx * dx + dy * dy) / var[None, :] / area[:, None] / 2.0
        term = np.exp(-e)
    counts = np.where(has, visible, True)
    s = np.zeros((d.size,), np.float64)
    for k in range(K):
        s = np.where(counts[:, k], s + term[:, k], s)
    return s / np.where(k1 > 0, k1, K).astype(np.float64), dt_area


# ------------------------------------------------------------------------------------------------ proposal recall
def proposal_iou(dt, gt):
    """boxlist_iou in fp32 numpy, one operation after the other (include/detops.h, "Proposal recall"): [P, 4], [G, 4] xyxy
    -> [P, G] float32"""
    dt, gt = np.asarray(dt, np.float32).reshape(-1, 4), np.asarray(gt, np.float32).reshape(-1, 4)
    one, zero = np.float32(1), np.float32(0)
    area_p = ((dt[:, 2] - dt[:, 0]) + one) * ((dt[:, 3] - dt[:, 1]) + one)
    area_g = ((gt[:, 2] - gt[:, 0]) + one) * ((gt[:, 3] - gt[:, 1]) + one)
    w = np.maximum((np.minimum(dt[:, None, 2], gt[None, :, 2]) - np.maximum(dt[:, None, 0], gt[None, :, 0])) + one, zero)
    h = np.maximum((np.minimum(dt[:, None, 3], gt[None, :, 3]) - np.maximum(dt[:, None, 1], gt[None, :, 1])) + one, zero)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return inter / ((area_p[:, None] + area_g[None, :]) - inter)


def eval_proposal_overlaps(dt_boxes, gt_boxes, dt_offset, gt_offset, gt_valid, limits):
    """include/detops.h, "Proposal recall": the proposals [D_total, 4] (objectness descending inside an image) and ground
    truths [G_total, 4] of a batch, fp32 xyxy, dt_offset / gt_offset [N + 1], gt_valid [A, G_total], limits [L] (<= 0: no
    limit) -> float32 [L, A, G_total]: the IoU every ground truth is matched with, 0 where no round reaches it, -1 outside
    the area range.  The rounds are the reference's loop (evaluate_box_proposals), numpy's max / argmax in torch's place:
    both take the first maximum."""
    dt_boxes, gt_boxes = np.asarray(dt_boxes, np.float32).reshape(-1, 4), np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    dt_offset, gt_offset = np.asarray(dt_offset, np.int64).reshape(-1), np.asarray(gt_offset, np.int64).reshape(-1)
    limits = np.asarray(limits, np.int64).reshape(-1)
    G_total = gt_boxes.shape[0]
    gt_valid = np.asarray(gt_valid).reshape(-1, G_total) != 0
    L, A = limits.size, gt_valid.shape[0]
    out = np.where(gt_valid, np.float32(0), np.float32(-1))[None].repeat(L, axis=0).astype(np.float32)
    for n in range(dt_offset.size - 1):
        d0, d1, g0, g1 = dt_offset[n], dt_offset[n + 1], gt_offset[n], gt_offset[n + 1]
        if d1 <= d0 or g1 <= g0:
            continue
        iou = proposal_iou(dt_boxes[d0:d1], gt_boxes[g0:g1])
        for li, limit in enumerate(limits):
            rows = iou[:limit] if limit > 0 else iou
            for a in range(A):
                cols = np.nonzero(gt_valid[a, g0:g1])[0]
                if cols.size == 0:
                    continue
                overlaps = rows[:, cols].copy()
                for _ in range(min(overlaps.shape)):
                    argmax_overlaps, max_overlaps = overlaps.argmax(axis=0), overlaps.max(axis=0)
                    gt_ind = int(max_overlaps.argmax())
                    box_ind = int(argmax_overlaps[gt_ind])
                    out[li, a, g0 + cols[gt_ind]] = overlaps[box_ind, gt_ind]
                    overlaps[box_ind, :] = -1
                    overlaps[:, gt_ind] = -1
    return out


# ------------------------------------------------------------------------------------------------ Cityscapes
def _window(box, H, W):
    """(xmin, ymin, xmax, ymax) -> the slices of rows [ymin, ymax) and columns [xmin, xmax) clamped to the image"""
    x0, y0, x1, y1 = (int(v) for v in box)
    clamp = lambda v, hi: min(max(v, 0), hi)  # noqa: E731
    return slice(clamp(y0, H), max(clamp(y1, H), clamp(y0, H))), slice(clamp(x0, W), max(clamp(x1, W), clamp(x0, W)))


def window_counts(dt_planes, dt_box, gt_planes, gt_box):
    """include/detops.h, "Cityscapes evaluation": planes [D, H, W] / [G, H, W] (non-zero = set), int boxes [D, 4] / [G, 4]
    (xmin, ymin, xmax, ymax; maxima exclusive) -> (dt_count [D], gt_count [G], pair_box [D, G], pair_mask [D, G]) int32.  The
    reference's loop (eval_instances.py: matchGtWithPred) with numpy sums in the place of its torch sums and .item()."""
    dt_planes, gt_planes = np.asarray(dt_planes) != 0, np.asarray(gt_planes) != 0
    dt_box, gt_box = np.asarray(dt_box, np.int64).reshape(-1, 4), np.asarray(gt_box, np.int64).reshape(-1, 4)
    D, G = dt_planes.shape[0], gt_planes.shape[0]
    H, W = dt_planes.shape[1:] if D else gt_planes.shape[1:]
    dt_count = np.array([np.count_nonzero(dt_planes[d][_window(dt_box[d], H, W)]) for d in range(D)], np.int32).reshape(D)
    gt_count = np.array([np.count_nonzero(gt_planes[g][_window(gt_box[g], H, W)]) for g in range(G)], np.int32).reshape(G)
    pair_box, pair_mask = np.zeros((D, G), np.int32), np.zeros((D, G), np.int32)
    lo = np.maximum(dt_box[:, None, :2], gt_box[None, :, :2])
    hi = np.minimum(dt_box[:, None, 2:], gt_box[None, :, 2:])
    # isOverlapping: strict on all four sides, each box's minimum against the OTHER box's maximum
    overlapping = ((dt_box[:, None, :2] < gt_box[None, :, 2:]) & (gt_box[None, :, :2] < dt_box[:, None, 2:])).all(axis=2)
    for d, g in zip(*np.nonzero(overlapping)):
        inter = int(hi[d, g, 0] - lo[d, g, 0]) * int(hi[d, g, 1] - lo[d, g, 1])
        pair_box[d, g] = min(max(inter, -2 ** 31), 2 ** 31 - 1)
        union = np.concatenate([np.minimum(dt_box[d, :2], gt_box[g, :2]), np.maximum(dt_box[d, 2:], gt_box[g, 2:])])
        win = _window(union, H, W)
        pair_mask[d, g] = np.count_nonzero(dt_planes[d][win] & gt_planes[g][win])
    return dt_count, gt_count, pair_box, pair_mask
