"""The COCO-style evaluation rules, literally: dicts and loops, nothing vectorised.  A restatement of
pycocotools.cocoeval (computeIoU, evaluateImg, accumulate, summarize) written from knowledge of that code; it has NOT been
checked against pycocotools, which is not available where this project is built and tested.  The evaluator
(maskrcnn_benchmark/data/datasets/evaluation/coco_style.py), the numpy path (_eval_cpu.py) and the kernels
(csrc/evaluate.hip) are pinned to this file.

An image is {"dt": [detection], "gt": [ground truth]}:
  detection     {"label", "score", "box": 4 np.float32 xyxy, "mask": bool [H, W] (segm only)}
  ground truth  {"label", "box", "mask", "iscrowd", "area"}
"""
import bisect
import math

import numpy as np

IOU_THRS = [float(v) for v in np.linspace(0.5, 0.95, 10)]
REC_THRS = [float(v) for v in np.linspace(0.0, 1.0, 101)]
AREA_RNGS = [[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]]
MAX_DETS = [1, 10, 100]


def xywh(box):
    """BoxList.convert("xywh") of an fp32 xyxy box: fp32 arithmetic, then Python floats"""
    x1, y1, x2, y2 = (np.float32(v) for v in box)
    w = np.float32(np.float32(x2 - x1) + np.float32(1))
    h = np.float32(np.float32(y2 - y1) + np.float32(1))
    return float(x1), float(y1), float(w), float(h)


def bbox_iou(d, g, crowd):
    dx, dy, dw, dh = xywh(d)
    gx, gy, gw, gh = xywh(g)
    w = min(dx + dw, gx + gw) - max(dx, gx)
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if w <= 0 or h <= 0:
        return 0.0
    i = w * h
    u = dw * dh if crowd else dw * dh + gw * gh - i
    return i / u if u > 0 else 0.0      # a union of 0: the original divides 0 by 0; this project's choice is 0


def mask_iou(d, g, crowd):
    i = float(np.logical_and(d, g).sum())
    da, ga = float(d.sum()), float(g.sum())
    u = da if crowd else da + ga - i
    return i / u if (i > 0 and u > 0) else 0.0


def dt_area(d, iou_type):
    if iou_type == "segm":
        return float(d["mask"].sum())
    _, _, w, h = xywh(d["box"])
    return w * h


def evaluate_img(dts, gts, iou_type, area_rng, max_det):
    """dts, gts: the detections / ground truths of one (image, category) pair, in input order
    -> None (both empty) or {"scores", "dt_match" [T][D] (index into `gts`, -1 unmatched), "dt_ignore" [T][D],
    "gt_ignore" [G] (in the order of `gts`)}"""
    if len(dts) == 0 and len(gts) == 0:
        return None
    ignore = [bool(g["iscrowd"]) or g["area"] < area_rng[0] or g["area"] > area_rng[1] for g in gts]
    gtind = sorted(range(len(gts)), key=lambda i: ignore[i])                 # stable: non-ignored first
    dtind = sorted(range(len(dts)), key=lambda i: -dts[i]["score"])[:max_det]    # stable: ties in input order
    gt = [gts[i] for i in gtind]
    dt = [dts[i] for i in dtind]
    gt_ig = [ignore[i] for i in gtind]
    iscrowd = [bool(g["iscrowd"]) for g in gt]
    iou_fn = mask_iou if iou_type == "segm" else bbox_iou
    key = "mask" if iou_type == "segm" else "box"
    ious = [[iou_fn(d[key], g[key], c) for g, c in zip(gt, iscrowd)] for d in dt]
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gtm = [[-1] * G for _ in range(T)]
    dtm = [[-1] * D for _ in range(T)]
    dt_ig = [[False] * D for _ in range(T)]
    for tind, t in enumerate(IOU_THRS):
        for dind in range(D):
            iou = min([t, 1 - 1e-10])
            m = -1
            for gind in range(G):
                if gtm[tind][gind] > -1 and not iscrowd[gind]:
                    continue
                if m > -1 and not gt_ig[m] and gt_ig[gind]:
                    break
                if ious[dind][gind] < iou:
                    continue
                iou = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind][dind] = gt_ig[m]
            dtm[tind][dind] = gtind[m]
            gtm[tind][m] = dind
    for tind in range(T):
        for dind, d in enumerate(dt):
            a = dt_area(d, iou_type)
            if dtm[tind][dind] == -1 and (a < area_rng[0] or a > area_rng[1]):
                dt_ig[tind][dind] = True
    return {"scores": [d["score"] for d in dt], "dt_match": dtm, "dt_ignore": dt_ig, "gt_ignore": ignore,
            "gt_ignore_sorted": gt_ig}


def evaluate(images, iou_type, num_classes):
    """-> {(category, area index, image index): evaluate_img(...)} at the largest maxDets"""
    out = {}
    for k in range(1, num_classes):
        for a, rng in enumerate(AREA_RNGS):
            for i, im in enumerate(images):
                out[(k, a, i)] = evaluate_img([d for d in im["dt"] if d["label"] == k], [g for g in im["gt"] if g["label"] == k],
                                              iou_type, rng, MAX_DETS[-1])
    return out


def accumulate(eval_imgs, num_images, num_classes):
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), num_classes - 1, len(AREA_RNGS), len(MAX_DETS)
    precision = np.full((T, R, K, A, M), -1.0)
    recall = np.full((T, K, A, M), -1.0)
    eps = float(np.spacing(1))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                E = [eval_imgs[(k + 1, a, i)] for i in range(num_images)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                scores, where = [], []
                for e in E:
                    for j, s in enumerate(e["scores"][:max_det]):
                        scores.append(s)
                        where.append((e, j))
                inds = sorted(range(len(scores)), key=lambda i: -scores[i])           # stable mergesort
                npig = 0
                for e in E:
                    for ig in e["gt_ignore"]:
                        if not ig:
                            npig += 1
                if npig == 0:
                    continue
                for t in range(T):
                    tp, fp, tps, fps = 0, 0, [], []
                    for i in inds:
                        e, j = where[i]
                        matched, ignored = e["dt_match"][t][j] > -1, e["dt_ignore"][t][j]
                        if matched and not ignored:
                            tp += 1
                        if not matched and not ignored:
                            fp += 1
                        tps.append(float(tp))
                        fps.append(float(fp))
                    nd = len(tps)
                    rc = [v / npig for v in tps]
                    pr = [v / (f + v + eps) for v, f in zip(tps, fps)]
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = [0.0] * R
                    for ri, thr in enumerate(REC_THRS):
                        pi = bisect.bisect_left(rc, thr)
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall):
    def stat(ap, thr=None, area=0, m=2):
        vals = []
        src = precision if ap else recall
        for t in range(len(IOU_THRS)):
            if thr is not None and not math.isclose(IOU_THRS[t], thr):
                continue
            block = src[t, :, :, area, m] if ap else src[t, :, area, m]
            for v in block.reshape(-1):
                if v > -1:
                    vals.append(float(v))
        return float(np.mean(np.array(vals))) if vals else -1.0

    return [stat(1), stat(1, 0.5), stat(1, 0.75), stat(1, area=1), stat(1, area=2), stat(1, area=3),
            stat(0, m=0), stat(0, m=1), stat(0, m=2), stat(0, area=1), stat(0, area=2), stat(0, area=3)]


def coco_stats(images, iou_type, num_classes):
    ev = evaluate(images, iou_type, num_classes)
    return ev, summarize(*accumulate(ev, len(images), num_classes))
