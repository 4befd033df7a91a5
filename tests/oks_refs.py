"""The keypoint evaluation rules (include/detops.h, "Keypoint evaluation (OKS)"), literally: dicts and loops, nothing
vectorised.  A restatement of pycocotools.cocoeval (computeOks, the keypoint branches of _prepare, evaluateImg and
setKpParams, loadRes for keypoint results, accumulate, summarize) written from knowledge of that code; it has NOT been
checked against pycocotools, which is not available where this project is built and tested.  The evaluator
(maskrcnn_benchmark/data/datasets/evaluation/keypoint_oks.py), the numpy path (_eval_cpu.eval_oks) and the kernel
(csrc/eval_oks.hip) are pinned to this file.

An image is {"dt": [detection], "gt": [ground truth]}:
  detection     {"label", "score", "keypoints": np.float32 [K, 3]}
  ground truth  {"label", "box": 4 np.float32 xyxy, "keypoints": np.float32 [K, 3] (x, y, visibility), "iscrowd", "area"}

The sum of an OKS runs in keypoint order, one term after the other (pycocotools' np.sum adds in another order): the last
bits are this library's choice.  exp is math.exp, the C library's.
"""
import bisect
import math

import numpy as np

from eval_refs import IOU_THRS, REC_THRS, xywh

AREA_RNGS = [[0.0, 1e10], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]]
MAX_DETS = [20]
SIGMAS = [v / 10.0 for v in (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89)]
STAT_NAMES = ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl")


def visible_count(g):
    return sum(1 for k in range(len(g["keypoints"])) if float(g["keypoints"][k][2]) > 0)


def oks(d, g, sigmas):
    """d, g: a detection and a ground truth -> the object keypoint similarity, a Python float"""
    K = len(sigmas)
    dk, gk = d["keypoints"], g["keypoints"]
    k1 = visible_count(g)
    bx, by, bw, bh = xywh(g["box"])
    x0, x1, y0, y1 = bx - bw, bx + 2 * bw, by - bh, by + 2 * bh
    total, n = 0.0, 0
    for k in range(K):
        xd, yd = float(dk[k][0]), float(dk[k][1])                   # the detection's third column is never read
        xg, yg, vg = float(gk[k][0]), float(gk[k][1]), float(gk[k][2])
        if k1 > 0:
            dx, dy = xd - xg, yd - yg
        else:
            dx = max(0.0, x0 - xd) + max(0.0, xd - x1)
            dy = max(0.0, y0 - yd) + max(0.0, yd - y1)
        var = (2 * sigmas[k]) * (2 * sigmas[k])
        e = (dx * dx + dy * dy) / var / (float(g["area"]) + 2.0 ** -52) / 2
        if k1 > 0 and not vg > 0:
            continue
        try:
            term = math.exp(-e)
        except OverflowError:           # (never: -e <= 0)
            term = math.inf
        total = total + term
        n += 1
    return total / n


def detection_area(d):
    """loadRes: the area of the box around all K keypoints"""
    xs = [np.float32(p[0]) for p in d["keypoints"]]
    ys = [np.float32(p[1]) for p in d["keypoints"]]
    return (float(max(xs)) - float(min(xs))) * (float(max(ys)) - float(min(ys)))


def evaluate_img(dts, gts, sigmas, area_rng, max_det):
    """dts, gts: the detections / ground truths of one (image, category) pair, in input order
    -> None (both empty) or {"scores", "ious" [D][G sorted], "dt_match" [T][D] (index into `gts`, -1 unmatched),
    "dt_ignore" [T][D], "gt_ignore" [G] (in the order of `gts`)}"""
    if len(dts) == 0 and len(gts) == 0:
        return None
    # _prepare: a ground truth without a labelled keypoint is ignored; then evaluateImg's area rule
    ignore = [bool(g["iscrowd"]) or visible_count(g) == 0 or g["area"] < area_rng[0] or g["area"] > area_rng[1] for g in gts]
    gtind = sorted(range(len(gts)), key=lambda i: ignore[i])                 # stable: non-ignored first
    dtind = sorted(range(len(dts)), key=lambda i: -dts[i]["score"])[:max_det]    # stable: ties in input order
    gt = [gts[i] for i in gtind]
    dt = [dts[i] for i in dtind]
    gt_ig = [ignore[i] for i in gtind]
    iscrowd = [bool(g["iscrowd"]) for g in gt]
    ious = [[oks(d, g, sigmas) for g in gt] for d in dt]
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
            a = detection_area(d)
            if dtm[tind][dind] == -1 and (a < area_rng[0] or a > area_rng[1]):
                dt_ig[tind][dind] = True
    return {"scores": [d["score"] for d in dt], "ious": ious, "dt_match": dtm, "dt_ignore": dt_ig, "gt_ignore": ignore}


def evaluate(images, num_classes, sigmas=SIGMAS):
    """-> {(category, area index, image index): evaluate_img(...)}"""
    out = {}
    for k in range(1, num_classes):
        for a, rng in enumerate(AREA_RNGS):
            for i, im in enumerate(images):
                out[(k, a, i)] = evaluate_img([d for d in im["dt"] if d["label"] == k], [g for g in im["gt"] if g["label"] == k],
                                              sigmas, rng, MAX_DETS[-1])
    return out


def accumulate(eval_imgs, num_images, num_classes):
    T, R, K, A = len(IOU_THRS), len(REC_THRS), num_classes - 1, len(AREA_RNGS)
    precision = np.full((T, R, K, A), -1.0)
    recall = np.full((T, K, A), -1.0)
    eps = float(np.spacing(1))
    for k in range(K):
        for a in range(A):
            E = [eval_imgs[(k + 1, a, i)] for i in range(num_images)]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            scores, where = [], []
            for e in E:
                for j, s in enumerate(e["scores"][:MAX_DETS[0]]):
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
                recall[t, k, a] = rc[-1] if nd else 0
                for i in range(nd - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                q = [0.0] * R
                for ri, thr in enumerate(REC_THRS):
                    pi = bisect.bisect_left(rc, thr)
                    if pi >= nd:
                        break
                    q[ri] = pr[pi]
                precision[t, :, k, a] = q
    return precision, recall


def summarize(precision, recall):
    def stat(ap, thr=None, area=0):
        vals = []
        src = precision if ap else recall
        for t in range(len(IOU_THRS)):
            if thr is not None and not math.isclose(IOU_THRS[t], thr):
                continue
            block = src[t, :, :, area] if ap else src[t, :, area]
            for v in block.reshape(-1):
                if v > -1:
                    vals.append(float(v))
        return float(np.mean(np.array(vals))) if vals else -1.0

    return [stat(1), stat(1, 0.5), stat(1, 0.75), stat(1, area=1), stat(1, area=2),
            stat(0), stat(0, 0.5), stat(0, 0.75), stat(0, area=1), stat(0, area=2)]


def coco_stats(images, num_classes, sigmas=SIGMAS):
    ev = evaluate(images, num_classes, sigmas)
    return ev, summarize(*accumulate(ev, len(images), num_classes))


# ------------------------------------------------------------------------------------------------ seeded test data
def random_images(seed, n_images=4, K=17, num_classes=3, size=(200, 160), max_dt=6, max_gt=4, empty=()):
    """Seeded images in the dict form above: ground truths with boxes of many sizes, keypoints inside them, random
    visibility (some without a visible keypoint), some crowds; detections = a ground truth's keypoints with noise, or
    random.  `empty`: {image index: "dt" | "gt" | "both"} left without detections / ground truths."""
    rng = np.random.RandomState(seed)
    W, H = size
    images = []
    for i in range(n_images):
        gts, dts = [], []
        for _ in range(rng.randint(1, max_gt + 1)):
            w, h = rng.uniform(8, 150), rng.uniform(8, 120)
            x1, y1 = rng.uniform(0, W - w), rng.uniform(0, H - h)
            box = np.array([x1, y1, x1 + w, y1 + h], np.float32)
            kp = np.zeros((K, 3), np.float32)
            kp[:, 0] = rng.uniform(x1, x1 + w, K)
            kp[:, 1] = rng.uniform(y1, y1 + h, K)
            kp[:, 2] = rng.randint(0, 3, K)
            if rng.rand() < 0.2:
                kp[:, 2] = 0                           # no labelled keypoint
            kp[kp[:, 2] == 0, :2] = 0
            gts.append({"label": int(rng.randint(1, num_classes)), "box": box, "keypoints": kp, "iscrowd": int(rng.rand() < 0.15),
                        "area": float(np.float32(w * h * rng.uniform(0.3, 0.9)))})
        for _ in range(rng.randint(1, max_dt + 1)):
            g = gts[rng.randint(len(gts))]
            kp = np.zeros((K, 3), np.float32)
            if rng.rand() < 0.7:
                scale = math.sqrt(g["area"]) * rng.choice([0.01, 0.03, 0.1])
                kp[:, :2] = g["keypoints"][:, :2] + rng.normal(0, scale, (K, 2))
                label = g["label"]
            else:
                kp[:, 0], kp[:, 1] = rng.uniform(0, W, K), rng.uniform(0, H, K)
                label = int(rng.randint(1, num_classes))
            kp[:, 2] = rng.uniform(0, 1, K)
            dts.append({"label": label, "score": float(np.float32(rng.rand())), "keypoints": kp})
        kind = dict(empty).get(i)
        images.append({"dt": [] if kind in ("dt", "both") else dts, "gt": [] if kind in ("gt", "both") else gts})
    return images


def to_boxlists(images, size=(200, 160), device="cpu"):
    """-> (predictions, targets) as BoxLists: `keypoints` fields, targets with iscrowd and area"""
    import torch
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.keypoint import Keypoints

    preds, tgts = [], []
    for im in images:
        dt, gt = im["dt"], im["gt"]
        K = len((dt + gt)[0]["keypoints"]) if dt or gt else 17
        dk = np.array([d["keypoints"] for d in dt], np.float32).reshape(-1, K, 3)
        gk = np.array([g["keypoints"] for g in gt], np.float32).reshape(-1, K, 3)
        ext = np.concatenate([dk[:, :, :2].min(axis=1), dk[:, :, :2].max(axis=1)], axis=1) if len(dt) else np.zeros((0, 4), np.float32)
        p = BoxList(torch.from_numpy(ext.astype(np.float32)), size)
        p.add_field("scores", torch.from_numpy(np.array([d["score"] for d in dt], np.float32).reshape(-1)))
        p.add_field("labels", torch.from_numpy(np.array([d["label"] for d in dt], np.int64).reshape(-1)))
        p.add_field("keypoints", Keypoints(torch.from_numpy(dk), size))
        t = BoxList(torch.from_numpy(np.array([g["box"] for g in gt], np.float32).reshape(-1, 4)), size)
        t.add_field("labels", torch.from_numpy(np.array([g["label"] for g in gt], np.int64).reshape(-1)))
        t.add_field("iscrowd", torch.from_numpy(np.array([g["iscrowd"] for g in gt], np.uint8).reshape(-1)))
        t.add_field("area", torch.from_numpy(np.array([g["area"] for g in gt], np.float64).reshape(-1)))
        t.add_field("keypoints", Keypoints(torch.from_numpy(gk), size))
        preds.append(p.to(device))
        tgts.append(t.to(device))
    return preds, tgts


def random_problems(seed, shapes, K, unlabelled=()):
    """Seeded raw problems for the operator: shapes = [(D_p, G_p)] -> (dict of numpy arrays in sorted order: dt_kpts, gt_kpts,
    gt_boxes, gt_area, dt_offset, gt_offset, iou_offset, and the literal loops' answers oks [total_pairs], dt_area
    [D_total]).  `unlabelled`: flat ground-truth indices whose visibility flags are all 0."""
    rng = np.random.RandomState(seed)
    D_total, G_total = sum(d for d, _ in shapes), sum(g for _, g in shapes)
    gt_boxes = np.zeros((G_total, 4), np.float32)
    gt_boxes[:, :2] = rng.uniform(0, 100, (G_total, 2))
    gt_boxes[:, 2:] = gt_boxes[:, :2] + rng.uniform(5, 120, (G_total, 2))
    gt_kpts = np.zeros((G_total, K, 3), np.float32)
    gt_kpts[:, :, 0] = rng.uniform(gt_boxes[:, None, 0], gt_boxes[:, None, 2], (G_total, K))
    gt_kpts[:, :, 1] = rng.uniform(gt_boxes[:, None, 1], gt_boxes[:, None, 3], (G_total, K))
    gt_kpts[:, :, 2] = rng.randint(0, 3, (G_total, K))
    for g in unlabelled:
        gt_kpts[g, :, 2] = 0
    gt_area = rng.uniform(20, 12000, G_total)
    dt_kpts = np.zeros((D_total, K, 3), np.float32)
    dt_kpts[:, :, 2] = rng.uniform(0, 1, (D_total, K))
    sigmas = (SIGMAS * (K // 17 + 1))[:K]
    dt_offset, gt_offset, iou_offset = [0], [0], [0]
    oks_ref, d0, g0 = [], 0, 0
    for D, G in shapes:
        for d in range(D):
            if G and rng.rand() < 0.8:      # near one of the problem's ground truths, noise of a few sigma
                g = g0 + rng.randint(G)
                dt_kpts[d0 + d, :, :2] = gt_kpts[g, :, :2] + rng.normal(0, math.sqrt(gt_area[g]) * 0.05, (K, 2))
            else:
                dt_kpts[d0 + d, :, :2] = rng.uniform(-50, 300, (K, 2))
            for g in range(G):
                oks_ref.append(oks({"keypoints": dt_kpts[d0 + d]}, {"keypoints": gt_kpts[g0 + g], "box": gt_boxes[g0 + g],
                                                                   "area": gt_area[g0 + g]}, sigmas))
        d0, g0 = d0 + D, g0 + G
        dt_offset.append(d0)
        gt_offset.append(g0)
        iou_offset.append(iou_offset[-1] + D * G)
    area_ref = [detection_area({"keypoints": dt_kpts[d]}) for d in range(D_total)]
    return {"dt_kpts": dt_kpts, "gt_kpts": gt_kpts, "gt_boxes": gt_boxes, "gt_area": gt_area, "sigmas": np.array(sigmas),
            "dt_offset": np.array(dt_offset, np.int32), "gt_offset": np.array(gt_offset, np.int32),
            "iou_offset": np.array(iou_offset, np.int64), "oks": np.array(oks_ref, np.float64).reshape(-1),
            "dt_area": np.array(area_ref, np.float64).reshape(-1)}


# ------------------------------------------------------------------------------------------------ shared by the tests
SHAPES = [(3, 2), (0, 3), (5, 4), (2, 0), (1, 1), (7, 3)]      # problems with D = 0 or G = 0 between full ones
SEED = 11                                                      # random_images(SEED, 8, empty=EMPTY): the evaluator's case, for
EMPTY = {1: "gt", 3: "dt", 5: "both"}                          # which no OKS lies within 1e-9 of a threshold (asserted)


def oks_tolerance(K):
    """the derived bound on |a - b| for two sequential sums of K terms in (0, 1], each exp within 1 ulp (see the tests)"""
    return 2 * (K + 1) * 2.0 ** -52


def run_op(pb, device="cpu"):
    import torch

    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    oks, area = _C().eval_oks(t(pb["dt_kpts"]), t(pb["gt_kpts"]), t(pb["gt_boxes"]), t(pb["gt_area"]), pb["sigmas"],
                              t(pb["dt_offset"]), t(pb["gt_offset"]), t(pb["iou_offset"]), int(pb["iou_offset"][-1]))
    return oks.cpu().numpy(), area.cpu().numpy()


def evaluate_boxlists(images, num_classes=3, device="cpu", batch=3, size=(200, 160)):
    ev = _KO().KeypointOKSEvaluator(num_classes)
    preds, tgts = to_boxlists(images, size, device)
    for i in range(0, len(images), batch):
        ev.update(preds[i:i + batch], tgts[i:i + batch])
    return ev


def all_oks(images, num_classes=3):
    """every OKS of the test data, from the numpy path"""
    vals = []
    for im in images:
        for k in range(1, num_classes):
            dts, gts = [d for d in im["dt"] if d["label"] == k], [g for g in im["gt"] if g["label"] == k]
            if dts and gts:
                pb = {"dt_kpts": np.array([d["keypoints"] for d in dts]), "gt_kpts": np.array([g["keypoints"] for g in gts]),
                      "gt_boxes": np.array([g["box"] for g in gts]), "gt_area": np.array([g["area"] for g in gts]),
                      "sigmas": np.array(SIGMAS), "dt_offset": np.array([0, len(dts)], np.int32),
                      "gt_offset": np.array([0, len(gts)], np.int32), "iou_offset": np.array([0, len(dts) * len(gts)], np.int64)}
                vals.append(run_op(pb)[0])
    return np.concatenate(vals)


def assert_clear_of_the_thresholds(images, num_classes=3):
    """the condition for comparing matches exactly: no OKS within 1e-9 of a threshold"""
    v = all_oks(images, num_classes)
    thr = np.minimum(np.array(IOU_THRS), 1 - 1e-10)
    assert np.abs(v[:, None] - thr[None, :]).min() > 1e-9
    return v


def _C():
    from maskrcnn_benchmark import _C as module
    return module


def _KO():
    from maskrcnn_benchmark.data.datasets.evaluation import keypoint_oks
    return keypoint_oks
