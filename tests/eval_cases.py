"""Seeded detection-evaluation cases shared by tests/test_evaluation_cpu.py and tests/test_evaluation_gpu.py, in the
form tests/eval_refs.py reads ({"dt": [...], "gt": [...]}, see there) and as BoxLists for the evaluator.

8 images of 40-130 pixels, 3 categories, 0-12 ground truths and 0-30 detections each: detections made by jittering ground
truth plus random ones, masks as ellipses and rectangles, 15 % crowd, areas on both sides of 32^2 and 96^2, scores rounded
to two decimals (ties), pairs whose IoU is exactly 0.5 and 0.75 (rectangles of integer pixel counts: 100 / 200 and 150 / 200
pixels), an empty detection mask, an image without ground truth (2) and one without detections (5).
"""
import numpy as np
import torch

from maskrcnn_benchmark.data.datasets.evaluation import voc
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

NUM_CLASSES = 4


def shape_mask(box, H, W, ellipse):
    """the pixels of an integer box (x1, y1, x2, y2, inclusive), or of the ellipse inscribed in it"""
    x1, y1, x2, y2 = (int(v) for v in box)
    m = np.zeros((H, W), dtype=bool)
    ys, xs = np.mgrid[0:H, 0:W]
    inside = (xs >= x1) & (xs <= x2) & (ys >= y1) & (ys <= y2)
    if ellipse:
        cx, cy, rx, ry = (x1 + x2) / 2.0, (y1 + y2) / 2.0, (x2 - x1 + 1) / 2.0, (y2 - y1 + 1) / 2.0
        inside &= ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0
    m[inside] = True
    return m


def rand_box(rng, H, W, big=False):
    hi_w, hi_h = (W - 2, H - 2) if big else (max(W // 2, 8), max(H // 2, 8))
    w, h = int(rng.randint(4, hi_w + 1)), int(rng.randint(4, hi_h + 1))
    x1, y1 = int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1))
    return [x1, y1, x1 + w - 1, y1 + h - 1]


def make_images(seed=7):
    rng = np.random.RandomState(seed)
    images = []
    for i in range(8):
        H, W = (130, 128) if i in (0, 6) else (int(rng.randint(40, 131)), int(rng.randint(40, 131)))
        gts, dts = [], []
        ng = 0 if i == 2 else int(rng.randint(1, 13))
        for k in range(ng):
            box = rand_box(rng, H, W, big=(k % 5 == 0))
            mask = shape_mask(box, H, W, ellipse=bool(k % 2))
            gts.append({"label": int(rng.randint(1, NUM_CLASSES)), "box": np.array(box, np.float32), "mask": mask,
                        "iscrowd": bool(rng.rand() < 0.15), "area": float(mask.sum()) + (0.5 if i % 2 else 0.0)})
        if i in (0, 6):
            # exact IoUs: a 20 x 10 ground truth, a 10 x 10 and a 15 x 10 detection inside it (rectangles)
            box = [3, 5, 22, 14]
            gts.append({"label": 1, "box": np.array(box, np.float32), "mask": shape_mask(box, H, W, False), "iscrowd": False,
                        "area": 200.0})
            for b, s in (([3, 5, 12, 14], 0.9), ([3, 5, 17, 14], 0.8)):
                dts.append({"label": 1, "score": np.float32(s), "box": np.array(b, np.float32), "mask": shape_mask(b, H, W, False)})
        if i != 5:
            for g in gts[:ng]:
                for _ in range(int(rng.randint(0, 4))):
                    j = rng.randint(-3, 4, 4)
                    x1 = min(max(int(g["box"][0]) + int(j[0]), 0), W - 2)
                    y1 = min(max(int(g["box"][1]) + int(j[1]), 0), H - 2)
                    b = [x1, y1, min(max(int(g["box"][2]) + int(j[2]), x1 + 1), W - 1),
                         min(max(int(g["box"][3]) + int(j[3]), y1 + 1), H - 1)]
                    lab = g["label"] if rng.rand() < 0.85 else int(rng.randint(1, NUM_CLASSES))
                    dts.append({"label": lab, "score": np.float32(round(float(rng.rand()), 2)), "box": np.array(b, np.float32),
                                "mask": shape_mask(b, H, W, ellipse=bool(rng.rand() < 0.5))})
            for _ in range(int(rng.randint(0, 8))):
                b = rand_box(rng, H, W, big=bool(rng.rand() < 0.2))
                dts.append({"label": int(rng.randint(1, NUM_CLASSES)), "score": np.float32(round(float(rng.rand()), 2)),
                            "box": np.array(b, np.float32), "mask": shape_mask(b, H, W, ellipse=bool(rng.rand() < 0.5))})
            dts = dts[:30]
        if i == 1 and dts:
            dts[0]["mask"] = np.zeros((H, W), dtype=bool)         # an empty detection mask
        # box coordinates off the integer grid for the bbox IoU (the masks stay as they are)
        for d in dts[2:]:
            d["box"] = (d["box"] + rng.uniform(-0.4, 0.4, 4).astype(np.float32)).astype(np.float32)
            d["box"][2:] = np.maximum(d["box"][2:], d["box"][:2])
        images.append({"size": (W, H), "dt": dts, "gt": gts})
    assert len(images[2]["gt"]) == 0 and len(images[5]["dt"]) == 0
    return images


def to_boxlists(images, device="cpu", with_masks=True, explicit_area=True):
    """-> (predictions, targets): dense bool planes [n, 1, H, W] in field `mask`, targets with masks / iscrowd / area"""
    preds, tgts = [], []
    for im in images:
        W, H = im["size"]
        dt, gt = im["dt"], im["gt"]
        p = BoxList(torch.from_numpy(np.array([d["box"] for d in dt], np.float32).reshape(-1, 4)), (W, H))
        p.add_field("scores", torch.from_numpy(np.array([d["score"] for d in dt], np.float32).reshape(-1)))
        p.add_field("labels", torch.from_numpy(np.array([d["label"] for d in dt], np.int64).reshape(-1)))
        t = BoxList(torch.from_numpy(np.array([g["box"] for g in gt], np.float32).reshape(-1, 4)), (W, H))
        t.add_field("labels", torch.from_numpy(np.array([g["label"] for g in gt], np.int64).reshape(-1)))
        t.add_field("iscrowd", torch.from_numpy(np.array([g["iscrowd"] for g in gt], np.uint8).reshape(-1)))
        if explicit_area:
            t.add_field("area", torch.from_numpy(np.array([g["area"] for g in gt], np.float64).reshape(-1)))
        if with_masks:
            p.add_field("mask", torch.from_numpy(np.array([d["mask"] for d in dt], bool).reshape(-1, 1, H, W)))
            t.add_field("masks", SegmentationMask(torch.from_numpy(np.array([g["mask"] for g in gt], np.uint8).reshape(-1, H, W)),
                                                  (W, H), mode="mask"))
        preds.append(p.to(device))
        tgts.append(t.to(device))
    return preds, tgts


def records_by_key(evaluator, iou_type):
    return {(r["image"], r["category"]): r for r in evaluator.records[iou_type]}


def boxlist(boxes, size, **fields):
    b = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), size)
    for k, v in fields.items():
        b.add_field(k, torch.as_tensor(v))
    return b


def voc_boxlists(fx, device="cpu"):
    """tests/golden/voc_eval_reference.npz -> (predictions, ground truths) as BoxLists"""
    preds, gts = [], []
    dp = np.concatenate([[0], np.cumsum(fx["pred_counts"])])
    gp = np.concatenate([[0], np.cumsum(fx["gt_counts"])])
    for i, size in enumerate(fx["sizes"]):
        size = (int(size[0]), int(size[1]))
        preds.append(boxlist(fx["pred_boxes"][dp[i]:dp[i + 1]], size, labels=fx["pred_labels"][dp[i]:dp[i + 1]],
                             scores=fx["pred_scores"][dp[i]:dp[i + 1]]))
        gts.append(boxlist(fx["gt_boxes"][gp[i]:gp[i + 1]], size, labels=fx["gt_labels"][gp[i]:gp[i + 1]],
                           difficult=fx["gt_difficult"][gp[i]:gp[i + 1]]))
    return [p.to(device) for p in preds], [g.to(device) for g in gts]


def check_voc_fixture(fx, preds, gts):
    """the reference's match values, prec, rec and both APs, reproduced exactly (APs to 1e-12)"""
    thresh = float(fx["iou_thresh"])
    n_pos, score, match = voc.voc_matches(gts, preds, thresh)
    prec, rec = voc.calc_detection_voc_prec_rec(gts, preds, thresh)
    assert sorted(n_pos) == [int(v) for v in fx["labels"]]
    for lab in n_pos:
        assert n_pos[lab] == int(fx["n_pos_%d" % lab])
        np.testing.assert_array_equal(np.array(score[lab], np.float32), fx["score_%d" % lab])
        np.testing.assert_array_equal(np.array(match[lab], np.int8), fx["match_%d" % lab])
        np.testing.assert_allclose(prec[lab], fx["prec_%d" % lab], rtol=0, atol=1e-12, equal_nan=True)
        if "rec_%d" % lab in fx:
            np.testing.assert_allclose(rec[lab], fx["rec_%d" % lab], rtol=0, atol=1e-12)
        else:
            assert rec[lab] is None
    for rule, key in ((True, "ap_07"), (False, "ap_area")):
        res = voc.eval_detection_voc(preds, gts, iou_thresh=thresh, use_07_metric=rule)
        np.testing.assert_allclose(res["ap"], fx[key], rtol=0, atol=1e-12, equal_nan=True)
        assert abs(res["map"] - np.nanmean(fx[key])) <= 1e-12
    assert abs(voc.eval_detection_voc(preds, gts, thresh, True)["map"] - float(fx["map_07"])) <= 1e-12
