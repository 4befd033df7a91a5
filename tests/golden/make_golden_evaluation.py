"""Generate tests/golden/voc_eval_reference.npz by running the REFERENCE's own VOC evaluation (build container only; never
runs on the GPU box).

The reference is made importable as in make_golden_masker.py (make_golden_whole_model's `install_reference`); its
data/datasets/evaluation/voc/voc_eval.py is pure numpy / torch and is loaded BY FILE PATH (the package's own __init__ chain
needs torchvision).  The file holds data only:
  sizes [I, 2] (W, H); pred_counts / gt_counts [I]; pred_boxes [Nd, 4] fp32 xyxy, pred_labels, pred_scores (all distinct:
  the reference ranks with an unstable sort); gt_boxes [Ng, 4], gt_labels, gt_difficult;
  labels: the labels that occur; per label l: prec_{l}, rec_{l} (absent without positives), match_{l} / score_{l}: the
  reference's per-detection match values (1 / 0 / -1) and scores, image after image, score descending inside an image;
  ap_07 / ap_area: calc_detection_voc_ap with use_07_metric True / False; iou_thresh.

Detections are jittered ground truths plus random boxes.  No IoU (the reference's, with its + 1) lies within 1e-5 of the
threshold, except ties built from integer boxes (intersection 50, union 100: exact in fp32); both are asserted.

Run:  python tests/golden/make_golden_evaluation.py
"""
import importlib.util
import os
import sys
from collections import defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_whole_model as W  # noqa: E402,F401  (installs the reference as `maskrcnn_benchmark`)

from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402
from maskrcnn_benchmark.structures.boxlist_ops import boxlist_iou  # noqa: E402

spec = importlib.util.spec_from_file_location(
    "ref_voc_eval", os.path.join(W.REF, "maskrcnn_benchmark", "data", "datasets", "evaluation", "voc", "voc_eval.py"))
voc = importlib.util.module_from_spec(spec)
spec.loader.exec_module(voc)

THRESH = 0.5
IMAGES = 36
LABELS = 4


class Recorded(defaultdict):
    """the dicts calc_detection_voc_prec_rec builds, in creation order: n_pos, score, match"""
    made = []

    def __init__(self, *a):
        super().__init__(*a)
        Recorded.made.append(self)


def main():
    rng = np.random.RandomState(20240911)
    sizes, preds, gts = [], [], []
    all_scores = rng.permutation(4000)[:2000] / 4000.0 + 0.0001          # distinct
    used = 0
    ties = 0
    for i in range(IMAGES):
        Wd, Hd = int(rng.randint(60, 200)), int(rng.randint(60, 200))
        ng = 0 if i == 3 else int(rng.randint(1, 7))
        x1 = rng.uniform(0, Wd - 20, ng)
        y1 = rng.uniform(0, Hd - 20, ng)
        gb = np.stack([x1, y1, x1 + rng.uniform(8, 50, ng), y1 + rng.uniform(8, 50, ng)], 1).reshape(-1, 4)
        gl = rng.randint(1, LABELS + 1, ng)
        gd = rng.rand(ng) < 0.2
        db, dl = [], []
        if i != 5:
            for k in range(ng):
                for _ in range(int(rng.randint(0, 4))):
                    db.append(gb[k] + rng.uniform(-6, 6, 4))
                    dl.append(gl[k] if rng.rand() < 0.85 else rng.randint(1, LABELS + 1))
            for _ in range(int(rng.randint(0, 5))):
                a, b = rng.uniform(0, Wd - 20), rng.uniform(0, Hd - 20)
                db.append([a, b, a + rng.uniform(8, 60), b + rng.uniform(8, 60)])
                dl.append(rng.randint(1, LABELS + 1))
        if i % 6 == 1:
            # integer boxes whose IoU is exactly the threshold: gt 10 x 10 (area 100 with the + 1s), detection 10 x 5 inside it
            ox, oy = int(rng.randint(0, 40)), int(rng.randint(0, 40))
            gb = np.concatenate([gb, [[ox, oy, ox + 8, oy + 8]]])
            gl = np.concatenate([gl, [LABELS]])
            gd = np.concatenate([gd, [False]])
            db.append([ox, oy, ox + 8, oy + 3])
            dl.append(LABELS)
            ties += 1
        db = np.array(db, dtype=np.float64).reshape(-1, 4)
        db[:, 2:] = np.maximum(db[:, 2:], db[:, :2] + 1)
        nd = db.shape[0]
        g = BoxList(torch.from_numpy(gb.astype(np.float32)).reshape(-1, 4), (Wd, Hd))
        g.add_field("labels", torch.from_numpy(np.asarray(gl, np.int64)))
        g.add_field("difficult", torch.from_numpy(np.asarray(gd, np.uint8)))
        p = BoxList(torch.from_numpy(db.astype(np.float32)).reshape(-1, 4), (Wd, Hd))
        p.add_field("labels", torch.from_numpy(np.asarray(dl, np.int64).reshape(-1)))
        p.add_field("scores", torch.from_numpy(all_scores[used:used + nd].astype(np.float32)))
        used += nd
        sizes.append((Wd, Hd))
        preds.append(p)
        gts.append(g)
    scores = torch.cat([p.get_field("scores") for p in preds]).numpy()
    assert np.unique(scores).size == scores.size, "scores must be distinct"

    # no IoU near the threshold, except exact ties of integer boxes
    exact = 0
    for p, g in zip(preds, gts):
        if len(p) == 0 or len(g) == 0:
            continue
        pb, gb_ = p.bbox.clone(), g.bbox.clone()
        pb[:, 2:] += 1
        gb_[:, 2:] += 1
        iou = boxlist_iou(BoxList(pb, p.size), BoxList(gb_, g.size)).numpy()
        for a in range(iou.shape[0]):
            for b in range(iou.shape[1]):
                if abs(float(iou[a, b]) - THRESH) <= 1e-5:
                    integer = bool((p.bbox[a] == p.bbox[a].round()).all() and (g.bbox[b] == g.bbox[b].round()).all())
                    assert integer and iou[a, b] == np.float32(THRESH), "an IoU within 1e-5 of the threshold: pick another seed"
                    exact += 1
    assert exact >= ties > 0

    voc.defaultdict = Recorded
    Recorded.made = []
    prec, rec = voc.calc_detection_voc_prec_rec(gt_boxlists=gts, pred_boxlists=preds, iou_thresh=THRESH)
    n_pos, score, match = Recorded.made[:3]
    out = {
        "iou_thresh": np.float64(THRESH), "sizes": np.array(sizes, np.int64),
        "pred_counts": np.array([len(p) for p in preds], np.int64), "gt_counts": np.array([len(g) for g in gts], np.int64),
        "pred_boxes": torch.cat([p.bbox for p in preds]).numpy(), "pred_labels": torch.cat([p.get_field("labels") for p in preds]).numpy(),
        "pred_scores": scores, "gt_boxes": torch.cat([g.bbox for g in gts]).numpy(),
        "gt_labels": torch.cat([g.get_field("labels") for g in gts]).numpy(),
        "gt_difficult": torch.cat([g.get_field("difficult") for g in gts]).numpy(),
        "labels": np.array(sorted(int(l) for l in n_pos.keys()), np.int64),
        "ap_07": voc.calc_detection_voc_ap(prec, rec, use_07_metric=True),
        "ap_area": voc.calc_detection_voc_ap(prec, rec, use_07_metric=False),
        "map_07": np.float64(voc.eval_detection_voc(preds, gts, THRESH, True)["map"]),
    }
    for l in n_pos.keys():
        out["n_pos_%d" % l] = np.int64(n_pos[l])
        out["prec_%d" % l] = np.asarray(prec[l], np.float64)
        if rec[l] is not None:
            out["rec_%d" % l] = np.asarray(rec[l], np.float64)
        out["match_%d" % l] = np.asarray(match[l], np.int8)
        out["score_%d" % l] = np.asarray(score[l], np.float32)
    counts = {v: int(sum((np.asarray(match[l]) == v).sum() for l in match)) for v in (1, 0, -1)}
    print("images %d, detections %d, ground truths %d, matches %s, exact ties %d, ap_07 %s" % (
        IMAGES, scores.size, int(out["gt_counts"].sum()), counts, exact, np.round(out["ap_07"], 4)))
    assert counts[1] > 20 and counts[0] > 20 and counts[-1] > 0
    path = os.path.join(HERE, "voc_eval_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
