"""Generate tests/golden/box_proposals_reference.npz by running the REFERENCE's own evaluate_box_proposals (build container
only; never runs on the GPU box).

The reference is made importable as in make_golden_evaluation.py (make_golden_whole_model's `install_reference`); its
data/datasets/evaluation/coco/coco_eval.py is loaded BY FILE PATH (the package's own __init__ chain needs pycocotools) and
handed a stub dataset: `id_to_img_map`, `get_img_info`, `coco.getAnnIds` / `coco.loadAnns`.  The file holds data only:
  sizes [I, 2] the images' (W, H); pred_sizes [I, 2] the sizes the proposals are given in; pred_counts / gt_counts [I];
  pred_boxes [Nd, 4] fp32 xyxy; pred_objectness [Nd] fp32 (all distinct, NOT sorted: the reference's sort is unstable);
  gt_xywh [Ng, 4] fp32, the json `bbox`; gt_area [Ng] fp32, the json `area` (floats, not the box area); gt_iscrowd [Ng];
  limits (0 stands for None); areas: the eight names;
  per call, under "<limit>/<area>/": ar, recalls, num_pos, gt_overlaps (sorted, as returned).

The cases the issue lists are built on purpose and asserted below: proposals given at other sizes than the image with unequal
ratios, areas exactly 32^2 and 96^2, crowds, an image without ground truth, one with only crowds, one without proposals, one
with more ground truths than proposals, ground truths that share their best proposal, and exact ties at IoU 0.5 from integer
boxes (intersection 50, union 100) whose resolution changes a later round.

Run:  python tests/golden/make_golden_box_proposals.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_whole_model as W  # noqa: E402,F401  (installs the reference as `maskrcnn_benchmark`)

from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402
from maskrcnn_benchmark.structures.boxlist_ops import boxlist_iou  # noqa: E402

spec = importlib.util.spec_from_file_location(
    "ref_coco_eval", os.path.join(W.REF, "maskrcnn_benchmark", "data", "datasets", "evaluation", "coco", "coco_eval.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

LIMITS = (None, 3, 100, 1000)
AREAS = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")
# an `area` for every range; 32^2 and 96^2 lie in both neighbouring ranges
AREA_POOL = (150.5, 900.25, 1024.0, 1024.0, 2500.75, 9216.0, 9216.0, 12000.5, 16384.0, 30000.25, 70000.5, 100000.0, 262144.0,
             300000.5)


class StubCOCO(object):
    def __init__(self, anns):
        self.anns = anns                      # {image id: [annotation]}

    def getAnnIds(self, imgIds):
        return [(imgIds, k) for k in range(len(self.anns[imgIds]))]

    def loadAnns(self, ids):
        return [self.anns[i][k] for i, k in ids]


class StubDataset(object):
    def __init__(self, sizes, anns):
        self.id_to_img_map = {i: 1000 + 7 * i for i in range(len(sizes))}
        self.sizes = sizes
        self.coco = StubCOCO({self.id_to_img_map[i]: a for i, a in enumerate(anns)})

    def get_img_info(self, index):
        return {"width": self.sizes[index][0], "height": self.sizes[index][1]}


def tie_image_proposals(ox, oy, first):
    """Two proposals tie at IoU 0.5 for ground truth 0 (its top and its bottom half); ground truth 1 overlaps the bottom
    half only.  The first maximum (the proposal of higher objectness) decides what is left for ground truth 1."""
    gts = [[ox, oy, 10, 10], [ox, oy + 8, 10, 10]]
    top, bottom = [ox, oy, ox + 9, oy + 4], [ox, oy + 5, ox + 9, oy + 9]
    return gts, ([top, bottom] if first == "top" else [bottom, top])


def tie_image_groundtruths(ox, oy):
    """Two ground truths tie at IoU 0.5 for one proposal (the bottom half of the first, the top half of the second); each
    has a fallback of its own, of different IoU.  The first maximum (the lower ground-truth index) takes the proposal."""
    gts = [[ox, oy, 10, 10], [ox, oy + 5, 10, 10]]
    shared = [ox, oy + 5, ox + 9, oy + 9]
    return gts, [shared, [ox, oy, ox + 9, oy + 2], [ox, oy + 11, ox + 9, oy + 14]]


def main():
    rng = np.random.RandomState(20241007)
    sizes, pred_sizes, preds, anns = [], [], [], []
    objectness = rng.permutation(8000)[:4000] / 8000.0 + 0.0001          # distinct
    used = pool = 0
    for i in range(12):
        Wd, Hd = int(rng.randint(120, 260)), int(rng.randint(120, 260))
        exact = i in (7, 8, 9)                                           # the built ties: integer boxes, no resize
        Wp, Hp = (Wd, Hd) if exact or i % 2 == 0 else (int(rng.randint(200, 400)), int(rng.randint(200, 400)))
        ng = {3: 0, 6: 6}.get(i, int(rng.randint(2, 7)))
        x1, y1 = rng.uniform(0, Wd - 60, ng), rng.uniform(0, Hd - 60, ng)
        gb = np.stack([x1, y1, rng.uniform(8, 58, ng), rng.uniform(8, 58, ng)], 1).reshape(-1, 4)      # xywh
        crowd = np.ones(ng, bool) if i == 4 else rng.rand(ng) < (0.25 if i not in (5, 6) else 0.0)
        db = []
        if i == 1:                                                       # two neighbours under one wide proposal
            gb = np.concatenate([gb, [[10, 12, 20, 20], [32, 12, 20, 20]]])
            crowd = np.concatenate([crowd, [False, False]])
            db.append([10, 12, 51, 31])
        if exact:
            ox, oy = 20 + 3 * i, 30
            g, d = tie_image_groundtruths(ox, oy) if i == 9 else tie_image_proposals(ox, oy, "top" if i == 7 else "bottom")
            gb, crowd = np.array(g, np.float64), np.zeros(len(g), bool)
            db = d + [[ox + 60.5, oy + 40.25, ox + 80.5, oy + 70.0]]
        elif i == 6:
            db = [list(gb[0, :2]) + list(gb[0, :2] + gb[0, 2:] - 1 + rng.uniform(-3, 3, 2)), [5.5, 6.5, 40.25, 50.0]]
        elif i != 5:
            for k in range(gb.shape[0]):
                for _ in range(int(rng.randint(0, 4))):
                    db.append(np.concatenate([gb[k, :2], gb[k, :2] + gb[k, 2:] - 1]) + rng.uniform(-7, 7, 4))
            for _ in range(int(rng.randint(1, 6))):
                a, b = rng.uniform(0, Wd - 40), rng.uniform(0, Hd - 40)
                db.append([a, b, a + rng.uniform(8, 60), b + rng.uniform(8, 60)])
        db = np.array(db, np.float64).reshape(-1, 4)
        db[:, 2:] = np.maximum(db[:, 2:], db[:, :2] + 1)
        db = db * np.array([Wp / Wd, Hp / Hd, Wp / Wd, Hp / Hd])           # given at the prediction's own size
        nd = db.shape[0]
        obj = objectness[used:used + nd].astype(np.float32)
        if exact:
            obj = np.sort(obj)[::-1].copy()                              # the built order IS the objectness order
        used += nd
        p = BoxList(torch.from_numpy(db.astype(np.float32)).reshape(-1, 4), (Wp, Hp))
        p.add_field("objectness", torch.from_numpy(obj))
        a = []
        for k in range(gb.shape[0]):
            a.append({"bbox": [float(np.float32(v)) for v in gb[k]], "area": float(np.float32(AREA_POOL[pool % len(AREA_POOL)])),
                      "iscrowd": int(crowd[k])})
            pool += 1
        sizes.append((Wd, Hd))
        pred_sizes.append((Wp, Hp))
        preds.append(p)
        anns.append(a)
    dataset = StubDataset(sizes, anns)

    # ---- the cases, asserted
    obj_all = torch.cat([p.get_field("objectness") for p in preds]).numpy()
    assert np.unique(obj_all).size == obj_all.size, "objectness must be distinct"
    assert any((np.diff(p.get_field("objectness").numpy()) > 0).any() for p in preds), "given in unsorted order"
    assert any(ps != s and ps[0] * s[1] != ps[1] * s[0] for ps, s in zip(pred_sizes, sizes)), "unequal w and h ratios"
    flat = [o for a in anns for o in a]
    assert any(o["area"] == 32.0 ** 2 for o in flat) and any(o["area"] == 96.0 ** 2 for o in flat)
    assert all(abs(o["area"] - o["bbox"][2] * o["bbox"][3]) > 1e-3 for o in flat), "the area is not the box area"
    assert any(o["iscrowd"] for o in flat)
    live = [[o for o in a if not o["iscrowd"]] for a in anns]
    assert len(anns[3]) == 0 and len(anns[4]) > 0 and len(live[4]) == 0
    assert len(preds[5]) == 0 and len(live[5]) > 0 and len(live[6]) > len(preds[6]) > 0
    assert any(len(p) > 3 for p, g in zip(preds, live) if g)
    shared = ties = 0
    for i, (p, g) in enumerate(zip(preds, live)):
        if not g or len(p) == 0:
            continue
        pr = p.resize(sizes[i])
        pr = pr[pr.get_field("objectness").sort(descending=True)[1]]
        gl = BoxList(torch.as_tensor([o["bbox"] for o in g]).reshape(-1, 4), sizes[i], mode="xywh").convert("xyxy")
        iou = boxlist_iou(pr, gl).numpy()
        best = iou.argmax(0)
        shared += int(len(best) - len(set(best.tolist())) > 0 and (iou.max(0) > 0).sum() >= 2)
        col_ties = ((iou == iou.max(0, keepdims=True)) & (iou > 0)).sum(0)           # proposals tied for a ground truth
        row_max = iou.max(0)
        ties += int((col_ties > 1).any()) + int(row_max.max() > 0 and (row_max == row_max.max()).sum() > 1)
        if i in (7, 8, 9):
            assert iou.max() == np.float32(0.5), iou
    assert shared >= 1, "several ground truths sharing one best proposal"
    assert ties >= 2, "at least two exact ties at a positive IoU"

    out = {
        "sizes": np.array(sizes, np.int64), "pred_sizes": np.array(pred_sizes, np.int64),
        "pred_counts": np.array([len(p) for p in preds], np.int64), "gt_counts": np.array([len(a) for a in anns], np.int64),
        "pred_boxes": torch.cat([p.bbox for p in preds]).numpy(), "pred_objectness": obj_all,
        "gt_xywh": np.array([o["bbox"] for o in flat], np.float32).reshape(-1, 4),
        "gt_area": np.array([o["area"] for o in flat], np.float32), "gt_iscrowd": np.array([o["iscrowd"] for o in flat], np.int64),
        "limits": np.array([0 if v is None else v for v in LIMITS], np.int64), "areas": np.array(AREAS),
    }
    for limit in LIMITS:
        for area in AREAS:
            r = ref.evaluate_box_proposals(preds, dataset, area=area, limit=limit)
            assert r["num_pos"] > 0, (limit, area)
            key = "%d/%s/" % (limit or 0, area)
            out[key + "ar"] = np.float32(r["ar"].item())
            out[key + "recalls"] = r["recalls"].numpy()
            out[key + "num_pos"] = np.int64(r["num_pos"])
            out[key + "gt_overlaps"] = r["gt_overlaps"].numpy()
            if area in ("all", "medium"):
                print("limit %s area %s: ar %.4f num_pos %d overlaps %s" % (limit, area, r["ar"].item(), r["num_pos"],
                                                                             np.round(r["gt_overlaps"].numpy(), 3)))
    out["thresholds"] = r["thresholds"].numpy()
    assert not np.array_equal(out["0/all/gt_overlaps"], out["3/all/gt_overlaps"])
    path = os.path.join(HERE, "box_proposals_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); images %d, proposals %d, ground truths %d" % (path, os.path.getsize(path), len(sizes), obj_all.size, len(flat)))


if __name__ == "__main__":
    main()
