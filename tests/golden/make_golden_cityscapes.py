"""Generate tests/golden/cityscapes_reference.npz by running the REFERENCE's own Cityscapes evaluation and dataset functions
(build container only; never runs on the GPU box).

The reference is made importable as in make_golden_box_proposals.py (make_golden_whole_model's `install_reference`), so
BoxList, SegmentationMask and Masker are the reference's own.  Its data/datasets/evaluation/cityscapes/eval_instances.py is
loaded BY FILE PATH with `np.float = float`, `np.bool = bool` and empty stand-ins for `cityscapesscripts.helpers.csHelpers`;
matchGtsWithPreds, evaluateBoxMatches, evaluateMaskMatches and computeAverages run unchanged on a stub dataset.
data/datasets/cityscapes.py is loaded by file path too (stand-ins for torchvision and its `.abstract`), and
`_processBinayMasks` / `_processPolygons` are called as plain functions on a stand-in object.

The file holds data only:
  classes: the names, `__background__` first; sizes [I, 2] the images' (W, H); gt_counts / pred_counts [I];
  gt_boxes [Ng, 4] fp32 xyxy; gt_labels [Ng]; gt_planes: per image "gt_planes_<i>" uint8 [n, H, W];
  pred_boxes [Nd, 4] fp32 xyxy; pred_labels, pred_scores [Nd]; pred_masks [Nd, 1, M, M] fp32 probabilities;
  "pred_planes_<i>" uint8 [n, H, W]: what the reference's Masker(threshold=0.5) pasted;
  gt_box_area, gt_pixel_count [Ng]; pred_box_area, pred_pixel_count [Nd], pred_kept [Nd] (0: dropped for zero pixels; such
  predictions are the last of their image, where the reference's slip of pairing masks by position has no effect);
  pairs [P, 5] int64: image, ground truth, prediction (both numbered inside the image, the prediction by its predID),
  boxIntersection, maskIntersection, sorted;
  box_ap, mask_ap [1, classes, 10] fp64 and box_avg / mask_avg [3 + 3 * classes]: allAp, allAp50%, allAp75%, then ap, ap50%,
  ap75% per class;
  id_map [h, w] int32 with ids_boxes [n, 4], ids_labels [n], ids_values [n] (the instance id of every mask, whose plane is
  id_map == id): _processBinayMasks;  poly_json (bytes of the json) with poly_boxes, poly_labels, poly_lengths and poly_flat
  (the polygons' coordinates, concatenated): _processPolygons.

The cases the issue lists are built on purpose and asserted below.

Run:  python tests/golden/make_golden_cityscapes.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

np.float = float  # noqa: removed from numpy >= 1.24, used by eval_instances.py
np.bool = bool  # noqa

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_whole_model as W  # noqa: E402,F401  (installs the reference as `maskrcnn_benchmark`)

from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402
from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask  # noqa: E402


def _stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


nothing = lambda *a, **k: None  # noqa: E731
_stand_in("cityscapesscripts")
_stand_in("cityscapesscripts.helpers", csHelpers=_stand_in(
    "cityscapesscripts.helpers.csHelpers", writeDict2JSON=nothing, ensurePath=nothing, colors=None, getColorEntry=nothing, labels=[]))
if "torchvision" not in sys.modules:
    _stand_in("torchvision")


def _load(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(W.REF, "maskrcnn_benchmark", *rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


ref = _load("ref_eval_instances", "data", "datasets", "evaluation", "cityscapes", "eval_instances.py")
_stand_in("refcs").__path__ = []
_stand_in("refcs.abstract", AbstractDataset=object)
ref_ds = _load("refcs.cityscapes", "data", "datasets", "cityscapes.py")

CLASSES = ["__background__", "person", "rider", "car", "truck"]      # car: ground truth only; truck: predictions only
M = 14


class StubDataset(object):
    CLASSES = CLASSES

    def __init__(self, sizes, targets):
        self.sizes, self.targets = sizes, targets
        self.id_to_name = dict(enumerate(CLASSES))

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, idx):
        return None, self.targets[idx], idx

    def get_img_info(self, idx):
        return {"width": self.sizes[idx][0], "height": self.sizes[idx][1]}


def rect_plane(size, box):
    """the filled rectangle of a box, maxima inclusive (a tight box of it is the box)"""
    w, h = size
    p = np.zeros((h, w), np.uint8)
    p[box[1]:box[3] + 1, box[0]:box[2] + 1] = 1
    return p


def blob_plane(size, box, rng):
    """an ellipse with a bite taken out, inside the box"""
    w, h = size
    ys, xs = np.mgrid[0:h, 0:w]
    cx, cy = (box[0] + box[2]) / 2.0, (box[1] + box[3]) / 2.0
    rx, ry = max((box[2] - box[0]) / 2.0, 0.5), max((box[3] - box[1]) / 2.0, 0.5)
    p = (((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0)
    p &= ~((xs > cx + rng.uniform(0, rx)) & (ys > cy + rng.uniform(0, ry)))
    return p.astype(np.uint8)


def tight_box(plane):
    ys, xs = np.nonzero(plane)
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def prob_mask(rng, kind):
    if kind == "ones":
        return np.ones((M, M), np.float32)
    if kind == "zeros":
        return np.zeros((M, M), np.float32)
    ys, xs = np.mgrid[0:M, 0:M]
    c = (M - 1) / 2.0
    r = np.sqrt(((xs - c - rng.uniform(-2, 2)) / (c + 1)) ** 2 + ((ys - c - rng.uniform(-2, 2)) / (c + 1)) ** 2)
    return np.clip(1.15 - r + rng.uniform(-0.05, 0.05, (M, M)), 0, 1).astype(np.float32)


def exact_plane(size, box, pred_plane, pred_box, ratio):
    """a ground-truth plane inside the window of `box` whose mask overlap with the pasted prediction is num / den exactly:
    `mi` pixels of the prediction's window and `gc - mi` pixels the prediction does not set, at least 100 in all"""
    w, h = size
    num, den = ratio
    win = np.zeros((h, w), bool)
    win[box[1]:box[3], box[0]:box[2]] = True
    pwin = np.zeros((h, w), bool)
    pwin[pred_box[1]:pred_box[3], pred_box[0]:pred_box[2]] = True
    pc = int((pred_plane.astype(bool) & pwin).sum())
    shared = np.argwhere(pred_plane.astype(bool) & pwin & win)
    free = np.argwhere(~pred_plane.astype(bool) & win)
    for mi in range(len(shared), 0, -1):
        for gc in range(max(mi, 100), mi + len(free) + 1):
            if num * (gc + pc - mi) == den * mi and float(mi) / (gc + pc - mi) == num / den:
                plane = np.zeros((h, w), np.uint8)
                plane[tuple(shared[:mi].T)] = 1
                plane[tuple(free[:gc - mi].T)] = 1
                return plane
    raise AssertionError("no exact plane for %s" % (ratio,))


def build_images():
    """-> [(size, [(box, label, plane)], [(box, label, score, mask kind)])]"""
    rng = np.random.RandomState(20)
    P, R, C, T = 1, 2, 3, 4
    images = []
    # 0: exact overlaps from integer rectangles.  person 10 x 10 = 100 (exactly minRegionSize); a prediction of 50 inside it:
    #    50 / 100 = 0.5, no match at the first threshold; a second, full prediction of lower score and a third of equal box:
    #    two predictions on one ground truth.  rider 20 x 10 = 200 with 150 / 200 = 0.75 and 120 / 200 = 0.6 inside it:
    #    0.75 > 0.7500000000000002 and 0.6 > 0.6000000000000001 are both false for the thresholds np.arange makes
    size = (97, 61)
    gts = [([20, 30, 30, 40], P), ([50, 10, 70, 20], R)]
    images.append((size, [(b, l, rect_plane(size, b)) for b, l in gts],
                   [([20, 30, 30, 35], P, 0.9, "ones"), ([20, 30, 30, 40], P, 0.8, "ones"), ([20, 30, 30, 40], P, 0.85, "ones"),
                    ([50, 10, 65, 20], R, 0.7, "ones"), ([50, 10, 62, 20], R, 0.7, "ones")]))
    # 1: ground truths on both sides of 100: box area 99 and 110, a box of 16 x 16 whose blob has under 100 pixels in its
    #    window; predictions over the small ones (the ignore rule) and one far from everything
    size = (80, 53)
    small = [4, 5, 13, 16]                # (13 - 4) * (16 - 5) = 99
    edge = [30, 6, 40, 17]                # 10 * 11 = 110
    thin = blob_plane(size, [50, 20, 66, 36], rng)
    thin[::2] = 0
    thin[1::4] = 0
    thin[28, 50:67] = 1
    thin[20:37, 58] = 1
    images.append((size, [(small, P, rect_plane(size, small)), (edge, P, rect_plane(size, edge)), (tight_box(thin), R, thin)],
                   [([4, 5, 13, 16], P, 0.6, "ones"), ([3, 4, 15, 18], P, 0.6, "blob"), ([30, 6, 40, 17], P, 0.95, "blob"),
                    ([50, 20, 66, 36], R, 0.5, "ones"), ([49, 19, 60, 30], R, 0.4, "blob"), ([70, 40, 78, 50], P, 0.3, "ones")]))
    # 2: predictions of another class over a ground truth: a rider over a person, a truck over a car, a person over a rider
    size = (120, 64)
    gts = [([10, 10, 40, 50], P), ([60, 8, 100, 30], C), ([50, 36, 90, 60], R)]
    images.append((size, [(b, l, blob_plane(size, b, rng)) for b, l in gts],
                   [([11, 10, 40, 49], R, 0.88, "blob"), ([60, 9, 99, 30], T, 0.77, "blob"), ([51, 36, 90, 59], P, 0.66, "blob"),
                    ([10, 12, 38, 50], P, 0.55, "blob")]))
    # 3: no predictions;  4: no ground truth
    size = (40, 47)
    gts = [([5, 5, 25, 30], P), ([20, 20, 38, 44], C)]
    images.append((size, [(b, l, blob_plane(size, b, rng)) for b, l in gts], []))
    images.append(((64, 40), [], [([5, 5, 30, 30], P, 0.45, "blob"), ([20, 10, 60, 35], T, 0.35, "ones")]))
    # 5: exact MASK overlaps.  The paste decides a prediction's pixels, so these ground-truth planes are made from the pasted
    #    planes (exact_plane): pixels of the prediction's window plus pixels outside it, counted so that
    #    maskIntersection / (pixelCount + pixelCount - maskIntersection) is the very ratio.  (plane: (prediction, ratio))
    size = (111, 90)
    images.append((size, [([5, 5, 45, 40], P, (0, (1, 2))), ([55, 5, 100, 38], R, (1, (3, 4))), ([8, 46, 60, 86], P, (2, (3, 5)))],
                   [([8, 8, 40, 36], P, 0.81, "blob"), ([58, 6, 98, 36], R, 0.71, "ones"), ([10, 48, 56, 84], P, 0.61, "blob")]))
    # 6 .. 12: seeded scenes; predictions are jittered ground truths with drawn labels and a few equal scores; images 7 and
    #    10 end in predictions whose probabilities are all zero (zero pixels: dropped)
    for i in range(6, 13):
        size = (int(rng.randint(40, 121)), int(rng.randint(40, 121)))
        w, h = size
        gts, preds = [], []
        for _ in range(rng.randint(2, 6)):
            bw, bh = rng.randint(6, w // 2), rng.randint(6, h // 2)
            x0, y0 = rng.randint(0, w - bw - 1), rng.randint(0, h - bh - 1)
            plane = blob_plane(size, [x0, y0, x0 + bw, y0 + bh], rng)
            gts.append((tight_box(plane), int(rng.choice([P, P, R, C])), plane))
        for b, l, _ in gts:
            for _ in range(rng.randint(0, 3)):
                j = rng.randint(-3, 4, 4)
                box = [max(b[0] + j[0], 0), max(b[1] + j[1], 0), min(b[2] + j[2], w - 1), min(b[3] + j[3], h - 1)]
                if box[2] - box[0] < 2 or box[3] - box[1] < 2:
                    continue
                label = l if l != C and rng.rand() < 0.7 else int(rng.choice([P, R, T]))
                preds.append((box, label, float(rng.choice([0.25, 0.5, 0.75, round(rng.rand(), 3)])), rng.choice(["blob", "blob", "ones"])))
        if i in (7, 10):
            preds += [([1, 1, 20, 20], P, 0.99, "zeros"), ([2, 3, 30, 33], R, 0.2, "zeros")]
        images.append((size, gts, preds))
    return images


def main():
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import Masker

    rng = np.random.RandomState(5)
    images = build_images()
    sizes = [im[0] for im in images]
    targets, predictions, out = [], [], {}
    pred_masks = []
    for i, (size, gts, preds) in enumerate(images):
        w, h = size
        p = BoxList(torch.tensor([q[0] for q in preds], dtype=torch.float32).reshape(-1, 4), size, mode="xyxy")
        p.add_field("labels", torch.tensor([q[1] for q in preds], dtype=torch.int64))
        p.add_field("scores", torch.tensor([q[2] for q in preds], dtype=torch.float32))
        masks = np.stack([prob_mask(rng, q[3]) for q in preds])[:, None] if preds else np.zeros((0, 1, M, M), np.float32)
        p.add_field("mask", torch.from_numpy(masks))
        pred_masks.append(masks)
        predictions.append(p)
        pasted = Masker(threshold=0.5).forward_single_image(torch.from_numpy(masks), p)[:, 0] if preds else torch.zeros((0, h, w))
        pasted = (pasted.numpy() != 0).astype(np.uint8).reshape(-1, h, w)
        out["pred_planes_%d" % i] = pasted
        gts = [(g[0], g[1], exact_plane(size, g[0], pasted[g[2][0]], preds[g[2][0]][0], g[2][1]) if isinstance(g[2], tuple) else g[2])
               for g in gts]
        t = BoxList(torch.tensor([g[0] for g in gts], dtype=torch.float32).reshape(-1, 4), size, mode="xyxy")
        t.add_field("labels", torch.tensor([g[1] for g in gts], dtype=torch.int64))
        planes = np.stack([g[2] for g in gts]) if gts else np.zeros((0, h, w), np.uint8)
        if gts:
            t.add_field("masks", SegmentationMask(torch.from_numpy(planes), size, mode="mask"))
        targets.append(t)
        out["gt_planes_%d" % i] = planes
        for b in [g[0] for g in gts] + [q[0] for q in preds]:
            assert 0 <= b[0] < b[2] <= w and 0 <= b[1] < b[3] <= h, (i, b)           # every box inside the image

    dataset = StubDataset(sizes, targets)
    matches = ref.matchGtsWithPreds(dataset, predictions)
    args = ref.deepcopy(ref.defaultArgs)
    args.instLabels = list(CLASSES)
    box_ap = ref.evaluateBoxMatches(matches, args)
    mask_ap = ref.evaluateMaskMatches(matches, args)
    box_avg, mask_avg = ref.computeAverages(box_ap, args), ref.computeAverages(mask_ap, args)

    def flat(avg):
        v = [avg["allAp"], avg["allAp50%"], avg["allAp75%"]]
        for name in CLASSES:
            v += [avg["classes"][name]["ap"], avg["classes"][name]["ap50%"], avg["classes"][name]["ap75%"]]
        return np.array(v, np.float64)

    gt_area, gt_count, pr_area, pr_count, pr_kept, pairs = [], [], [], [], [], []
    for i, m in enumerate(matches):
        gts = sorted((g for v in m["groundTruth"].values() for g in v), key=lambda g: g["instID"])
        prs = {p["predID"]: p for v in m["prediction"].values() for p in v}
        assert [g["instID"] for g in gts] == list(range(len(targets[i])))
        gt_area += [g["boxArea"] for g in gts]
        gt_count += [g["pixelCount"] for g in gts]
        bb = predictions[i].bbox.long()
        dropped = [k for k in range(len(predictions[i])) if k not in prs]
        assert dropped == list(range(len(prs), len(predictions[i]))), "zero-pixel predictions last in their image only"
        for k in range(len(predictions[i])):
            pr_area.append(int((bb[k, 2] - bb[k, 0]) * (bb[k, 3] - bb[k, 1])))
            pr_count.append(prs[k]["pixelCount"] if k in prs else 0)
            pr_kept.append(int(k in prs))
            if k in prs:
                assert prs[k]["boxArea"] == pr_area[-1]
        for g in gts:
            for p in g["matchedPred"]:
                pairs.append((i, g["instID"], p["predID"], int(p["boxIntersection"]), int(p["maskIntersection"])))
    pairs = np.array(sorted(pairs), np.int64).reshape(-1, 5)

    # ---- the cases the issue lists
    ga, gc = np.array(gt_area), np.array(gt_count)
    assert (ga < 100).any() and (ga == 100).any() and (ga > 100).any() and (gc < 100).any() and (gc >= 100).any()
    assert ((ga >= 100) & (gc < 100)).any()
    assert sum(pr_kept) < len(pr_kept)
    offs_g, offs_p = np.cumsum([0] + [len(t) for t in targets]), np.cumsum([0] + [len(p) for p in predictions])
    gl = np.concatenate([t.get_field("labels").numpy() for t in targets])
    pl = np.concatenate([p.get_field("labels").numpy() for p in predictions])
    ratios_b, ratios_m, cross, per_gt = [], [], 0, {}
    for i, g, p, bi, mi in pairs:
        G, Pd = offs_g[i] + g, offs_p[i] + p
        ratios_b.append(float(bi) / (ga[G] + pr_area[Pd] - bi))
        ratios_m.append(float(mi) / (gc[G] + pr_count[Pd] - mi))
        cross += int(gl[G] != pl[Pd] and ratios_b[-1] > 0.5)
        if ratios_b[-1] > 0.5:
            per_gt[(i, g)] = per_gt.get((i, g), 0) + 1
    for r in (ratios_b, ratios_m):                       # exactly 50 / 100, and exactly at two later thresholds' round values
        assert 0.5 in r and 0.75 in r and 0.6 in r, sorted(set(r))
    assert cross >= 3 and max(per_gt.values()) >= 2
    assert set(gl) == {1, 2, 3} and set(pl) == {1, 2, 4}
    assert any(len(t) and not len(p) for t, p in zip(targets, predictions)) and any(len(p) and not len(t) for t, p in zip(targets, predictions))
    assert np.isnan(box_ap[0, 0]).all() and np.isnan(box_ap[0, 4]).all() and (box_ap[0, 3] == 0).all() and (mask_ap[0, 3] == 0).all()
    assert np.nanmax(box_ap) > 0.3 and np.nanmax(mask_ap) > 0.3 and not np.array_equal(box_ap, mask_ap, equal_nan=True)

    # ---- the dataset's two functions
    stand = types.SimpleNamespace(CLASSES=["__background__", "person", "rider", "car"], name_to_id={"__background__": 0, "person": 1, "rider": 2, "car": 3},
                                  cityscapesID_to_ind={24: 1, 25: 2, 26: 3})
    id_map = np.full((40, 56), 7, np.int32)
    id_map[30:, :] = 26                                   # a group of cars: below 1000, no instance
    id_map[2:12, 3:9] = 24001
    id_map[5:25, 20:31] = 26000
    id_map[8:14, 22:27] = 24000                           # splits nothing: an island inside the car
    id_map[15:29, 40:55] = 25002
    id_map[0, 55] = 25002                                 # one far pixel stretches the tight box
    id_map[20:22, 2:4] = 24017
    boxes, masks, labels = ref_ds.CityScapesDataset._processBinayMasks(stand, torch.from_numpy(id_map))
    ids = [int(id_map[m.numpy()][0]) for m in masks]
    for m, v in zip(masks, ids):
        assert np.array_equal(m.numpy(), id_map == v)
    assert ids == sorted(ids) and len(ids) == 5
    ann = {"imgHeight": 40, "imgWidth": 56, "objects": [
        {"label": "road", "polygon": [[0, 30], [55, 30], [55, 39], [0, 39]]},
        {"label": "person", "polygon": [[3, 2], [8, 2], [9, 11], [5, 12], [3, 11]]},
        {"label": "cargroup", "polygon": [[0, 31], [30, 31], [30, 38]]},
        {"label": "car", "polygon": [[20.5, 5.25], [30.75, 5], [31, 24.5], [20, 24]]},
        {"label": "rider", "polygon": [[40, 15], [54, 16], [50, 28], [41, 27]]},
        {"label": "person", "polygon": [[2, 20], [4, 20], [3, 22]]}]}
    pboxes, polys, plabels = ref_ds.CityScapesDataset._processPolygons(stand, ann)
    assert len(polys) == 4 and all(len(p) == 1 for p in polys)

    out.update(
        classes=np.array(CLASSES), sizes=np.array(sizes, np.int64), gt_counts=np.array([len(t) for t in targets], np.int64),
        pred_counts=np.array([len(p) for p in predictions], np.int64),
        gt_boxes=torch.cat([t.bbox for t in targets]).numpy(), gt_labels=gl.astype(np.int64),
        pred_boxes=torch.cat([p.bbox for p in predictions]).numpy(), pred_labels=pl.astype(np.int64),
        pred_scores=torch.cat([p.get_field("scores") for p in predictions]).numpy(), pred_masks=np.concatenate(pred_masks),
        gt_box_area=ga.astype(np.int64), gt_pixel_count=gc.astype(np.int64), pred_box_area=np.array(pr_area, np.int64),
        pred_pixel_count=np.array(pr_count, np.int64), pred_kept=np.array(pr_kept, np.int64), pairs=pairs,
        box_ap=box_ap, mask_ap=mask_ap, box_avg=flat(box_avg), mask_avg=flat(mask_avg), overlaps=args.overlaps,
        id_map=id_map, ids_boxes=np.array(boxes, np.int64), ids_labels=np.array(labels, np.int64), ids_values=np.array(ids, np.int64),
        poly_json=np.frombuffer(json.dumps(ann).encode(), np.uint8), poly_boxes=np.array(pboxes, np.int64),
        poly_labels=np.array(plabels, np.int64), poly_lengths=np.array([len(p[0]) for p in polys], np.int64),
        poly_flat=np.array([v for p in polys for v in p[0]], np.float64))
    path = os.path.join(HERE, "cityscapes_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): %d images, %d ground truths, %d predictions (%d dropped), %d pairs" % (
        path, os.path.getsize(path), len(images), len(ga), len(pr_area), len(pr_kept) - sum(pr_kept), len(pairs)))
    print("box AP\n", np.round(box_ap[0], 4), "\nmask AP\n", np.round(mask_ap[0], 4))
    print("box avg", np.round(flat(box_avg)[:3], 4), "mask avg", np.round(flat(mask_avg)[:3], 4))


if __name__ == "__main__":
    main()
