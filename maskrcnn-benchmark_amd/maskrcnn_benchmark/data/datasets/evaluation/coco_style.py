"""COCO-style detection evaluation as a streaming evaluator.

Per batch the detections and the ground truth are matched where they live (on the device: csrc/evaluate.hip through
maskrcnn_benchmark._C; CPU tensors: _eval_cpu.py) and only the match records are kept, a few KB per image; precision and
recall are accumulated from them once, on the host, in fp64 numpy.

The rules are a restatement of pycocotools.cocoeval (evaluateImg, accumulate, summarize) written from knowledge of that
code.  It has NOT been checked against pycocotools, which is not available where this project is built and tested;
tests/eval_refs.py is the literal, loop-by-loop form everything here is pinned to.
"""
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from maskrcnn_benchmark import _C
from maskrcnn_benchmark.structures.rle_masks import RLEMasks
from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREA_RNGS = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)
MAX_DETS = (1, 10, 100)
# The statistics of an IoU type, in the order they are reported: (name, 1 precision | 0 recall, IoU threshold or None for
# all ten, index into the evaluator's area ranges, index into its max_dets).  The keypoint evaluator has the area ranges
# (all, medium, large) and max_dets (20,): keypoint_oks.py.
_DETECTION_STATS = (("AP", 1, None, 0, 2), ("AP50", 1, 0.5, 0, 2), ("AP75", 1, 0.75, 0, 2), ("APs", 1, None, 1, 2),
                    ("APm", 1, None, 2, 2), ("APl", 1, None, 3, 2), ("AR1", 0, None, 0, 0), ("AR10", 0, None, 0, 1),
                    ("AR100", 0, None, 0, 2), ("ARs", 0, None, 1, 2), ("ARm", 0, None, 2, 2), ("ARl", 0, None, 3, 2))
STAT_ROWS = {
    "bbox": _DETECTION_STATS,
    "segm": _DETECTION_STATS,
    "keypoints": (("AP", 1, None, 0, 0), ("AP50", 1, 0.5, 0, 0), ("AP75", 1, 0.75, 0, 0), ("APm", 1, None, 1, 0),
                  ("APl", 1, None, 2, 0), ("AR", 0, None, 0, 0), ("AR50", 0, 0.5, 0, 0), ("AR75", 0, 0.75, 0, 0),
                  ("ARm", 0, None, 1, 0), ("ARl", 0, None, 2, 0)),
}
STAT_NAMES = tuple(row[0] for row in STAT_ROWS["bbox"])
_MATCH_MODE = {"bbox": _C.EVAL_COCO_BBOX, "segm": _C.EVAL_COCO_SEGM, "keypoints": _C.EVAL_COCO_BBOX}    # of _C.eval_match


Batch = namedtuple("Batch", "preds tgts dt_img gt_img dt_box gt_box dt_label gt_label dt_score gt_ignore counts")


def flatten_batch(predictions, targets, ignore_field="iscrowd", resize=True, first_image=0, num_classes=None):
    """Two lists of BoxList (one per image) -> a Batch, everything on the first target's device (no targets: the CPU):
    preds / tgts, the images' BoxLists in xyxy, a prediction resized to its target's size when `resize`; dt_img / gt_img
    int64, the image index of every row counted from `first_image`; dt_box / gt_box [n, 4]; dt_label / gt_label int64;
    dt_score; gt_ignore bool, the targets' `ignore_field` ("iscrowd" or "difficult") != 0, False where a target lacks the
    field; counts = (images, detections, ground truths).  ValueError: with `num_classes`, a label outside [0, num_classes)."""
    dev = targets[0].bbox.device if targets else torch.device("cpu")
    preds, tgts = [], []
    for pred, tgt in zip(predictions, targets):
        tgt = tgt.convert("xyxy")
        if resize and tuple(pred.size) != tuple(tgt.size):
            pred = pred.resize(tgt.size)
        preds.append(pred.convert("xyxy").to(dev))
        tgts.append(tgt)
    n_dt, n_gt = [len(p) for p in preds], [len(t) for t in tgts]
    i64 = dict(dtype=torch.int64, device=dev)
    img = torch.arange(len(preds), **i64) + first_image
    dt_img, gt_img = img.repeat_interleave(torch.tensor(n_dt, **i64)), img.repeat_interleave(torch.tensor(n_gt, **i64))
    cat = lambda ts, **kw: torch.cat(ts) if ts else torch.zeros((0,), **kw)  # noqa: E731
    dt_box = cat([p.bbox for p in preds]).reshape(-1, 4)
    gt_box = cat([t.bbox for t in tgts]).reshape(-1, 4)
    dt_label = cat([p.get_field("labels").to(**i64) for p in preds], **i64)
    gt_label = cat([t.get_field("labels").to(**i64) for t in tgts], **i64)
    dt_score = cat([p.get_field("scores").reshape(-1) for p in preds], device=dev)
    gt_ignore = cat([(t.get_field(ignore_field).to(dev) != 0) if t.has_field(ignore_field)
                     else torch.zeros((len(t),), dtype=torch.bool, device=dev) for t in tgts], dtype=torch.bool, device=dev)
    if num_classes is not None:
        for name, lab in (("prediction", dt_label), ("target", gt_label)):
            if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= num_classes):
                raise ValueError("%s labels must lie in [0, %d), got %d .. %d" % (name, num_classes, int(lab.min()), int(lab.max())))
    return Batch(preds, tgts, dt_img, gt_img, dt_box, gt_box, dt_label, gt_label, dt_score, gt_ignore,
                 (len(preds), sum(n_dt), sum(n_gt)))


def build_problems(dt_img, dt_label, dt_score, gt_img, gt_label, num_classes, max_dets=MAX_DETS[-1]):
    """The (image, category) problems of a batch, with torch sorts on the tensors' device.
    -> dict: dt_order / gt_order (indices into the inputs, sorted by problem; detections by score descending inside a
    problem, ties in input order, at most `max_dets` per problem), dt_offset / gt_offset [P + 1] int32, iou_offset [P + 1]
    int64 (device), and on the host: image / category [P], D / G [P] (numpy), total_pairs."""
    dev = dt_img.device
    dt_key = dt_img.to(torch.int64) * num_classes + dt_label.to(torch.int64)
    gt_key = gt_img.to(torch.int64) * num_classes + gt_label.to(torch.int64)
    keys = torch.unique(torch.cat([dt_key, gt_key]), sorted=True)
    P = keys.numel()
    dt_prob, gt_prob = torch.searchsorted(keys, dt_key), torch.searchsorted(keys, gt_key)
    by_score = torch.sort(dt_score.to(torch.float64), descending=True, stable=True)[1]
    dt_order = by_score[torch.sort(dt_prob[by_score], stable=True)[1]]
    gt_order = torch.sort(gt_prob, stable=True)[1]
    D = torch.bincount(dt_prob, minlength=P)[:P] if P else torch.zeros((0,), dtype=torch.int64, device=dev)
    G = torch.bincount(gt_prob, minlength=P)[:P] if P else torch.zeros((0,), dtype=torch.int64, device=dev)
    zero = torch.zeros((1,), dtype=torch.int64, device=dev)
    if P and int(D.max()) > max_dets:
        start = torch.cat([zero, torch.cumsum(D, 0)])[:-1]
        rank = torch.arange(dt_order.numel(), device=dev) - start[dt_prob[dt_order]]
        dt_order = dt_order[rank < max_dets]
        D = D.clamp(max=max_dets)
    dt_offset = torch.cat([zero, torch.cumsum(D, 0)])
    gt_offset = torch.cat([zero, torch.cumsum(G, 0)])
    iou_offset = torch.cat([zero, torch.cumsum(D * G, 0)])
    keys_h, D_h, G_h = keys.cpu().numpy(), D.cpu().numpy(), G.cpu().numpy()
    return {"dt_order": dt_order, "gt_order": gt_order, "dt_offset": dt_offset.to(torch.int32),
            "gt_offset": gt_offset.to(torch.int32), "iou_offset": iou_offset, "image": keys_h // num_classes,
            "category": keys_h % num_classes, "D": D_h, "G": G_h, "total_pairs": int((D_h * G_h).sum()),
            "counts_host": (int(D_h.sum()), int(G_h.sum()), int(G_h.max()) if P else 0)}


def _pack_masks(per_image):
    """per image a [n, H, W] uint8 / bool tensor or an RLEMasks -> the five tensors of _C.mask_pack over all of them, in
    order.  Dense planes alone are one _C.mask_pack call, as ever; runs go to _C.mask_pack_rle (consecutive RLE images
    share a call) and the packs are joined."""
    if not any(isinstance(m, RLEMasks) for m in per_image):
        return _C.mask_pack(per_image)
    packs, i = [], 0
    while i < len(per_image):
        rle, j = isinstance(per_image[i], RLEMasks), i
        while j < len(per_image) and isinstance(per_image[j], RLEMasks) == rle:
            j += 1
        if rle:
            seg, base, offsets = per_image[i:j], 0, [per_image[i].run_offset[:1]]
            for m in seg:
                offsets.append(m.run_offset[1:] + base)
                base += m.counts.numel()
            packs.append(_C.mask_pack_rle(torch.cat([m.counts for m in seg]), torch.cat(offsets), [hw for m in seg for hw in m.hw()]))
        else:
            packs.append(_C.mask_pack(per_image[i:j]))
        i = j
    sizes = [int(p[0].numel()) for p in packs]
    word_offset = torch.cat([p[1] + sum(sizes[:k]) for k, p in enumerate(packs)])
    return (torch.cat([p[0] for p in packs]), word_offset) + tuple(torch.cat([p[k] for p in packs]) for k in (2, 3, 4))


def _planes_of_target(target):
    masks = target.get_field("masks")
    if isinstance(masks, RLEMasks):
        if tuple(masks.size) != tuple(target.size):
            raise ValueError("ground-truth RLE masks of an image of %s for an image of %s" % (masks.size, tuple(target.size)))
        return masks.to(target.bbox.device)
    if isinstance(masks, SegmentationMask):
        masks = masks.convert("mask").instances.masks
    if masks.dim() == 2:
        masks = masks[None]
    W, H = target.size
    if tuple(masks.shape[-2:]) != (H, W):
        raise ValueError("ground-truth masks of size %s for an image of %s" % (tuple(masks.shape[-2:]), (H, W)))
    return (masks != 0) if masks.dtype not in (torch.uint8, torch.bool) else masks


def groundtruth_planes(tgts, dev):
    """per target its mask planes (_planes_of_target), all-zero planes for a target without masks"""
    return [_planes_of_target(t) if t.has_field("masks") else torch.zeros((len(t), t.size[1], t.size[0]), dtype=torch.uint8, device=dev)
            for t in tgts]


def groundtruth_area(tgts, gt_box, gt_pack):
    """The ground truths' areas, fp64 [G]: the `area` field; else the mask's pixel count (gt_pack: _pack_masks of
    groundtruth_planes, needed only then); else w * h of the xywh box.  gt_box: the targets' xyxy boxes, concatenated."""
    dev = gt_box.device
    gt_wh = (gt_box[:, 2:] - gt_box[:, :2]) + 1
    box_area = gt_wh[:, 0].to(torch.float64) * gt_wh[:, 1].to(torch.float64)
    parts, k = [], 0
    for t in tgts:
        n = len(t)
        if t.has_field("area"):
            parts.append(t.get_field("area").to(device=dev, dtype=torch.float64).reshape(-1))
        elif t.has_field("masks"):
            parts.append(gt_pack[3][k:k + n].to(torch.float64))
        else:
            parts.append(box_area[k:k + n])
        k += n
    return torch.cat(parts) if parts else torch.zeros((0,), dtype=torch.float64, device=dev)


def needs_mask_area(tgts):
    return any(t.has_field("masks") and not t.has_field("area") for t in tgts)


class COCOStyleEvaluator(object):
    """evaluator = COCOStyleEvaluator(("bbox", "segm"), num_classes); evaluator.update(predictions, targets) per batch;
    evaluator.summarize() -> {iou type: the 12 numbers AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl}.

    Labels are the contiguous ones (1 .. num_classes - 1).  The largest number of ground truths of one (image, category)
    pair the device matches is _C.EVAL_MAX_GT; larger problems are matched on the host."""

    def __init__(self, iou_types=("bbox",), num_classes=81):
        iou_types = tuple(iou_types)
        for t in iou_types:
            if t == "keypoints":
                raise NotImplementedError("the keypoints IoU type is scored by keypoint_oks.KeypointOKSEvaluator, not by this class")
            if t not in ("bbox", "segm"):
                raise ValueError("unknown IoU type %r" % (t,))
        self.iou_types = iou_types
        self.num_classes = int(num_classes)
        self.iou_thrs, self.rec_thrs, self.area_rngs, self.max_dets = IOU_THRS, REC_THRS, AREA_RNGS, MAX_DETS
        self.records = {t: [] for t in iou_types}
        self.num_images = self.num_detections = self.num_groundtruths = 0
        self.eval = {}

    # ------------------------------------------------------------------ per batch
    def update(self, predictions, targets):
        """predictions, targets: two lists of BoxList (one per image), on the device or the CPU.  Predictions carry
        `scores`, `labels` and, for segm, `mask`: dense bool planes [n, 1, H, W] of the image's size, or probabilities
        [n, 1, M, M], which Masker(threshold=0.5, padding=1) pastes, or an RLEMasks (the runs of a result file), which goes
        to bit rows without a plane.  Targets carry `labels` and may carry `masks` (either SegmentationMask mode, or an
        RLEMasks), `iscrowd` and `area`."""
        assert len(predictions) == len(targets), "one prediction per target"
        self._check_fields(predictions, targets)
        segm = "segm" in self.iou_types
        b = flatten_batch(predictions, targets, "iscrowd", True, self.num_images, self.num_classes)
        self.num_images += b.counts[0]
        self.num_detections += b.counts[1]        # before the cut to max_dets per problem
        self.num_groundtruths += b.counts[2]
        pr = build_problems(b.dt_img, b.dt_label, b.dt_score, b.gt_img, b.gt_label, self.num_classes, self.max_dets[-1])
        do, go = pr["dt_order"], pr["gt_order"]
        gt_pack = dt_pack = None
        if segm or needs_mask_area(b.tgts):    # planes, or their pixel counts
            gt_planes = groundtruth_planes(b.tgts, b.gt_box.device)
            if segm and not all(t.has_field("masks") or len(t) == 0 for t in b.tgts):
                raise ValueError("segm evaluation needs ground-truth masks")
            gt_pack = _pack_masks(gt_planes)
        if segm:
            dt_pack = _pack_masks(self._prediction_planes(b.preds))
        gt_area = groundtruth_area(b.tgts, b.gt_box, gt_pack)
        offs = (pr["dt_offset"], pr["gt_offset"], pr["iou_offset"])
        thrs, rngs = torch.from_numpy(self.iou_thrs), torch.from_numpy(self.area_rngs)
        for iou_type in self.iou_types:
            iou, dt_area, match_area = self._similarity(iou_type, b, pr, offs, gt_area, dt_pack, gt_pack)
            dtm, dti, gti = _C.eval_match(_MATCH_MODE[iou_type], iou, *offs, pr["counts_host"], b.gt_ignore[go], thrs,
                                          dt_area=dt_area, gt_area=match_area[go], area_rngs=rngs)
            self._keep(iou_type, pr, b.dt_score[do].to(torch.float64).cpu().numpy(), dtm.cpu().numpy(), dti.cpu().numpy(),
                       gti.cpu().numpy())

    def _check_fields(self, predictions, targets):
        """what a subclass requires of the BoxLists before anything is computed"""

    def _similarity(self, iou_type, b, pr, offs, gt_area, dt_pack, gt_pack):
        """-> (the fp64 similarities of every problem's pairs [total_pairs], the detections' areas in problem order, the
        ground truths' areas the matching takes, in input order).  b: the Batch; pr: its problems; offs: their offsets"""
        do, go = pr["dt_order"], pr["gt_order"]
        if iou_type == "bbox":
            iou = _C.eval_iou(_C.EVAL_COCO_BBOX, *offs, pr["total_pairs"], dt_boxes=b.dt_box[do], gt_boxes=b.gt_box[go],
                              gt_crowd=b.gt_ignore[go])
            dt_wh = (b.dt_box[:, 2:] - b.dt_box[:, :2]) + 1
            return iou, (dt_wh[:, 0].to(torch.float64) * dt_wh[:, 1].to(torch.float64))[do], gt_area
        dpk = (dt_pack[0], dt_pack[1][do], dt_pack[2][do], dt_pack[4][do])
        gpk = (gt_pack[0], gt_pack[1][go], gt_pack[2][go], gt_pack[4][go])
        counts = _C.mask_pair_counts(dpk, gpk, *offs, pr["total_pairs"])
        iou = _C.eval_iou(_C.EVAL_COCO_SEGM, *offs, pr["total_pairs"], counts=counts, dt_area=dt_pack[3][do],
                          gt_area=gt_pack[3][go], gt_crowd=b.gt_ignore[go])
        return iou, dt_pack[3][do].to(torch.float64), gt_area

    def _prediction_planes(self, preds):
        """-> per image a [n_i, H_i, W_i] uint8 / bool tensor, or the prediction's RLEMasks as it is"""
        from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import Masker

        out, paste = [None] * len(preds), []
        for i, p in enumerate(preds):
            W, H = p.size
            if len(p) == 0:
                out[i] = torch.zeros((0, H, W), dtype=torch.uint8, device=p.bbox.device)
                continue
            masks = p.get_field("mask")
            if isinstance(masks, RLEMasks):
                if tuple(masks.size) != (W, H):
                    raise ValueError("RLE prediction masks of an image of %s for an image of %s" % (masks.size, (W, H)))
                out[i] = masks
                continue
            if masks.dim() != 4 or masks.shape[1] != 1:
                raise ValueError("prediction masks must be [n, 1, H, W] planes or [n, 1, M, M] probabilities, got %s" % (tuple(masks.shape),))
            if masks.dtype == torch.bool or masks.dtype == torch.uint8:
                if tuple(masks.shape[-2:]) != (H, W):
                    raise ValueError("dense prediction masks of size %s for an image of %s" % (tuple(masks.shape[-2:]), (H, W)))
                out[i] = masks[:, 0].to(p.bbox.device)
            else:
                paste.append(i)
        if paste:
            pasted = Masker(threshold=0.5, padding=1)([preds[i].get_field("mask").to(preds[i].bbox.device) for i in paste],
                                                      [preds[i] for i in paste])
            for i, m in zip(paste, pasted):
                out[i] = m[:, 0]
        return out

    def _keep(self, iou_type, pr, scores, dtm, dti, gti):
        d, g = np.concatenate([[0], np.cumsum(pr["D"])]), np.concatenate([[0], np.cumsum(pr["G"])])
        for p in range(len(pr["D"])):
            self.records[iou_type].append({
                "image": int(pr["image"][p]), "category": int(pr["category"][p]), "scores": scores[d[p]:d[p + 1]].copy(),
                "dt_match": dtm[:, :, d[p]:d[p + 1]].copy(), "dt_ignore": dti[:, :, d[p]:d[p + 1]].copy(),
                "gt_ignore": gti[:, g[p]:g[p + 1]].copy()})

    # ------------------------------------------------------------------ once per evaluation
    def accumulate(self):
        """-> {iou type: {"precision": [T, R, K, A, M], "recall": [T, K, A, M]}}, K = num_classes - 1 (category k + 1), cells
        never filled are -1"""
        for iou_type in self.iou_types:
            self.eval[iou_type] = accumulate(self.records[iou_type], self.num_classes, self.iou_thrs, self.rec_thrs,
                                             len(self.area_rngs), self.max_dets)
        return self.eval

    def summarize(self):
        self.accumulate()
        self.stats = OrderedDict((t, summarize(self.eval[t], self.iou_thrs, STAT_ROWS[t])) for t in self.iou_types)
        return self.stats


def accumulate(records, num_classes, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, num_areas=len(AREA_RNGS), max_dets=MAX_DETS):
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), num_classes - 1, num_areas, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    by_cat = {}
    for r in sorted(records, key=lambda r: r["image"]):       # a stable sort: images in the order they arrived
        by_cat.setdefault(r["category"], []).append(r)
    for k in range(K):
        E = by_cat.get(k + 1, [])
        if not E:
            continue
        for a in range(A):
            gt_ig = np.concatenate([e["gt_ignore"][a] for e in E])
            npig = np.count_nonzero(gt_ig == 0)
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                scores = np.concatenate([e["scores"][:max_det] for e in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["dt_match"][a][:, :max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ignore"][a][:, :max_det] for e in E], axis=1)[:, inds]
                tps = np.logical_and(dtm >= 0, np.logical_not(dt_ig))
                fps = np.logical_and(dtm < 0, np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]          # non-increasing from the right
                    q = np.zeros((R,))
                    idx = np.searchsorted(rc, rec_thrs, side="left")
                    ok = idx < nd
                    q[ok] = pr[idx[ok]]
                    precision[t, :, k, a, m] = q
    return {"precision": precision, "recall": recall}


def summarize(ev, iou_thrs=IOU_THRS, rows=STAT_ROWS["bbox"]):
    """-> one number per row of `rows` (STAT_ROWS): the mean of the cells greater than -1, or -1 when there are none"""
    def stat(ap, thr, area, m):
        s = ev["precision"] if ap else ev["recall"]
        if thr is not None:
            s = s[np.nonzero(np.isclose(iou_thrs, thr))[0]]
        s = s[:, :, :, area, m] if ap else s[:, :, area, m]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    return np.array([stat(*row[1:]) for row in rows])


# ------------------------------------------------------------------------------------------------ scoring stored predictions
def _groundtruth(dataset, index):
    return dataset.get_groundtruth(index) if hasattr(dataset, "get_groundtruth") else dataset[index][1]


def _num_classes(dataset, default):
    return getattr(dataset, "num_classes", None) or default


def _feed(evaluator, predictions, dataset, batch, device=None):
    """`predictions` (one per image, in dataset order) go to evaluator.update `batch` images at a time, against the
    dataset's ground truth moved to `device` (None: where the batch's first prediction lives) -> evaluator"""
    for i in range(0, len(predictions), batch):
        preds = list(predictions[i:i + batch])
        dev = preds[0].bbox.device if device is None else device
        evaluator.update(preds, [_groundtruth(dataset, j).to(dev) for j in range(i, i + len(preds))])
    return evaluator
