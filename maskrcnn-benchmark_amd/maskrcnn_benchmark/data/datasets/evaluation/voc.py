"""PASCAL VOC detection evaluation (reference data/datasets/evaluation/voc/voc_eval.py) with the reference's signatures
and result dict.  IoU and the per-image matching run where the boxes live (on the device: csrc/evaluate.hip; CPU
tensors: _eval_cpu.py); precision, recall and both AP rules are host numpy.

Within an (image, label) problem the detections are taken by score descending with a STABLE sort (ties keep their input
order; the reference's `argsort()[::-1]` leaves the order of ties to numpy's quicksort), and so is the final ranking.
"""
import os

import numpy as np

from maskrcnn_benchmark import _C

from .coco_style import build_problems, flatten_batch


def voc_matches(gt_boxlists, pred_boxlists, iou_thresh=0.5):
    """-> (n_pos, score, match): dicts by label; score[l] / match[l] hold the detections of label l image after image, by
    score descending inside an image; match values 1 (true positive), 0 (false positive), -1 (a difficult ground truth)"""
    assert len(gt_boxlists) == len(pred_boxlists), "Length of gt and pred lists need to be same."
    b = flatten_batch(pred_boxlists, gt_boxlists, "difficult", resize=False)       # no class range: the largest label seen
    C = int(max(int(b.dt_label.max()) if b.dt_label.numel() else 0, int(b.gt_label.max()) if b.gt_label.numel() else 0)) + 1
    pr = build_problems(b.dt_img, b.dt_label, b.dt_score, b.gt_img, b.gt_label, C, max_dets=2 ** 31 - 1)
    do, go = pr["dt_order"], pr["gt_order"]
    offs = (pr["dt_offset"], pr["gt_offset"], pr["iou_offset"])
    iou = _C.eval_iou(_C.EVAL_VOC, *offs, pr["total_pairs"], dt_boxes=b.dt_box[do], gt_boxes=b.gt_box[go])
    m = _C.eval_match(_C.EVAL_VOC, iou, *offs, pr["counts_host"], b.gt_ignore[go], [float(iou_thresh)]).cpu().numpy()
    scores = b.dt_score[do].cpu().numpy()
    hard = b.gt_ignore[go].cpu().numpy()
    d = np.concatenate([[0], np.cumsum(pr["D"])])
    g = np.concatenate([[0], np.cumsum(pr["G"])])
    n_pos, score, match = {}, {}, {}
    for p in np.argsort(pr["category"], kind="mergesort"):        # label by label, images in order
        lab = int(pr["category"][p])
        n_pos[lab] = n_pos.get(lab, 0) + int(np.logical_not(hard[g[p]:g[p + 1]]).sum())
        score.setdefault(lab, []).extend(scores[d[p]:d[p + 1]])
        match.setdefault(lab, []).extend(m[d[p]:d[p + 1]])
    return n_pos, score, match


def calc_detection_voc_prec_rec(gt_boxlists, pred_boxlists, iou_thresh=0.5):
    """-> (prec, rec): lists indexed by label; None for a label that does not occur, rec[l] None without positives"""
    n_pos, score, match = voc_matches(gt_boxlists, pred_boxlists, iou_thresh)
    n = max(n_pos.keys()) + 1 if n_pos else 0
    prec, rec = [None] * n, [None] * n
    for lab in n_pos:
        order = np.argsort(-np.array(score[lab], dtype=np.float64), kind="mergesort")
        m = np.array(match[lab], dtype=np.int8)[order]
        tp, fp = np.cumsum(m == 1), np.cumsum(m == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            prec[lab] = tp / (fp + tp)                  # nan while only difficult matches have been seen
        if n_pos[lab] > 0:
            rec[lab] = tp / n_pos[lab]
    return prec, rec


def calc_detection_voc_ap(prec, rec, use_07_metric=False):
    """The two VOC rules: the 2007 one averages, over recall levels 0, 0.1 .. 1, the best precision at a recall of at least
    that level; the later one is the area under the precision envelope.  nan for a label without prec or rec."""
    ap = np.full((len(prec),), np.nan)
    for lab, (p, r) in enumerate(zip(prec, rec)):
        if p is None or r is None:
            continue
        p = np.nan_to_num(p)
        if use_07_metric:
            total = 0
            for level in np.arange(0.0, 1.1, 0.1):
                reached = r >= level
                total += (np.max(p[reached]) if reached.any() else 0) / 11
            ap[lab] = total
        else:
            envelope = np.maximum.accumulate(np.concatenate(([0], p, [0]))[::-1])[::-1]
            levels = np.concatenate(([0], r, [1]))
            step = np.where(levels[1:] != levels[:-1])[0]
            ap[lab] = np.sum((levels[step + 1] - levels[step]) * envelope[step + 1])
    return ap


def eval_detection_voc(pred_boxlists, gt_boxlists, iou_thresh=0.5, use_07_metric=False):
    """pred_boxlists carry `labels` and `scores`, gt_boxlists `labels` and `difficult` -> {"ap": per label, "map": nanmean}"""
    prec, rec = calc_detection_voc_prec_rec(gt_boxlists=gt_boxlists, pred_boxlists=pred_boxlists, iou_thresh=iou_thresh)
    ap = calc_detection_voc_ap(prec, rec, use_07_metric=use_07_metric)
    return {"ap": ap, "map": np.nanmean(ap)}


def do_voc_evaluation(dataset, predictions, output_folder, logger):
    preds, gts = [], []
    for image_id, prediction in enumerate(predictions):
        info = dataset.get_img_info(image_id)
        preds.append(prediction.resize((info["width"], info["height"])))
        gts.append(dataset.get_groundtruth(image_id))
    result = eval_detection_voc(pred_boxlists=preds, gt_boxlists=gts, iou_thresh=0.5, use_07_metric=True)
    text = "mAP: {:.4f}\n".format(result["map"])
    for i, ap in enumerate(result["ap"]):
        if i == 0:       # background
            continue
        name = dataset.map_class_id_to_class_name(i) if hasattr(dataset, "map_class_id_to_class_name") else str(i)
        text += "{:<16}: {:.4f}\n".format(name, ap)
    logger.info(text)
    if output_folder:
        with open(os.path.join(output_folder, "result.txt"), "w") as f:
            f.write(text)
    return result
