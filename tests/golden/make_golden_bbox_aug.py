"""Generate tests/golden/bbox_aug_reference.npz by running the REFERENCE's own box-augmentation merge on the CPU (build
container only; never runs on the GPU box).

The reference is made importable as in make_golden_evaluation.py (make_golden_whole_model's `install_reference`).  What
engine/bbox_aug.py does with the passes' outputs is replayed with the reference's own objects: per (image, pass) group a
BoxList of the per-class boxes [n*C, 4] with `scores` [n*C] in the pass's frame, clip_to_image(remove_empty=False) (the
PostProcessor.forward of a model built with BBOX_AUG), transpose(0) for a flipped pass, resize to the first pass's frame for
every pass but the first, torch.cat per image, and PostProcessor.filter_results.  The file holds data only:
  boxes [R, 4C], scores [R, C] fp32: the rows of every group, image-major, passes in order (NOT yet clipped);
  row_offset int32 [N*T + 1]; frames int32 [N, T, 2] (w, h); flips int32 [T]; score_thresh, nms, detections_per_img;
  merged [R*C, 4]: every box after clip / transpose / resize (row-major over (row, class));
  det_counts [N]; det_boxes [D, 4], det_scores [D], det_labels [D]: filter_results' output, image after image.

3 images, C = 5, 0-40 rows per group, 4 passes: identity, flip (odd width), a scale with unequal w / h ratios, that scale
flipped.  Asserted here: distinct scores, no candidate pair of one (image, class) with an IoU within 1e-5 of the NMS
threshold, no score within 1e-6 of the score threshold, an image with more detections than detections_per_img before the
limit, an image with none, a group without rows.

Run:  python tests/golden/make_golden_bbox_aug.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_whole_model as W  # noqa: E402,F401  (installs the reference as `maskrcnn_benchmark`)

from maskrcnn_benchmark.modeling.roi_heads.box_head.inference import PostProcessor  # noqa: E402
from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402
from maskrcnn_benchmark.structures.boxlist_ops import boxlist_iou  # noqa: E402

C = 5
SCORE_THRESH, NMS, DETECTIONS_PER_IMG = 0.05, 0.5, 10
FLIPS = (0, 1, 0, 1)
FRAMES = [[(101, 75), (101, 75), (151, 113), (151, 113)],        # ratios 101/151 != 75/113
          [(67, 90), (67, 90), (95, 127), (95, 127)],
          [(83, 83), (83, 83), (120, 121), (120, 121)]]
ROWS = [[40, 31, 36, 17], [12, 0, 25, 9], [7, 11, 0, 5]]


def main():
    rng = np.random.RandomState(20241019)
    N, T = len(FRAMES), len(FLIPS)
    R = sum(sum(r) for r in ROWS)
    pool = rng.permutation(20000)[:R * C] / 20000.0 + 0.00002    # distinct, none at the threshold
    pool = pool.astype(np.float32).reshape(R, C)
    assert len(np.unique(pool)) == R * C
    boxes, scores, row_offset = [], [], [0]
    r0 = 0
    for i in range(N):
        w0, h0 = FRAMES[i][0]
        objects = np.stack([rng.uniform(0, w0 - 30, 6), rng.uniform(0, h0 - 30, 6)], 1)
        objects = np.concatenate([objects, objects + rng.uniform(12, 40, (6, 2))], 1)
        for t in range(T):
            w, h = FRAMES[i][t]
            n = ROWS[i][t]
            b = objects[rng.randint(0, 6, (n, C))] + rng.uniform(-5, 5, (n, C, 4))     # first-frame coordinates
            b[rng.rand(n, C) < 0.15] += rng.uniform(-40, 40, 4)                          # some leave the frame: clipped
            b = b * np.array([w / w0, h / h0, w / w0, h / h0])
            if FLIPS[t]:
                b = np.stack([w - 1 - b[..., 2], b[..., 1], w - 1 - b[..., 0], b[..., 3]], -1)
            s = pool[r0:r0 + n].copy()
            # about a third of the pairs are candidates; image 2 has none
            low = rng.rand(n, C) < 0.65 if i != 2 else np.ones((n, C), bool)
            s[low] = s[low] * np.float32(0.04)
            r0 += n
            boxes.append(b.reshape(n, 4 * C).astype(np.float32))
            scores.append(s.astype(np.float32))
            row_offset.append(row_offset[-1] + n)
    boxes, scores = np.concatenate(boxes), np.concatenate(scores)
    assert len(np.unique(scores)) == scores.size, "scores must be distinct"
    assert np.abs(scores - np.float32(SCORE_THRESH)).min() > 1e-6
    assert min(min(r) for r in ROWS) == 0

    post = PostProcessor(SCORE_THRESH, NMS, DETECTIONS_PER_IMG)
    unlimited = PostProcessor(SCORE_THRESH, NMS, 0)
    merged, det_counts, det_boxes, det_scores, det_labels = [], [], [], [], []
    over = 0
    for i in range(N):
        lists = []
        for t in range(T):
            g = i * T + t
            lo, hi = row_offset[g], row_offset[g + 1]
            bl = BoxList(torch.from_numpy(boxes[lo:hi]).reshape(-1, 4).clone(), FRAMES[i][t], mode="xyxy")
            bl.add_field("scores", torch.from_numpy(scores[lo:hi]).reshape(-1))
            bl = bl.clip_to_image(remove_empty=False)
            if FLIPS[t]:
                bl = bl.transpose(0)
            lists.append(bl if t == 0 else bl.resize(lists[0].size))
        bbox = torch.cat([b.bbox for b in lists])
        sc = torch.cat([b.get_field("scores") for b in lists])
        assert bbox.dtype == torch.float32
        whole = BoxList(bbox, lists[0].size, lists[0].mode)
        whole.add_field("scores", sc)
        merged.append(bbox.numpy().copy())
        # no candidate pair of one class at the NMS threshold
        b2, s2 = bbox.reshape(-1, C * 4), sc.reshape(-1, C)
        for j in range(1, C):
            sel = (s2[:, j] > SCORE_THRESH).nonzero().squeeze(1)
            if sel.numel() > 1:
                cls = BoxList(b2[sel, 4 * j:4 * j + 4], whole.size)
                iou = boxlist_iou(cls, cls)
                assert (iou - NMS).abs().min() > 1e-5, "a pair at the NMS threshold"
        out = post.filter_results(whole, C)
        over += len(unlimited.filter_results(whole, C)) > DETECTIONS_PER_IMG
        det_counts.append(len(out))
        det_boxes.append(out.bbox.numpy())
        det_scores.append(out.get_field("scores").numpy())
        det_labels.append(out.get_field("labels").numpy())
    assert over >= 1, "no image goes over detections_per_img"
    assert min(det_counts) == 0, "no image without detections"
    path = os.path.join(HERE, "bbox_aug_reference.npz")
    np.savez_compressed(
        path, boxes=boxes, scores=scores, row_offset=np.array(row_offset, np.int32), frames=np.array(FRAMES, np.int32),
        flips=np.array(FLIPS, np.int32), score_thresh=np.float64(SCORE_THRESH), nms=np.float64(NMS),
        detections_per_img=np.int32(DETECTIONS_PER_IMG), merged=np.concatenate(merged).astype(np.float32),
        det_counts=np.array(det_counts, np.int32), det_boxes=np.concatenate(det_boxes).astype(np.float32).reshape(-1, 4),
        det_scores=np.concatenate(det_scores).astype(np.float32), det_labels=np.concatenate(det_labels).astype(np.int64))
    print("wrote", path, "rows", boxes.shape[0], "detections per image", det_counts)


if __name__ == "__main__":
    main()
