"""Generate tests/golden/model_keypoints.npz and whole_model_keypoint_rcnn.npz by running the REFERENCE's own keypoint code
(build container only; never runs on the GPU box).

The reference is made importable exactly as in make_golden_whole_model.py (its `install_reference`: yacs / apex / cv2 /
pycocotools stubs, the reference's own CPU kernels as `_C`).  OpenCV is absent here, so the `cv2.resize(..., INTER_CUBIC)`
that the reference's `heatmaps_to_keypoints` calls (roi_heads/keypoint_head/inference.py:70-72) is supplied by fp64
`torch.nn.functional.interpolate(mode="bicubic", align_corners=False)` — the same kernel (A = -0.75, source coordinate
(d + 0.5) * in / out - 0.5, border taps clamped), evaluated in float64 instead of OpenCV's float32.  The argmax, the
width / height correction and the offset arithmetic of the fixture are the reference's; the resize is the stand-in.

model_keypoints.npz
  * structures/keypoint.py: PersonKeypoints resize / transpose(FLIP_LEFT_RIGHT) / indexing, and as a BoxList field through
    clip_to_image(remove_empty=True);
  * keypoints_to_heat_map on random points, on the boundary cases (x == x2, points on and just outside the box edges,
    v = 0) and on integer-aligned boxes and points (where the rounding of M / (x2 - x1) decides the cell);
  * KeypointRCNNLossComputation.subsample (loss.py:79-143) on box-head-like proposal sets whose positives never exceed the
    sampler's positive quota (so no random stream decides which ROIs are kept), and the loss value (loss.py:145-169) on
    deterministic logits (`_logits` below: a closed form, nothing stored);
  * heatmaps_to_keypoints outputs with the fp64 stand-in, and the top-two margin of every resized map.
whole_model_keypoint_rcnn.npz
  the reference's GeneralizedRCNN with KEYPOINT_ON on the narrow R-50-FPN of whole_model_mask_rcnn with
  ROI_KEYPOINT_HEAD.CONV_LAYERS (16, 16): state_dict, a two-image batch with keypoints, the loss dict.

Run:  python tests/golden/make_golden_keypoint.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_whole_model as W  # noqa: E402  (installs the reference as `maskrcnn_benchmark`)

cv2 = sys.modules["cv2"]
cv2.INTER_CUBIC = 2


def _resize_fp64(img, dsize, interpolation=None):
    """cv2.resize stand-in: HWC float map -> (dsize[1], dsize[0], C) float64 bicubic"""
    t = torch.from_numpy(np.ascontiguousarray(img)).double().permute(2, 0, 1)[None]
    out = F.interpolate(t, size=(int(dsize[1]), int(dsize[0])), mode="bicubic", align_corners=False)
    return out[0].permute(1, 2, 0).numpy()


cv2.resize = _resize_fp64

from maskrcnn_benchmark.config import cfg as ref_cfg  # noqa: E402
from maskrcnn_benchmark.modeling.detector import build_detection_model  # noqa: E402
from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.inference import heatmaps_to_keypoints  # noqa: E402
from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.loss import make_roi_keypoint_loss_evaluator  # noqa: E402
from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402
from maskrcnn_benchmark.structures.image_list import to_image_list  # noqa: E402
from maskrcnn_benchmark.structures.keypoint import FLIP_LEFT_RIGHT, PersonKeypoints, keypoints_to_heat_map  # noqa: E402


def _logits(n, K=17, M=56):
    """deterministic keypoint logits [n, K, M, M] (the test rebuilds them from this formula)"""
    i = torch.arange(n * K * M * M, dtype=torch.float64)
    return (4.0 * torch.sin(i * 0.37) + torch.cos(i * 0.011)).float().view(n, K, M, M)


def _keypoints(rng, boxes, K=17, outside=0.1):
    n = boxes.shape[0]
    u = rng.uniform(0, 1, (n, K, 2))
    out = rng.uniform(0, 1, (n, K)) < outside
    u = np.where(out[..., None], np.where(u < 0.5, -0.1 * u, 1.0 + 0.1 * u), u)
    xy = boxes[:, None, :2] + u * (boxes[:, None, 2:] - boxes[:, None, :2])
    v = rng.choice([0.0, 1.0, 2.0], size=(n, K), p=[0.2, 0.3, 0.5])
    xy = np.where((v == 0)[..., None], 0.0, xy)
    return np.concatenate([xy, v[..., None]], 2).astype(np.float32)


def structures(rng, out):
    W_, H_ = 100, 80
    boxes = np.array([[5, 5, 40, 60], [50, 10, 99, 79], [0, 0, 10, 10], [90, 70, 120, 95], [30, 30, 30, 50]], np.float32)
    kp = _keypoints(rng, boxes)
    out["st_kp"], out["st_boxes"] = kp, boxes
    k = PersonKeypoints(torch.from_numpy(kp), (W_, H_))
    out["st_resize"] = k.resize((150, 60)).keypoints.numpy()
    out["st_flip"] = k.transpose(FLIP_LEFT_RIGHT).keypoints.numpy()
    out["st_index"] = k[torch.tensor([0, 2, 4])].keypoints.numpy()
    out["st_mask_index"] = k[torch.tensor([True, False, True, True, False])].keypoints.numpy()
    out["st_flip_inds"] = PersonKeypoints.FLIP_INDS.numpy()
    out["st_connections"] = np.array(PersonKeypoints.CONNECTIONS, np.int64)
    out["st_names"] = np.array(PersonKeypoints.NAMES)
    bl = BoxList(torch.from_numpy(boxes.copy()), (W_, H_), mode="xyxy")
    bl.add_field("keypoints", k)
    c = bl.clip_to_image(remove_empty=True)
    out["st_clip_boxes"], out["st_clip_kp"] = c.bbox.numpy(), c.get_field("keypoints").keypoints.numpy()
    r = bl.resize((200, 40))
    out["st_bl_resize_kp"] = r.get_field("keypoints").keypoints.numpy()
    f = bl.transpose(FLIP_LEFT_RIGHT)
    out["st_bl_flip_kp"] = f.get_field("keypoints").keypoints.numpy()


def heat_maps(rng, out):
    M = 56
    n = 64
    x1, y1 = rng.uniform(0, 300, n), rng.uniform(0, 300, n)
    rois = np.stack([x1, y1, x1 + rng.uniform(0.5, 400, n), y1 + rng.uniform(0.5, 400, n)], 1).astype(np.float32)
    kp = _keypoints(rng, rois, outside=0.15)
    # boundary cases on the first 8 rois: on x2 / y2 exactly, on x1 / y1, one ulp outside, v = 0 inside the box
    b = rois[:8]
    kp[:8, 0, :2] = b[:, 2:4]
    kp[:8, 1, 0], kp[:8, 1, 1] = b[:, 0], b[:, 1]
    kp[:8, 2, 0] = np.nextafter(b[:, 2], np.float32(np.inf))
    kp[:8, 3, 1] = np.nextafter(b[:, 1], np.float32(-np.inf))
    kp[:8, 4, 0], kp[:8, 4, 1] = b[:, 2], (b[:, 1] + b[:, 3]) / 2
    kp[:8, 5] = [(b[0, 0] + b[0, 2]) / 2, (b[0, 1] + b[0, 3]) / 2, 0]
    kp[:8, :6, 2] = np.where(np.arange(6) == 5, 0, 2)
    heat, valid = keypoints_to_heat_map(torch.from_numpy(kp), torch.from_numpy(rois), M)
    out["hm_rois"], out["hm_kp"], out["hm_heat"], out["hm_valid"] = rois, kp, heat.numpy(), valid.numpy()


def heat_maps_integer(out):
    """integer-aligned boxes and points: integer widths w and points at x1 + j / 2, where (x - x1) * (M / w) lands on
    or next to an integer and the rounding of M / w decides the floor"""
    M = 56
    rois, kps = [], []
    for w in range(1, 120):
        for x0 in (0, 3, 17):
            rois.append([x0, x0 + 1, x0 + w, x0 + 1 + w])
            j = np.arange(17) * max(1, (2 * w) // 17)
            pts = np.stack([x0 + j / 2, x0 + 1 + (2 * w - j) / 2, np.full(17, 2.0)], 1)
            kps.append(pts)
    rois, kp = np.array(rois, np.float32), np.array(kps, np.float32)
    heat, valid = keypoints_to_heat_map(torch.from_numpy(kp), torch.from_numpy(rois), M)
    out["hi_rois"], out["hi_kp"], out["hi_heat"], out["hi_valid"] = rois, kp, heat.numpy(), valid.numpy()


def loss_case(rng, out):
    cfg = ref_cfg.clone()
    cfg.merge_from_list(["MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 56, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 512])
    ev = make_roi_keypoint_loss_evaluator(cfg)
    proposals, targets = [], []
    for i, (W_, H_, n_gt, n_prop) in enumerate([(320, 240, 4, 90), (280, 300, 6, 110)]):
        w, h = rng.uniform(30, 120, n_gt), rng.uniform(30, 120, n_gt)
        x1, y1 = rng.uniform(0, W_ - 121, n_gt), rng.uniform(0, H_ - 121, n_gt)
        gt = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
        kp = _keypoints(rng, gt)
        kp[0, :, 2] = 0                       # a ground truth without a labelled keypoint: never a keypoint ROI
        kp[1, :, :2] = gt[1, None, 2:] + 5    # ... and one whose labelled keypoints all lie outside its box
        kp[1, :, 2] = 2
        # proposals: jittered ground-truth boxes (most IoU >= 0.5) and random boxes (background)
        j = rng.randint(0, n_gt, n_prop)
        jit = gt[j] + rng.normal(0, 8, (n_prop, 4)).astype(np.float32)
        rnd = rng.uniform(0, min(W_, H_) - 40, (n_prop, 2))
        rnd = np.concatenate([rnd, rnd + rng.uniform(10, 40, (n_prop, 2))], 1).astype(np.float32)
        pb = np.where((rng.uniform(0, 1, n_prop) < 0.5)[:, None], jit, rnd).astype(np.float32)
        pb[:, 2:] = np.maximum(pb[:, 2:], pb[:, :2] + 1)
        p = BoxList(torch.from_numpy(pb), (W_, H_), mode="xyxy")
        t = BoxList(torch.from_numpy(gt), (W_, H_), mode="xyxy")
        t.add_field("labels", torch.ones(n_gt, dtype=torch.int64))
        t.add_field("keypoints", PersonKeypoints(torch.from_numpy(kp), (W_, H_)))
        proposals.append(p)
        targets.append(t)
        out["ls_props_%d" % i], out["ls_gt_%d" % i], out["ls_gtkp_%d" % i] = pb, gt, kp
        out["ls_size_%d" % i] = np.array([W_, H_], np.int64)
    sub = ev.subsample(proposals, targets)
    n = 0
    for i, s in enumerate(sub):
        assert len(s) <= 128, "positives exceed the sampler's quota: the random stream would decide"
        out["ls_sub_boxes_%d" % i] = s.bbox.numpy()
        out["ls_sub_kp_%d" % i] = s.get_field("keypoints").keypoints.numpy()
        n += len(s)
    logits = _logits(n)
    out["ls_loss"] = np.float64(float(ev(sub, logits)))
    out["ls_n"] = np.int64(n)


def decode_case(rng, out):
    K, M = 4, 56
    sides = [(0.3, 0.7), (1.0, 1.0), (1.5, 2.25), (7.2, 56.0), (56.0, 13.9), (119.6, 212.3), (800.0, 31.0), (1333.0, 640.5)]
    n = len(sides)
    x1 = rng.uniform(0, 500, n).astype(np.float32)
    y1 = rng.uniform(0, 500, n).astype(np.float32)
    wh = np.array(sides, np.float32)
    boxes = np.stack([x1, y1, x1 + wh[:, 0], y1 + wh[:, 1]], 1).astype(np.float32)
    maps = (rng.randn(n, K, M, M) * 2).astype(np.float32)
    xy, scores = heatmaps_to_keypoints(maps, boxes)
    margin = np.zeros((n, K))
    widths, heights = np.maximum(boxes[:, 2] - boxes[:, 0], 1), np.maximum(boxes[:, 3] - boxes[:, 1], 1)
    for i in range(n):
        r = _resize_fp64(maps[i].transpose(1, 2, 0), (np.ceil(widths[i]), np.ceil(heights[i])))
        flat = np.sort(r.reshape(-1, K), axis=0)
        margin[i] = flat[-1] - flat[-2] if flat.shape[0] > 1 else np.inf
    out["dc_maps"], out["dc_boxes"], out["dc_xy"], out["dc_scores"], out["dc_margin"] = maps, boxes, xy, scores, margin


def whole_model(out):
    extra = ["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 100, "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", 150,
             "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 32768, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 512]
    common = [v for v in W.COMMON]
    i = common.index("MODEL.ROI_MASK_HEAD.CONV_LAYERS")
    common[i:i + 2] = ["MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", (16, 16)]
    yaml_rel = "e2e_keypoint_rcnn_R_50_FPN_1x.yaml"
    cfg = ref_cfg.clone()
    cfg.merge_from_file(os.path.join(W.REF, "configs", yaml_rel))
    cfg.merge_from_list(common + extra)
    torch.manual_seed(7)
    model = build_detection_model(cfg).train()
    rng = np.random.RandomState(13)
    images, targets, arrays = W.make_batch(rng, False)
    for i, t in enumerate(targets):
        n = len(t)
        t.add_field("labels", torch.ones(n, dtype=torch.int64))
        kp = _keypoints(rng, t.bbox.numpy())
        t.add_field("keypoints", PersonKeypoints(torch.from_numpy(kp), t.size))
        arrays["labels_%d" % i], arrays["keypoints_%d" % i] = np.ones(n, np.int64), kp
    il = to_image_list(images, cfg.DATALOADER.SIZE_DIVISIBILITY)
    with torch.no_grad():
        losses = model(il, targets)
    arrays.update({"loss__" + k: np.float64(float(v)) for k, v in losses.items()})
    sd = model.state_dict()
    arrays.update({"sd__" + k: v.detach().cpu().numpy() for k, v in sd.items()})
    arrays["opts"] = np.array(repr(common + extra))
    arrays["yaml"] = np.array(yaml_rel)
    arrays["size_divisibility"] = np.int64(cfg.DATALOADER.SIZE_DIVISIBILITY)
    path = os.path.join(HERE, "whole_model_keypoint_rcnn.npz")
    np.savez_compressed(path, **arrays)
    print("whole model", {k: float(v) for k, v in losses.items()}, "file MB: %.2f" % (os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    rng = np.random.RandomState(5)
    out = {}
    structures(rng, out)
    heat_maps(rng, out)
    loss_case(rng, out)
    decode_case(rng, out)
    heat_maps_integer(out)
    path = os.path.join(HERE, "model_keypoints.npz")
    np.savez_compressed(path, **out)
    print("model_keypoints: loss %.6f over %d ROIs, file MB: %.2f" % (out["ls_loss"], out["ls_n"], os.path.getsize(path) / 1e6))
    whole_model({})
