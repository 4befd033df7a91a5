"""Keypoint R-CNN on the CPU (`-m "not gpu"`): the keypoint yaml builds, and the torch formulations of the keypoint head
(structures, heatmap targets, ROI selection, loss, decoding, the whole model) reproduce the reference's own code
(tests/golden/make_golden_keypoint.py wrote the fixtures)."""
import ast
import hashlib
import os

import numpy as np
import pytest
import torch

import cpu_shim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "model_keypoints.npz"), allow_pickle=False)
T = torch.from_numpy

# sha256 of one synthetic batch of the mask config (two 128 x 160 samples of seed 3: pixels, boxes, labels, masks), taken
# on the tree before the keypoint head existed: adding keypoints to the generator must not move any existing draw
MASK_BATCH_SHA256 = "2f80e2b7a2b102be9a898e3834cb14eaa3dfba4842db688368b2cd3391c151b5"


def _logits(n, K=17, M=56):
    i = torch.arange(n * K * M * M, dtype=torch.float64)
    return (4.0 * torch.sin(i * 0.37) + torch.cos(i * 0.011)).float().view(n, K, M, M)


def _narrow_cfg(extra=()):
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    return load_cfg("e2e_keypoint_rcnn_R_50_FPN_1x.yaml",
                    ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", 16, "MODEL.RESNETS.WIDTH_PER_GROUP", 4,
                     "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 32,
                     "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", (16, 16)] + list(extra))


def test_keypoint_yaml_builds_the_keypoint_head():
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    cfg = load_cfg("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", ["MODEL.DEVICE", "cpu"])
    assert cfg.MODEL.KEYPOINT_ON and cfg.MODEL.ROI_KEYPOINT_HEAD.RESOLUTION == 56
    model = build_detection_model(cfg)
    kp = model.roi_heads["keypoint"]
    assert [n for n, _ in kp.feature_extractor.named_children() if n.startswith("conv_fcn")] == \
        ["conv_fcn%d" % i for i in range(1, 9)]
    assert tuple(kp.predictor.kps_score_lowres.weight.shape) == (512, 17, 4, 4)


def test_share_box_feature_extractor_is_refused():
    with pytest.raises(ValueError, match="SHARE_BOX_FEATURE_EXTRACTOR"):
        from maskrcnn_benchmark.modeling.detector import build_detection_model
        build_detection_model(_narrow_cfg(["MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", True]))


def test_defaults_have_the_reference_keypoint_keys():
    from maskrcnn_benchmark.config import cfg
    H = cfg.MODEL.ROI_KEYPOINT_HEAD
    assert H.FEATURE_EXTRACTOR == "KeypointRCNNFeatureExtractor" and H.PREDICTOR == "KeypointRCNNPredictor"
    assert (H.POOLER_RESOLUTION, H.POOLER_SAMPLING_RATIO, H.POOLER_SCALES) == (14, 0, (1.0 / 16,))
    assert (H.MLP_HEAD_DIM, H.CONV_LAYERS, H.RESOLUTION, H.NUM_CLASSES) == (1024, (512,) * 8, 14, 17)
    assert H.SHARE_BOX_FEATURE_EXTRACTOR is True


def test_person_keypoints_match_the_reference():
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.keypoint import FLIP_LEFT_RIGHT, PersonKeypoints
    assert PersonKeypoints.NAMES == [str(s) for s in G["st_names"]]
    assert np.array_equal(PersonKeypoints.FLIP_INDS.numpy(), G["st_flip_inds"])
    assert np.array_equal(np.array(PersonKeypoints.CONNECTIONS), G["st_connections"])
    k = PersonKeypoints(T(G["st_kp"]), (100, 80))
    assert np.array_equal(k.resize((150, 60)).keypoints.numpy(), G["st_resize"])
    assert np.array_equal(k.transpose(FLIP_LEFT_RIGHT).keypoints.numpy(), G["st_flip"])
    assert np.array_equal(k[torch.tensor([0, 2, 4])].keypoints.numpy(), G["st_index"])
    assert np.array_equal(k[torch.tensor([True, False, True, True, False])].keypoints.numpy(), G["st_mask_index"])
    with pytest.raises(NotImplementedError):
        k.crop((0, 0, 10, 10))
    bl = BoxList(T(G["st_boxes"].copy()), (100, 80), mode="xyxy")
    bl.add_field("keypoints", k)
    c = bl.clip_to_image(remove_empty=True)
    assert np.array_equal(c.bbox.numpy(), G["st_clip_boxes"])
    assert np.array_equal(c.get_field("keypoints").keypoints.numpy(), G["st_clip_kp"])
    assert np.array_equal(bl.resize((200, 40)).get_field("keypoints").keypoints.numpy(), G["st_bl_resize_kp"])
    assert np.array_equal(bl.transpose(FLIP_LEFT_RIGHT).get_field("keypoints").keypoints.numpy(), G["st_bl_flip_kp"])
    k.add_field("logits", torch.arange(5.0))
    assert k.to("cpu")[torch.tensor([1, 3])].get_field("logits").tolist() == [1.0, 3.0]


def test_heat_map_projection_is_bit_equal_to_the_reference():
    from maskrcnn_benchmark.structures.keypoint import keypoints_to_heat_map
    heat, valid = keypoints_to_heat_map(T(G["hm_kp"]), T(G["hm_rois"]), 56)
    assert np.array_equal(heat.numpy(), G["hm_heat"]) and np.array_equal(valid.numpy(), G["hm_valid"])
    assert G["hm_valid"][:8].sum() > 0 and (G["hm_valid"] == 0).sum() > 0


def test_heat_map_projection_on_integer_aligned_boxes_is_bit_equal_to_the_reference():
    """integer widths and half-integer points, where torch's `M / w` (reciprocal, then multiply) and one correctly rounded
    division land on different sides of an integer"""
    from maskrcnn_benchmark.structures.keypoint import keypoints_to_heat_map
    heat, valid = keypoints_to_heat_map(T(G["hi_kp"]), T(G["hi_rois"]), 56)
    assert np.array_equal(heat.numpy(), G["hi_heat"]) and np.array_equal(valid.numpy(), G["hi_valid"])
    heat, _ = keypoints_to_heat_map(torch.tensor([[[7.0, 7.0, 2.0]]]), torch.tensor([[0.0, 0.0, 49.0, 49.0]]), 56)
    assert heat.item() == 7 * 56 + 7


def _loss_case():
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.keypoint import PersonKeypoints
    props, targets = [], []
    for i in range(2):
        W, H = G["ls_size_%d" % i].tolist()
        t = BoxList(T(G["ls_gt_%d" % i]), (W, H))
        t.add_field("labels", torch.ones(len(t), dtype=torch.int64))
        t.add_field("keypoints", PersonKeypoints(T(G["ls_gtkp_%d" % i]), (W, H)))
        props.append(BoxList(T(G["ls_props_%d" % i]), (W, H)))
        targets.append(t)
    return props, targets


def test_keypoint_rois_are_the_reference_subsample_positives():
    """box-head matching (FG = BG = 0.5), positives, then the keypoint head's slot mask == the reference's `subsample`"""
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.loss import KeypointRCNNLossComputation, keypoint_slots
    from maskrcnn_benchmark.structures.boxlist_ops import boxlist_iou
    props, targets = _loss_case()
    matcher = Matcher(0.5, 0.5, allow_low_quality_matches=False)
    slots = []
    for p, t in zip(props, targets):
        m = matcher(boxlist_iou(t, p))
        p.add_field("matched_idxs", m)
        p.add_field("labels", (m >= 0).long())
        slots.append(p)
    _, matched, labels, gt_boxes, gt_kps = KeypointRCNNLossComputation(56).batch(slots, targets, 17)
    kept = keypoint_slots(matched, labels, gt_boxes, gt_kps)
    base = 0
    for i, p in enumerate(slots):
        mine = {tuple(b) for b in p.bbox[kept[base:base + len(p)]].tolist()}
        ref = {tuple(b) for b in G["ls_sub_boxes_%d" % i].tolist()}
        assert mine == ref and len(ref) > 0, i
        base += len(p)


def test_cpu_loss_matches_the_reference():
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.loss import keypoint_loss_torch, keypoint_targets_torch
    boxes = torch.cat([T(G["ls_sub_boxes_%d" % i]) for i in range(2)])
    kps = torch.cat([T(G["ls_sub_kp_%d" % i]) for i in range(2)])
    n = boxes.shape[0]
    # every reference ROI is its own ground truth row (the matched keypoints it carries); the box is a qualifying one
    heat, valid = keypoint_targets_torch(boxes, torch.arange(n), torch.ones(n, dtype=torch.int64),
                                         torch.tensor([[-1e9, -1e9, 1e9, 1e9]]).expand(n, 4), kps, 56)
    loss = keypoint_loss_torch(_logits(n), heat, valid)
    ref = float(G["ls_loss"])
    assert abs(float(loss) - ref) <= 1e-6 * abs(ref), (float(loss), ref)
    empty = keypoint_loss_torch(_logits(2), torch.zeros(2, 17, dtype=torch.int64), torch.zeros(2, 17, dtype=torch.bool))
    assert float(empty) == 0.0


def test_cpu_decoder_matches_the_reference():
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.inference import heatmaps_to_keypoints_torch
    kps, scores = heatmaps_to_keypoints_torch(T(G["dc_maps"]), T(G["dc_boxes"]))
    ref_xy, ref_s, margin = G["dc_xy"], G["dc_scores"], G["dc_margin"]
    sharp = margin > 1e-4 * np.abs(ref_s)
    assert sharp.mean() > 0.9
    assert np.array_equal(kps.numpy()[sharp], ref_xy[sharp])
    np.testing.assert_allclose(scores.numpy(), ref_s, rtol=1e-5, atol=1e-6)


def _whole_model_case():
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.image_list import to_image_list
    from maskrcnn_benchmark.structures.keypoint import PersonKeypoints
    g = np.load(os.path.join(GOLDEN, "whole_model_keypoint_rcnn.npz"), allow_pickle=False)
    cfg = load_cfg(str(g["yaml"]), list(ast.literal_eval(str(g["opts"]))))
    model = build_detection_model(cfg)
    ref_sd = {k[len("sd__"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd__")}
    images, targets = [], []
    for i in range(2):
        im = torch.from_numpy(g["image_%d" % i])
        H, W = im.shape[-2:]
        t = BoxList(torch.from_numpy(g["boxes_%d" % i]), (W, H), mode="xyxy")
        t.add_field("labels", torch.from_numpy(g["labels_%d" % i]))
        t.add_field("keypoints", PersonKeypoints(torch.from_numpy(g["keypoints_%d" % i]), (W, H)))
        images.append(im)
        targets.append(t)
    il = to_image_list(images, int(g["size_divisibility"]))
    ref_losses = {k[len("loss__"):]: float(g[k]) for k in g.files if k.startswith("loss__")}
    return model, ref_sd, il, targets, ref_losses


def test_whole_keypoint_model_matches_the_reference_on_the_cpu():
    model, ref_sd, il, targets, ref_losses = _whole_model_case()
    mine = model.state_dict()
    assert list(mine) == list(ref_sd)
    for k, v in ref_sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
    model.load_state_dict(ref_sd, strict=True)
    model.train()
    with cpu_shim.install("oracle"), torch.no_grad():
        losses = model(il, targets)
    got = {k: float(v) for k, v in losses.items()}
    assert set(got) == set(ref_losses) and "loss_kp" in got
    for k, ref in ref_losses.items():
        assert abs(got[k] - ref) <= 1e-4 * max(1.0, abs(ref)), (k, got, ref_losses)


def test_eval_forward_gives_keypoints_for_every_image():
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.engine.bench_step import make_device_batches
    cfg = _narrow_cfg()
    torch.manual_seed(0)
    model = build_detection_model(cfg).eval()
    (images, _), = make_device_batches(cfg, "cpu", images_per_gpu=2, num_batches=1, height=96, width=128)
    with cpu_shim.install("oracle"), torch.no_grad():
        dets = model(images)
    assert len(dets) == 2
    for d in dets:
        kp = d.get_field("keypoints")
        assert tuple(kp.keypoints.shape) == (len(d), 17, 3) and tuple(kp.get_field("logits").shape) == (len(d), 17)


def _batch_digest(ds):
    from maskrcnn_benchmark.data.synthetic import BatchCollator
    images, targets, _ = BatchCollator(32)([ds[0], ds[1]])
    h = hashlib.sha256()
    h.update(images.tensors.numpy().tobytes())
    for t in targets:
        h.update(t.bbox.numpy().tobytes())
        h.update(t.get_field("labels").numpy().tobytes())
        h.update(t.get_field("masks").instances.masks.numpy().tobytes())
    return h.hexdigest()


def test_synthetic_mask_samples_are_unchanged():
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset
    ds = SyntheticCOCODataset(length=2, height=128, width=160, num_classes=81, with_masks=True, seed=3)
    assert _batch_digest(ds) == MASK_BATCH_SHA256


def test_synthetic_keypoints_exercise_every_case():
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.loss import within_box
    ds = SyntheticCOCODataset(length=4, height=320, width=480, num_classes=2, with_masks=False, seed=0, with_keypoints=True)
    plain = SyntheticCOCODataset(length=4, height=320, width=480, num_classes=2, with_masks=False, seed=0)
    kps, inside, v = [], [], []
    for i in range(4):
        img, t, _ = ds[i]
        img0, t0, _ = plain[i]
        assert torch.equal(img, img0) and torch.equal(t.bbox, t0.bbox)
        k = t.get_field("keypoints").keypoints
        assert tuple(k.shape) == (len(t), 17, 3)
        kps.append(k)
        inside.append(within_box(k[..., :2], t.bbox))
        v.append(k[..., 2])
    k, inside, v = torch.cat(kps), torch.cat(inside), torch.cat(v)
    assert set(v.unique().tolist()) == {0.0, 1.0, 2.0}
    assert (k[v == 0][:, :2] == 0).all()
    assert ((v > 0) & ~inside).any() and ((v > 0) & inside).float().mean() > 0.6
