"""Shared by tests/test_bbox_aug_cpu.py and tests/test_bbox_aug_gpu.py: the merge cases, the reference's fixture
(tests/golden/bbox_aug_reference.npz, made by tests/golden/make_golden_bbox_aug.py), a 2-image COCO-json set the tests write
themselves and the narrow random-init Faster R-CNN the model-level checks run."""
import json
import os

import numpy as np
import torch

from maskrcnn_benchmark._bbox_aug_torch import bbox_aug_merge as torch_merge
from maskrcnn_benchmark._bbox_aug_torch import group_records

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THRESH = 0.05


def make_case(seed, C, rows, frames, flips, pass_rate=0.5, agnostic=False):
    """rows[i][t]: rows of image i's pass t; frames[i][t] = (w, h); flips[t].  Boxes reach past the frame on every side (the
    clamp works), scores are `pass_rate` above THRESH.  -> dict of CPU tensors and N, T"""
    rng = np.random.RandomState(seed)
    N, T = len(rows), len(flips)
    counts = [n for per_image in rows for n in per_image]
    R = sum(counts)
    group = np.repeat(np.arange(N * T), counts)
    wh = np.array([frames[g // T][g % T] for g in range(N * T)], np.float64).reshape(N * T, 2)[group]       # [R, 2]
    lo = rng.uniform(-0.2, 0.9, (R, 1 if agnostic else C, 2))
    b = np.concatenate([lo, lo + rng.uniform(0.02, 0.5, lo.shape)], -1) * np.concatenate([wh, wh], 1)[:, None, :]
    if agnostic:                                                  # CLS_AGNOSTIC_BBOX_REG: the one box, repeated per class
        b = np.repeat(b, C, 1)
    s = np.where(rng.rand(R, C) < pass_rate, rng.uniform(THRESH + 0.01, 1.0, (R, C)), rng.uniform(0.0, THRESH - 0.01, (R, C)))
    geom, ratio = group_records(frames, flips)
    return dict(boxes=torch.from_numpy(b.reshape(R, 4 * C).astype(np.float32)), scores=torch.from_numpy(s.astype(np.float32)),
                row_offset=torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32), geom=geom, ratio=ratio,
                N=N, T=T)


def _frames(N, T, odd=True):
    """first pass (and its flip) at an odd width; later passes at a scale whose w and h ratios differ"""
    out = []
    for i in range(N):
        w0, h0 = 101 + 2 * i, 76 + i
        out.append([(w0, h0) if t < 2 else (151 + 3 * i + 7 * t, 113 + i + 4 * t) for t in range(T)])
    return out


# name -> arguments of make_case.  Every size at which the kernel takes another route: C = 2 (32 rows per wave step),
# C = 3 / 21 (16 / 2 rows per step), C = 81 (three column tiles of 32 lanes), C = 64 / 120 (one / two tiles of 64); groups of 65, 257 and 513 rows cross a wave's 32
# rows, a workgroup's 128 and several workgroups
MERGE_CASES = {
    "c2_n1_t1": dict(seed=1, C=2, rows=[[37]], frames=[[(101, 76)]], flips=[0]),
    "c2_n3_t4": dict(seed=2, C=2, rows=[[65, 0, 257, 33], [0, 0, 0, 0], [513, 1, 2, 129]], frames=_frames(3, 4), flips=[0, 1, 0, 1]),
    "c81_n1_t1_flip": dict(seed=3, C=81, rows=[[70]], frames=[[(101, 76)]], flips=[1]),
    "c81_n3_t4": dict(seed=4, C=81, rows=[[65, 40, 0, 31], [0, 0, 0, 0], [130, 7, 64, 1]], frames=_frames(3, 4), flips=[0, 1, 0, 1],
                      pass_rate=0.05),
    "c81_boundaries": dict(seed=5, C=81, rows=[[65, 257, 513]], frames=_frames(1, 3), flips=[0, 1, 1]),
    "c3_boundaries": dict(seed=6, C=3, rows=[[65, 257, 513], [513, 65, 257]], frames=_frames(2, 3), flips=[0, 1, 0]),
    "c21_n3_t4": dict(seed=7, C=21, rows=[[65, 0, 40, 3], [1, 1, 1, 1], [0, 0, 200, 0]], frames=_frames(3, 4), flips=[0, 1, 0, 1]),
    "c64_one_tile_of_64": dict(seed=11, C=64, rows=[[65, 3], [0, 130]], frames=_frames(2, 2), flips=[0, 1], pass_rate=0.2),
    "c120_two_tiles_of_64": dict(seed=12, C=120, rows=[[65, 130]], frames=_frames(1, 2), flips=[0, 1], pass_rate=0.1),
    "nothing_passes": dict(seed=8, C=5, rows=[[40, 3], [0, 130]], frames=_frames(2, 2), flips=[0, 1], pass_rate=0.0),
    "no_rows": dict(seed=9, C=5, rows=[[0, 0], [0, 0]], frames=_frames(2, 2), flips=[0, 1]),
    "class_agnostic": dict(seed=10, C=6, rows=[[65, 130], [33, 0]], frames=_frames(2, 2), flips=[0, 1], agnostic=True),
    # the offsets scan's tile of 1024 segments, S = N * (C - 1) = 1023, 1024, 1025 and 1040; few rows per image and a low pass
    # rate leave many segments empty
    "s1023_c94_n11": dict(seed=13, C=94, rows=[[1 + i % 4] for i in range(11)], frames=_frames(11, 1), flips=[0], pass_rate=0.3),
    "s1024_c65_n16": dict(seed=14, C=65, rows=[[1 + i % 3] for i in range(16)], frames=_frames(16, 1), flips=[1], pass_rate=0.3),
    "s1025_c42_n25": dict(seed=15, C=42, rows=[[i % 3] for i in range(25)], frames=_frames(25, 1), flips=[0], pass_rate=0.3),
    "s1040_c81_n13": dict(seed=16, C=81, rows=[[2, i % 2] for i in range(13)], frames=_frames(13, 2), flips=[0, 1], pass_rate=0.2),
    # a segment of 68 count slots (17 tiles of 128 rows, 4 waves each): the prefix scan's tile of 64 slots and its carry
    "c3_68_slots": dict(seed=17, C=3, rows=[[2100, 5]], frames=_frames(1, 2), flips=[0, 1], pass_rate=0.3),
}


def reference(case, thresh=THRESH):
    """the torch formulation on the CPU"""
    return torch_merge(case["boxes"], case["scores"], case["row_offset"], case["geom"], case["ratio"], case["N"], case["T"], thresh)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def load_fixture():
    g = np.load(os.path.join(GOLDEN, "bbox_aug_reference.npz"), allow_pickle=False)
    frames = [[tuple(int(v) for v in f) for f in per_image] for per_image in g["frames"]]
    flips = [int(f) for f in g["flips"]]
    geom, ratio = group_records(frames, flips)
    return dict(boxes=torch.from_numpy(g["boxes"]), scores=torch.from_numpy(g["scores"]),
                row_offset=torch.from_numpy(g["row_offset"]), geom=geom, ratio=ratio, N=len(frames), T=len(flips),
                sizes=[f[0] for f in frames], score_thresh=float(g["score_thresh"]), nms=float(g["nms"]),
                detections_per_img=int(g["detections_per_img"]), merged=torch.from_numpy(g["merged"]),
                det_counts=g["det_counts"].tolist(), det_boxes=torch.from_numpy(g["det_boxes"]),
                det_scores=torch.from_numpy(g["det_scores"]), det_labels=torch.from_numpy(g["det_labels"]))


def check_fixture_detections(fx, device):
    """merge + NMS + top-k of the product over the fixture's rows = the reference's filter_results output: boxes bit for bit,
    scores and labels exactly, in the reference's order"""
    from maskrcnn_benchmark.engine.bbox_aug import merge_detections

    out = merge_detections(fx["boxes"].to(device), fx["scores"].to(device), fx["row_offset"], fx["geom"], fx["ratio"], fx["sizes"],
                           fx["T"], fx["score_thresh"], fx["nms"], fx["detections_per_img"])
    assert [len(o) for o in out] == fx["det_counts"]
    assert max(fx["det_counts"]) == fx["detections_per_img"] and min(fx["det_counts"]) == 0
    at = 0
    for o, n, size in zip(out, fx["det_counts"], fx["sizes"]):
        assert o.size == size and o.mode == "xyxy"
        assert torch.equal(bits(o.bbox), bits(fx["det_boxes"][at:at + n]))
        assert torch.equal(o.get_field("scores").cpu(), fx["det_scores"][at:at + n])
        assert torch.equal(o.get_field("labels").cpu(), fx["det_labels"][at:at + n])
        at += n


# ---------------------------------------------------------------------------------------- the model-level checks
SIZES = {1: (64, 48), 2: (40, 56)}     # id -> (w, h)


def write_coco(root):
    """two PNGs and their COCO json under `root` -> (ann_file, root)"""
    from PIL import Image

    rng = np.random.RandomState(5)
    images, ann = [], []
    for i, (w, h) in SIZES.items():
        name = "img%d.png" % i
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), "RGB").save(os.path.join(root, name))
        images.append({"id": i, "file_name": name, "width": w, "height": h})
        ann.append({"id": i, "image_id": i, "category_id": 3, "bbox": [4.0, 5.0, 20.0, 18.0], "area": 360.0, "iscrowd": 0,
                    "segmentation": [[4, 5, 24, 5, 24, 23, 4, 23]]})
    path = os.path.join(root, "instances.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": ann, "categories": [{"id": 3, "name": "a"}, {"id": 7, "name": "b"},
                                                                        {"id": 9, "name": "c"}]}, f)
    return path, root


def narrow_cfg(name, device, opts=()):
    from maskrcnn_benchmark.engine.bench_step import load_cfg

    base = ["MODEL.DEVICE", device, "MODEL.RESNETS.RES2_OUT_CHANNELS", 16, "MODEL.RESNETS.WIDTH_PER_GROUP", 4,
            "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 32, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 4,
            "MODEL.RPN.PRE_NMS_TOP_N_TEST", 100, "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", 50, "TEST.DETECTIONS_PER_IMG", 20,
            "INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 128, "TEST.IMS_PER_BATCH", 2, "DATALOADER.NUM_WORKERS", 0,
            "DATALOADER.SIZE_DIVISIBILITY", 32, "DATALOADER.ASPECT_RATIO_GROUPING", False, "DATASETS.TEST", (name,)]
    return load_cfg("e2e_faster_rcnn_R_50_FPN_1x.yaml", base + list(opts))


def build_model(cfg, device, layout="nchw", state=None):
    from maskrcnn_benchmark.modeling.detector import build_detection_model

    torch.manual_seed(0)
    model = build_detection_model(cfg)
    if state is not None:
        model.load_state_dict(state, strict=True)
    model.to(device).eval()
    if layout != "nchw":
        model.set_channels_last(True, heads=layout == "all")
    return model


def canonical(boxlist):
    """the detections of one image as rows (label, score, x1, y1, x2, y2) in lexicographic order: a comparison in value"""
    rows = torch.cat([boxlist.get_field("labels").double()[:, None], boxlist.get_field("scores").double()[:, None],
                      boxlist.bbox.double()], 1).cpu().numpy()
    return rows[np.lexsort(rows.T[::-1])]


def plain_and_augmented(name, device, layout, aug_opts):
    """-> (plain detections, augmented detections) of the one batch of the 2-image set: the same weights, the plain model
    through model(images.to(device)), the BBOX_AUG model through im_detect_bbox_aug"""
    from maskrcnn_benchmark.data import make_data_loader
    from maskrcnn_benchmark.data.collate_batch import RawImageBatch
    from maskrcnn_benchmark.engine.bbox_aug import im_detect_bbox_aug

    plain_cfg = narrow_cfg(name, device)
    aug_cfg = narrow_cfg(name, device, ["TEST.BBOX_AUG.ENABLED", True] + list(aug_opts))
    plain = build_model(plain_cfg, device, layout)
    aug = build_model(aug_cfg, device, layout, state=plain.state_dict())
    (images, _, ids), = list(make_data_loader(aug_cfg, is_train=False))
    assert isinstance(images, RawImageBatch) and ids == (0, 1)
    with torch.no_grad():
        a = plain(images.to(device))
        b = im_detect_bbox_aug(aug, images, device, aug_cfg)
    assert len(a) == len(b) == 2 and all(len(x) > 0 for x in a)
    return a, b
