"""Generate tests/golden/coco_results_reference.json by running the REFERENCE's own `prepare_for_coco_detection` and
`prepare_for_coco_keypoint` (data/datasets/evaluation/coco/coco_eval.py:70-101, 158-186) on seeded predictions (build
container only; never runs on the GPU box).

The reference is made importable as in make_golden_bbox_aug.py (make_golden_whole_model's `install_reference`) and
coco_eval.py is loaded as a file, as make_golden_evaluation.py loads voc_eval.py; `tqdm`, which coco_eval.py imports and
the two functions never call, is stubbed when it is missing.  The reference's segmentation function needs pycocotools
and is not run.  The file holds data only:
  images: per dataset index the json image id and the original width / height;
  categories: contiguous label -> json category id (non-contiguous ids);
  predictions: per image the prediction's (w, h), boxes [n, 4] xyxy, scores, labels and keypoints [n, 17, 3], as the
    float32 values' exact decimal expansions (Python floats of `tolist()`);
  bbox, keypoints: the reference's two result lists, entry by entry, in order.

3 images; image 1 has no detections; every prediction's size differs from the original size with unequal w / h ratios.

Run:  python tests/golden/make_golden_coco_results.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
try:
    import tqdm  # noqa: F401
except ImportError:
    stub = types.ModuleType("tqdm")
    stub.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = stub
import make_golden_whole_model as W  # noqa: E402,F401  (installs the reference as `maskrcnn_benchmark`)

from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402
from maskrcnn_benchmark.structures.keypoint import PersonKeypoints  # noqa: E402

# the file alone, as make_golden_evaluation.py loads voc_eval.py: the reference's `data` package imports torchvision
spec = importlib.util.spec_from_file_location(
    "ref_coco_eval", os.path.join(W.REF, "maskrcnn_benchmark", "data", "datasets", "evaluation", "coco", "coco_eval.py"))
coco_eval = importlib.util.module_from_spec(spec)
spec.loader.exec_module(coco_eval)
prepare_for_coco_detection, prepare_for_coco_keypoint = coco_eval.prepare_for_coco_detection, coco_eval.prepare_for_coco_keypoint

IMAGES = [{"id": 139, "width": 640, "height": 426}, {"id": 285, "width": 586, "height": 640},
          {"id": 632, "width": 333, "height": 500}]
PRED_SIZES = [(1201, 800), (733, 800), (533, 801)]            # (w, h): ratios differ in w and h for every image
COUNTS = [7, 0, 4]
CATEGORIES = {1: 1, 2: 3, 3: 18, 4: 44, 5: 90}                # contiguous label -> json id


class _Coco(object):
    def __init__(self):
        self.imgs = {im["id"]: im for im in IMAGES}


class _Dataset(object):
    """what the two functions read of a COCODataset"""

    def __init__(self):
        self.id_to_img_map = {i: im["id"] for i, im in enumerate(IMAGES)}
        self.contiguous_category_id_to_json_id = dict(CATEGORIES)
        self.coco = _Coco()

    def get_img_info(self, index):
        return IMAGES[index]


def main():
    rng = np.random.RandomState(20241020)
    predictions, stored = [], []
    for (w, h), n in zip(PRED_SIZES, COUNTS):
        lo = rng.uniform(0, 0.6, (n, 2)) * [w, h]
        boxes = np.concatenate([lo, lo + rng.uniform(0.05, 0.4, (n, 2)) * [w, h]], 1).astype(np.float32)
        scores = rng.uniform(0.05, 1.0, n).astype(np.float32)
        labels = rng.randint(1, 6, n).astype(np.int64)
        kps = np.concatenate([rng.uniform(0, 1, (n, 17, 2)) * [w, h], rng.randint(0, 3, (n, 17, 1))], 2).astype(np.float32)
        p = BoxList(torch.from_numpy(boxes).reshape(-1, 4), (w, h), mode="xyxy")
        p.add_field("scores", torch.from_numpy(scores))
        p.add_field("labels", torch.from_numpy(labels))
        p.add_field("keypoints", PersonKeypoints(torch.from_numpy(kps).reshape(-1, 17, 3), (w, h)))
        predictions.append(p)
        stored.append({"size": [w, h], "boxes": boxes.reshape(-1, 4).tolist(), "scores": scores.tolist(),
                       "labels": labels.tolist(), "keypoints": kps.reshape(-1, 17, 3).tolist()})
    dataset = _Dataset()
    bbox = prepare_for_coco_detection(predictions, dataset)
    keypoints = prepare_for_coco_keypoint(predictions, dataset)
    assert len(bbox) == len(keypoints) == sum(COUNTS) and min(COUNTS) == 0
    for (w, h), im in zip(PRED_SIZES, IMAGES):
        assert im["width"] / w != im["height"] / h
    path = os.path.join(HERE, "coco_results_reference.json")
    with open(path, "w") as f:
        json.dump({"images": IMAGES, "categories": {str(k): v for k, v in CATEGORIES.items()}, "predictions": stored,
                   "bbox": bbox, "keypoints": keypoints}, f)
    back = json.load(open(path))
    assert back["bbox"] == bbox and back["keypoints"] == keypoints       # json round-trips every float exactly
    print("wrote", path, "entries", len(bbox), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
