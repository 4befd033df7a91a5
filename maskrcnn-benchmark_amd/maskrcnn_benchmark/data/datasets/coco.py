"""COCODataset (reference data/datasets/coco.py) over `json` and Pillow only: no pycocotools.

Training items follow the reference: images in id order; an image is dropped when it has no annotations, when every box
has w or h <= 1 or, for keypoint annotations, when it has fewer than 10 visible keypoints; category ids map to 1..K in
sorted order; crowd annotations are dropped per item; boxes go from xywh to xyxy; the target carries `labels`, `masks`
(polygons) and `keypoints` when present and is clipped to the image before the transforms.

For evaluation `get_groundtruth(index)` keeps the crowds and adds `iscrowd` and `area`, at the image's own size; with
`groundtruth_targets` set (the test loader does) `__getitem__` hands that out as the target, so the streaming evaluator
of engine/inference.py scores the detections at the original image size as the reference's COCO evaluation does."""
import json
import os

import torch
import torch.utils.data

from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.keypoint import PersonKeypoints
from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

min_keypoints_per_image = 10


def _count_visible_keypoints(anno):
    return sum(sum(1 for v in ann["keypoints"][2::3] if v > 0) for ann in anno)


def _has_only_empty_bbox(anno):
    return all(any(o <= 1 for o in obj["bbox"][2:]) for obj in anno)


def has_valid_annotation(anno):
    if len(anno) == 0:
        return False
    if _has_only_empty_bbox(anno):
        return False
    if "keypoints" not in anno[0]:
        return True
    return _count_visible_keypoints(anno) >= min_keypoints_per_image


def rle_to_mask(rle):
    """an uncompressed COCO RLE {"size": [h, w], "counts": [runs of 0s and 1s alternating, column-major]} -> uint8 [h, w]"""
    counts = rle["counts"]
    if not isinstance(counts, (list, tuple)):
        raise NotImplementedError("compressed RLE strings are not built: only uncompressed counts lists are decoded")
    h, w = (int(v) for v in rle["size"])
    runs = torch.tensor(counts, dtype=torch.int64)
    if int(runs.sum()) != h * w or (runs < 0).any():
        raise ValueError("RLE counts sum to %d for a %d x %d mask" % (int(runs.sum()), h, w))
    values = (torch.arange(len(counts)) % 2).to(torch.uint8)
    return torch.repeat_interleave(values, runs).reshape(w, h).t().contiguous()


def decode_rle(rle):
    """a COCO RLE {"size": [h, w], "counts": ...} -> uint8 [h, w].  `counts` is an uncompressed list (rle_to_mask) or the
    COMPRESSED string every converter built on pycocotools' encode writes: that goes through _C.rle_string_decode_list
    (include/detops.h, "Reading compressed RLE strings"); a malformed string, or runs that do not sum to h * w, raise
    ValueError."""
    counts = rle["counts"]
    if isinstance(counts, (list, tuple)):
        return rle_to_mask(rle)
    from maskrcnn_benchmark import _C

    h, w = (int(v) for v in rle["size"])
    if isinstance(counts, bytes):
        counts = counts.decode("latin-1")
    runs, _ = _C.rle_string_decode_list([counts], [(h, w)])
    values = (torch.arange(runs.numel()) % 2).to(torch.uint8)
    return torch.repeat_interleave(values, runs.to(torch.int64)).reshape(w, h).t().contiguous()


class COCODataset(torch.utils.data.Dataset):
    evaluation_style = "coco"

    def __init__(self, ann_file, root, remove_images_without_annotations, transforms=None):
        with open(ann_file) as f:
            data = json.load(f)
        self.root = root
        self.images = {im["id"]: im for im in data["images"]}
        self.annotations = {i: [] for i in self.images}
        for ann in data.get("annotations", []):
            self.annotations[ann["image_id"]].append(ann)
        self.ids = sorted(self.images)
        if remove_images_without_annotations:
            self.ids = [i for i in self.ids if has_valid_annotation(self.annotations[i])]
        self.categories = {c["id"]: c for c in data.get("categories", [])}
        self.json_category_id_to_contiguous_id = {v: i + 1 for i, v in enumerate(sorted(self.categories))}
        self.contiguous_category_id_to_json_id = {v: k for k, v in self.json_category_id_to_contiguous_id.items()}
        self.num_classes = len(self.categories) + 1           # with the background
        self.id_to_img_map = {k: v for k, v in enumerate(self.ids)}
        self._transforms = transforms
        self.groundtruth_targets = False

    def __len__(self):
        return len(self.ids)

    def get_img_info(self, index):
        return self.images[self.id_to_img_map[index]]

    def _load_image(self, index):
        from PIL import Image

        return Image.open(os.path.join(self.root, self.get_img_info(index)["file_name"])).convert("RGB")

    def _target(self, anno, size):
        """the annotations of one image as a BoxList of `size` (w, h)"""
        boxes = torch.as_tensor([obj["bbox"] for obj in anno], dtype=torch.float32).reshape(-1, 4)
        target = BoxList(boxes, size, mode="xywh").convert("xyxy")
        classes = [self.json_category_id_to_contiguous_id[obj["category_id"]] for obj in anno]
        target.add_field("labels", torch.tensor(classes, dtype=torch.int64))
        return target

    def __getitem__(self, index):
        img = self._load_image(index)
        anno = [obj for obj in self.annotations[self.id_to_img_map[index]] if obj.get("iscrowd", 0) == 0]
        target = self._target(anno, img.size)
        if anno and "segmentation" in anno[0]:
            target.add_field("masks", SegmentationMask([obj["segmentation"] for obj in anno], img.size, mode="poly"))
        if anno and "keypoints" in anno[0]:
            target.add_field("keypoints", PersonKeypoints([obj["keypoints"] for obj in anno], img.size))
        target = target.clip_to_image(remove_empty=True)
        if self._transforms is not None:
            img, target = self._transforms(img, target)
        if self.groundtruth_targets:
            target = self.get_groundtruth(index)
        return img, target, index

    def get_groundtruth(self, index):
        info = self.get_img_info(index)
        size = (int(info["width"]), int(info["height"]))
        anno = self.annotations[self.id_to_img_map[index]]
        target = self._target(anno, size)
        target.add_field("iscrowd", torch.tensor([int(obj.get("iscrowd", 0)) for obj in anno], dtype=torch.int64))
        target.add_field("area", torch.tensor([float(obj.get("area", obj["bbox"][2] * obj["bbox"][3])) for obj in anno],
                                              dtype=torch.float64))
        segs = [obj.get("segmentation") for obj in anno]
        if anno and all(s is not None for s in segs):
            if any(isinstance(s, dict) for s in segs):         # a crowd's RLE: the image's masks as planes
                planes = [decode_rle(s) if isinstance(s, dict)
                          else SegmentationMask([s], size, mode="poly").get_mask_tensor().reshape(size[1], size[0]).to(torch.uint8)
                          for s in segs]
                for s, p in zip(segs, planes):
                    if tuple(p.shape) != (size[1], size[0]):
                        raise ValueError("an RLE of size %s in an image of %s" % (s["size"], size))
                target.add_field("masks", SegmentationMask(torch.stack(planes), size, mode="mask"))
            else:
                target.add_field("masks", SegmentationMask(segs, size, mode="poly"))
        if anno and "keypoints" in anno[0]:
            target.add_field("keypoints", PersonKeypoints([obj["keypoints"] for obj in anno], size))
        return target
