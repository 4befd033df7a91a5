"""CityScapesDataset (reference data/datasets/cityscapes.py) over `json`, numpy and Pillow only: no cityscapesscripts.

Files, as the reference finds them: img_dir/split/*/*_leftImg8bit.png and ann_dir/split/*/*_instanceIds.png ("mask" mode)
or *_polygons.json ("poly" mode), both sorted; `mini` keeps every (len // mini + 1)-th of them.

"mask" mode (the reference's _processBinayMasks): the instances are the ids >= 1000 of the 16-bit id map, ascending; the
label is id // 1000 through the table of the ten Cityscapes labels that have instances (ids 24 .. 33); the box is the tight
(min x, min y, max x, max y) with INCLUSIVE maxima.  One vectorised numpy pass finds all boxes; it runs in the loader's
workers, so it is host code by design.  "poly" mode (_processPolygons): the objects whose label is in CLASSES, one polygon
each, the box from int(min), int(max).  `min_area` drops instances whose (xmax - xmin) * (ymax - ymin) is below it.

When training (`remove_images_without_annotations`, as data/build.py sets it) an image left without instances is replaced
by the next one, as in the reference; nothing is scanned when the dataset is built.  For evaluation `get_groundtruth(index)`
is the target at the image's own size; with `groundtruth_targets` set (the test loader does) `__getitem__` hands that out, so
the Cityscapes evaluator scores at the original size without resizing the ground truth down and back up.
`get_img_info` reads the real width and height (the PNG header, or imgWidth / imgHeight of the json); the reference
hardcodes 2048 x 1024, which is the same thing on the real data."""
import glob
import json
import os

import numpy as np
import torch
import torch.utils.data

from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask


class CityScapesDataset(torch.utils.data.Dataset):
    evaluation_style = "cityscapes"
    CLASSES = ["__background__", "person", "rider", "car", "truck", "bus", "caravan", "trailer", "train", "motorcycle", "bicycle"]
    FIRST_LABEL_ID = 24            # Cityscapes label ids 24 .. 33 are CLASSES[1:], in order: the labels with instances

    def __init__(self, img_dir, ann_dir, split, mode="mask", transforms=None, min_area=0, mini=None,
                 remove_images_without_annotations=False):
        assert split in ("train", "val", "test"), split
        img_dir, ann_dir = os.path.abspath(os.path.join(img_dir, split)), os.path.abspath(os.path.join(ann_dir, split))
        assert os.path.exists(img_dir), img_dir
        assert os.path.exists(ann_dir), ann_dir
        if mode not in ("mask", "poly"):
            raise NotImplementedError("Mode is not implemented yet: %s" % mode)
        self.ann_dir, self.split, self.mode = ann_dir, split, mode
        self.name_to_id = dict(zip(self.CLASSES, range(len(self.CLASSES))))          # AbstractDataset.initMaps
        self.id_to_name = dict(zip(range(len(self.CLASSES)), self.CLASSES))
        self.cityscapesID_to_ind = {self.FIRST_LABEL_ID + i: i + 1 for i in range(len(self.CLASSES) - 1)}
        self.num_classes = len(self.CLASSES)
        self.transforms = transforms
        self.min_area = int(min_area)
        img_paths = sorted(glob.glob(os.path.join(img_dir, "*", "*_leftImg8bit.png")))
        ann_paths = sorted(glob.glob(os.path.join(ann_dir, "*", "*_instanceIds.png" if mode == "mask" else "*_polygons.json")))
        if mini is not None:
            img_paths = img_paths[::len(img_paths) // mini + 1]
            ann_paths = ann_paths[::len(ann_paths) // mini + 1]
        assert len(img_paths) == len(ann_paths), (len(img_paths), len(ann_paths))
        self.img_paths, self.ann_paths = img_paths, ann_paths
        self.substitute_empty = bool(remove_images_without_annotations)
        self.groundtruth_targets = False
        self._sizes = {}

    def __len__(self):
        return len(self.img_paths)

    # ------------------------------------------------------------------ annotations
    def _process_binary_masks(self, ann):
        """ann: the id map, an integer array [H, W] -> (boxes int64 [n, 4], masks uint8 [n, H, W], labels [n])"""
        ann = np.asarray(ann).astype(np.int64)
        ys, xs = np.nonzero(ann >= 1000)                     # below 1000: stuff and group labels
        ids, inst = np.unique(ann[ys, xs], return_inverse=True)
        n = len(ids)
        boxes = np.empty((n, 4), np.int64)
        boxes[:, :2], boxes[:, 2:] = max(ann.shape), -1
        np.minimum.at(boxes[:, 0], inst, xs)
        np.minimum.at(boxes[:, 1], inst, ys)
        np.maximum.at(boxes[:, 2], inst, xs)
        np.maximum.at(boxes[:, 3], inst, ys)
        unknown = [int(v) for v in ids if int(v) // 1000 not in self.cityscapesID_to_ind]
        if unknown:
            raise ValueError("instance ids %s: their labels have no instances in Cityscapes (ids 24 .. 33 do)" % unknown)
        labels = [self.cityscapesID_to_ind[int(v) // 1000] for v in ids]
        masks = (ann[None] == ids[:, None, None]).astype(np.uint8)
        return boxes, masks, labels

    def _process_polygons(self, ann):
        """ann: the parsed *_polygons.json -> (boxes int64 [n, 4], [[x1, y1, x2, y2, ...]] per instance, labels [n])"""
        boxes, polys, labels = [], [], []
        for inst in ann["objects"]:
            if inst["label"] not in self.CLASSES:
                continue
            poly = [v for xy in inst["polygon"] for v in (xy[0], xy[1])]
            boxes.append([int(min(poly[::2])), int(min(poly[1::2])), int(max(poly[::2])), int(max(poly[1::2]))])
            polys.append([poly])
            labels.append(self.name_to_id[inst["label"]])
        return np.array(boxes, np.int64).reshape(-1, 4), polys, labels

    def _annotations(self, index):
        """-> (boxes int64 [n, 4], masks uint8 [n, H, W] or polygon lists, labels), after the min_area filter (_filterGT)"""
        if self.mode == "mask":
            from PIL import Image

            boxes, segs, labels = self._process_binary_masks(np.asarray(Image.open(self.ann_paths[index])))
        else:
            with open(self.ann_paths[index]) as f:
                boxes, segs, labels = self._process_polygons(json.load(f))
        keep = [k for k in range(len(labels)) if (boxes[k, 2] - boxes[k, 0]) * (boxes[k, 3] - boxes[k, 1]) >= self.min_area]
        if len(keep) != len(labels):
            boxes, labels = boxes[keep], [labels[k] for k in keep]
            segs = segs[keep] if self.mode == "mask" else [segs[k] for k in keep]
        return boxes, segs, labels

    def _target(self, boxes, segs, labels, size, with_masks=True):
        target = BoxList(torch.from_numpy(boxes).to(torch.float32).reshape(-1, 4), size, mode="xyxy")
        target.add_field("labels", torch.tensor(labels, dtype=torch.int64))
        if with_masks and len(labels):
            target.add_field("masks", SegmentationMask(torch.from_numpy(segs) if self.mode == "mask" else segs, size, mode=self.mode))
        return target

    # ------------------------------------------------------------------ items
    def __getitem__(self, index):
        from PIL import Image

        boxes, segs, labels = self._annotations(index)
        if len(labels) == 0 and self.substitute_empty and len(self) > 1:
            img, target, _ = self[(index + 1) % len(self)]        # just override this image with the next
            return img, target, index
        img = Image.open(self.img_paths[index]).convert("RGB")
        # a test loader's target is replaced below: its transforms get the boxes alone, no full-size planes to resize
        target = self._target(boxes, segs, labels, img.size, with_masks=not self.groundtruth_targets)
        if self.transforms is not None:
            img, target = self.transforms(img, target)
        if self.groundtruth_targets:
            target = self._target(boxes, segs, labels, self._size(index))
        return img, target, index

    def get_groundtruth(self, index):
        return self._target(*self._annotations(index), self._size(index))

    def _size(self, index):
        if index not in self._sizes:
            if self.mode == "poly":
                with open(self.ann_paths[index]) as f:
                    ann = json.load(f)
                self._sizes[index] = (int(ann["imgWidth"]), int(ann["imgHeight"]))
            else:
                from PIL import Image

                with Image.open(self.img_paths[index]) as im:          # reads the header only
                    self._sizes[index] = tuple(int(v) for v in im.size)
        return self._sizes[index]

    def get_img_info(self, index):
        w, h = self._size(index)
        return {"height": h, "width": w, "idx": index, "img_path": self.img_paths[index], "ann_path": self.ann_paths[index]}
