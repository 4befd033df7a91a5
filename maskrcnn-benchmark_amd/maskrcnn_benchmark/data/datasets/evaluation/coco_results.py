"""COCO result files (reference data/datasets/evaluation/coco/coco_eval.py:70-186): the detections of a run in the COCO
results format, `bbox.json`, `segm.json` and `keypoints.json` — what the COCO servers accept and what any other tool,
pycocotools among them, reads.

`prepare_for_coco_detection`, `prepare_for_coco_segmentation` and `prepare_for_coco_keypoint` have the reference's names
and signatures, (predictions, dataset) -> list of dict; `COCOResultsWriter` is the same per image, fed batch by batch by
the inference loop.  Per image, as in the reference: resize to the image's original size (`get_img_info`), boxes in xywh,
`image_id` through `id_to_img_map`, `category_id` through `contiguous_category_id_to_json_id`, images without detections
skipped.  A dataset without those maps (the synthetic one) uses the index as the image id and the label as the category id.

Masks are dense planes of the image's ORIGINAL size or M x M floating-point probabilities; anything else raises (planes
pasted at the network's input size cannot be pasted again).  Probabilities are pasted at the original size with
Masker(0.5, padding=1)'s parameters: device tensors by `_C.paste_masks_rle` (planes never stored), CPU tensors by
`paste_masks_torch`; dense planes are run-length coded by torch operators where they live.  Either way the runs go to
`_C.rle_strings` (include/detops.h, "Compressed RLE strings"), so one image leaves the device as boxes, scores, labels,
keypoints, the strings' bytes and their offsets.

Reading them back: `load_results` turns `bbox.json` / `segm.json` (this project's or another tool's) into the BoxLists the
evaluator takes, the masks as RLEMasks decoded by `_C.rle_string_decode_list` (include/detops.h, "Reading compressed RLE
strings"); `evaluate_result_files` scores the files against a dataset's ground truth (tools/evaluate_results.py).

`keypoints.json` is read back and scored under names of their own, keypoint_oks.load_keypoint_results and
keypoint_oks.evaluate_keypoint_file (tools/evaluate_keypoints.py); `load_results` and `evaluate_result_files` still refuse
"keypoints".

No file is written for `box_only` proposals: they are scored in the loop (box_proposals.py)."""
import json
import os

import numpy as np
import torch

from maskrcnn_benchmark import _C, _rle_cpu
from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import paste_masks_torch
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.rle_masks import RLEMasks

from .coco_style import COCOStyleEvaluator, _feed, _num_classes

IOU_TYPES = ("bbox", "segm", "keypoints")
MASK_THRESHOLD, MASK_PADDING = 0.5, 1      # the reference's Masker(threshold=0.5, padding=1)


def _image_id(dataset, index):
    ids = getattr(dataset, "id_to_img_map", None)
    return int(index) if ids is None else ids[index]


def _category_ids(dataset, labels):
    table = getattr(dataset, "contiguous_category_id_to_json_id", None)
    return list(labels) if table is None else [table[i] for i in labels]


def _original(dataset, index, prediction):
    """the prediction in the frame of the image as it is on disk -> (BoxList, width, height)"""
    info = dataset.get_img_info(index)
    width, height = info["width"], info["height"]
    return prediction.resize((width, height)), width, height


def plane_runs(planes):
    """bool / uint8 [n, H, W] -> (counts int32 [total], run_offset int64 [n + 1]) on the planes' device: `rle_encode` of
    every plane (column-major runs starting with a 0-run), back to back, without a Python loop over the planes"""
    n, H, W = planes.shape
    dev = planes.device
    if n == 0:
        return torch.empty((0,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev)
    flat = planes.transpose(1, 2).reshape(n, H * W).to(torch.int8)
    before = torch.cat([flat.new_zeros((n, 1)), flat[:, :-1]], dim=1)
    row, pos = torch.nonzero(flat != before, as_tuple=True)          # row-major: plane after plane, positions ascending
    edges = torch.bincount(row, minlength=n)
    edge_start = torch.cumsum(edges, 0) - edges
    start = torch.cumsum(edges + 2, 0) - (edges + 2)                 # a plane's bounds: 0, its edges, H * W
    bounds = torch.zeros((int(pos.numel()) + 2 * n,), dtype=torch.int64, device=dev)
    bounds[start + edges + 1] = H * W
    bounds[start[row] + 1 + torch.arange(pos.numel(), device=dev) - edge_start[row]] = pos
    keep = torch.ones((bounds.numel() - 1,), dtype=torch.bool, device=dev)
    keep[start[1:] - 1] = False                                      # the difference across two planes
    counts = (bounds[1:] - bounds[:-1])[keep].to(torch.int32)
    run_offset = torch.cat([edges.new_zeros(1), torch.cumsum(edges + 1, 0)])
    return counts, run_offset


def mask_strings(masks, boxes, height, width):
    """the masks of one image, [n, 1, H, W] planes of the image's size or [n, 1, M, M] floating-point probabilities with
    their xyxy `boxes` in the image -> a list of n compressed `counts` strings; ValueError for anything else"""
    if masks.dim() == 3:
        masks = masks[:, None]
    if list(masks.shape[-2:]) == [height, width]:
        counts, run_offset = plane_runs(masks[:, 0] != 0)
    elif masks.shape[-1] != masks.shape[-2] or not masks.is_floating_point():
        # e.g. POSTPROCESS_MASKS planes pasted at the network's input size: they cannot be pasted again as probabilities
        raise ValueError("result files: masks of shape %s and dtype %s are neither planes of the image's original size "
                         "%d x %d nor M x M probability maps" % (tuple(masks.shape), masks.dtype, height, width))
    elif masks.is_cuda:
        counts, run_offset = _C.paste_masks_rle(masks, boxes, [(height, width)], MASK_THRESHOLD, MASK_PADDING,
                                                counts=[masks.shape[0]])
    else:
        counts, run_offset = plane_runs(paste_masks_torch(masks, boxes, height, width, MASK_THRESHOLD, MASK_PADDING)[:, 0])
    return _C.rle_string_list(*_C.rle_strings(counts, run_offset))


def detection_entries(dataset, index, prediction):
    if len(prediction) == 0:
        return []
    original_id = _image_id(dataset, index)
    prediction, _, _ = _original(dataset, index, prediction)
    prediction = prediction.convert("xywh")
    boxes = prediction.bbox.tolist()
    scores = prediction.get_field("scores").tolist()
    labels = _category_ids(dataset, prediction.get_field("labels").tolist())
    return [{"image_id": original_id, "category_id": labels[k], "bbox": box, "score": scores[k]}
            for k, box in enumerate(boxes)]


def segmentation_entries(dataset, index, prediction):
    if len(prediction) == 0:
        return []
    original_id = _image_id(dataset, index)
    prediction, width, height = _original(dataset, index, prediction)
    strings = mask_strings(prediction.get_field("mask"), prediction.convert("xyxy").bbox, height, width)
    scores = prediction.get_field("scores").tolist()
    labels = _category_ids(dataset, prediction.get_field("labels").tolist())
    return [{"image_id": original_id, "category_id": labels[k],
             "segmentation": {"size": [height, width], "counts": s}, "score": scores[k]}
            for k, s in enumerate(strings)]


def keypoint_entries(dataset, index, prediction):
    if len(prediction.bbox) == 0:
        return []
    original_id = _image_id(dataset, index)
    prediction, width, height = _original(dataset, index, prediction)
    scores = prediction.get_field("scores").tolist()
    labels = _category_ids(dataset, prediction.get_field("labels").tolist())
    keypoints = prediction.get_field("keypoints").resize((width, height))
    keypoints = keypoints.keypoints.reshape(keypoints.keypoints.shape[0], -1).tolist()
    return [{"image_id": original_id, "category_id": labels[k], "keypoints": keypoint, "score": scores[k]}
            for k, keypoint in enumerate(keypoints)]


_ENTRIES = {"bbox": detection_entries, "segm": segmentation_entries, "keypoints": keypoint_entries}


def _prepare(iou_type, predictions, dataset):
    results = []
    for index, prediction in enumerate(predictions):
        results.extend(_ENTRIES[iou_type](dataset, index, prediction))
    return results


def prepare_for_coco_detection(predictions, dataset):
    return _prepare("bbox", predictions, dataset)


def prepare_for_coco_segmentation(predictions, dataset):
    return _prepare("segm", predictions, dataset)


def prepare_for_coco_keypoint(predictions, dataset):
    return _prepare("keypoints", predictions, dataset)


# ------------------------------------------------------------------------------------------------ reading them back
def _read_entries(path_or_list):
    if isinstance(path_or_list, (str, bytes, os.PathLike)):
        with open(path_or_list) as f:
            path_or_list = json.load(f)
    if not isinstance(path_or_list, list):
        raise ValueError("a result file holds a list of entries, got %s" % type(path_or_list).__name__)
    return path_or_list


def _group_entries(path_or_list, dataset):
    """-> (the file's entries, per image of the dataset its entries in file order, the map from category id to label or
    None): entries go to their image through the inverse of `id_to_img_map`, labels come through
    `json_category_id_to_contiguous_id`; a dataset without these maps uses the index and the label, as the writer does.
    ValueError: an image id or a category id the dataset does not have."""
    entries = _read_entries(path_or_list)
    ids = getattr(dataset, "id_to_img_map", None)
    index_of = {v: k for k, v in ids.items()} if ids is not None else None
    labels_of = getattr(dataset, "json_category_id_to_contiguous_id", None)
    if labels_of is None and getattr(dataset, "contiguous_category_id_to_json_id", None) is not None:
        labels_of = {v: k for k, v in dataset.contiguous_category_id_to_json_id.items()}
    per_image = [[] for _ in range(len(dataset))]
    for e in entries:
        image_id = e["image_id"]
        index = index_of.get(image_id) if index_of is not None else (image_id if isinstance(image_id, int) else None)
        if index is None or not 0 <= index < len(per_image):
            raise ValueError("result files: image_id %r is not in the dataset" % (image_id,))
        if labels_of is not None and e["category_id"] not in labels_of:
            raise ValueError("result files: category_id %r is not in the dataset" % (e["category_id"],))
        per_image[index].append(e)
    return entries, per_image, labels_of


def _scored_boxlist(boxes, size, mode, es, labels_of):
    """the xyxy BoxList of an image's entries `es`, with their `scores` and `labels`; boxes: theirs, [len(es), 4] in `mode`"""
    boxlist = BoxList(boxes, size, mode=mode).convert("xyxy")
    boxlist.add_field("scores", torch.tensor([e["score"] for e in es], dtype=torch.float32))
    cats = [e["category_id"] for e in es]
    boxlist.add_field("labels", torch.tensor(cats if labels_of is None else [labels_of[c] for c in cats], dtype=torch.int64))
    return boxlist


def _segmentation_string(entry, height, width):
    """the entry's `segmentation` as a compressed string; an uncompressed counts list is coded by the numpy coder, so that
    one decode call checks and unpacks every mask of the file alike"""
    seg = entry.get("segmentation")
    if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
        raise ValueError("result files: a segmentation must be an RLE {size, counts}; polygons are not read (image %r)"
                         % (entry.get("image_id"),))
    if [int(v) for v in seg["size"]] != [height, width]:
        raise ValueError("result files: an RLE of size %s for image %r of %d x %d" % (seg["size"], entry["image_id"], height, width))
    counts = seg["counts"]
    if isinstance(counts, bytes):
        counts = counts.decode("latin-1")
    if isinstance(counts, str):
        return counts
    runs = np.asarray(counts, dtype=np.int64).reshape(-1)
    if runs.size and (runs.min() < 0 or runs.max() >= 2 ** 31):
        raise ValueError("result files: uncompressed counts outside [0, 2^31) (image %r)" % (entry["image_id"],))
    return _rle_cpu.to_str_list(*_rle_cpu.rle_strings(runs.astype(np.int32), np.array([0, runs.size])))[0]


def load_results(path_or_list, dataset, iou_type, device=None):
    """A `bbox.json` / `segm.json` result file (a path, or its list of entries) -> a list of BoxList in dataset order, what
    COCOStyleEvaluator.update takes: the inverse of the writer.  Entries are grouped by image and labelled as
    _group_entries does, and keep the file's order inside an image (the evaluator's stable sort then reproduces ties).
    `bbox` goes from xywh through BoxList(mode="xywh").convert("xyxy"); a segm entry without `bbox` gets the
    full-image box, which the segm rules never read.  `segmentation` is a compressed string or an uncompressed list and
    becomes the `mask` field, an RLEMasks on `device` (every string of the file in ONE _C.rle_string_decode_list call).
    ValueError: an unknown image id or category id, a polygon, an RLE of another size than its image, malformed strings."""
    if iou_type == "keypoints":
        raise NotImplementedError("keypoints.json is read by keypoint_oks.load_keypoint_results, not by load_results")
    if iou_type not in ("bbox", "segm"):
        raise ValueError("load_results: unknown iou type %r" % (iou_type,))
    _, per_image, labels_of = _group_entries(path_or_list, dataset)
    device = torch.device("cpu" if device is None else device)
    sizes = []
    for index in range(len(per_image)):
        info = dataset.get_img_info(index)
        sizes.append((int(info["width"]), int(info["height"])))
    rle = None
    if iou_type == "segm":
        strings = [_segmentation_string(e, sizes[i][1], sizes[i][0]) for i, es in enumerate(per_image) for e in es]
        hw = [(sizes[i][1], sizes[i][0]) for i, es in enumerate(per_image) for _ in es]
        rle = _C.rle_string_decode_list(strings, hw, device)
        starts = rle[1].tolist()                     # one host read for the whole file
    out, first = [], 0
    for index, es in enumerate(per_image):
        W, H = sizes[index]
        if es and all("bbox" in e for e in es):
            boxes, mode = torch.tensor([e["bbox"] for e in es], dtype=torch.float32).reshape(-1, 4), "xywh"
        elif iou_type == "bbox" and es:
            raise ValueError("result files: a bbox entry without `bbox` (image %r)" % (es[0]["image_id"],))
        else:
            boxes, mode = torch.tensor([[0.0, 0.0, W - 1.0, H - 1.0]] * len(es)).reshape(-1, 4), "xyxy"
        boxlist = _scored_boxlist(boxes, (W, H), mode, es, labels_of).to(device)
        if rle is not None:                          # the image's slice of the file's runs
            a, b = starts[first], starts[first + len(es)]
            boxlist.add_field("mask", RLEMasks(rle[0][a:b], rle[1][first:first + len(es) + 1] - a, (W, H)))
        out.append(boxlist)
        first += len(es)
    return out


def evaluate_result_files(dataset, files, output_folder=None, batch=8, device="cpu", expected_results=(),
                          expected_results_sigma_tol=4):
    """Score saved result files against `dataset`'s ground truth: files = {"bbox": path, "segm": path} (either or both; a
    list of entries serves as a path).  One COCOStyleEvaluator per file, fed `batch` images at a time on `device`; the
    masks of segm.json go from runs to bit rows there (_C.mask_pack_rle), no plane is laid out.  -> the COCOResults of
    finish_coco, which also logs the tables and, with `output_folder`, writes coco_results.pth / coco_results.txt.
    `keypoints` raises NotImplementedError: keypoints.json is scored by keypoint_oks.evaluate_keypoint_file."""
    from . import finish_coco

    if "keypoints" in files:
        raise NotImplementedError("keypoints.json is scored by keypoint_oks.evaluate_keypoint_file (tools/evaluate_keypoints.py), "
                                  "not by evaluate_result_files")
    iou_types = tuple(t for t in ("bbox", "segm") if t in files)
    unknown = sorted(set(files) - set(iou_types))
    if unknown or not iou_types:
        raise ValueError("evaluate_result_files: expected files for bbox and / or segm, got %s" % sorted(files))
    num_classes = _num_classes(dataset, 81)
    device = torch.device(device)
    merged = COCOStyleEvaluator(iou_types, num_classes)
    for t in iou_types:
        evaluator = _feed(COCOStyleEvaluator((t,), num_classes), load_results(files[t], dataset, t, device), dataset, batch, device)
        merged.records[t] = evaluator.records[t]
        merged.num_images, merged.num_groundtruths = evaluator.num_images, evaluator.num_groundtruths
        merged.num_detections = max(merged.num_detections, evaluator.num_detections)
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
    return finish_coco(merged, output_folder, expected_results, expected_results_sigma_tol)


class COCOResultsWriter(object):
    """The result files of a run, image by image: `update(predictions, image_indices)` per batch (BoxLists on any device and
    their indices in `dataset`), `save(folder)` at the end -> <folder>/<iou_type>.json for each of `iou_types`."""

    def __init__(self, dataset, iou_types):
        unknown = [t for t in iou_types if t not in IOU_TYPES]
        if unknown:
            raise ValueError("COCOResultsWriter: unknown iou types %s (of %s)" % (unknown, list(IOU_TYPES)))
        self.dataset = dataset
        self.iou_types = tuple(iou_types)
        self.results = {t: [] for t in self.iou_types}
        self.num_images = 0

    def update(self, predictions, image_indices):
        if len(predictions) != len(image_indices):
            raise ValueError("COCOResultsWriter.update: %d predictions for %d image indices"
                             % (len(predictions), len(image_indices)))
        for prediction, index in zip(predictions, image_indices):
            for t in self.iou_types:
                self.results[t].extend(_ENTRIES[t](self.dataset, int(index), prediction))
            self.num_images += 1

    def save(self, folder):
        """-> {iou_type: path}"""
        os.makedirs(folder, exist_ok=True)
        paths = {}
        for t in self.iou_types:
            paths[t] = os.path.join(folder, t + ".json")
            with open(paths[t], "w") as f:
                json.dump(self.results[t], f)
        return paths
