"""Mask post-processing for inference (reference roi_heads/mask_head/inference.py:12-209): sigmoid, pick each detection's
class channel, attach as field "mask" — [n,1,M,M] probabilities, or with MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS the
image-size masks of `Masker` ([n,1,H,W] bool), or with `MaskPostProcessorCOCOFormat` their uncompressed COCO RLE.

The reference pastes in a Python loop over the detections on the CPU (`interpolate`, threshold, slice assignment) and
encodes every plane with pycocotools.  Here device tensors take one launch for the whole batch (csrc/masker.hip:
`_C.paste_masks`), and the RLE path never stores the planes (`_C.paste_masks_rle`).  `paste_masks_torch` is the same
definition in torch operators: the CPU path and the yardstick of the kernels.

The definition's two traps: the expanded box goes to integers by truncation toward zero (a left edge of -0.4 becomes 0,
floor would give -1), and a box whose integer window misses the image gives an all-zero plane (the reference's slice
bounds go negative there: this project's own choice)."""
import torch
import torch.nn.functional as F
from torch import nn

from maskrcnn_benchmark import _C
from maskrcnn_benchmark.structures.bounding_box import BoxList


def expand_boxes(boxes, scale):
    """boxes [n, 4] xyxy scaled about their centres; each step one rounding in the boxes' dtype"""
    half = (boxes[:, 2:] - boxes[:, :2]) * 0.5
    centre = (boxes[:, 2:] + boxes[:, :2]) * 0.5
    half = half * scale
    return torch.cat([centre - half, centre + half], dim=1)


def expand_masks(mask, padding):
    """mask [n, 1, M, M] (or [n, M, M]) -> (zero-padded [n, 1, M + 2p, M + 2p], scale (M + 2p) / M as a Python float)"""
    if padding < 1:
        raise ValueError("expand_masks: padding must be at least 1, got %r" % (padding,))
    M = mask.shape[-1]
    scale = float(M + 2 * padding) / M
    return F.pad(mask.reshape(-1, 1, M, M), (padding, padding, padding, padding)), scale


def paste_masks_torch(masks, boxes, im_h, im_w, threshold=0.5, padding=1):
    """The masks of ONE image in torch operators: masks [n, 1, M, M] or [n, M, M], boxes [n, 4] xyxy -> bool
    [n, 1, im_h, im_w] on the masks' device.  Per detection: pad, expand the box, truncate to int32, bilinear resize to the
    integer box (ATen, align_corners=False), threshold (`threshold < 0`: value * 255 != 0), copy the clipped window."""
    n = masks.shape[0]
    out = torch.zeros((n, 1, im_h, im_w), dtype=torch.bool, device=masks.device)
    if n == 0:
        return out
    padded, scale = expand_masks(masks.float(), padding)
    int_boxes = expand_boxes(boxes.float(), scale).to(torch.int32).tolist()
    for i, (x1, y1, x2, y2) in enumerate(int_boxes):
        w, h = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
        x_lo, x_hi = max(x1, 0), min(x2 + 1, im_w)
        y_lo, y_hi = max(y1, 0), min(y2 + 1, im_h)
        if x_hi <= x_lo or y_hi <= y_lo:
            continue
        m = F.interpolate(padded[i:i + 1], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
        m = m > threshold if threshold >= 0 else (m * 255).to(torch.bool)
        out[i, 0, y_lo:y_hi, x_lo:x_hi] = m[y_lo - y1:y_hi - y1, x_lo - x1:x_hi - x1]
    return out


def rle_encode(plane):
    """bool [H, W] -> {"size": [H, W], "counts": [...]}: uncompressed COCO RLE, the run lengths of the plane in column-major
    order, alternating 0-runs and 1-runs and starting with a 0-run (of length 0 when pixel (0, 0) is set)"""
    H, W = plane.shape
    flat = plane.t().reshape(-1).to(torch.int8)
    before = torch.cat([flat.new_zeros(1), flat[:-1]])
    edges = torch.nonzero(flat != before).flatten()
    edges = torch.cat([edges.new_zeros(1), edges, edges.new_full((1,), H * W)])
    return {"size": [H, W], "counts": (edges[1:] - edges[:-1]).tolist()}


def compress_rles(rles):
    """a list of uncompressed {"size", "counts": [...]} -> the same masks with `counts` as COCO's compressed strings"""
    runs = [torch.tensor(r["counts"], dtype=torch.int32) for r in rles]
    run_offset = torch.tensor([0] + [len(r) for r in runs], dtype=torch.int64).cumsum(0)
    strings = _C.rle_string_list(*_C.rle_strings(torch.cat(runs) if runs else torch.empty(0, dtype=torch.int32), run_offset))
    return [{"size": list(r["size"]), "counts": s} for r, s in zip(rles, strings)]


class Masker(object):
    """Projects the masks of each image into the image at the locations of its boxes (reference :162-199)"""

    def __init__(self, threshold=0.5, padding=1):
        self.threshold = threshold
        self.padding = padding

    def forward_single_image(self, masks, boxes):
        return self._paste([masks], [boxes])[0]

    def _paste(self, masks, boxes):
        boxes = [b.convert("xyxy") for b in boxes]
        sizes = [(b.size[1], b.size[0]) for b in boxes]
        full = [i for i, b in enumerate(boxes) if len(b) > 0]
        # an image without detections: the reference's empty result, of the probability maps' shape and dtype
        results = [m.new_empty((0, 1, m.shape[-2], m.shape[-1])) for m in masks]
        if not full:
            return results
        if _C.on_device(masks[full[0]]):
            _, views = _C.paste_masks(torch.cat([masks[i] for i in full]), torch.cat([boxes[i].bbox for i in full]),
                                      [sizes[i] for i in full], self.threshold, self.padding,
                                      counts=[len(boxes[i]) for i in full])
            for i, v in zip(full, views):
                results[i] = v
        else:
            for i in full:
                results[i] = paste_masks_torch(masks[i], boxes[i].bbox, sizes[i][0], sizes[i][1], self.threshold,
                                               self.padding)
        return results

    def __call__(self, masks, boxes):
        """masks: a list of [n_i, 1, M, M] tensors (or a tensor whose first index is the image), boxes: a list of BoxLists
        -> a list of [n_i, 1, H_i, W_i] bool.  A single BoxList is wrapped in a list as in the reference; one step beyond
        the reference, a 4-D masks tensor passed with it is wrapped too (the reference would iterate over its detections
        and fail its own length assertion)."""
        if isinstance(boxes, BoxList):
            boxes = [boxes]
            if isinstance(masks, torch.Tensor) and masks.dim() == 4:
                masks = [masks]
        assert len(boxes) == len(masks), "Masks and boxes should have the same length."
        for mask, box in zip(masks, boxes):
            assert mask.shape[0] == len(box), "Number of objects should be the same."
        return self._paste(list(masks), list(boxes))


class MaskPostProcessor(nn.Module):
    def __init__(self, masker=None):
        super(MaskPostProcessor, self).__init__()
        self.masker = masker

    def _probabilities(self, x, boxes):
        prob = x.sigmoid()
        labels = torch.cat([b.get_field("labels") for b in boxes])
        prob = prob[torch.arange(prob.shape[0], device=labels.device), labels][:, None]
        return prob.split([len(b) for b in boxes], dim=0)

    def forward(self, x, boxes):
        prob = self._probabilities(x, boxes)
        if self.masker:
            prob = self.masker(prob, boxes)
        results = []
        for p, b in zip(prob, boxes):
            out = b.copy_with_fields(b.fields())
            out.add_field("mask", p)
            results.append(out)
        return results


class MaskPostProcessorCOCOFormat(MaskPostProcessor):
    """The pasted masks in COCO format (reference :64-85): field "mask" is a list with one
    {"size": [H, W], "counts": [...]} per detection — UNCOMPRESSED RLE, which pycocotools reads itself (frPyObjects); the
    reference's compressed strings need pycocotools.  On the device the image-size planes are never stored.
    `compressed=True`: {"size": [H, W], "counts": "<str>"} as the reference's field holds, the strings of COCO result files
    (include/detops.h, "Compressed RLE strings": `_C.rle_strings` behind `_C.paste_masks_rle`; on the device the runs never
    become Python lists, only the strings' bytes cross)."""

    def __init__(self, masker=None, compressed=False):
        super(MaskPostProcessorCOCOFormat, self).__init__(masker)
        self.compressed = compressed

    def forward(self, x, boxes):
        if not self.masker:
            raise ValueError("MaskPostProcessorCOCOFormat needs a Masker (threshold and padding of the pasted masks)")
        prob = self._probabilities(x, boxes)
        threshold, padding = self.masker.threshold, self.masker.padding
        xyxy = [b.convert("xyxy") for b in boxes]
        sizes = [(b.size[1], b.size[0]) for b in boxes]
        per_image = [len(b) for b in boxes]
        if _C.on_device(x) and sum(per_image):
            counts, run_offset = _C.paste_masks_rle(torch.cat(prob), torch.cat([b.bbox for b in xyxy]), sizes, threshold,
                                                    padding, counts=per_image)
            if self.compressed:
                flat = _C.rle_string_list(*_C.rle_strings(counts, run_offset))
            else:
                offs, runs = run_offset.cpu().tolist(), counts.cpu().tolist()
                flat = [runs[offs[i]:offs[i + 1]] for i in range(sum(per_image))]
            rles, k = [], 0
            for (h, w), c in zip(sizes, per_image):
                rles.append([{"size": [h, w], "counts": r} for r in flat[k:k + c]])
                k += c
        else:
            rles = [[rle_encode(m[0]) for m in paste_masks_torch(p, b.bbox, h, w, threshold, padding).cpu()]
                    for p, b, (h, w) in zip(prob, xyxy, sizes)]
            if self.compressed:
                rles = [compress_rles(r) for r in rles]
        results = []
        for r, b in zip(rles, boxes):
            out = b.copy_with_fields(b.fields())
            out.add_field("mask", r)
            results.append(out)
        return results


def make_roi_mask_post_processor(cfg):
    if cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS:
        masker = Masker(threshold=cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD, padding=1)
    else:
        masker = None
    return MaskPostProcessor(masker)
