"""Keypoints / PersonKeypoints — per-instance keypoint sets (reference structures/keypoint.py:8-188).

`keypoints` is a float32 tensor [n, K, 3] of (x, y, v) in image pixels; v is the COCO visibility flag (0 = not labelled,
1 = labelled but hidden, 2 = visible).  The object travels as a BoxList field: it follows `resize`, `transpose`,
indexing (hence `clip_to_image(remove_empty=True)`) and device moves, and carries extra fields of its own (the
post-processor attaches the keypoint scores as "logits").

`keypoints_to_heat_map` is the loss' target projection in plain torch: the CPU path of the keypoint head and the yardstick
of the device kernel (csrc/keypoint.hip, `detops_keypoint_targets`)."""
import torch

from .bounding_box import FLIP_LEFT_RIGHT


class Keypoints(object):
    def __init__(self, keypoints, size, mode=None):
        device = keypoints.device if isinstance(keypoints, torch.Tensor) else torch.device("cpu")
        keypoints = torch.as_tensor(keypoints, dtype=torch.float32, device=device)
        if keypoints.shape[0]:
            keypoints = keypoints.view(keypoints.shape[0], -1, 3)
        self.keypoints = keypoints
        self.size = size            # (image_width, image_height)
        self.mode = mode
        self.extra_fields = {}

    def _like(self, data, size=None):
        out = type(self)(data, self.size if size is None else size, self.mode)
        out.extra_fields = dict(self.extra_fields)
        return out

    def crop(self, box):
        raise NotImplementedError("Keypoints.crop is not supported (as in the reference)")

    def resize(self, size, *args, **kwargs):
        rw, rh = (float(s) / float(o) for s, o in zip(size, self.size))
        data = self.keypoints.clone()
        data[..., 0] *= rw
        data[..., 1] *= rh
        return self._like(data, size)

    def transpose(self, method):
        if method != FLIP_LEFT_RIGHT:
            raise NotImplementedError("Only FLIP_LEFT_RIGHT implemented")
        if self.keypoints.shape[0] == 0:
            return self._like(self.keypoints.clone())
        data = self.keypoints[:, type(self).FLIP_INDS.to(self.keypoints.device)]
        data[..., 0] = self.size[0] - data[..., 0] - 1
        # COCO convention: an unlabelled point (v == 0) has x = y = 0
        data = torch.where((data[..., 2] == 0)[..., None], torch.zeros_like(data), data)
        return self._like(data)

    def to(self, *args, **kwargs):
        out = type(self)(self.keypoints.to(*args, **kwargs), self.size, self.mode)
        for k, v in self.extra_fields.items():
            out.add_field(k, v.to(*args, **kwargs) if hasattr(v, "to") else v)
        return out

    def __getitem__(self, item):
        out = type(self)(self.keypoints[item], self.size, self.mode)
        for k, v in self.extra_fields.items():
            out.add_field(k, v[item])
        return out

    def __len__(self):
        return self.keypoints.shape[0]

    def add_field(self, field, field_data):
        self.extra_fields[field] = field_data

    def get_field(self, field):
        return self.extra_fields[field]

    def has_field(self, field):
        return field in self.extra_fields

    def __repr__(self):
        return "{}(num_instances={}, image_width={}, image_height={})".format(
            type(self).__name__, len(self.keypoints), self.size[0], self.size[1])


_COCO_NAMES = ("nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow",
               "right_elbow", "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle",
               "right_ankle")
# skeleton edges as name pairs (drawing order of the reference's kp_connections)
_COCO_EDGES = (("left_eye", "right_eye"), ("left_eye", "nose"), ("right_eye", "nose"), ("right_eye", "right_ear"),
               ("left_eye", "left_ear"), ("right_shoulder", "right_elbow"), ("right_elbow", "right_wrist"),
               ("left_shoulder", "left_elbow"), ("left_elbow", "left_wrist"), ("right_hip", "right_knee"),
               ("right_knee", "right_ankle"), ("left_hip", "left_knee"), ("left_knee", "left_ankle"),
               ("right_shoulder", "left_shoulder"), ("right_hip", "left_hip"))


def _mirror(name):
    if name.startswith("left_"):
        return "right_" + name[5:]
    if name.startswith("right_"):
        return "left_" + name[6:]
    return name


class PersonKeypoints(Keypoints):
    """the 17 COCO person keypoints"""
    NAMES = list(_COCO_NAMES)
    FLIP_MAP = {n: _mirror(n) for n in _COCO_NAMES if n.startswith("left_")}
    FLIP_INDS = torch.tensor([_COCO_NAMES.index(_mirror(n)) for n in _COCO_NAMES])
    CONNECTIONS = [[_COCO_NAMES.index(a), _COCO_NAMES.index(b)] for a, b in _COCO_EDGES]


def keypoints_to_heat_map(keypoints, rois, heatmap_size):
    """keypoints [P, K, 3], rois [P, 4] xyxy -> (heatmaps [P, K] int64 linear index y * M + x, valid [P, K] int64).
    Per axis: floor((x - x1) * (M / (x2 - x1))) with x == x2 mapped to M - 1 (every step an fp32 rounding, no fused
    multiply-add: torch evaluates the element-wise ops one by one); valid = inside [0, M)^2 and v > 0."""
    if rois.numel() == 0:
        return rois.new_zeros((0,), dtype=torch.int64), rois.new_zeros((0,), dtype=torch.int64)
    M = heatmap_size
    x, y = keypoints[..., 0], keypoints[..., 1]

    def axis(p, lo, hi):
        scale = M / (hi - lo)        # Tensor.__rtruediv__: reciprocal() * M, two fp32 roundings (as in the reference)
        q = ((p - lo[:, None]) * scale[:, None]).floor().long()
        return torch.where(p == hi[:, None], torch.full_like(q, M - 1), q)

    xi = axis(x, rois[:, 0], rois[:, 2])
    yi = axis(y, rois[:, 1], rois[:, 3])
    valid = ((xi >= 0) & (yi >= 0) & (xi < M) & (yi < M) & (keypoints[..., 2] > 0)).long()
    return (yi * M + xi) * valid, valid
