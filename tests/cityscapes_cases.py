"""Shared by tests/test_cityscapes_cpu.py and tests/test_cityscapes_gpu.py: the fixture the reference's Cityscapes
evaluation wrote (tests/golden/cityscapes_reference.npz, made by tests/golden/make_golden_cityscapes.py) as BoxLists and a
dataset, problems for `_C.window_counts` at the shapes where the kernel can go wrong, the counts as literal Python loops, a
Cityscapes tree written with PIL, and the kernel under the host emulation (tests/emu_cityscapes: the emulation library of
tests/emu does not hold csrc/cityscapes_eval.hip)."""
import contextlib
import ctypes
import json
import os
import subprocess

import numpy as np
import torch

from maskrcnn_benchmark import _C, _abi
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cityscapes_reference.npz")
_EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_cityscapes")
_EMU = None


def emu_cityscapes_lib():
    """csrc/cityscapes_eval.hip compiled as host C++ over the fiber emulation (tests/emu/hip_cpu_emu.h), built when needed
    and bound from the table the device build is bound from (maskrcnn_benchmark/_abi.py)"""
    global _EMU
    if _EMU is None:
        subprocess.check_call(["make", "-s", "-C", _EMU_DIR])
        _EMU = ctypes.CDLL(os.path.join(_EMU_DIR, "libdetops_emu_cityscapes.so"))
        assert _abi.bind(_EMU, require_all=False) == {"detops_window_counts"}
    return _EMU


class _WithWindowCounts(object):
    """the emulation library of tests/emu, with detops_window_counts from emu_cityscapes_lib()"""

    def __init__(self, base):
        self._base = base
        self.detops_window_counts = emu_cityscapes_lib().detops_window_counts

    def __getattr__(self, name):
        return getattr(self._base, name)


@contextlib.contextmanager
def emulated():
    """cpu_shim's "emu-lib" backend (the product's own `_C` wrappers on CPU tensors take their device branches over the
    emulation library) with the emulated window-count kernel added to the library handle"""
    import cpu_shim

    with cpu_shim.install("emu-lib"):
        base = _C.lib
        _C.lib = _WithWindowCounts(base)
        try:
            yield _C.lib
        finally:
            _C.lib = base


# ------------------------------------------------------------------------------------------------ the fixture
def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


class FixtureDataset(object):
    """the fixture's ground truth as the test loader hands it out: original-size targets with labels and binary masks"""
    evaluation_style = "cityscapes"

    def __init__(self, fx):
        self.CLASSES = [str(c) for c in fx["classes"]]
        self.sizes = [tuple(int(v) for v in s) for s in fx["sizes"]]
        self.targets = []
        g = _offsets(fx["gt_counts"])
        for i, size in enumerate(self.sizes):
            t = BoxList(torch.from_numpy(fx["gt_boxes"][g[i]:g[i + 1]]).reshape(-1, 4), size, mode="xyxy")
            t.add_field("labels", torch.from_numpy(fx["gt_labels"][g[i]:g[i + 1]]))
            if len(t):
                t.add_field("masks", SegmentationMask(torch.from_numpy(fx["gt_planes_%d" % i]), size, mode="mask"))
            self.targets.append(t)

    def __len__(self):
        return len(self.targets)

    def get_groundtruth(self, index):
        return self.targets[index]

    def __getitem__(self, index):
        w, h = self.sizes[index]
        return torch.zeros((3, h, w)), self.targets[index], index

    def get_img_info(self, index):
        return {"width": self.sizes[index][0], "height": self.sizes[index][1]}


def fixture_predictions(fx, device="cpu", masks="probabilities"):
    """the predictions as the reference got them; masks: "probabilities" [n, 1, M, M] | "planes" (what the reference's Masker
    pasted, bool [n, 1, H, W]) | None (no `mask` field)"""
    out, d = [], _offsets(fx["pred_counts"])
    for i, size in enumerate(fx["sizes"]):
        p = BoxList(torch.from_numpy(fx["pred_boxes"][d[i]:d[i + 1]]).reshape(-1, 4), tuple(int(v) for v in size), mode="xyxy")
        p.add_field("labels", torch.from_numpy(fx["pred_labels"][d[i]:d[i + 1]]))
        p.add_field("scores", torch.from_numpy(fx["pred_scores"][d[i]:d[i + 1]]))
        if masks == "probabilities":
            p.add_field("mask", torch.from_numpy(fx["pred_masks"][d[i]:d[i + 1]]))
        elif masks == "planes":
            p.add_field("mask", torch.from_numpy(fx["pred_planes_%d" % i])[:, None] != 0)
        out.append(p.to(device))
    return out


def flat_averages(avg, classes):
    v = [avg["allAp"], avg["allAp50%"], avg["allAp75%"]]
    for name in classes:
        v += [avg["classes"][name]["ap"], avg["classes"][name]["ap50%"], avg["classes"][name]["ap75%"]]
    return np.array(v, np.float64)


AP_TOL = 1e-12        # the values lie in [0, 1]; the only freedom is the order of an fp64 dot product of a few hundred terms


def assert_reference_ap(fx, results):
    classes = [str(c) for c in fx["classes"]]
    for iou_type, ap_key, avg_key in (("bbox", "box_ap", "box_avg"), ("segm", "mask_ap", "mask_avg")):
        got, want = results[iou_type]["ap"], fx[ap_key]
        assert got.shape == want.shape == (1, len(classes), 10) and got.dtype == np.float64
        assert np.array_equal(np.isnan(got), np.isnan(want)), iou_type
        err = np.nanmax(np.abs(got - want))
        avg = flat_averages(results[iou_type]["averages"], classes)
        assert np.array_equal(np.isnan(avg), np.isnan(fx[avg_key]))
        err_avg = np.nanmax(np.abs(avg - fx[avg_key]))
        print("%s: largest AP difference %.3g, largest average difference %.3g" % (iou_type, err, err_avg))
        assert err <= AP_TOL and err_avg <= AP_TOL, (iou_type, err, err_avg)


def assert_reference_records(fx, evaluator):
    """every per-instance boxArea / pixelCount and every recorded pair of the fixture, exactly"""
    g, d = _offsets(fx["gt_counts"]), _offsets(fx["pred_counts"])
    assert len(evaluator.images) == len(fx["sizes"])
    pairs = []
    for i, im in enumerate(evaluator.images):
        np.testing.assert_array_equal(im["gt_box_area"], fx["gt_box_area"][g[i]:g[i + 1]])
        np.testing.assert_array_equal(im["gt_pixel_count"], fx["gt_pixel_count"][g[i]:g[i + 1]])
        kept = np.nonzero(fx["pred_kept"][d[i]:d[i + 1]])[0]
        np.testing.assert_array_equal(im["dt_index"], kept)
        np.testing.assert_array_equal(im["dt_box_area"], fx["pred_box_area"][d[i]:d[i + 1]][kept])
        np.testing.assert_array_equal(im["dt_pixel_count"], fx["pred_pixel_count"][d[i]:d[i + 1]][kept])
        pairs += [(i, int(gt), int(dt), int(b), int(m)) for dt, gt, b, m in im["pairs"]]
    np.testing.assert_array_equal(np.array(sorted(pairs), np.int64).reshape(-1, 5), fx["pairs"])


# ------------------------------------------------------------------------------------------------ problems for the operator
def problem(seed, D, G, H, W, values=(0, 1), dtype=np.uint8, boxes=None):
    """-> planes [D, H, W] / [G, H, W] with about half the pixels set to values[1], and boxes: `boxes` ([(xmin, ymin, xmax,
    ymax)] cycled over predictions and ground truths), or drawn: inside, across and outside the image, some empty"""
    rng = np.random.RandomState(seed)
    pl = lambda n: np.where(rng.rand(n, H, W) < 0.5, values[1], values[0]).astype(dtype)  # noqa: E731

    def draw(n):
        x0, y0 = rng.randint(-3, W + 2, n), rng.randint(-3, H + 2, n)
        b = np.stack([x0, y0, x0 + rng.randint(0, W + 4, n), y0 + rng.randint(0, H + 4, n)], 1)
        return b.astype(np.int32).reshape(-1, 4)

    if boxes is None:
        db, gb = draw(D), draw(G)
    else:
        boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
        db, gb = boxes[np.arange(D) % len(boxes)], boxes[(np.arange(G) + 1) % len(boxes)]
    return {"dt_planes": pl(D), "dt_box": db.reshape(-1, 4), "gt_planes": pl(G), "gt_box": gb.reshape(-1, 4)}


def edge_boxes(H, W):
    """width 1, height 1, empty, the whole plane, touching the right and bottom edges, a start at every column residue
    modulo 16, outside the image on every side, and two that only touch"""
    b = [(0, 0, 1, H), (0, 0, W, 1), (2, 1, 2, H), (1, 2, W, 2), (0, 0, W, H), (W - 1, 0, W, H), (0, H - 1, W, H),
         (W // 2, H // 2, W, H), (-5, -7, W + 9, H + 4), (-4, 1, 3, H + 2), (W - 2, -3, W + 6, 2), (W, 0, W + 5, H), (-9, -9, 0, 0),
         (0, 0, W // 2, H), (W // 2, 0, W, H), (3, 5, 1, 2)]
    b += [(x, x % max(H, 1), x + 17, H) for x in range(min(16, W))]
    return b


def run_op(pb, device=None):
    """_C.window_counts on `device` (None: CPU tensors, i.e. the numpy path unless _C is patched) -> four numpy arrays"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device or "cpu")  # noqa: E731
    out = _C.window_counts(t(pb["dt_planes"]), t(pb["dt_box"]), t(pb["gt_planes"]), t(pb["gt_box"]))
    assert all(o.dtype == torch.int32 for o in out)
    return tuple(o.cpu().numpy() for o in out)


def literal_counts(pb):
    """the definition of include/detops.h ("Cityscapes evaluation") as loops over single pixels"""
    dp, gp = pb["dt_planes"], pb["gt_planes"]
    D, G = len(dp), len(gp)
    H, W = (dp if D else gp).shape[1:]

    def count(planes, box):
        x0, y0, x1, y1 = (int(v) for v in box)
        n = 0
        for y in range(max(y0, 0), min(y1, H)):
            for x in range(max(x0, 0), min(x1, W)):
                n += int(all(p[y, x] != 0 for p in planes))
        return n

    dt_count = np.array([count([dp[d]], pb["dt_box"][d]) for d in range(D)], np.int32).reshape(D)
    gt_count = np.array([count([gp[g]], pb["gt_box"][g]) for g in range(G)], np.int32).reshape(G)
    pair_box, pair_mask = np.zeros((D, G), np.int32), np.zeros((D, G), np.int32)
    for d in range(D):
        for g in range(G):
            a, b = [int(v) for v in pb["dt_box"][d]], [int(v) for v in pb["gt_box"][g]]
            if a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]:
                pair_box[d, g] = (min(a[2], b[2]) - max(a[0], b[0])) * (min(a[3], b[3]) - max(a[1], b[1]))
                pair_mask[d, g] = count([dp[d], gp[g]], (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])))
    return dt_count, gt_count, pair_box, pair_mask


def assert_same(got, want):
    for name, a, b in zip(("dt_count", "gt_count", "pair_box", "pair_mask"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype == np.int32, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), "%s: %d of %d differ" % (name, int((a != b).sum()), a.size)


# ------------------------------------------------------------------------------------------------ a Cityscapes tree
def write_tree(root, fx, images=3, size=(56, 40)):
    """leftImg8bit/<split>/<city>/*_leftImg8bit.png and gtFine/<split>/<city>/*_instanceIds.png / *_polygons.json under
    `root`, for train and val: image 0 carries the fixture's id map and polygon json, image 1 has no instances, the others a
    shifted copy of the id map -> (img_dir, ann_dir)"""
    from PIL import Image

    w, h = size
    id_map = fx["id_map"].astype(np.int32)
    assert id_map.shape == (h, w)
    poly = json.loads(fx["poly_json"].tobytes().decode())
    rng = np.random.RandomState(3)
    for split in ("train", "val"):
        for k in range(images):
            city = ("aachen", "bochum", "cologne", "dusseldorf")[k % 4]              # sorted by path = by k
            stem = "%s_%06d_000019" % (city, k)
            img_dir, ann_dir = os.path.join(root, "leftImg8bit", split, city), os.path.join(root, "gtFine", split, city)
            os.makedirs(img_dir, exist_ok=True)
            os.makedirs(ann_dir, exist_ok=True)
            Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(img_dir, stem + "_leftImg8bit.png"))
            ids = id_map if k == 0 else (np.full_like(id_map, 7) if k == 1 else np.roll(id_map, 2 * k, axis=1))
            Image.fromarray(ids.astype(np.uint16)).save(os.path.join(ann_dir, stem + "_gtFine_instanceIds.png"))
            ann = dict(poly) if k != 1 else dict(poly, objects=[o for o in poly["objects"] if o["label"] == "road"])
            with open(os.path.join(ann_dir, stem + "_gtFine_polygons.json"), "w") as f:
                json.dump(ann, f)
    return os.path.join(root, "leftImg8bit"), os.path.join(root, "gtFine")
