"""Shared by tests/test_box_proposals_cpu.py and tests/test_box_proposals_gpu.py: the fixture the reference's
evaluate_box_proposals wrote (tests/golden/box_proposals_reference.npz, made by tests/golden/make_golden_box_proposals.py) as
BoxLists and a dataset, seeded problems for `_C.eval_proposal_overlaps` at the shapes where the kernel can go wrong, and the
matching as literal Python loops; and the kernel under the host emulation (tests/emu_proposals: the emulation library of
tests/emu does not hold csrc/eval_proposals.hip)."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import torch

from maskrcnn_benchmark import _C, _abi
from maskrcnn_benchmark.structures.bounding_box import BoxList

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_proposals_reference.npz")
LIMITS = (None, 3, 100, 1000)
AREAS = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")


_EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_proposals")
_EMU = None


def emu_proposals_lib():
    """csrc/eval_proposals.hip compiled as host C++ over the fiber emulation (tests/emu/hip_cpu_emu.h), built when needed
    and bound from the table the device build is bound from (maskrcnn_benchmark/_abi.py)"""
    global _EMU
    if _EMU is None:
        subprocess.check_call(["make", "-s", "-C", _EMU_DIR])
        _EMU = ctypes.CDLL(os.path.join(_EMU_DIR, "libdetops_emu_proposals.so"))
        assert _abi.bind(_EMU, require_all=False) == {"detops_eval_proposal_overlaps"}
    return _EMU


class _WithProposals(object):
    """the emulation library of tests/emu, with detops_eval_proposal_overlaps from emu_proposals_lib()"""

    def __init__(self, base):
        self._base = base
        self.detops_eval_proposal_overlaps = emu_proposals_lib().detops_eval_proposal_overlaps

    def __getattr__(self, name):
        return getattr(self._base, name)


@contextlib.contextmanager
def emulated():
    """cpu_shim's "emu-lib" backend (the product's own `_C` wrappers on CPU tensors take their device branches over the
    emulation library) with the emulated proposal kernel added to the library handle"""
    import cpu_shim

    with cpu_shim.install("emu-lib"):
        base = _C.lib
        _C.lib = _WithProposals(base)
        try:
            yield _C.lib
        finally:
            _C.lib = base


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


class FixtureDataset(object):
    """the fixture's ground truth as the test loader hands it out: get_groundtruth(i) -> BoxList with labels, iscrowd, area"""

    def __init__(self, fx):
        self.sizes = [tuple(int(v) for v in s) for s in fx["sizes"]]
        self.targets, g = [], 0
        for i, n in enumerate(fx["gt_counts"]):
            t = BoxList(torch.from_numpy(fx["gt_xywh"][g:g + n]).reshape(-1, 4), self.sizes[i], mode="xywh").convert("xyxy")
            t.add_field("labels", torch.ones((int(n),), dtype=torch.int64))
            t.add_field("iscrowd", torch.from_numpy(fx["gt_iscrowd"][g:g + n]))
            t.add_field("area", torch.from_numpy(fx["gt_area"][g:g + n]))
            self.targets.append(t)
            g += n

    def __len__(self):
        return len(self.targets)

    def get_groundtruth(self, index):
        return self.targets[index]

    def get_img_info(self, index):
        return {"width": self.sizes[index][0], "height": self.sizes[index][1]}


def fixture_predictions(fx, device="cpu"):
    """the proposals as the reference got them: at their own size, objectness not sorted"""
    out, d = [], 0
    for i, n in enumerate(fx["pred_counts"]):
        p = BoxList(torch.from_numpy(fx["pred_boxes"][d:d + n]).reshape(-1, 4), tuple(int(v) for v in fx["pred_sizes"][i]))
        p.add_field("objectness", torch.from_numpy(fx["pred_objectness"][d:d + n]))
        out.append(p.to(device))
        d += n
    return out


def reference_call(fx, limit, area):
    key = "%d/%s/" % (limit or 0, area)
    return {k: fx[key + k] for k in ("ar", "recalls", "num_pos", "gt_overlaps")}


# ------------------------------------------------------------------------------------------------ problems for the operator
def _boxes(rng, n, extent=300.0):
    x1, y1 = rng.uniform(0, extent, n), rng.uniform(0, extent, n)
    return np.stack([x1, y1, x1 + rng.uniform(4, 90, n), y1 + rng.uniform(4, 90, n)], 1).astype(np.float32).reshape(-1, 4)


def random_problem(seed, shapes, limits=(0, 3, 100), A=3, dead_range=True):
    """shapes: [(P, G)] per image -> the arguments of _C.eval_proposal_overlaps as numpy arrays.  Half of the proposals are
    jittered ground truths; range 0 counts every ground truth, the others a random half, the last none (`dead_range`)."""
    rng = np.random.RandomState(seed)
    dt, gt = [], []
    for P, G in shapes:
        g = _boxes(rng, G)
        d = _boxes(rng, P)
        if G and P:
            k = rng.randint(0, G, P)
            near = g[k] + rng.uniform(-9, 9, (P, 4)).astype(np.float32)
            near[:, 2:] = np.maximum(near[:, 2:], near[:, :2] + 1)
            d = np.where((rng.rand(P) < 0.5)[:, None], near, d).astype(np.float32)
        dt.append(d)
        gt.append(g)
    G_total = sum(G for _, G in shapes)
    valid = rng.rand(A, G_total) < 0.5
    valid[0] = True
    if dead_range and A > 1:
        valid[-1] = False
    return {"dt_boxes": np.concatenate(dt).reshape(-1, 4), "gt_boxes": np.concatenate(gt).reshape(-1, 4),
            "dt_offset": np.cumsum([0] + [P for P, _ in shapes]).astype(np.int32),
            "gt_offset": np.cumsum([0] + [G for _, G in shapes]).astype(np.int32), "gt_valid": valid.astype(np.uint8),
            "limits": np.asarray(limits, np.int32)}


def nested_problem(G=65, P=70):
    """G equal ground truths side by side, every proposal a box around all of them, each larger than the one before: every
    ground truth prefers proposal 0, then proposal 1, ... so EVERY round scans every open column again, and all the
    ground truths tie in every round (equal areas, integer boxes)."""
    gt = np.array([[100 + 6 * (k % 9), 100 + 6 * (k // 9), 104 + 6 * (k % 9), 104 + 6 * (k // 9)] for k in range(G)], np.float32)
    dt = np.array([[100 - k, 100 - k, 160 + k, 160 + k] for k in range(P)], np.float32)
    return {"dt_boxes": dt, "gt_boxes": gt, "dt_offset": np.array([0, P], np.int32), "gt_offset": np.array([0, G], np.int32),
            "gt_valid": np.ones((1, G), np.uint8), "limits": np.array([0, 7], np.int32)}


def tie_problem():
    """the fixture's built ties as three images (tests/golden/make_golden_box_proposals.py): two proposals tied at 0.5 for
    ground truth 0, in both orders, and two ground truths tied at 0.5 for proposal 0.  -> (problem, the overlaps the
    first-maximum rule gives, per ground truth)"""
    f = lambda rows: np.array(rows, np.float32)  # noqa: E731
    top, bottom = [20, 30, 29, 34], [20, 35, 29, 39]
    gts_a = [[20, 30, 29, 39], [20, 38, 29, 47]]
    gts_b, shared, lo, hi = [[20, 30, 29, 39], [20, 35, 29, 44]], [20, 35, 29, 39], [20, 30, 29, 32], [20, 41, 29, 44]
    dt = f([top, bottom] + [bottom, top] + [shared, lo, hi])
    gt = f(gts_a + gts_a + gts_b)
    pb = {"dt_boxes": dt, "gt_boxes": gt, "dt_offset": np.array([0, 2, 4, 7], np.int32), "gt_offset": np.array([0, 2, 4, 6], np.int32),
          "gt_valid": np.ones((1, 6), np.uint8), "limits": np.array([0], np.int32)}
    small = np.float32(20) / np.float32(130)
    return pb, f([0.5, small, 0.5, 0.0, 0.5, 0.4])


def run_op(pb, device=None, **kw):
    """_C.eval_proposal_overlaps on `device` (None: the CPU tensors, i.e. the numpy path unless _C is patched) -> numpy"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device or "cpu")  # noqa: E731
    out = _C.eval_proposal_overlaps(t(pb["dt_boxes"]), t(pb["gt_boxes"]), t(pb["dt_offset"]), t(pb["gt_offset"]), t(pb["gt_valid"]),
                                    [int(v) for v in pb["limits"]], **kw)
    return out.cpu().numpy()


def literal_overlaps(pb):
    """the definition of include/detops.h ("Proposal recall") as loops over single fp32 numbers"""
    f = np.float32

    def iou(p, g):
        area_p = f(f(f(p[2] - p[0]) + f(1)) * f(f(p[3] - p[1]) + f(1)))
        area_g = f(f(f(g[2] - g[0]) + f(1)) * f(f(g[3] - g[1]) + f(1)))
        w = max(f(f(min(p[2], g[2]) - max(p[0], g[0])) + f(1)), f(0))
        h = max(f(f(min(p[3], g[3]) - max(p[1], g[1])) + f(1)), f(0))
        inter = f(w * h)
        return f(inter / f(f(area_p + area_g) - inter))

    L, (A, G_total) = len(pb["limits"]), pb["gt_valid"].shape
    out = np.zeros((L, A, G_total), np.float32)
    for n in range(len(pb["dt_offset"]) - 1):
        d0, d1, g0, g1 = pb["dt_offset"][n], pb["dt_offset"][n + 1], pb["gt_offset"][n], pb["gt_offset"][n + 1]
        for li, limit in enumerate(pb["limits"]):
            P = min(d1 - d0, limit) if limit > 0 else d1 - d0
            for a in range(A):
                open_g = [g for g in range(g0, g1) if pb["gt_valid"][a, g]]
                open_p = list(range(d0, d0 + P))
                for g in range(g0, g1):
                    out[li, a, g] = 0 if pb["gt_valid"][a, g] else -1
                for _ in range(min(len(open_g), len(open_p))):
                    best = None                                       # (value, g, p): the first maximum at both levels
                    for g in open_g:
                        col = None
                        for p in open_p:
                            v = iou(pb["dt_boxes"][p], pb["gt_boxes"][g])
                            if col is None or v > col[0]:
                                col = (v, g, p)
                        if best is None or col[0] > best[0]:
                            best = col
                    out[li, a, best[1]] = best[0]
                    open_g.remove(best[1])
                    open_p.remove(best[2])
    return out
