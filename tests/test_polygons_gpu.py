"""Polygon masks on the device (csrc/polygon.hip) against the literal restatement of the definition (tests/poly_refs.py),
after the geometry that tests/golden/polygons_reference.npz pins.  Everything is exact: the kernels' output is 0 / 1."""
import math
import os

import numpy as np
import pytest
import torch

import poly_refs as R
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.segmentation_mask import PolygonList, SegmentationMask

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polygons_reference.npz")


def device_targets(lists, slot_list, M, raw_abi=False):
    """slot_list: (image index, instance index in that image, box) -> [S, M, M] float32 (cpu) from ONE launch"""
    from maskrcnn_benchmark import _C, _lib

    packed = PolygonList.pack(lists).to(DEV)
    inst = torch.tensor([packed.inst_base[i] + g for i, g, _ in slot_list], dtype=torch.int64).reshape(-1).to(DEV)
    boxes = torch.tensor([[float(v) for v in b] for _, _, b in slot_list], dtype=torch.float32).reshape(-1, 4).to(DEV)
    wh = torch.tensor([lists[i].size for i, _, _ in slot_list], dtype=torch.int32).reshape(-1, 2).to(DEV)
    if not raw_abi:
        return _C.polygon_mask_targets(packed.verts, packed.poly_offset, packed.inst_offset, inst, boxes, wh, M).cpu()
    S = len(slot_list)
    out = torch.full((S, M, M), -7.0, dtype=torch.float32, device=DEV)      # a sentinel: every element must be written
    rc = _lib.lib.detops_polygon_mask_targets(packed.verts.data_ptr(), packed.poly_offset.data_ptr(),
                                              packed.inst_offset.data_ptr(), packed.V, packed.P, packed.G, inst.data_ptr(),
                                              boxes.data_ptr(), wh.data_ptr(), S, M, out.data_ptr(), _lib.stream_of(out))
    assert rc == 0
    return out.cpu()


def literal_targets(lists, slot_list, M):
    return np.stack([R.slot_target(lists[i].polygons[g], torch.tensor([float(v) for v in b], dtype=torch.float32), M)
                     for i, g, b in slot_list]).astype(np.float32)


@pytest.fixture(scope="module")
def fixture_slots():
    """the fixture's two images (different (W, H)) and their boxes, grown to 67 slots by jittered copies"""
    fx = np.load(GOLDEN)
    lists, slot_list = [], []
    for i in range(2):
        raw, size, boxes, box_inst = R.fixture_image(fx, i)
        lists.append(PolygonList(raw, size))
        slot_list.extend((i, int(g), b.tolist()) for b, g in zip(boxes, box_inst))
    rng = np.random.RandomState(5)
    base = list(slot_list)
    while len(slot_list) < 67:
        i, g, b = base[len(slot_list) % len(base)]
        j = rng.uniform(-2.5, 2.5, 4)
        b = [b[0] + j[0], b[1] + j[1], max(b[2] + j[2], b[0] + j[0]), max(b[3] + j[3], b[1] + j[1])]
        slot_list.append((i, (g + 1) % len(lists[i]), np.float32(b).tolist()))
    return lists, slot_list


@pytest.mark.parametrize("M", (28, 14, 7))
def test_targets_equal_the_restatement_on_the_fixture_geometry(fixture_slots, M):
    lists, slot_list = fixture_slots
    assert len(slot_list) == 67 and {i for i, _, _ in slot_list} == {0, 1}
    want = literal_targets(lists, slot_list, M)
    got = device_targets(lists, slot_list, M)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(device_targets(lists, slot_list, M, raw_abi=True).numpy(), want)
    assert np.array_equal(device_targets(lists, slot_list[3:4], M).numpy(), want[3:4])          # S = 1
    assert tuple(device_targets(lists, [], M).shape) == (0, M, M)                               # S = 0


def big_shapes():
    """an 800-pixel image with: a triangle, a 300-gon, three overlapping polygons, a polygon with repeated vertices, and
    an 800-pixel quadrilateral (few edges: the restatement walks its upsampled boundary point by point)"""
    rng = np.random.RandomState(9)
    a = np.arange(300) * (2 * math.pi / 300)
    r = 260 + 25 * rng.uniform(-1, 1, 300)
    gon = np.stack([400 + r * np.cos(a), 390 + r * np.sin(a)], axis=1).reshape(-1).tolist()
    tri = [100.25, 120.5, 700.75, 180.0, 350.5, 690.25]
    three = [[200.0, 200.0, 420.5, 210.0, 410.0, 430.5, 190.5, 400.0], [350.0, 330.0, 600.0, 350.5, 560.5, 620.0, 330.0, 580.0],
             [280.0, 150.0, 520.0, 300.0, 300.0, 560.0]]
    rep = [150.0, 150.0, 150.0, 150.0, 650.0, 160.0, 650.0, 160.0, 650.0, 160.0, 640.0, 650.0, 140.0, 640.0, 150.0, 150.0]
    quad = [0.5, 1.25, 799.0, 0.75, 798.5, 799.25, 1.0, 798.0]
    return PolygonList([[tri], [gon], three, [rep], [quad]], (800, 800))


BIG_SLOTS = [
    (0, 0, (90.3, 110.2, 710.1, 700.7)),           # the triangle in its box
    (0, 0, (330.0, 300.0, 370.0, 340.0)),          # a box inside the triangle: all ones
    (0, 0, (720.0, 700.0, 790.0, 790.0)),          # a box that misses the triangle: all zeros
    (0, 1, (100.5, 90.25, 700.0, 690.5)),          # 300 vertices: more than a wave, more than one LDS chunk of edges
    (0, 1, (380.2, 100.9, 640.4, 333.3)),
    (0, 2, (180.0, 140.0, 610.0, 630.0)),          # three overlapping polygons
    (0, 2, (340.5, 320.5, 430.25, 440.75)),
    (0, 3, (130.0, 140.0, 660.0, 660.0)),          # repeated vertices
    (0, 4, (400.2, 300.6, 401.2, 301.6)),          # a 1-pixel box inside an 800-pixel polygon
    (0, 1, (-30.0, 200.0, 300.0, 500.0)),          # clamped at the left, top, right and bottom border
    (0, 1, (200.0, -12.5, 500.0, 300.0)),
    (0, 1, (500.0, 200.0, 830.5, 500.0)),
    (0, 1, (200.0, 500.0, 500.0, 845.0)),
    (0, 4, (805.0, 10.0, 820.0, 30.0)),            # right of the image: xmin clamped to W - 1
]


@pytest.fixture(scope="module")
def big_reference():
    lists = [big_shapes()]
    return lists, literal_targets(lists, BIG_SLOTS, 28)


def test_targets_of_large_instances_and_extreme_boxes(big_reference):
    lists, want = big_reference
    assert want[1].all() and not want[2].any() and want[8].all()
    assert 0.2 < want[3].mean() < 0.9 and 0.2 < want[5].mean() < 0.95 and all(0.1 < want[s].mean() < 0.9 for s in (9, 10, 11, 12))
    got = device_targets(lists, BIG_SLOTS, 28).numpy()
    bad = [s for s in range(len(BIG_SLOTS)) if not np.array_equal(got[s], want[s])]
    assert not bad, bad


def edge_chunk_shapes():
    """a 200-pixel image with polygons of 3, 255, 256 and 257 edges (a chunk of 256 staged edges not full, full, and one edge
    more) and one of 258 whose long sides are 128 collinear vertices each: 254 vertical edges, which cross no column boundary
    and share their place in the chunk's work list with the next edge that does"""
    rng = np.random.RandomState(12)

    def gon(k):
        a = np.arange(k) * (2 * math.pi / k) + 0.1
        r = 80 + 6 * rng.uniform(-1, 1, k)
        return np.stack([100.3 + r * np.cos(a), 99.6 + r * np.sin(a)], axis=1).reshape(-1).tolist()

    ys = np.linspace(20.25, 180.5, 128)
    comb = [v for y in ys for v in (30.5, float(y))] + [100.0, 195.0] + [v for y in ys[::-1] for v in (169.25, float(y))] + [100.0, 5.0]
    return PolygonList([[gon(3)], [gon(255)], [gon(256)], [gon(257)], [comb]], (200, 200))


def test_polygons_around_one_chunk_of_edges_and_mostly_vertical_edges():
    plist = edge_chunk_shapes()
    assert [len(inst.polygons[0]) // 2 for inst in plist] == [3, 255, 256, 257, 258]
    lists = [plist]
    slots = [(0, g, box) for g in range(5) for box in ((10.2, 8.7, 190.4, 191.1), (60.5, 20.0, 150.25, 120.75))]
    want = literal_targets(lists, slots, 28)
    assert all(0.05 < w.mean() < 1 for w in want[::2])
    assert np.array_equal(device_targets(lists, slots, 28).numpy(), want)
    H = W = 200
    planes = np.stack([R.fill_instance([p.tolist() for p in inst.polygons], H, W) for inst in plist])
    assert all(0 < p.sum() < H * W for p in planes)
    got = SegmentationMask(plist.to(DEV), (W, H), mode="poly").get_mask_tensor().cpu().numpy()
    assert np.array_equal(got, planes)


def plane_instances(H, W):
    """five instances on an H x W image: a polygon leaving the image on each side, one inside, one with two polygons"""
    return [
        [[-0.3 * W - 2, 0.2 * H, 0.5 * W, -0.4 * H - 2, 1.3 * W + 2, 0.6 * H, 0.4 * W, 1.5 * H + 3]],
        [[0.2 * W, 0.2 * H, 0.8 * W, 0.3 * H, 0.7 * W, 0.9 * H]],
        [[0.0, 0.0, float(W), 0.0, float(W), float(H), 0.0, float(H)]],
        [[0.1 * W, 0.1 * H, 0.6 * W, 0.15 * H, 0.5 * W, 0.6 * H, 0.05 * W, 0.5 * H],
         [0.4 * W, 0.4 * H, 0.95 * W, 0.45 * H, 0.9 * W, 0.95 * H, 0.35 * W, 0.9 * H]],
        [[0.5 * W, -3.0, W + 4.0, 0.5 * H, 0.5 * W, H + 2.5, -1.5, 0.5 * H]],
    ]


@pytest.mark.parametrize("H,W", ((33, 17), (7, 1), (64, 80), (200, 333)))
def test_polygons_to_masks_equal_the_restatement(H, W):
    from maskrcnn_benchmark import _C, _lib

    plist = PolygonList(plane_instances(H, W), (W, H))
    assert len(plist) == 5
    want = np.stack([R.fill_instance([p.tolist() for p in inst.polygons], H, W) for inst in plist])
    assert want[2].all() and 0 < want[1].sum() < H * W
    seg = SegmentationMask(plist.to(DEV), (W, H), mode="poly")
    dense = seg.convert("mask")
    assert dense.mode == "mask" and dense.instances.masks.is_cuda and dense.instances.masks.dtype == torch.uint8
    assert np.array_equal(dense.instances.masks.cpu().numpy(), want)
    assert np.array_equal(seg.get_mask_tensor().cpu().numpy(), want)
    k = plist.packed().to(DEV)
    out = torch.full((5 * H * W + 32,), 9, dtype=torch.uint8, device=DEV)    # guard bytes behind the planes
    rc = _lib.lib.detops_polygons_to_masks(k.verts.data_ptr(), k.poly_offset.data_ptr(), k.inst_offset.data_ptr(), k.V, k.P,
                                           k.G, H, W, out.data_ptr(), _lib.stream_of(out))
    assert rc == 0
    out = out.cpu().numpy()
    assert np.array_equal(out[:5 * H * W].reshape(5, H, W), want) and (out[5 * H * W:] == 9).all()
    empty = PolygonList([], (W, H)).to(DEV).convert_to_binarymask()          # G = 0
    assert tuple(empty.masks.shape) == (0, H, W)
    e = PolygonList([], (W, H)).packed().to(DEV)
    assert tuple(_C.polygons_to_masks(e.verts, e.poly_offset, e.inst_offset, H, W).shape) == (0, H, W)


def test_entry_points_refuse_bad_arguments():
    from maskrcnn_benchmark import _lib

    t = torch.zeros(8, dtype=torch.int32, device=DEV)
    p, s = t.data_ptr(), _lib.stream_of(t)
    f = _lib.lib.detops_polygon_mask_targets
    assert f(p, p, p, 1, 1, 1, p, p, p, 1, 0, p, s) == -1          # M < 1
    assert f(p, p, p, 1, 1, 1, p, p, p, 1, 257, p, s) == -1        # M > 256
    assert f(p, p, p, 1, 1, 1, p, p, p, -1, 28, p, s) == -1        # S < 0
    assert f(p, p, p, 1, 1, 1, p, p, p, 1, 28, None, s) == -1      # null output
    assert f(None, None, None, 0, 0, 0, None, None, None, 0, 28, None, s) == 0
    g = _lib.lib.detops_polygons_to_masks
    assert g(p, p, p, 1, 1, 1, 3585, 8, p, s) == -1                # H beyond the LDS strip
    assert g(p, p, p, 1, 1, 1, 8, 8, None, s) == -1
    assert g(None, None, None, 0, 0, 0, 8, 8, None, s) == 0


def test_mask_loss_on_device_polygon_targets(fixture_slots):
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.loss import MaskRCNNLossComputation, project_polygons_on_boxes

    lists, slot_list = fixture_slots
    M, C = 28, 4
    proposals, targets = [], []
    for i in range(2):
        mine = [(g, b) for j, g, b in slot_list if j == i]
        p = BoxList(torch.tensor([b for _, b in mine], dtype=torch.float32), lists[i].size, mode="xyxy")
        p.add_field("matched_idxs", torch.tensor([g for g, _ in mine]))
        p.add_field("labels", torch.tensor([1 + k % (C - 1) if k % 5 else 0 for k in range(len(mine))]))
        proposals.append(p)
        t = BoxList(torch.zeros(len(lists[i]), 4), lists[i].size, mode="xyxy")
        t.add_field("masks", SegmentationMask(lists[i], lists[i].size, mode="poly"))
        targets.append(t)
    host = project_polygons_on_boxes(proposals, lists, M, torch.device("cpu"))
    dev_props = [p.to(torch.device(DEV)) for p in proposals]
    dev = project_polygons_on_boxes(dev_props, lists, M, torch.device(DEV))
    assert dev.is_cuda and torch.equal(dev.cpu(), host)                       # bit for bit
    logits = torch.randn(host.shape[0], C, M, M, generator=torch.Generator().manual_seed(4))
    x = logits.to(DEV).requires_grad_()
    loss = MaskRCNNLossComputation(None, M)(dev_props, x, [t.to(torch.device(DEV)) for t in targets])
    loss.backward()
    labels = torch.cat([p.get_field("labels") for p in proposals])
    pos = labels > 0
    ref = torch.nn.functional.binary_cross_entropy_with_logits(logits.double()[pos, labels[pos]], host.double()[pos])
    rel = abs(loss.item() - ref.item()) / abs(ref.item())
    print("FIGURE mask loss on polygon targets: relative error %.3g" % rel)
    assert rel <= max(8 * 1.02e-07, 4 * 2.0 ** -23)           # the value bound of tests/test_targets_edges_gpu.py's mask_loss
    assert torch.isfinite(x.grad).all() and not bool(x.grad[~pos].any())
