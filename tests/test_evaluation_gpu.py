"""Detection evaluation on the device (csrc/evaluate.hip) against the numpy path (_eval_cpu.py) on the same inputs: integer
and match outputs exactly, fp64 IoU bit for bit.  The shapes are the smallest at which the kernels can go wrong."""
import os

import numpy as np
import pytest
import torch

import eval_cases as C
from maskrcnn_benchmark import _eval_cpu as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voc_eval_reference.npz")
IOU_THRS = np.linspace(0.5, 0.95, 10)
AREA_RNGS = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)


def offsets(sizes):
    """[(D_p, G_p)] -> dt_offset, gt_offset int32 and iou_offset int64 (cpu tensors)"""
    D, G = np.array([s[0] for s in sizes], np.int64), np.array([s[1] for s in sizes], np.int64)
    cs = lambda v: torch.from_numpy(np.concatenate([[0], np.cumsum(v)]))  # noqa: E731
    return cs(D).to(torch.int32), cs(G).to(torch.int32), cs(D * G)


def dev(*ts):
    return [t.to(DEV) if isinstance(t, torch.Tensor) else t for t in ts]


def same_pack(got, want):
    for g, w, name in zip(got, want, ("words", "word_offset", "hw", "area", "extent")):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), name


# ------------------------------------------------------------------ pack
def plane_groups():
    """[n, H, W] groups: 7 x 1, 33 x 17 (a tail word), 64 x 80 (two words), 20 x 130 (three words, a two-pixel tail),
    5 x 64 (exactly one word); random planes with an all-zero and an all-one plane among them"""
    rng = np.random.RandomState(3)
    groups = []
    for n, H, W in ((3, 7, 1), (4, 33, 17), (3, 64, 80), (5, 20, 130), (3, 5, 64)):
        g = (rng.rand(n, H, W) < 0.3).astype(np.uint8)
        g[0] = 0
        g[1] = 1
        if n > 3:
            g[2] = 0
            g[2, H // 2, W - 1] = 7                # one pixel, in the last valid bit of the row's last word; any non-zero byte counts
        groups.append(torch.from_numpy(g))
    return groups


def test_pack_matches_numpy_for_every_word_shape():
    from maskrcnn_benchmark import _C

    groups = plane_groups()
    want = _C.mask_pack(groups)                                   # CPU tensors: the numpy path
    assert want[3][1].item() == 7 and want[4][0].tolist() == [7, -1, 1, -1]        # all-one 7 x 1, all-zero 7 x 1
    same_pack(_C.mask_pack([g.to(DEV) for g in groups]), want)   # a launch per tensor
    same_pack(_C.mask_pack([g.to(DEV).bool() for g in groups]), want)
    # planes of different sizes as views of ONE buffer: one launch
    flat = torch.cat([g.reshape(-1) for g in groups]).to(DEV)
    views, k = [], 0
    for g in groups:
        views.append(flat[k:k + g.numel()].view(g.shape))
        k += g.numel()
    same_pack(_C.mask_pack(views), want)
    # bits at or beyond W are zero
    words, word_offset, hw, area, _ = want
    w = words.numpy().view(np.uint64)
    for n in range(hw.shape[0]):
        H, W = hw[n].tolist()
        WW = (W + 63) // 64
        if W % 64:
            last = w[int(word_offset[n]):int(word_offset[n]) + H * WW].reshape(H, WW)[:, -1]
            assert not (last >> np.uint64(W % 64)).any()


def test_pack_of_no_planes():
    from maskrcnn_benchmark import _C

    out = _C.mask_pack([torch.zeros((0, 9, 70), dtype=torch.uint8, device=DEV)])
    assert [tuple(t.shape) for t in out] == [(0,), (0,), (0, 2), (0,), (0, 4)]
    out = _C.mask_pack([torch.zeros((2, 0, 5), dtype=torch.uint8, device=DEV)])           # planes without pixels
    assert out[0].numel() == 0 and out[3].tolist() == [0, 0] and out[4].tolist() == [[0, -1, 1, -1]] * 2


# ------------------------------------------------------------------ pair counts
def test_pair_counts_disjoint_identical_tail_bit_and_empty_problems():
    from maskrcnn_benchmark import _C

    rng = np.random.RandomState(4)
    H, W = 20, 130
    a = np.zeros((6, H, W), np.uint8)
    a[0, 2:6, 3:40] = 1                    # far from a[1]: disjoint extents
    a[1, 12:18, 70:129] = 1
    a[2] = rng.rand(H, W) < 0.4
    a[3, 7, 129] = 1                       # the last bit of the tail word ...
    a[4, 0:10, 100:130] = 1                # ... shared with this one only at (7, 129)
    a[4, 7, 100:129] = 0
    a[5] = 0
    b = np.zeros((3, 33, 17), np.uint8)    # a second image
    b[:] = rng.rand(3, 33, 17) < 0.5
    dt_planes = [torch.from_numpy(a[[0, 2, 3, 5]]), torch.from_numpy(b[:2])]     # sorted order: 4 + 2 detections
    gt_planes = [torch.from_numpy(a[[1, 2, 4]]), torch.from_numpy(b[1:])]        # 3 + 2 ground truths
    # problems: (4 x 3) on image one; D = 0; G = 0; (1 x 2) on image two
    sizes = [(4, 3), (0, 0), (1, 0), (1, 2)]
    offs = offsets(sizes)
    total = int(offs[2][-1])

    def run(where):
        dp = _C.mask_pack([t.to(where) for t in dt_planes])
        gp = _C.mask_pack([t.to(where) for t in gt_planes])
        pick = lambda p: (p[0], p[1], p[2], p[4])  # noqa: E731
        return _C.mask_pair_counts(pick(dp), pick(gp), *[o.to(where) for o in offs], total).cpu()

    want = run("cpu")
    brute = [int((d.bool() & g.bool()).sum()) for d in dt_planes[0] for g in gt_planes[0]]
    brute += [int((dt_planes[1][1].bool() & g.bool()).sum()) for g in gt_planes[1]]
    assert want.tolist() == brute
    assert brute[0] == 0 and brute[4] == int(a[2].sum()) and brute[8] == 1
    got = run(DEV)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    # problems with D_p = 0 or G_p = 0 only
    offs0 = offsets([(0, 2), (3, 0)])
    dp, gp = _C.mask_pack([dt_planes[0][:3].to(DEV)]), _C.mask_pack([gt_planes[0][:2].to(DEV)])
    out = _C.mask_pair_counts((dp[0], dp[1], dp[2], dp[4]), (gp[0], gp[1], gp[2], gp[4]), *dev(*offs0), 0)
    assert out.numel() == 0


# ------------------------------------------------------------------ IoU
def test_iou_modes_bit_for_bit():
    from maskrcnn_benchmark import _C

    rng = np.random.RandomState(5)
    sizes = [(5, 4), (0, 3), (7, 1), (2, 0), (70, 3)]
    offs = offsets(sizes)
    Dt, Gt, total = int(offs[0][-1]), int(offs[1][-1]), int(offs[2][-1])
    crowd = torch.from_numpy((rng.rand(Gt) < 0.4).astype(np.uint8))
    # segm: counts consistent with the areas; an empty detection against a crowd and an empty pair: a union of 0
    dt_area = torch.from_numpy(rng.randint(0, 5000, Dt).astype(np.int32))
    gt_area = torch.from_numpy(rng.randint(0, 5000, Gt).astype(np.int32))
    dt_area[0], gt_area[0], crowd[1] = 0, 0, 1
    d_idx, g_idx = E._pairs(offs[0].numpy(), offs[1].numpy(), offs[2].numpy())
    counts = torch.from_numpy((rng.rand(total) * np.minimum(dt_area.numpy()[d_idx], gt_area.numpy()[g_idx])).astype(np.int32))
    kw = dict(counts=counts, dt_area=dt_area, gt_area=gt_area, gt_crowd=crowd)
    want = _C.eval_iou(_C.EVAL_COCO_SEGM, *offs, total, **kw)
    assert want[0] == 0 and want[1] == 0 and torch.isfinite(want).all() and want.max() <= 1
    got = _C.eval_iou(_C.EVAL_COCO_SEGM, *dev(*offs), total, **{k: v.to(DEV) for k, v in kw.items()})
    assert got.dtype == torch.float64 and torch.equal(got.cpu().view(torch.int64), want.view(torch.int64))
    # boxes: fractional coordinates, copies (IoU 1), integer ties, degenerate boxes (a union of 0 in the VOC form)
    xy = rng.uniform(0, 60, (Gt, 2))
    gt_boxes = np.concatenate([xy, xy + rng.uniform(1, 50, (Gt, 2))], 1).astype(np.float32)
    dt_boxes = (gt_boxes[rng.randint(0, Gt, Dt)] + rng.uniform(-8, 8, (Dt, 4))).astype(np.float32)
    dt_boxes[1], gt_boxes[0] = gt_boxes[1], [3, 5, 22, 14]
    dt_boxes[2] = [3, 5, 12, 14]
    dt_boxes[3], gt_boxes[2] = [5, 5, 3, 3], [5, 5, 3, 3]
    kw = dict(dt_boxes=torch.from_numpy(dt_boxes), gt_boxes=torch.from_numpy(gt_boxes), gt_crowd=crowd)
    for mode in (_C.EVAL_COCO_BBOX, _C.EVAL_VOC):
        want = _C.eval_iou(mode, *offs, total, **kw)
        assert torch.isfinite(want).all() and want.min() >= 0 and want.max() <= 1 and (want > 0.3).any()
        got = _C.eval_iou(mode, *dev(*offs), total, **{k: v.to(DEV) for k, v in kw.items()})
        assert torch.equal(got.cpu().view(torch.int64), want.view(torch.int64)), mode
    assert want[3 * 4 + 2] == 0                                   # VOC, two boxes without area: 0, not 0 / 0


def test_voc_fixture_on_the_device():
    """the fixture's boxes: IoU bit for bit against the numpy path; match values, prec, rec and both APs as the reference's"""
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.data.datasets.evaluation.coco_style import build_problems

    fx = np.load(GOLDEN)
    preds, gts = C.voc_boxlists(fx, DEV)
    C.check_voc_fixture(fx, preds, gts)
    i64 = lambda v: torch.from_numpy(np.asarray(v, np.int64))  # noqa: E731
    img = torch.arange(len(preds))
    dt_img, gt_img = img.repeat_interleave(i64(fx["pred_counts"])), img.repeat_interleave(i64(fx["gt_counts"]))
    pr = build_problems(dt_img, i64(fx["pred_labels"]), torch.from_numpy(fx["pred_scores"]), gt_img, i64(fx["gt_labels"]), 8,
                        max_dets=10 ** 6)
    offs = (pr["dt_offset"], pr["gt_offset"], pr["iou_offset"])
    kw = dict(dt_boxes=torch.from_numpy(fx["pred_boxes"])[pr["dt_order"]], gt_boxes=torch.from_numpy(fx["gt_boxes"])[pr["gt_order"]])
    want = _C.eval_iou(_C.EVAL_VOC, *offs, pr["total_pairs"], **kw)
    got = _C.eval_iou(_C.EVAL_VOC, *dev(*offs), pr["total_pairs"], **{k: v.to(DEV) for k, v in kw.items()})
    assert (want == 0.5).sum() >= 6 and torch.equal(got.cpu().view(torch.int64), want.view(torch.int64))


# ------------------------------------------------------------------ match
def match_inputs(sizes, seed):
    """random problems: IoUs on a grid of 0.05 (ties, values exactly at the thresholds), 25 % crowd, areas on both sides
    of 32^2 and 96^2"""
    rng = np.random.RandomState(seed)
    offs = offsets(sizes)
    Dt, Gt, total = int(offs[0][-1]), int(offs[1][-1]), int(offs[2][-1])
    grid = np.concatenate([IOU_THRS, np.arange(0, 10) * 0.05, [1.0]])
    iou = torch.from_numpy(np.where(rng.rand(total) < 0.6, 0.0, grid[rng.randint(0, grid.size, total)]))
    flag = torch.from_numpy((rng.rand(Gt) < 0.25).astype(np.uint8))
    areas = np.array([10.0, 1024.0, 1024.5, 5000.0, 9216.0, 9217.0, 20000.0])
    dt_area = torch.from_numpy(areas[rng.randint(0, areas.size, Dt)])
    gt_area = torch.from_numpy(areas[rng.randint(0, areas.size, Gt)])
    return offs, (Dt, Gt, max([g for _, g in sizes] + [0])), iou, flag, dt_area, gt_area


def run_match(mode, where, offs, counts_host, iou, flag, dt_area, gt_area, thrs, rngs):
    from maskrcnn_benchmark import _C

    mv = lambda t: t.to(where)  # noqa: E731
    out = _C.eval_match(mode, mv(iou), *[mv(o) for o in offs], counts_host, mv(flag), thrs, dt_area=mv(dt_area),
                        gt_area=mv(gt_area), area_rngs=rngs)
    return [out.cpu()] if mode == _C.EVAL_VOC else [o.cpu() for o in out]


SHAPES = {
    "registers": [(1, 1), (100, 64), (3, 0), (0, 5), (100, 1), (7, 33)],             # every G_p <= 64: no LDS
    "lds": [(1, 1), (100, 65), (1, 64), (0, 70), (5, 200), (100, 64)],              # 65: the first size in LDS
    "cap": [(1, 4096), (2, 3)],                                                      # the largest G_p served
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("lanes", ["4x10", "1x1", "4x20"])
def test_match_equals_numpy(shape, lanes):
    from maskrcnn_benchmark import _C

    inputs = match_inputs(SHAPES[shape], seed=len(shape))
    # 4 x 20 = 80 lanes: the wave goes through the lanes in two rounds (the second one partly idle)
    thrs, rngs = {"4x10": (IOU_THRS, AREA_RNGS), "1x1": (IOU_THRS[2:3], AREA_RNGS[2:3]),
                  "4x20": (np.linspace(0.025, 0.975, 20), AREA_RNGS)}[lanes]
    for mode in (_C.EVAL_COCO_SEGM, _C.EVAL_VOC):
        want = run_match(mode, "cpu", *inputs, thrs, rngs)
        got = run_match(mode, DEV, *inputs, thrs, rngs)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (shape, lanes, mode)
        if mode == _C.EVAL_VOC:
            assert set(want[0].tolist()) <= {-1, 0, 1}
        elif shape != "cap":
            assert (want[0] >= 0).any() and (want[0] < 0).any() and want[1].any() and want[2].any()


def test_match_hand_cases():
    """the `break` (a non-ignored match is held when the first ignored ground truth comes up), the re-match of a crowd, and
    an IoU exactly at a threshold; one detection row each unless said otherwise"""
    from maskrcnn_benchmark import _C

    sizes = [(1, 2), (2, 1), (1, 1)]
    offs = offsets(sizes)
    #            break: g0 better but large (ignored in 'small'), g1 small    crowd: both detections    exactly 0.5
    iou = torch.tensor([0.9, 0.6, 0.8, 0.8, 0.5], dtype=torch.float64)
    gt_area = torch.tensor([20000.0, 100.0, 100.0, 100.0], dtype=torch.float64)
    flag = torch.tensor([0, 0, 1, 0], dtype=torch.uint8)
    dt_area = torch.tensor([100.0, 100.0, 100.0, 100.0], dtype=torch.float64)
    rngs = AREA_RNGS[:2]                                                     # all, small
    thrs = np.array([0.5, 0.55])
    for where in ("cpu", DEV):
        dtm, dti, gti = run_match(_C.EVAL_COCO_SEGM, where, offs, (4, 4, 2), iou, flag, dt_area, gt_area, thrs, rngs)
        assert dtm[0, 0, 0] == 0 and dti[0, 0, 0] == 0                     # all: the better ground truth
        assert dtm[1, 0, 0] == 1 and dti[1, 0, 0] == 0                     # small: the walk stops in front of the ignored one
        assert gti.tolist() == [[0, 0, 1, 0], [1, 0, 1, 0]]
        assert dtm[0, 0, 1:3].tolist() == [0, 0] and dti[0, 0, 1:3].tolist() == [1, 1]      # the crowd is matched twice
        assert dtm[0, 0, 3] == 0 and dtm[0, 1, 3] == -1                     # 0.5 >= 0.5, 0.5 < 0.55


def test_more_ground_truths_than_the_cap_take_the_host_path():
    from maskrcnn_benchmark import _C, _lib

    sizes = [(2, 5), (1, _C.EVAL_MAX_GT + 1), (3, 70)]
    inputs = match_inputs(sizes, seed=9)
    offs, counts_host, iou, flag, dt_area, gt_area = inputs
    for mode in (_C.EVAL_COCO_BBOX, _C.EVAL_VOC):
        want = run_match(mode, "cpu", *inputs, IOU_THRS, AREA_RNGS)
        got = run_match(mode, DEV, *inputs, IOU_THRS, AREA_RNGS)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    # the entry point's own code: not DETOPS_EINVAL
    d = dev(iou, *offs, flag, torch.from_numpy(IOU_THRS))
    out = torch.zeros((counts_host[0],), dtype=torch.int8, device=DEV)
    args = [_C.EVAL_VOC, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(sizes), counts_host[0],
            counts_host[1], counts_host[2], None, None, d[4].data_ptr(), d[5].data_ptr(), 1, None, 0, None, None, None,
            out.data_ptr(), _lib.stream_of(out)]
    rc = _lib.lib.detops_eval_match(*args)
    torch.cuda.synchronize()
    assert rc == -4
    args[11] = None                                   # the flags are needed: G_total > 0
    assert _lib.lib.detops_eval_match(*args) == -1


# ------------------------------------------------------------------ evaluator
@pytest.fixture(scope="module")
def cpu_run():
    from maskrcnn_benchmark.data.datasets.evaluation import COCOStyleEvaluator

    images = C.make_images()
    ev = COCOStyleEvaluator(("bbox", "segm"), C.NUM_CLASSES)
    ev.update(*C.to_boxlists(images))
    ev.summarize()
    return images, ev


def same_evaluation(a, b):
    for iou_type in b.iou_types:
        ra, rb = C.records_by_key(a, iou_type), C.records_by_key(b, iou_type)
        assert sorted(ra) == sorted(rb)
        for key in rb:
            for field in ("scores", "dt_match", "dt_ignore", "gt_ignore"):
                np.testing.assert_array_equal(ra[key][field], rb[key][field], err_msg="%s %s %s" % (iou_type, key, field))
        np.testing.assert_array_equal(a.stats[iou_type], b.stats[iou_type])


def test_evaluator_on_the_device_equals_the_cpu_path(cpu_run):
    from maskrcnn_benchmark.data.datasets.evaluation import COCOStyleEvaluator

    images, want = cpu_run
    preds, tgts = C.to_boxlists(images, DEV)
    ev = COCOStyleEvaluator(("bbox", "segm"), C.NUM_CLASSES)
    ev.update(preds[:5], tgts[:5])
    ev.update(preds[5:], tgts[5:])
    ev.summarize()
    same_evaluation(ev, want)
    assert 0 < ev.stats["segm"][0] < 1


def test_evaluator_pastes_mask_probabilities_itself(cpu_run):
    """predictions with M = 28 probabilities: the evaluator runs Masker(0.5, padding 1) on the device; its result equals the
    evaluation of those pasted planes handed over as dense planes (on the CPU path)"""
    from maskrcnn_benchmark.data.datasets.evaluation import COCOStyleEvaluator
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import Masker

    images, _ = cpu_run
    preds, tgts = C.to_boxlists(images, DEV)
    g = torch.Generator().manual_seed(2)
    for p in preds:
        p.add_field("mask", torch.sigmoid(3 * torch.randn(len(p), 1, 28, 28, generator=g)).to(DEV))
    ev = COCOStyleEvaluator(("segm",), C.NUM_CLASSES)
    ev.update(preds, tgts)
    ev.summarize()
    pasted = Masker(threshold=0.5, padding=1)([p.get_field("mask") for p in preds], preds)
    cpu_preds, cpu_tgts = C.to_boxlists(images)
    for p, m in zip(cpu_preds, pasted):
        p.add_field("mask", m.cpu())
    want = COCOStyleEvaluator(("segm",), C.NUM_CLASSES)
    want.update(cpu_preds, cpu_tgts)
    want.summarize()
    same_evaluation(ev, want)
    assert any(r["dt_match"].max() >= 0 for r in ev.records["segm"])
