"""csrc/cityscapes_eval.hip on the device: bit for bit against the numpy twin (_eval_cpu.window_counts, pinned to the fixture
of the REFERENCE's functions and to literal loops by tests/test_cityscapes_cpu.py) at the shapes where the kernel can go
wrong, every case twice with equal bits and once more on dirtied allocator memory; the fixture through CityscapesEvaluator
on the device; and a small Mask R-CNN on a Cityscapes tree through `inference()` against the CPU path on the same
predictions.  Everything here is integers, so everything is compared exactly; the AP against the reference within 1e-12
(tests/test_cityscapes_cpu.py says why)."""
import numpy as np
import pytest
import torch

import cityscapes_cases as C
from dirty_memory import _clean_then_dirty
from maskrcnn_benchmark import _C, _eval_cpu
from maskrcnn_benchmark.data.datasets import evaluation as E
from maskrcnn_benchmark.data.datasets.evaluation import cityscapes as CE

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("dt_count", "gt_count", "pair_box", "pair_mask")


def _both(pb):
    """the device's result: equal to the numpy path's, twice with equal bits, and again on dirtied free blocks"""
    want = C.run_op(pb)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    args = [t(pb[k]) for k in ("dt_planes", "dt_box", "gt_planes", "gt_box")]

    def run():
        out = _C.window_counts(*args)
        C.assert_same(tuple(o.cpu().numpy() for o in out), want)
        return dict(zip(NAMES, out))

    _clean_then_dirty(run)
    return want


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (37, 53), (64, 64), (65, 130)])
@pytest.mark.parametrize("D,G", [(0, 0), (0, 3), (1, 0), (1, 1), (3, 65), (65, 3)])
def test_shapes_counts_and_edge_windows(H, W, D, G):
    # (37, 53): an odd plane size, so the planes of a batch start unaligned; D, G in 0, 1, 3, 65; the edge windows: width 1,
    # height 1, empty, the whole plane, the right and bottom edges, every column residue modulo 16, outside the image, pairs
    # that only touch; then drawn boxes
    _both(C.problem(3 * D + G, D, G, H, W, boxes=C.edge_boxes(H, W)))
    _both(C.problem(5 * D + G, D, G, H, W))


@pytest.mark.parametrize("values,dtype", [((0, 1), np.uint8), ((0, 255), np.uint8), ((0, 1), bool), ((0, 128), np.uint8)])
def test_byte_values(values, dtype):
    pb = C.problem(17, 5, 4, 37, 53, values, dtype, C.edge_boxes(37, 53))
    got = _both(pb)
    one = C.run_op(dict(pb, dt_planes=(pb["dt_planes"] != 0).astype(np.uint8), gt_planes=(pb["gt_planes"] != 0).astype(np.uint8)))
    C.assert_same(got, one)


def test_pairs_that_only_touch_give_zeros_and_read_no_plane():
    H, W = 20, 40
    boxes = [(0, 0, 10, 10), (10, 0, 20, 10), (0, 10, 10, 20), (10, 10, 20, 20)]             # they share edges and a corner only
    pb = C.problem(23, 4, 4, H, W, boxes=boxes)
    pb["gt_box"] = pb["dt_box"].copy()
    got = _both(pb)
    off = ~np.eye(4, dtype=bool)
    assert (got[2][off] == 0).all() and (got[3][off] == 0).all() and (np.diag(got[2]) == 100).all()
    # (that no plane is read for such a pair is the kernel's early return; the zeros are what can be observed)
    assert (np.diag(got[3]) > 0).all()


def test_full_size_image():
    H, W = 1024, 2048
    boxes = [(0, 0, W, H), (100, 200, 1900, 900), (7, 3, 8, H), (1001, 500, 1118, 640), (2047, 0, 2048, 1024), (-50, 1000, 300, 1100)]
    pb = C.problem(29, 4, 3, H, W, boxes=boxes)
    got = _both(pb)
    assert got[0][0] == np.count_nonzero(pb["dt_planes"][0]) and (got[2] > 0).sum() >= 6


def test_plane_offsets_beyond_2_31():
    """D = 1025 planes of 1024 x 2048 (2.1 GB); only the last is non-empty and overlaps the single ground truth, and its
    offset, 1024 * 2^21 = 2^31, does not fit 32 bits"""
    H, W, D = 1024, 2048, 1025
    rng = np.random.RandomState(31)
    last = (rng.rand(1, H, W) < 0.5).astype(np.uint8)
    gt = (rng.rand(1, H, W) < 0.5).astype(np.uint8)
    dt_box = np.tile(np.array([[0, 0, 64, 64]], np.int32), (D, 1))
    dt_box[-1] = (900, 300, 1500, 800)
    gt_box = np.array([[1000, 350, 1400, 900]], np.int32)
    want = _eval_cpu.window_counts(last, dt_box[-1:], gt, gt_box)
    planes = torch.zeros((D, H, W), dtype=torch.uint8, device=DEV)
    planes[-1] = torch.from_numpy(last[0]).to(DEV)
    args = (planes, torch.from_numpy(dt_box).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(gt_box).to(DEV))
    first = [o.cpu().numpy() for o in _C.window_counts(*args)]
    again = [o.cpu().numpy() for o in _C.window_counts(*args)]
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    dt_count, gt_count, pair_box, pair_mask = first
    assert (dt_count[:-1] == 0).all() and (pair_box[:-1] == 0).all() and (pair_mask[:-1] == 0).all()
    assert dt_count[-1] == want[0][0] > 0 and gt_count[0] == want[1][0]
    assert pair_box[-1, 0] == want[2][0, 0] == 400 * 450 and pair_mask[-1, 0] == want[3][0, 0] > 0


def test_entry_point_refuses_without_writing():
    out = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (2, 2, 4, 4)]
    planes = torch.ones((2, 4, 4), dtype=torch.uint8, device=DEV)
    box = torch.tensor([[0, 0, 4, 4], [1, 1, 3, 3]], dtype=torch.int32, device=DEV)

    def call(D=2, G=2, H=4, W=4, dp=planes.data_ptr(), o0=out[0].data_ptr()):
        rc = _C.lib.detops_window_counts(dp, box.data_ptr(), D, planes.data_ptr(), box.data_ptr(), G, H, W, o0,
                                         *(o.data_ptr() for o in out[1:]), _C.stream_of(planes))
        torch.cuda.synchronize()
        return rc

    for kw in (dict(D=-1), dict(H=-1), dict(H=1 << 16, W=1 << 15), dict(dp=None), dict(o0=None), dict(D=4096, G=4096)):
        assert call(**kw) == -1, kw
        assert all(bool((o == -7).all()) for o in out)
    assert call() == 0
    assert out[0].tolist() == [16, 4] and out[3].reshape(2, 2).tolist() == [[16, 16], [16, 4]]


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("masks", ["planes", "probabilities"])
def test_fixture_through_the_evaluator_on_the_device(masks):
    fx = C.load_fixture()
    ds = C.FixtureDataset(fx)
    ev = E._feed(CE.CityscapesEvaluator(ds.CLASSES), C.fixture_predictions(fx, DEV, masks), ds, 5, DEV)
    C.assert_reference_records(fx, ev)
    C.assert_reference_ap(fx, ev.summarize())


TINY = ["MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4", "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16",
        "MODEL.RPN.PRE_NMS_TOP_N_TEST", "200", "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "60", "MODEL.ROI_HEADS.DETECTIONS_PER_IMG", "20",
        "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", "32", "MODEL.ROI_MASK_HEAD.CONV_LAYERS", "(8, 8)", "INPUT.MIN_SIZE_TEST", "80",
        "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0", "DATALOADER.SIZE_DIVISIBILITY", "32"]


class _Recorded(torch.nn.Module):
    """the model, keeping a CPU copy of what it returned: at the original image size, the masks pasted there on the device
    (what the evaluator does with the model's output), so the CPU path gets the same planes"""

    def __init__(self, model, size):
        super().__init__()
        self.model, self.size, self.outputs = model, size, []

    def forward(self, images):
        from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import Masker

        out = self.model(images)
        for o in out:
            r = o.resize(self.size)
            if len(r):
                r.add_field("mask", Masker(threshold=0.5).forward_single_image(r.get_field("mask").float(), r))
            self.outputs.append(r.to("cpu"))
        return out


@pytest.mark.parametrize("mode", ["mask", "poly"])
def test_mask_rcnn_through_inference_gives_the_cpu_paths_result(mode, tmp_path, monkeypatch):
    from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog
    from maskrcnn_benchmark.data import make_data_loader
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.engine.inference import inference
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    import os

    fx = C.load_fixture()
    C.write_tree(os.path.join(str(tmp_path), "cityscapes"), fx, images=4)
    monkeypatch.setattr(DatasetCatalog, "DATA_DIR", str(tmp_path))
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    yaml = "cityscapes/e2e_mask_rcnn_R_50_FPN_1x_%s.yaml" % ("binarymask" if mode == "mask" else "poly")
    cfg = load_cfg(yaml, TINY)
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(DEV)
    recorded = _Recorded(model, (56, 40))
    loader = make_data_loader(cfg, is_train=False)
    assert loader.dataset.mode == mode and len(loader.dataset) == 4
    got = inference(recorded, loader, "cityscapes_val", iou_types=("bbox", "segm"), device=DEV, output_folder=str(tmp_path / "out"))
    assert len(recorded.outputs) == 4
    print("%s: detections per image %s, bbox allAp %.4f, segm allAp %.4f" % (
        mode, [len(o) for o in recorded.outputs], got["bbox"]["averages"]["allAp"], got["segm"]["averages"]["allAp"]))
    assert sum(len(o) for o in recorded.outputs) > 0
    cpu = E.do_cityscapes_evaluation(loader.dataset, recorded.outputs, False, None, ("bbox", "segm"))
    for t in ("bbox", "segm"):
        assert got[t]["ap"].shape == (1, 11, 10)
        assert np.array_equal(got[t]["ap"], cpu[t]["ap"], equal_nan=True), t
    assert os.path.exists(os.path.join(str(tmp_path), "out", "evaluationResults", "maskResult.json"))
    # a model of random weights scores nothing, so the records themselves are compared too: every count and pair of the
    # device's evaluator against the CPU's on the same predictions
    dev_ev = E._feed(CE.CityscapesEvaluator(loader.dataset.CLASSES), recorded.outputs, loader.dataset, 2, DEV)
    cpu_ev = E._feed(CE.CityscapesEvaluator(loader.dataset.CLASSES), recorded.outputs, loader.dataset, 2, "cpu")
    pairs = pixels = 0
    for a, b in zip(dev_ev.images, cpu_ev.images):
        assert sorted(a) == sorted(b)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        pairs, pixels = pairs + len(a["pairs"]), pixels + int(a["dt_pixel_count"].sum()) + int(a["gt_pixel_count"].sum())
    assert pairs > 0 and pixels > 0
