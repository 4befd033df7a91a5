"""Cityscapes without a GPU: the numpy twin (_eval_cpu.window_counts) and csrc/cityscapes_eval.hip under the host emulation
against the fixture the REFERENCE's own functions wrote (tests/golden/cityscapes_reference.npz) and against literal loops;
the AP against the reference's matrices; the three library choices; the dataset against the reference's two annotation
functions on a tree written with PIL; the catalog, the loader, `inference()` and the result files.

Counts and pairs are integers and compared exactly.  AP values and averages lie in [0, 1] and differ from the reference's at
most by the summation order of an fp64 dot product of a few hundred terms (about 1e-14): the bound is 1e-12."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import cityscapes_cases as C
from maskrcnn_benchmark import _C, _eval_cpu
from maskrcnn_benchmark.data.datasets import evaluation as E
from maskrcnn_benchmark.data.datasets.evaluation import cityscapes as CE
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


def _evaluate(fx, batch, masks="planes", iou_types=("bbox", "segm")):
    ds = C.FixtureDataset(fx)
    return E._feed(CE.CityscapesEvaluator(ds.CLASSES, iou_types), C.fixture_predictions(fx, masks=masks), ds, batch)


# ------------------------------------------------------------------------------------------------ against the fixture
@pytest.mark.parametrize("masks", ["planes", "probabilities"])
def test_numpy_path_reproduces_the_reference(fx, masks):
    ev = _evaluate(fx, 4, masks)
    C.assert_reference_records(fx, ev)
    C.assert_reference_ap(fx, ev.summarize())
    assert (ev.num_images, ev.num_detections, ev.num_groundtruths) == (13, int(fx["pred_counts"].sum()), int(fx["gt_counts"].sum()))


def test_emulated_kernel_reproduces_the_reference(fx, monkeypatch):
    calls = []
    with C.emulated():
        raw = _C.lib.detops_window_counts
        monkeypatch.setattr(_C.lib, "detops_window_counts", lambda *a: calls.append(a) or raw(*a), raising=False)
        try:
            ev = _evaluate(fx, 5)
        finally:
            monkeypatch.undo()
    # one call per image; the image without predictions asks for its ground truths' counts alone
    assert len(calls) == 13
    C.assert_reference_records(fx, ev)
    C.assert_reference_ap(fx, ev.summarize())


def test_stored_planes_give_every_count_of_the_fixture_through_the_operator(fx):
    g, d = C._offsets(fx["gt_counts"]), C._offsets(fx["pred_counts"])
    for i in range(len(fx["sizes"])):
        pb = {"dt_planes": fx["pred_planes_%d" % i], "gt_planes": fx["gt_planes_%d" % i],
              "dt_box": fx["pred_boxes"][d[i]:d[i + 1]].astype(np.int32), "gt_box": fx["gt_boxes"][g[i]:g[i + 1]].astype(np.int32)}
        want = C.run_op(pb)
        with C.emulated():
            C.assert_same(C.run_op(pb), want)
        np.testing.assert_array_equal(want[0], fx["pred_pixel_count"][d[i]:d[i + 1]])
        np.testing.assert_array_equal(want[1], fx["gt_pixel_count"][g[i]:g[i + 1]])
        for _, gt, dt, box, mask in fx["pairs"][fx["pairs"][:, 0] == i]:
            assert (want[2][dt, gt], want[3][dt, gt]) == (box, mask)
        kept = fx["pred_kept"][d[i]:d[i + 1]] != 0
        assert int(((want[2] > 0) & kept[:, None]).sum()) == int((fx["pairs"][:, 0] == i).sum())


def test_the_issues_worked_example():
    # a ground truth whose tight box is (5, 5, 24, 19) and whose mask is 15 x 20 = 300 pixels has pixelCount 266; a prediction
    # (0, 0, 10, 10) against it gives boxIntersection 25 and maskIntersection 36 when its plane fills its box
    gt = np.zeros((1, 30, 40), np.uint8)
    gt[0, 5:20, 5:25] = 1
    dt = np.zeros((1, 30, 40), np.uint8)
    dt[0, 0:11, 0:11] = 1
    pb = {"dt_planes": dt, "dt_box": np.array([[0, 0, 10, 10]], np.int32), "gt_planes": gt, "gt_box": np.array([[5, 5, 24, 19]], np.int32)}
    for ctx in (contextlib.nullcontext(), C.emulated()):
        with ctx:
            dt_count, gt_count, pair_box, pair_mask = C.run_op(pb)
        assert (int(dt_count[0]), int(gt_count[0]), int(pair_box[0, 0]), int(pair_mask[0, 0])) == (100, 266, 25, 36)


def test_batches_of_one_and_all_give_identical_results(fx):
    whole, single = _evaluate(fx, 13).summarize(), _evaluate(fx, 1).summarize()
    for t in ("bbox", "segm"):
        assert whole[t]["ap"].tobytes() == single[t]["ap"].tobytes()


def test_ties_in_score_do_not_depend_on_the_order(fx):
    ds = C.FixtureDataset(fx)
    preds = C.fixture_predictions(fx, masks="planes")
    ev = E._feed(CE.CityscapesEvaluator(ds.CLASSES), preds, ds, 13)
    base = ev.summarize()
    for im in ev.images:                                  # the same records with the predictions of every image reversed
        for k in ("dt_index", "dt_label", "dt_box_area", "dt_pixel_count", "dt_score"):
            im[k] = im[k][::-1].copy()
    again = ev.summarize()
    for t in ("bbox", "segm"):
        np.testing.assert_allclose(again[t]["ap"], base[t]["ap"], rtol=0, atol=C.AP_TOL, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("emulated", [False, True], ids=["numpy", "emulated"])
def test_operator_against_the_literal_loops(emulated):
    problems = [C.problem(1, 3, 2, 7, 9), C.problem(2, 1, 1, 1, 1, boxes=[(0, 0, 1, 1)]), C.problem(3, 4, 5, 12, 37, values=(0, 255)),
                C.problem(4, 2, 3, 9, 20, dtype=bool), C.problem(5, 0, 2, 5, 6), C.problem(6, 3, 0, 5, 6),
                C.problem(7, 6, 7, 10, 19, boxes=C.edge_boxes(10, 19))]
    with (C.emulated() if emulated else contextlib.nullcontext()):
        for pb in problems:
            C.assert_same(C.run_op(pb), C.literal_counts(pb))


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (37, 53), (64, 64), (65, 130)])
def test_emulated_kernel_against_numpy_at_the_kernels_edges(H, W):
    boxes = C.edge_boxes(H, W)
    for seed, (D, G, values, dtype) in enumerate([(3, 1, (0, 1), np.uint8), (1, 3, (0, 255), np.uint8), (len(boxes), 3, (0, 1), bool),
                                                  (0, 3, (0, 1), np.uint8), (3, 0, (0, 1), np.uint8), (0, 0, (0, 1), np.uint8)]):
        for bx in (boxes, None):
            pb = C.problem(40 + seed, D, G, H, W, values, dtype, bx)
            want = C.run_op(pb)
            with C.emulated():
                C.assert_same(C.run_op(pb), want)


def test_emulated_kernel_with_more_strips_than_one_and_unaligned_planes():
    # 200 rows: four strips of 50; 53 columns: H * W is odd, so the second plane of a batch starts at an odd address
    pb = C.problem(9, 3, 2, 201, 53, boxes=[(0, 0, 53, 201), (5, 49, 40, 152), (1, 100, 52, 101), (17, 0, 18, 201)])
    want = C.run_op(pb)
    with C.emulated():
        C.assert_same(C.run_op(pb), want)
    assert want[0][0] == np.count_nonzero(pb["dt_planes"][0])


def test_entry_point_refuses_bad_arguments_and_touches_nothing():
    lib = C.emu_cityscapes_lib()
    planes = np.ones((2, 4, 4), np.uint8)
    box = np.array([[0, 0, 4, 4], [1, 1, 3, 3]], np.int32)
    out = [np.full((n,), -7, np.int32) for n in (2, 2, 4, 4)]
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(dp=p(planes), db=p(box), D=2, gp=p(planes), gb=p(box), G=2, H=4, W=4, o=None):
        o = [p(a) for a in out] if o is None else o
        return lib.detops_window_counts(dp, db, D, gp, gb, G, H, W, *o, None)

    for kw in (dict(D=-1), dict(G=-1), dict(H=-1), dict(W=-1), dict(H=1 << 16, W=1 << 15), dict(dp=None), dict(gb=None),
               dict(o=[None] + [p(a) for a in out[1:]]), dict(o=[p(a) for a in out[:3]] + [None]), dict(D=4096, G=4096)):
        assert call(**kw) == -1, kw
        assert all((a == -7).all() for a in out)
    assert call() == 0
    assert out[0].tolist() == [16, 4] and out[2].reshape(2, 2).tolist() == [[16, 4], [4, 4]] and out[3].reshape(2, 2).tolist() == [[16, 16], [16, 4]]
    with pytest.raises(ValueError):
        _C.window_counts(torch.zeros((1, 4, 4)), torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 4, 5)), torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        _C.window_counts(torch.zeros((1, 4, 4), dtype=torch.uint8), torch.zeros((1, 4)), torch.zeros((1, 4, 4), dtype=torch.uint8),
                         torch.zeros((1, 4), dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ the three choices
def _boxlist(boxes, size, labels, scores=None, planes=None):
    b = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), size, mode="xyxy")
    b.add_field("labels", torch.tensor(labels, dtype=torch.int64))
    if scores is not None:
        b.add_field("scores", torch.tensor(scores, dtype=torch.float32))
    return b


def test_choice_1_a_prediction_keeps_its_own_mask_after_one_was_dropped():
    size, (W, H) = (60, 40), (60, 40)
    gt_plane = np.zeros((1, H, W), np.uint8)
    gt_plane[0, 10:30, 10:40] = 1
    t = _boxlist([[10, 10, 39, 29]], size, [1])
    t.add_field("masks", SegmentationMask(torch.from_numpy(gt_plane), size, mode="mask"))
    planes = np.zeros((2, 1, H, W), bool)               # prediction 0 has no pixels and is dropped; prediction 1 covers the ground truth
    planes[1, 0, 10:30, 10:40] = True
    p = _boxlist([[10, 10, 39, 29], [10, 10, 39, 29]], size, [1, 1], [0.9, 0.8])
    p.add_field("mask", torch.from_numpy(planes))
    ev = CE.CityscapesEvaluator(["__background__", "person"])
    ev.update([p], [t])
    im = ev.images[0]
    # literal: the kept prediction is predID 1 and its counts come from plane 1 (the reference would pair it with plane 0: 0)
    own = int(planes[1, 0, 10:29, 10:39].sum())
    assert im["dt_index"].tolist() == [1] and im["dt_pixel_count"].tolist() == [own] and own == 19 * 29
    assert im["pairs"].tolist() == [[1, 0, 19 * 29, own]]
    res = ev.summarize()
    assert res["segm"]["ap"][0, 1].tolist() == [1.0] * 10 and res["bbox"]["ap"][0, 1].tolist() == [1.0] * 10


def test_choice_2_windows_are_clamped_to_the_image():
    pb = C.problem(8, 2, 2, 6, 8, boxes=[(-3, -2, 5, 4), (2, -1, 12, 9), (-1, 3, 9, 7)])
    got = C.run_op(pb)
    C.assert_same(got, C.literal_counts(pb))
    # literal: a negative minimum stands for 0, where the reference's slice -3:5 of 8 columns would be empty
    assert got[0][0] == np.count_nonzero(pb["dt_planes"][0][0:4, 0:5]) and got[0][0] > 0
    # pair_box is made from the boxes as given: (2 .. 5) x (-1 .. 4) = 3 * 5
    assert got[2][0, 0] == 15


def test_choice_3_the_ground_truth_is_taken_at_its_own_size_and_predictions_are_resized_to_it():
    size = (80, 60)
    plane = np.zeros((1, 60, 80), np.uint8)
    plane[0, 11:41, 21:61] = 1
    t = _boxlist([[21, 11, 60, 40]], size, [1])
    t.add_field("masks", SegmentationMask(torch.from_numpy(plane), size, mode="mask"))
    p = _boxlist([[10.5, 5.5, 30.25, 20.0]], (40, 30), [1], [0.5])                        # given at half the size
    ev = CE.CityscapesEvaluator(["__background__", "person"], ("bbox",))
    ev.update([p], [t])
    im = ev.images[0]
    # literal: the prediction's box times (2, 2), truncated: (21, 11, 60, 40); the target's box as given
    assert im["dt_box_area"].tolist() == [39 * 29] and im["gt_box_area"].tolist() == [39 * 29]
    assert im["pairs"].tolist() == [[0, 0, 39 * 29, 0]] and im["gt_pixel_count"].tolist() == [0]          # bbox only: no plane is made


def test_overlap_thresholds_are_the_references_fp64_values():
    assert CE.OVERLAPS.tobytes() == np.arange(0.5, 1.0, 0.05).tobytes() and CE.OVERLAPS[2] != 0.6 and CE.OVERLAPS[5] != 0.75
    # a pair at exactly 0.6 does not match at the third threshold (0.6000000000000001)
    t = _boxlist([[0, 0, 20, 10]], (50, 50), [1])
    p = _boxlist([[0, 0, 12, 10]], (50, 50), [1], [0.5])
    ev = CE.CityscapesEvaluator(["__background__", "person"], ("bbox",))
    ev.update([p], [t])
    assert ev.summarize()["bbox"]["ap"][0, 1].tolist() == [1.0, 1.0] + [0.0] * 8


# ------------------------------------------------------------------------------------------------ the dataset
def _datasets(tmp_path, fx, **kw):
    from maskrcnn_benchmark.data.datasets import CityScapesDataset

    img_dir, ann_dir = C.write_tree(str(tmp_path), fx)
    return (CityScapesDataset(img_dir, ann_dir, "val", mode="mask", **kw), CityScapesDataset(img_dir, ann_dir, "val", mode="poly", **kw))


def test_dataset_reads_both_modes_as_the_references_functions_do(tmp_path, fx):
    mask_ds, poly_ds = _datasets(tmp_path, fx)
    assert mask_ds.evaluation_style == "cityscapes" and len(mask_ds) == len(poly_ds) == 3
    assert mask_ds.CLASSES == ["__background__", "person", "rider", "car", "truck", "bus", "caravan", "trailer", "train", "motorcycle", "bicycle"]
    assert mask_ds.name_to_id["bicycle"] == 10 and mask_ds.id_to_name[3] == "car" and mask_ds.cityscapesID_to_ind == {24 + i: 1 + i for i in range(10)}
    t = mask_ds.get_groundtruth(0)
    assert t.size == (56, 40) and t.mode == "xyxy"
    np.testing.assert_array_equal(t.bbox.numpy(), fx["ids_boxes"].astype(np.float32))
    np.testing.assert_array_equal(t.get_field("labels").numpy(), fx["ids_labels"])
    planes = t.get_field("masks").get_mask_tensor().numpy().reshape(-1, 40, 56)
    for plane, v in zip(planes, fx["ids_values"]):
        np.testing.assert_array_equal(plane != 0, fx["id_map"] == v)
    t = poly_ds.get_groundtruth(0)
    np.testing.assert_array_equal(t.bbox.numpy(), fx["poly_boxes"].astype(np.float32))
    np.testing.assert_array_equal(t.get_field("labels").numpy(), fx["poly_labels"])
    polys = t.get_field("masks").instances.polygons
    assert [len(p.polygons) for p in polys] == [1] * len(fx["poly_lengths"])
    flat = np.concatenate([np.asarray(p.polygons[0], np.float64).reshape(-1) for p in polys])
    np.testing.assert_array_equal(flat, fx["poly_flat"])
    assert t.get_field("masks").get_mask_tensor().shape[-2:] == (40, 56)


def test_dataset_min_area_mini_img_info_and_items(tmp_path, fx):
    from maskrcnn_benchmark.data.datasets import CityScapesDataset

    mask_ds, poly_ds = _datasets(tmp_path, fx)
    info = mask_ds.get_img_info(2)
    assert (info["width"], info["height"], info["idx"]) == (56, 40, 2) and info["img_path"].endswith("_leftImg8bit.png")
    assert info["ann_path"].endswith("_instanceIds.png") and poly_ds.get_img_info(0)["ann_path"].endswith("_polygons.json")
    assert (poly_ds.get_img_info(1)["width"], poly_ds.get_img_info(1)["height"]) == (56, 40)
    boxes = fx["ids_boxes"]
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    img_dir, ann_dir = os.path.join(str(tmp_path), "leftImg8bit"), os.path.join(str(tmp_path), "gtFine")
    big = CityScapesDataset(img_dir, ann_dir, "val", mode="mask", min_area=int(np.sort(area)[2]))
    np.testing.assert_array_equal(big.get_groundtruth(0).bbox.numpy(), boxes[area >= np.sort(area)[2]].astype(np.float32))
    mini = CityScapesDataset(img_dir, ann_dir, "val", mode="mask", mini=2)                # stride 3 // 2 + 1 = 2
    assert [os.path.basename(p)[:13] for p in mini.img_paths] == ["aachen_000000", "cologne_00000"] and len(mini.ann_paths) == 2
    img, target, idx = mask_ds[0]
    assert img.size == (56, 40) and idx == 0 and target.has_field("masks") and len(target) == len(fx["ids_labels"])
    # image 1 has no instances: kept (empty) for testing, replaced by the next one when training
    img, target, idx = mask_ds[1]
    assert idx == 1 and len(target) == 0 and not target.has_field("masks")
    train = CityScapesDataset(img_dir, ann_dir, "train", mode="poly", remove_images_without_annotations=True)
    img, target, idx = train[1]
    assert idx == 1 and len(target) == len(fx["poly_labels"])
    np.testing.assert_array_equal(target.bbox.numpy(), train[2][1].bbox.numpy())
    mask_ds.groundtruth_targets = True
    assert mask_ds[0][1].get_field("masks").get_mask_tensor().shape[-2:] == (40, 56)


def test_catalog_names_and_the_loader_for_both_configs(tmp_path, fx, monkeypatch):
    from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog
    from maskrcnn_benchmark.data import make_data_loader
    from maskrcnn_benchmark.engine.bench_step import load_cfg

    C.write_tree(os.path.join(str(tmp_path), "cityscapes"), fx)
    monkeypatch.setattr(DatasetCatalog, "DATA_DIR", str(tmp_path))
    for mode in ("poly", "mask"):
        for name, split, mini in (("train", "train", None), ("val", "val", None), ("minival", "val", 10)):
            got = DatasetCatalog.get("cityscapes_%s_instance_%s" % (mode, name))
            want = {"img_dir": os.path.join(str(tmp_path), "cityscapes/leftImg8bit"), "ann_dir": os.path.join(str(tmp_path), "cityscapes/gtFine"),
                    "split": split, "mode": mode}
            assert got == {"factory": "CityScapesDataset", "args": dict(want, **({"mini": mini} if mini else {}))}
    small = ["INPUT.MIN_SIZE_TEST", "40", "INPUT.MAX_SIZE_TEST", "64", "INPUT.MIN_SIZE_TRAIN", "(40,)", "INPUT.MAX_SIZE_TRAIN", "64",
             "DATALOADER.NUM_WORKERS", "0", "TEST.IMS_PER_BATCH", "2", "SOLVER.IMS_PER_BATCH", "2", "SOLVER.MAX_ITER", "2", "MODEL.DEVICE", "cpu"]
    for yaml, mode in (("cityscapes/e2e_mask_rcnn_R_50_FPN_1x_binarymask.yaml", "mask"), ("cityscapes/e2e_mask_rcnn_R_50_FPN_1x_poly.yaml", "poly")):
        cfg = load_cfg(yaml, small)
        assert cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES == 11 and cfg.SOLVER.BASE_LR == 0.01 and tuple(cfg.SOLVER.STEPS) == (18000,)
        loader = make_data_loader(cfg, is_train=False)
        assert loader.dataset.mode == mode and loader.dataset.groundtruth_targets and len(loader.dataset) == 3
        images, targets, ids = next(iter(loader))
        assert list(ids) == [0, 1] and targets[0].size == (56, 40) and targets[0].has_field("masks") and len(targets[1]) == 0
        train = make_data_loader(cfg, is_train=True)
        images, targets, ids = next(iter(train))
        assert len(targets) == 2 and all(len(t) > 0 and t.has_field("masks") for t in targets)


# ------------------------------------------------------------------------------------------------ the entry points
class _Stub(torch.nn.Module):
    """a model that returns the stored predictions of the images it is asked for"""

    def __init__(self, predictions):
        super().__init__()
        self.predictions, self.next = predictions, 0

    def forward(self, images):
        out = self.predictions[self.next:self.next + images.shape[0]]
        self.next += images.shape[0]
        return out


class _Loader(object):
    def __init__(self, dataset, batch):
        self.dataset, self.batch = dataset, batch

    def __iter__(self):
        for i in range(0, len(self.dataset), self.batch):
            ids = list(range(i, min(i + self.batch, len(self.dataset))))
            yield torch.zeros((len(ids), 1)), [self.dataset.get_groundtruth(j) for j in ids], ids


def test_inference_equals_the_stored_predictions_entry_and_writes_the_result_files(tmp_path, fx):
    from maskrcnn_benchmark.engine.inference import inference

    ds = C.FixtureDataset(fx)
    preds = C.fixture_predictions(fx)
    got = inference(_Stub(preds), _Loader(ds, 3), "fixture", iou_types=("bbox", "segm"), device="cpu", output_folder=str(tmp_path / "a"))
    want = E.do_cityscapes_evaluation(ds, preds, False, str(tmp_path / "b"), ("bbox", "segm"), (), 4)
    C.assert_reference_ap(fx, got)
    for t, fname in (("bbox", "boxResult.json"), ("segm", "maskResult.json")):
        assert got[t]["ap"].tobytes() == want[t]["ap"].tobytes()
        for folder in ("a", "b"):
            with open(os.path.join(str(tmp_path), folder, "evaluationResults", fname)) as f:
                data = json.load(f)
            assert sorted(data) == ["averages", "instLabels", "minRegionSizes", "overlaps", "resultApMatrix"]
            np.testing.assert_array_equal(np.array(data["resultApMatrix"], np.float64), got[t]["ap"])
            assert data["instLabels"] == ds.CLASSES and data["minRegionSizes"] == [100] and data["overlaps"] == CE.OVERLAPS.tolist()
            assert data["averages"]["allAp"] == float(got[t]["averages"]["allAp"]) and sorted(data["averages"]["classes"]) == sorted(ds.CLASSES)
        assert not os.path.exists(os.path.join(str(tmp_path), "a", "evaluationResults", "matches.json"))
    assert not os.path.exists(os.path.join(str(tmp_path), "a", "bbox.json"))
    # bbox alone: no plane is made, so nothing is dropped for having no pixels; without those predictions it is the fixture's
    d = C._offsets(fx["pred_counts"])
    kept = [p[torch.from_numpy(fx["pred_kept"][d[i]:d[i + 1]] != 0)] for i, p in enumerate(C.fixture_predictions(fx, masks=None))]
    bbox_only = inference(_Stub(kept), _Loader(ds, 13), "fixture", iou_types=("bbox",), device="cpu")
    assert list(bbox_only) == ["bbox"] and np.allclose(bbox_only["bbox"]["ap"], fx["box_ap"], rtol=0, atol=C.AP_TOL, equal_nan=True)


def test_the_table_is_the_references_text_without_colour_codes(fx):
    res = _evaluate(fx, 13).summarize()
    text = CE.format_results(res["bbox"]["averages"], [str(c) for c in fx["classes"]])
    lines = text.split("\n")
    assert lines[0] == "" and lines[1] == "#" * 65 and lines[3] == "#" * 65 and lines[-4] == "-" * 65 and lines[-1] == "" and lines[-2] == ""
    assert lines[2] == "what           :             AP         AP_50%         AP_75%"
    assert lines[4] == "__background__ :            nan            nan            nan"
    assert lines[-3] == "average        :" + "".join("{:>15.3f}".format(v) for v in fx["box_avg"][:3])


def test_generic_entry_points_refuse_and_name_the_way_in(fx):
    from maskrcnn_benchmark.engine.inference import inference

    ds = C.FixtureDataset(fx)
    with pytest.raises(NotImplementedError, match="Cityscapes.*CityscapesEvaluator"):
        E.evaluate(ds, [], None)
    preds = C.fixture_predictions(fx)
    for kw in (dict(keypoint_oks=True), dict(box_only=True), dict(evaluate=False, output_folder="unused")):
        with pytest.raises(NotImplementedError, match="Cityscapes"):
            inference(_Stub(preds), _Loader(ds, 3), "fixture", device="cpu", **kw)
    with pytest.raises(NotImplementedError, match="box augmentation"):
        inference(_Stub(preds), _Loader(ds, 3), "fixture", iou_types=("bbox", "segm"), device="cpu", bbox_aug=True, cfg=object())
    with pytest.raises(ValueError, match="keypoints"):
        CE.CityscapesEvaluator(ds.CLASSES, ("keypoints",))
    assert _eval_cpu.window_counts(np.zeros((0, 3, 3), np.uint8), np.zeros((0, 4)), np.zeros((0, 3, 3), np.uint8), np.zeros((0, 4)))[2].shape == (0, 0)
