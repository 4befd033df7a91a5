"""Detection evaluation without a GPU: the numpy path (_eval_cpu.py) behind maskrcnn_benchmark._C and the evaluators
(data/datasets/evaluation/).  The first four tests are independent of the restatement in tests/eval_refs.py; then the
evaluator is pinned to it, the VOC path to the reference's own results (tests/golden/voc_eval_reference.npz)."""
import logging
import os

import numpy as np
import pytest
import torch

import eval_cases as C
import eval_refs as R
from maskrcnn_benchmark.data.datasets.evaluation import (COCOResults, COCOStyleEvaluator, check_expected_results, evaluate,
                                                         voc)
from maskrcnn_benchmark.structures.bounding_box import BoxList

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voc_eval_reference.npz")


boxlist = C.boxlist


def test_perfect_detections_score_one_where_a_ground_truth_lies():
    """copies of the ground truth with score 1: 1.0 for every statistic whose area range holds a ground truth, -1 elsewhere
    (here: a small and a medium box, nothing large)"""
    gt = [[10, 10, 29, 29], [50, 40, 99, 89]]                      # 20 x 20 = 400 (small), 50 x 50 = 2500 (medium)
    ev = COCOStyleEvaluator(("bbox",), num_classes=3)
    ev.update([boxlist(gt, (120, 100), scores=[1.0, 1.0], labels=[1, 2])], [boxlist(gt, (120, 100), labels=[1, 2])])
    s = ev.summarize()["bbox"]
    expect = np.array([1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1], dtype=np.float64)
    np.testing.assert_allclose(s, expect, rtol=0, atol=1e-12)


def test_no_detections_score_zero():
    """ground truth in every area range (small 400, medium 2500, large 10070) and no detection: all 12 statistics are 0"""
    gt = [[10, 10, 29, 29], [5, 5, 110, 99], [40, 40, 89, 89]]
    ev = COCOStyleEvaluator(("bbox",), num_classes=3)
    ev.update([boxlist([], (120, 100), scores=torch.zeros(0), labels=torch.zeros(0, dtype=torch.int64))],
              [boxlist(gt, (120, 100), labels=[1, 2, 2])])
    np.testing.assert_array_equal(ev.summarize()["bbox"], np.zeros((12,), dtype=np.float64))


def test_hand_case_ap50():
    """one category, 2 ground truths; detections TP (0.9), FP (0.8), TP (0.7) at IoU 0.5:
    AP50 = (51 * 1 + 50 * 2/3) / 101"""
    gt = [[0, 0, 19, 19], [50, 50, 69, 69]]
    dt = [[0, 0, 19, 19], [30, 0, 39, 9], [50, 50, 69, 69]]
    ev = COCOStyleEvaluator(("bbox",), num_classes=2)
    ev.update([boxlist(dt, (100, 100), scores=[0.9, 0.8, 0.7], labels=[1, 1, 1])], [boxlist(gt, (100, 100), labels=[1, 1])])
    s = ev.summarize()["bbox"]
    assert abs(s[1] - (51 + 50 * 2.0 / 3.0) / 101) <= 1e-9
    assert abs(s[1] - 0.834983) <= 1e-6


def test_score_ties_keep_input_order():
    """two detections of equal score on one ground truth: the first in input order is the match, whichever fits better"""
    gt = [[0, 0, 19, 19]]
    loose, tight = [0, 0, 19, 14], [0, 0, 19, 19]                   # IoU 0.75 and 1.0
    for order, first_iou_at_90 in (([loose, tight], False), ([tight, loose], True)):
        ev = COCOStyleEvaluator(("bbox",), num_classes=2)
        ev.update([boxlist(order, (40, 40), scores=[0.5, 0.5], labels=[1, 1])], [boxlist(gt, (40, 40), labels=[1])])
        rec = ev.records["bbox"][0]
        np.testing.assert_array_equal(rec["dt_match"][0, 0], [0, -1])          # threshold 0.5: the first takes it
        t90 = 8
        np.testing.assert_array_equal(rec["dt_match"][0, t90], [0, -1] if first_iou_at_90 else [-1, 0])


@pytest.fixture(scope="module")
def seeded():
    images = C.make_images()
    return images, {t: R.coco_stats(images, t, C.NUM_CLASSES) for t in ("bbox", "segm")}


def compare_with_refs(evaluator, images, refs):
    for iou_type, (ev, stats) in refs.items():
        recs = C.records_by_key(evaluator, iou_type)
        seen = 0
        for (k, a, i), e in ev.items():
            if e is None:
                assert (i, k) not in recs
                continue
            r = recs[(i, k)]
            np.testing.assert_array_equal(r["dt_match"][a], np.array(e["dt_match"], np.int32).reshape(len(R.IOU_THRS), -1))
            np.testing.assert_array_equal(r["dt_ignore"][a] != 0, np.array(e["dt_ignore"], bool).reshape(len(R.IOU_THRS), -1))
            np.testing.assert_array_equal(r["gt_ignore"][a] != 0, np.array(e["gt_ignore"], bool))
            np.testing.assert_array_equal(r["scores"], np.array(e["scores"], np.float64))
            seen += 1
        assert seen == 4 * len(recs)
        got = evaluator.stats[iou_type]
        print(iou_type, np.round(got, 6))
        np.testing.assert_allclose(got, np.array(stats), rtol=0, atol=1e-12)


def test_evaluator_equals_the_literal_restatement(seeded):
    images, refs = seeded
    preds, tgts = C.to_boxlists(images)
    ev = COCOStyleEvaluator(("bbox", "segm"), C.NUM_CLASSES)
    ev.update(preds[:3], tgts[:3])             # batches of different sizes: the records do not depend on the batching
    ev.update(preds[3:], tgts[3:])
    ev.summarize()
    compare_with_refs(ev, images, refs)
    # the cases hold what they are meant to hold
    segm = refs["segm"][0]
    all_ig = [e for e in segm.values() if e is not None]
    assert any(any(e["gt_ignore"]) for e in all_ig) and any(-1 in e["dt_match"][0] for e in all_ig if e["scores"])
    assert 0 < refs["segm"][1][0] < 1 and 0 < refs["bbox"][1][0] < 1


def test_missing_iscrowd_and_area_take_their_defaults(seeded):
    """no `iscrowd`: all 0; no `area`: the mask's pixel count, without masks w * h of the xywh box"""
    images, _ = seeded
    plain = [{"size": im["size"], "dt": im["dt"],
              "gt": [dict(g, iscrowd=False, area=float(g["mask"].sum())) for g in im["gt"]]} for im in images]
    preds, tgts = C.to_boxlists(plain, explicit_area=False)
    for t in tgts:
        del t.extra_fields["iscrowd"]
    ev = COCOStyleEvaluator(("segm",), C.NUM_CLASSES)
    ev.update(preds, tgts)
    ev.summarize()
    compare_with_refs(ev, plain, {"segm": R.coco_stats(plain, "segm", C.NUM_CLASSES)})
    boxes = [{"size": im["size"], "dt": im["dt"],
              "gt": [dict(g, iscrowd=False, area=R.xywh(g["box"])[2] * R.xywh(g["box"])[3]) for g in im["gt"]]} for im in images]
    preds, tgts = C.to_boxlists(boxes, with_masks=False, explicit_area=False)
    ev = COCOStyleEvaluator(("bbox",), C.NUM_CLASSES)
    ev.update(preds, tgts)
    ev.summarize()
    compare_with_refs(ev, boxes, {"bbox": R.coco_stats(boxes, "bbox", C.NUM_CLASSES)})


def test_dense_planes_of_another_size_raise(seeded):
    images, _ = seeded
    preds, tgts = C.to_boxlists(images[:1])
    preds[0].add_field("mask", preds[0].get_field("mask")[:, :, :-1])
    with pytest.raises(ValueError, match="dense prediction masks"):
        COCOStyleEvaluator(("segm",), C.NUM_CLASSES).update(preds, tgts)


def test_labels_outside_the_class_range_raise(seeded):
    """a label >= num_classes would share its problem key with another image's category"""
    images, _ = seeded
    preds, tgts = C.to_boxlists(images[:1], with_masks=False)
    with pytest.raises(ValueError, match="labels must lie in"):
        COCOStyleEvaluator(("bbox",), num_classes=2).update(preds, tgts)


def test_voc_fixture_is_reproduced_exactly():
    fx = np.load(GOLDEN)
    C.check_voc_fixture(fx, *C.voc_boxlists(fx))


def test_check_expected_results_passes_and_fails_as_the_reference(caplog):
    res = COCOResults("bbox", "segm")
    assert list(res.results["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and res.results["segm"]["AP"] == -1
    res.results["bbox"]["AP"] = 0.377
    res.results["segm"]["AP"] = 0.30
    with caplog.at_level(logging.INFO, logger="maskrcnn_benchmark.inference"):
        check_expected_results(res, [], 4)
        assert not caplog.records                                              # nothing expected, nothing said
        check_expected_results(res, [("bbox", "AP", (0.3775, 0.001)), ("segm", "AP", (0.342, 0.001))], 4)
    assert [r.levelname for r in caplog.records] == ["INFO", "ERROR"]
    assert caplog.records[0].getMessage().startswith("PASS: bbox > AP sanity check (actual vs. expected): 0.377 vs. mean=0.3775")
    assert caplog.records[1].getMessage().startswith("FAIL: segm > AP sanity check")
    assert "range=(0.3380, 0.3460)" in caplog.records[1].getMessage()
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="maskrcnn_benchmark.inference"):
        check_expected_results(res, [("bbox", "AP", (0.373, 0.001))], 4)       # the bounds are exclusive: 0.377 is the upper one
    assert caplog.records[0].levelname == "ERROR"
    assert "Task: bbox\nAP, AP50, AP75, APs, APm, APl\n0.3770, -1.0000" in repr(res)


def test_out_of_scope_requests_raise():
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset

    ds = SyntheticCOCODataset(length=1, height=40, width=48)
    with pytest.raises(NotImplementedError, match="box_only"):
        evaluate(ds, [], None, box_only=True, iou_types=("bbox",))
    with pytest.raises(NotImplementedError, match="keypoints"):
        evaluate(ds, [], None, box_only=False, iou_types=("bbox", "keypoints"))
    with pytest.raises(NotImplementedError, match="keypoints"):
        COCOStyleEvaluator(("keypoints",))
    with pytest.raises(NotImplementedError, match="Unsupported dataset type"):
        evaluate(object(), [], None)

    class Cityscapes(object):
        evaluation_style = "cityscapes"

    with pytest.raises(NotImplementedError, match="Cityscapes"):
        evaluate(Cityscapes(), [], None)


def test_evaluate_from_stored_predictions_equals_streaming(tmp_path):
    """`evaluate(dataset, predictions, folder)`: ground truth from the dataset; jittered copies of it as predictions"""
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset

    ds = SyntheticCOCODataset(length=3, height=64, width=80, num_classes=5, min_objects=2, max_objects=4)
    preds = []
    for i in range(len(ds)):
        t = ds.get_groundtruth(i)
        p = BoxList(t.bbox + 1.0, t.size)
        p.add_field("scores", torch.linspace(0.9, 0.5, len(t)))
        p.add_field("labels", t.get_field("labels"))
        p.add_field("mask", t.get_field("masks").instances.masks[:, None] != 0)
        preds.append(p)
    res = evaluate(ds, preds, str(tmp_path), iou_types=("bbox", "segm"))
    assert res.results["segm"]["AP"] == pytest.approx(1.0) and 0.3 < res.results["bbox"]["AP"] < 1.0
    assert os.path.exists(tmp_path / "coco_results.pth") and "segm" in open(tmp_path / "coco_results.txt").read()


def test_test_net_runs_end_to_end_on_a_tiny_cpu_config(tmp_path, capsys):
    import cpu_shim
    import test_net

    opts = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4",
            "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16", "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", "32",
            "MODEL.ROI_MASK_HEAD.CONV_LAYERS", "(16, 16)", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "100",
            "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "50", "MODEL.ROI_HEADS.SCORE_THRESH", "0.0", "TEST.DETECTIONS_PER_IMG", "20",
            "INPUT.MIN_SIZE_TEST", "96", "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "OUTPUT_DIR", str(tmp_path)]
    torch.manual_seed(0)
    with cpu_shim.install():
        results = test_net.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml", "--images", "4"] + opts)
    out = capsys.readouterr().out
    assert "Task: bbox" in out and "Task: segm" in out
    (name,) = os.listdir(tmp_path / "inference")              # the config's DATASETS.TEST entry
    table = open(tmp_path / "inference" / name / "coco_results.txt").read()
    assert "AR100" in table
    r = results[0].results
    assert all(-1 <= v <= 1 for task in r.values() for v in task.values())
