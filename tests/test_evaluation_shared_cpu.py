"""What the evaluators share (data/datasets/evaluation/coco_style.py): the flattening of a batch of BoxLists against tensors
written out by hand, and the statistics table against the two lists of `stat(...)` calls it replaced."""
import re

import numpy as np
import pytest
import torch

from eval_cases import boxlist
from maskrcnn_benchmark.data.datasets.evaluation import coco_style as CS
from maskrcnn_benchmark.data.datasets.evaluation import keypoint_oks as KO

FIELDS = ("dt_img", "gt_img", "dt_box", "gt_box", "dt_label", "gt_label", "dt_score", "gt_ignore")


def _batch(ignore_field):
    """three images: one without detections, one without ground truth (and a prediction in xywh), one whose prediction was
    made at half the target's size; the last target has no ignore field"""
    none = dict(scores=torch.zeros(0), labels=torch.zeros(0, dtype=torch.int64))
    preds = [boxlist([], (100, 80), **none),
             boxlist([[5, 5, 11, 11], [0, 2, 4, 6]], (60, 40), scores=[0.5, 0.9], labels=[2, 1]),
             boxlist([[10, 5, 30, 20]], (100, 50), scores=[0.7], labels=[3])]
    preds[1].mode = "xywh"
    tgts = [boxlist([[1, 2, 30, 40], [50, 10, 90, 70]], (100, 80), labels=[1, 2], **{ignore_field: torch.tensor([0, 1], dtype=torch.uint8)}),
            boxlist([], (60, 40), labels=torch.zeros(0, dtype=torch.int64), **{ignore_field: torch.zeros(0, dtype=torch.uint8)}),
            boxlist([[20, 10, 60, 40]], (200, 100), labels=[3])]
    return preds, tgts


def _expected(first_image, resized):
    i64, f32 = torch.int64, torch.float32
    return {"dt_img": torch.tensor([1, 1, 2], dtype=i64) + first_image,
            "gt_img": torch.tensor([0, 0, 2], dtype=i64) + first_image,
            "dt_box": torch.tensor([[5, 5, 15, 15], [0, 2, 3, 7], [20, 10, 60, 40] if resized else [10, 5, 30, 20]], dtype=f32),
            "gt_box": torch.tensor([[1, 2, 30, 40], [50, 10, 90, 70], [20, 10, 60, 40]], dtype=f32),
            "dt_label": torch.tensor([2, 1, 3], dtype=i64),
            "gt_label": torch.tensor([1, 2, 3], dtype=i64),
            "dt_score": torch.tensor([0.5, 0.9, 0.7], dtype=f32),
            "gt_ignore": torch.tensor([False, True, False])}


def _check(b, want):
    for name in FIELDS:
        got = getattr(b, name)
        assert got.dtype == want[name].dtype and torch.equal(got, want[name]), name
    assert b.counts == (3, 3, 3) and [len(p) for p in b.preds] == [0, 2, 1] and [len(t) for t in b.tgts] == [2, 0, 1]
    assert all(x.mode == "xyxy" for x in b.preds + b.tgts)


def test_flattening_against_tensors_written_out_by_hand():
    preds, tgts = _batch("iscrowd")
    b = CS.flatten_batch(preds, tgts, "iscrowd", True, 0, num_classes=4)
    _check(b, _expected(0, resized=True))
    assert b.preds[2].size == (200, 100) and torch.equal(b.preds[2].bbox, b.dt_box[2:])
    _check(CS.flatten_batch(preds, tgts, "iscrowd", True, 3, num_classes=4), _expected(3, resized=True))      # a second call
    _check(CS.flatten_batch(preds, tgts), _expected(0, resized=True))                                         # the defaults
    with pytest.raises(ValueError, match=re.escape("prediction labels must lie in [0, 3), got 1 .. 3")):
        CS.flatten_batch(preds, tgts, "iscrowd", True, 0, num_classes=3)
    preds[2].get_field("labels")[0] = 0
    with pytest.raises(ValueError, match=re.escape("target labels must lie in [0, 3), got 1 .. 3")):
        CS.flatten_batch(preds, tgts, "iscrowd", True, 0, num_classes=3)
    # the evaluators pass it their own running image count and their class range
    ev = CS.COCOStyleEvaluator(("bbox",), num_classes=4)
    ev.update(*_batch("iscrowd"))
    ev.update(*_batch("iscrowd"))
    assert (ev.num_images, ev.num_detections, ev.num_groundtruths) == (6, 6, 6)
    assert sorted(r["image"] for r in ev.records["bbox"]) == [0, 0, 1, 1, 2, 3, 3, 4, 4, 5]
    with pytest.raises(ValueError, match=re.escape("prediction labels must lie in [0, 3), got 1 .. 3")):
        CS.COCOStyleEvaluator(("bbox",), num_classes=3).update(*_batch("iscrowd"))


def test_flattening_in_the_voc_form():
    """`difficult` as the ignore field, no resizing, no class range"""
    preds, tgts = _batch("difficult")
    b = CS.flatten_batch(preds, tgts, "difficult", resize=False)
    _check(b, _expected(0, resized=False))
    assert b.preds[2].size == (100, 50)
    # the other field's name is not read: no target is ignored
    b = CS.flatten_batch(preds, tgts, "iscrowd", resize=False)
    assert torch.equal(b.gt_ignore, torch.zeros(3, dtype=torch.bool))


def test_flattening_an_empty_batch():
    b = CS.flatten_batch([], [])
    assert b.preds == [] and b.tgts == [] and b.counts == (0, 0, 0)
    for name, dtype, shape in (("dt_img", torch.int64, (0,)), ("gt_img", torch.int64, (0,)), ("dt_box", torch.float32, (0, 4)),
                               ("gt_box", torch.float32, (0, 4)), ("dt_label", torch.int64, (0,)), ("gt_label", torch.int64, (0,)),
                               ("dt_score", torch.float32, (0,)), ("gt_ignore", torch.bool, (0,))):
        got = getattr(b, name)
        assert got.dtype == dtype and tuple(got.shape) == shape and got.device.type == "cpu", name
    ev = CS.COCOStyleEvaluator(("bbox",), num_classes=4)
    ev.update([], [])
    assert ev.records == {"bbox": []} and (ev.num_images, ev.num_detections, ev.num_groundtruths) == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ the statistics table
def test_the_names_are_the_tuples_they_were():
    assert CS.STAT_NAMES == ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
    assert KO.STAT_NAMES == ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl")
    assert sorted(CS.STAT_ROWS) == ["bbox", "keypoints", "segm"] and CS.STAT_ROWS["segm"] == CS.STAT_ROWS["bbox"]


def _detection_formula(ev, iou_thrs, max_dets):
    """the twelve statistics as coco_style.summarize stated them before the table"""
    def stat(ap, thr=None, area=0, m=len(max_dets) - 1):
        s = ev["precision"] if ap else ev["recall"]
        if thr is not None:
            s = s[np.nonzero(np.isclose(iou_thrs, thr))[0]]
        s = s[:, :, :, area, m] if ap else s[:, :, area, m]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    return np.array([stat(1), stat(1, 0.5), stat(1, 0.75), stat(1, area=1), stat(1, area=2), stat(1, area=3),
                     stat(0, m=0), stat(0, m=1), stat(0, m=2), stat(0, area=1), stat(0, area=2), stat(0, area=3)])


def _keypoint_formula(ev, iou_thrs):
    """the ten statistics as keypoint_oks.summarize stated them before the table"""
    def stat(ap, thr=None, area=0):
        s = ev["precision"] if ap else ev["recall"]
        if thr is not None:
            s = s[np.nonzero(np.isclose(iou_thrs, thr))[0]]
        s = s[:, :, :, area, 0] if ap else s[:, :, area, 0]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    return np.array([stat(1), stat(1, 0.5), stat(1, 0.75), stat(1, area=1), stat(1, area=2),
                     stat(0), stat(0, 0.5), stat(0, 0.75), stat(0, area=1), stat(0, area=2)])


def _random_eval(rng, A, M):
    ev = {"precision": rng.rand(10, 101, 2, A, M), "recall": rng.rand(10, 2, A, M)}
    for a in ev.values():
        a[rng.rand(*a.shape) < 0.3] = -1
    ev["precision"][:, :, :, A - 1, :] = -1                      # one area range never filled
    ev["recall"][:, :, A - 1, :] = -1
    return ev


def test_the_table_gives_both_of_the_formulas_it_replaced():
    rng = np.random.RandomState(5)
    ev = _random_eval(rng, A=4, M=3)
    got = CS.summarize(ev, CS.IOU_THRS, CS.STAT_ROWS["bbox"])
    np.testing.assert_array_equal(got, _detection_formula(ev, CS.IOU_THRS, CS.MAX_DETS))
    np.testing.assert_array_equal(CS.summarize(ev), got)                                        # the defaults: the twelve
    assert got[5] == -1.0 and got[11] == -1.0 and (got[:5] > 0).all() and len(set(got[6:9])) == 3
    ev = _random_eval(rng, A=3, M=1)
    got = CS.summarize(ev, KO.IOU_THRS, CS.STAT_ROWS["keypoints"])
    np.testing.assert_array_equal(got, _keypoint_formula(ev, KO.IOU_THRS))
    np.testing.assert_array_equal(KO.summarize(ev), got)
    assert got.shape == (10,) and got[4] == -1.0 and got[9] == -1.0 and (got[:4] > 0).all()


def test_nothing_filled_gives_minus_one_everywhere():
    for iou_type, (A, M) in (("bbox", (4, 3)), ("segm", (4, 3)), ("keypoints", (3, 1))):
        ev = {"precision": -np.ones((10, 101, 2, A, M)), "recall": -np.ones((10, 2, A, M))}
        got = CS.summarize(ev, CS.IOU_THRS, CS.STAT_ROWS[iou_type])
        np.testing.assert_array_equal(got, -np.ones(len(CS.STAT_ROWS[iou_type])))
