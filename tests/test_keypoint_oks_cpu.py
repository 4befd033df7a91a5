"""Keypoint evaluation (OKS) without a GPU: the numpy path (_eval_cpu.eval_oks through _C.eval_oks) and the evaluator
(data/datasets/evaluation/keypoint_oks.py) against the literal loops of tests/oks_refs.py, hand cases, the rules around the
similarity, keypoints.json there and back, and tools/evaluate_keypoints.py both ways.

Tolerance for OKS values, numpy against the loops (and device against numpy, tests/test_keypoint_oks_gpu.py): both sides
form e[k] from the same IEEE operations, so e is bit-equal; each exp is within 1 ulp of the true value (glibc documents
< 1 ulp for exp; numpy's own vector exp claims the same); the terms lie in (0, 1] and are added in the same order, so
|a - b| <= 2 (K + 1) 2^-52.  Where every e is 0 both sides give exactly 1.0.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import oks_refs as R
from maskrcnn_benchmark import _C
from maskrcnn_benchmark.data.datasets import evaluation as E
from maskrcnn_benchmark.data.datasets.evaluation import coco_results as CR
from maskrcnn_benchmark.data.datasets.evaluation import keypoint_oks as KO
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.keypoint import PersonKeypoints

@pytest.mark.parametrize("K", [1, 5, 17])
def test_numpy_path_against_the_literal_loops(K):
    pb = R.random_problems(100 + K, R.SHAPES, K, unlabelled=(1, 6))
    oks, area = R.run_op(pb)
    assert oks.dtype == np.float64 and oks.shape == pb["oks"].shape and area.shape == pb["dt_area"].shape
    diff = float(np.abs(oks - pb["oks"]).max())
    print("K = %d: largest |numpy - loops| = %.3g (bound %.3g), OKS in [%.3g, %.3g]" % (K, diff, R.oks_tolerance(K), oks.min(), oks.max()))
    assert diff <= R.oks_tolerance(K)
    assert 0.05 < np.mean(oks > 0.5) < 0.95                      # both sides of the thresholds are populated
    np.testing.assert_array_equal(area, pb["dt_area"])


def _one(dk, gk, box=(10.0, 20.0, 49.0, 79.0), area=1000.0, sigmas=None):
    """the OKS of one detection and one ground truth through _C.eval_oks, and the loops' value"""
    dk, gk = np.asarray(dk, np.float32).reshape(-1, 3), np.asarray(gk, np.float32).reshape(-1, 3)
    K = dk.shape[0]
    sig = np.asarray(R.SIGMAS[:K] if sigmas is None else sigmas, np.float64)
    pb = {"dt_kpts": dk[None], "gt_kpts": gk[None], "gt_boxes": np.asarray([box], np.float32), "gt_area": np.asarray([area]),
          "sigmas": sig, "dt_offset": np.array([0, 1], np.int32), "gt_offset": np.array([0, 1], np.int32),
          "iou_offset": np.array([0, 1], np.int64)}
    ref = R.oks({"keypoints": dk}, {"keypoints": gk, "box": np.asarray(box, np.float32), "area": area}, list(sig))
    return float(R.run_op(pb)[0][0]), ref


def test_hand_cases():
    rng = np.random.RandomState(3)
    gk = np.concatenate([rng.uniform(0, 100, (17, 2)), rng.randint(1, 3, (17, 1))], axis=1)
    dk = gk.copy()
    dk[:, 2] = np.nan                                            # the detection's third column is never read
    assert _one(dk, gk) == (1.0, 1.0)                            # detection == ground truth: exactly 1
    # one keypoint shifted by (3, 4): e = 25 / (2 sigma)^2 / (area + 2^-52) / 2
    sigma, area = 0.5, 50.0
    got, ref = _one([[13.0, 24.0, 0.0]], [[10.0, 20.0, 2.0]], area=area, sigmas=[sigma])
    want = math.exp(-(25.0 / ((2 * sigma) * (2 * sigma)) / (area + 2.0 ** -52) / 2))
    assert ref == want and abs(got - want) <= R.oks_tolerance(1) and 0.7 < want < 0.8
    # no visible keypoint: the distance to the box doubled around itself.  The box (10, 20, 49, 79) is x 10 w 40, y 20 h 60
    # in xywh, doubled: x in [-30, 90], y in [-40, 140]
    hidden = [[0.0, 0.0, 0.0]]
    assert _one([[89.0, -39.0, 1.0]], hidden, sigmas=[sigma]) == (1.0, 1.0)              # inside
    got, ref = _one([[-36.0, 0.0, 1.0]], hidden, area=area, sigmas=[sigma])             # 6 left of it
    want = math.exp(-(36.0 / 1.0 / (area + 2.0 ** -52) / 2))
    assert ref == want and abs(got - want) <= R.oks_tolerance(1) and want < 0.75
    got, ref = _one([[0.0, 148.0, 1.0]], hidden, area=area, sigmas=[sigma])             # 8 below it
    want = math.exp(-(64.0 / 1.0 / (area + 2.0 ** -52) / 2))
    assert ref == want and abs(got - want) <= R.oks_tolerance(1)
    # a hidden keypoint does not count when another one is visible: the far-off hidden point changes nothing
    assert _one([[10.0, 20.0, 0.0], [500.0, 500.0, 0.0]], [[10.0, 20.0, 1.0], [0.0, 0.0, 0.0]], sigmas=[sigma, sigma]) == (1.0, 1.0)


def test_the_cap_and_what_the_wrapper_refuses():
    assert _C.EVAL_OKS_MAX_K == 32 >= 17
    pb = R.random_problems(5, [(2, 2)], 33)                      # beyond the cap: the same numpy path
    assert float(np.abs(R.run_op(pb)[0] - pb["oks"]).max()) <= R.oks_tolerance(33)
    with pytest.raises(ValueError, match="K = 17"):
        _C.eval_oks(torch.zeros((1, 5, 3)), torch.zeros((1, 5, 3)), torch.zeros((1, 4)), torch.ones((1,), dtype=torch.float64),
                    R.SIGMAS, *(torch.tensor([0, 1], dtype=dt) for dt in (torch.int32, torch.int32, torch.int64)), 1)


# ------------------------------------------------------------------------------------------------ the evaluator
@pytest.fixture(scope="module")
def seeded():
    images = R.random_images(R.SEED, n_images=8, empty=R.EMPTY)
    return images, R.coco_stats(images, 3)


def test_evaluator_against_the_literal_loops(seeded):
    images, (ref_eval, ref_stats) = seeded
    v = R.assert_clear_of_the_thresholds(images)
    assert (v > 0.95).any() and (v < 0.5).any()
    ev = R.evaluate_boxlists(images)
    assert ev.iou_types == ("keypoints",) and (ev.num_images, ev.num_detections) == (8, sum(len(im["dt"]) for im in images))
    stats = ev.summarize()
    assert list(stats) == ["keypoints"] and stats["keypoints"].shape == (10,) and KO.STAT_NAMES == R.STAT_NAMES
    np.testing.assert_allclose(stats["keypoints"], ref_stats, rtol=0, atol=1e-12)
    assert 0.05 < stats["keypoints"][0] < 0.95
    # the match records themselves: every (image, category) pair the loops evaluate, nothing else
    recs = {(r["image"], r["category"]): r for r in ev.records["keypoints"]}
    assert sorted(recs) == sorted((i, k) for (k, a, i), e in ref_eval.items() if a == 0 and e is not None)
    assert not any(i == 5 for i, _ in recs)                      # the image without detections and ground truth
    for (k, a, i), e in ref_eval.items():
        if e is None:
            continue
        r = recs[(i, k)]
        np.testing.assert_array_equal(r["scores"], np.array(e["scores"], np.float64))
        np.testing.assert_array_equal(r["dt_match"][a], np.array(e["dt_match"], np.int32).reshape(10, -1))
        np.testing.assert_array_equal(r["dt_ignore"][a] != 0, np.array(e["dt_ignore"], bool).reshape(10, -1))
        np.testing.assert_array_equal(r["gt_ignore"][a] != 0, np.array(e["gt_ignore"], bool))


def _instance(rng, label=1, visible=True, crowd=0, area=3000.0):
    kp = np.concatenate([rng.uniform(40, 90, (17, 2)), np.full((17, 1), 2.0 if visible else 0.0)], axis=1).astype(np.float32)
    return {"label": label, "box": np.array([40, 40, 90, 90], np.float32), "keypoints": kp, "iscrowd": crowd, "area": area}


def _detection(g, score, shift=0.0):
    kp = g["keypoints"].copy()
    kp[:, :2] += shift
    kp[:, 2] = 1.0
    return {"label": g["label"], "score": score, "keypoints": kp}


def test_unlabelled_ground_truth_is_ignored_and_not_matched_again_and_a_crowd_is():
    rng = np.random.RandomState(0)
    for crowd in (0, 1):
        g = _instance(rng, visible=bool(crowd), crowd=crowd)      # no visible keypoint and no crowd / a crowd
        images = [{"dt": [_detection(g, 0.9), _detection(g, 0.8)], "gt": [g]}]
        ev = R.evaluate_boxlists(images, 2)
        (r,) = ev.records["keypoints"]
        assert r["gt_ignore"].tolist() == [[1], [1], [1]]
        first, second = r["dt_match"][:, :, 0], r["dt_match"][:, :, 1]
        assert (first == 0).all() and (r["dt_ignore"][:, :, 0] == 1).all()
        assert (second == (0 if crowd else -1)).all()
        ref = R.evaluate_img(images[0]["dt"], images[0]["gt"], R.SIGMAS, R.AREA_RNGS[0], 20)
        assert np.array_equal(r["dt_match"][0], np.array(ref["dt_match"]))
        # the unmatched second detection: its own area decides (50 x 50 keypoint extents at most: small, outside medium / large)
        if not crowd:
            assert r["dt_ignore"][0, :, 1].tolist() == [0] * 10 and r["dt_ignore"][2, :, 1].tolist() == [1] * 10


def test_the_cut_to_twenty_detections():
    rng = np.random.RandomState(1)
    g = _instance(rng)
    scores = [float(np.float32(s)) for s in rng.permutation(25) / 25.0]
    images = [{"dt": [_detection(g, s, shift=3.0) for s in scores], "gt": [g]}]
    ev = R.evaluate_boxlists(images, 2)
    (r,) = ev.records["keypoints"]
    assert r["scores"].tolist() == sorted(scores, reverse=True)[:20] and r["dt_match"].shape == (3, 10, 20)
    np.testing.assert_allclose(ev.summarize()["keypoints"], R.coco_stats(images, 2)[1], rtol=0, atol=1e-12)
    assert ev.num_detections == 25


def test_perfect_detections_and_no_detections():
    rng = np.random.RandomState(2)
    gts = [[_instance(rng, label=1 + (i + j) % 2, area=a) for j, a in enumerate((2000.0, 5000.0, 20000.0))] for i in range(3)]
    perfect = [{"dt": [_detection(g, 0.5 + 0.1 * j) for j, g in enumerate(gt)], "gt": gt} for gt in gts]
    stats = R.evaluate_boxlists(perfect).summarize()["keypoints"]
    np.testing.assert_allclose(stats, np.ones(10), rtol=0, atol=2.0 ** -52)      # (precision is tp / (tp + fp + 2^-52))
    stats = R.evaluate_boxlists([{"dt": [], "gt": gt} for gt in gts]).summarize()["keypoints"]
    np.testing.assert_array_equal(stats, np.zeros(10))


def test_what_update_refuses():
    rng = np.random.RandomState(4)
    g = _instance(rng)
    preds, tgts = R.to_boxlists([{"dt": [_detection(g, 0.9)], "gt": [g]}])
    with pytest.raises(ValueError, match="K = 5"):
        KO.KeypointOKSEvaluator(2, sigmas=R.SIGMAS[:5]).update(preds, tgts)
    bare = BoxList(tgts[0].bbox, tgts[0].size)
    bare.add_field("labels", tgts[0].get_field("labels"))
    with pytest.raises(ValueError, match="ground-truth keypoints"):
        KO.KeypointOKSEvaluator(2).update(preds, [bare])
    # a prediction made at another size is resized to the target's, keypoints included
    small = preds[0].resize((100, 80))
    a, b = KO.KeypointOKSEvaluator(2), KO.KeypointOKSEvaluator(2)
    a.update(preds, tgts)
    b.update([small], tgts)
    assert np.array_equal(a.records["keypoints"][0]["dt_match"], b.records["keypoints"][0]["dt_match"])
    assert (a.records["keypoints"][0]["dt_match"] == 0).all()


def test_the_ground_truth_area_falls_back_to_the_box():
    rng = np.random.RandomState(6)
    g = _instance(rng, area=51.0 * 51.0)                           # the xywh area of the box (40, 40, 90, 90)
    preds, tgts = R.to_boxlists([{"dt": [_detection(g, 0.9, shift=4.0)], "gt": [g]}])
    without = BoxList(tgts[0].bbox, tgts[0].size)
    for f in ("labels", "keypoints"):
        without.add_field(f, tgts[0].get_field(f))
    a, b = KO.KeypointOKSEvaluator(2), KO.KeypointOKSEvaluator(2)
    a.update(preds, tgts)
    b.update(preds, [without])
    for key in ("dt_match", "dt_ignore", "gt_ignore"):
        assert np.array_equal(a.records["keypoints"][0][key], b.records["keypoints"][0][key])
    # ... and to the mask's pixel count before that: a 30 x 20 mask is small, so the ground truth is ignored in medium and large
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    planes = torch.zeros((1, 160, 200), dtype=torch.uint8)
    planes[0, 40:60, 40:70] = 1
    without.add_field("masks", SegmentationMask(planes, (200, 160), mode="mask"))
    c = KO.KeypointOKSEvaluator(2)
    c.update(preds, [without])
    assert c.records["keypoints"][0]["gt_ignore"].tolist() == [[0], [1], [1]] and b.records["keypoints"][0]["gt_ignore"].tolist() == [[0], [0], [1]]


# ------------------------------------------------------------------------------------------------ tables
def test_tables_the_keypoint_one_under_its_own_names_and_the_others_unchanged():
    stats = {"bbox": np.arange(12) / 16.0, "keypoints": np.arange(10) / 8.0}
    text = E.format_stats(stats)
    bbox = "bbox\n" + "".join("  %-6s %8.4f\n" % (n, v) for n, v in zip(E.STAT_NAMES, stats["bbox"]))
    kps = "keypoints\n" + "".join("  %-6s %8.4f\n" % (n, v) for n, v in zip(R.STAT_NAMES, stats["keypoints"]))
    assert text == "\n" + bbox + kps and E.format_stats({"bbox": stats["bbox"]}) == "\n" + bbox
    assert "  AR50     0.7500\n" in kps and "APs" not in kps
    rng = np.random.RandomState(2)
    g = _instance(rng)
    ev = R.evaluate_boxlists([{"dt": [_detection(g, 0.9)], "gt": [g]}], 2)
    res = E.finish_coco(ev)
    assert list(res.results) == ["keypoints"] and list(res.results["keypoints"]) == ["AP", "AP50", "AP75", "APm", "APl"]
    # (one true positive: precision 1 / (1 + 2^-52), pycocotools' own epsilon)
    assert abs(res.results["keypoints"]["AP"] - 1.0) <= 2.0 ** -52 and res.results["keypoints"]["APl"] == -1.0
    assert repr(res) == "\nTask: keypoints\nAP, AP50, AP75, APm, APl\n1.0000, 1.0000, 1.0000, 1.0000, -1.0000\n"


# ------------------------------------------------------------------------------------------------ keypoints.json
def _dataset(length=5):
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset

    return SyntheticCOCODataset(length=length, height=120, width=160, num_classes=3, min_objects=1, max_objects=4, with_masks=False,
                                with_keypoints=True)


def _predictions(dataset, seed=8):
    g = torch.Generator().manual_seed(seed)
    preds = []
    for i in range(len(dataset)):
        t = dataset.get_groundtruth(i)
        kp = t.get_field("keypoints").keypoints.repeat(2, 1, 1)
        kp[:, :, :2] += torch.randn(kp[:, :, :2].shape, generator=g) * 4.0
        p = BoxList(t.bbox.repeat(2, 1), t.size)
        p.add_field("scores", torch.rand((len(p),), generator=g))
        p.add_field("labels", t.get_field("labels").repeat(2))
        p.add_field("keypoints", PersonKeypoints(kp, t.size))
        preds.append(p if i != 2 else p[:0])                      # an image without detections
    return preds


def test_a_result_file_reproduces_the_direct_evaluation(tmp_path):
    dataset = _dataset()
    preds = _predictions(dataset)
    tgts = [dataset.get_groundtruth(i) for i in range(len(dataset))]
    direct = KO.KeypointOKSEvaluator(3)
    direct.update(preds, tgts)
    writer = CR.COCOResultsWriter(dataset, ("keypoints",))
    writer.update(preds, list(range(len(dataset))))
    path = writer.save(str(tmp_path))["keypoints"]
    loaded = KO.load_keypoint_results(path, dataset)
    assert [len(b) for b in loaded] == [len(p) for p in preds]
    for b, p in zip(loaded, preds):
        assert torch.equal(b.get_field("keypoints").keypoints, p.get_field("keypoints").keypoints.reshape(-1, 17, 3))
        assert torch.equal(b.get_field("scores"), p.get_field("scores")) and torch.equal(b.get_field("labels"), p.get_field("labels"))
        if len(b):
            xy = b.get_field("keypoints").keypoints[:, :, :2]
            assert torch.equal(b.bbox, torch.cat([xy.min(dim=1)[0], xy.max(dim=1)[0]], dim=1))       # the keypoint extents
    again = KO.KeypointOKSEvaluator(3)
    again.update(loaded, tgts)
    assert len(again.records["keypoints"]) == len(direct.records["keypoints"]) > 0
    for a, b in zip(again.records["keypoints"], direct.records["keypoints"]):
        assert (a["image"], a["category"]) == (b["image"], b["category"])
        for key in ("scores", "dt_match", "dt_ignore", "gt_ignore"):
            assert np.array_equal(a[key], b[key]), key
    res = KO.evaluate_keypoint_file(dataset, path, output_folder=str(tmp_path / "scored"), batch=2)
    np.testing.assert_array_equal([res.results["keypoints"][n] for n in ("AP", "AP50", "AP75", "APm", "APl")],
                                  direct.summarize()["keypoints"][:5])
    assert 0.0 < res.results["keypoints"]["AP"] < 1.0
    assert "Task: keypoints" in open(str(tmp_path / "scored" / "coco_results.txt")).read()
    entries = json.load(open(path))
    with pytest.raises(ValueError, match="image_id"):
        KO.load_keypoint_results([dict(entries[0], image_id=99)], dataset)
    with pytest.raises(ValueError, match="multiple of 3"):
        KO.load_keypoint_results([dict(entries[0], keypoints=entries[0]["keypoints"][:50])], dataset)
    # the file's order is kept inside an image
    flipped = KO.load_keypoint_results(entries[::-1], dataset)
    assert torch.equal(flipped[0].get_field("scores"), loaded[0].get_field("scores").flip(0))


# ------------------------------------------------------------------------------------------------ the ways in
class _Stub(torch.nn.Module):
    """a detector's output, without the detector: the ground truth's keypoints, shifted, as detections"""

    def __init__(self, dataset):
        super().__init__()
        self.dataset, self.seen = dataset, 0

    def forward(self, images):
        out = []
        for _ in images.image_sizes:
            t = self.dataset.get_groundtruth(self.seen)
            self.seen += 1
            kp = t.get_field("keypoints").keypoints.clone()
            kp[:, :, :2] += 1.5
            b = BoxList(t.bbox.clone(), t.size)
            b.add_field("scores", torch.linspace(0.9, 0.5, len(t)))
            b.add_field("labels", t.get_field("labels").clone())
            b.add_field("keypoints", PersonKeypoints(kp, t.size))
            out.append(b)
        return out


def _loader(dataset):
    from maskrcnn_benchmark.data.synthetic import BatchCollator

    return torch.utils.data.DataLoader(dataset, batch_size=2, shuffle=False, num_workers=0, collate_fn=BatchCollator(0))


def test_inference_with_keypoint_oks(tmp_path):
    from maskrcnn_benchmark.engine.inference import inference

    dataset = _dataset(3)
    folder = str(tmp_path / "out")
    res = inference(_Stub(dataset), _loader(dataset), "synthetic", iou_types=("bbox",), device="cpu", output_folder=folder,
                    keypoint_oks=True)
    assert list(res.results) == ["bbox", "keypoints"] and res.results["bbox"]["AP"] == 1.0
    assert 0.0 < res.results["keypoints"]["AP"] <= 1.0
    assert {"bbox.json", "keypoints.json", "coco_results.txt"} <= set(os.listdir(folder))
    text = open(os.path.join(folder, "coco_results.txt")).read()
    assert "Task: keypoints" in text and "keypoints\n  AP  " in text and "  ARl  " in text
    scored = KO.evaluate_keypoint_file(dataset, os.path.join(folder, "keypoints.json"))
    assert scored.results["keypoints"] == res.results["keypoints"]
    # the default: no keypoints row, no keypoints.json; and "keypoints" among the iou types is still refused
    plain = inference(_Stub(dataset), _loader(dataset), "synthetic", iou_types=("bbox",), device="cpu",
                      output_folder=str(tmp_path / "plain"))
    assert list(plain.results) == ["bbox"] and os.listdir(str(tmp_path / "plain")).count("keypoints.json") == 0
    with pytest.raises(NotImplementedError, match="keypoints"):
        inference(_Stub(dataset), _loader(dataset), "synthetic", iou_types=("bbox", "keypoints"), device="cpu", keypoint_oks=True)


TINY = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4",
        "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16", "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", "32",
        "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", "(16, 16)", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "100",
        "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "50", "MODEL.ROI_HEADS.SCORE_THRESH", "0.0", "TEST.DETECTIONS_PER_IMG", "20",
        "INPUT.MIN_SIZE_TEST", "96", "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0",
        "DATALOADER.SIZE_DIVISIBILITY", "32"]


def test_the_tool_both_ways_prints_equal_keypoint_tables(tmp_path, capsys):
    import cpu_shim
    import evaluate_keypoints
    import test_net

    out = tmp_path / "run"
    torch.manual_seed(0)
    with cpu_shim.install():
        ran = evaluate_keypoints.main(["--config-file", "e2e_keypoint_rcnn_R_50_FPN_1x.yaml", "--images", "4"] + TINY
                                      + ["OUTPUT_DIR", str(out)])
    printed = capsys.readouterr().out
    assert "Task: bbox" in printed and "Task: keypoints" in printed
    assert not hasattr(test_net.inference, "__wrapped__") and test_net.inference.__name__ == "inference"        # put back
    folder = out / "inference" / "synthetic_coco_keypoints_val"
    assert {"bbox.json", "keypoints.json"} <= set(os.listdir(folder)) and len(json.load(open(folder / "keypoints.json"))) > 0
    scored = evaluate_keypoints.main(["--config-file", "e2e_keypoint_rcnn_R_50_FPN_1x.yaml", "--images", "4", "--results",
                                      str(folder)] + TINY)
    again = capsys.readouterr().out
    table = lambda text: text[text.index("Task: keypoints"):].split("\n")[:3]  # noqa: E731
    assert table(again) == table(printed) and "Task: bbox" not in again
    assert scored[0].results["keypoints"] == ran[0].results["keypoints"]
    with pytest.raises(SystemExit, match="no keypoints.json"):
        evaluate_keypoints.main(["--config-file", "e2e_keypoint_rcnn_R_50_FPN_1x.yaml", "--results", str(tmp_path)] + TINY)
