"""COCO result files without a GPU: the compressed RLE string coding (include/detops.h, "Compressed RLE strings") as the
literal coder of tests/rle_string_refs.py and as the numpy path, the reference's own bbox and keypoint entries
(tests/golden/coco_results_reference.json, made by tests/golden/make_golden_coco_results.py), the segmentation entries
through the test-only decoder, the compressed mode of MaskPostProcessorCOCOFormat, and the inference loop,
tools/test_net.py and tools/write_results.py writing the files (the detector's operators served by the oracle: tests/cpu_shim.py)."""
import json
import logging
import os
import re

import numpy as np
import pytest
import torch

import bbox_aug_cases as B
import cpu_shim
import rle_string_refs as R

from maskrcnn_benchmark import _C, _rle_cpu
from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog
from maskrcnn_benchmark.data.datasets.evaluation import coco_results as CR
from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import (Masker, MaskPostProcessorCOCOFormat, paste_masks_torch,
                                                                      rle_encode)
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.keypoint import PersonKeypoints

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_results_reference.json")


def _flat(masks):
    counts = np.concatenate([np.asarray(m, np.int32) for m in masks]) if masks else np.zeros(0, np.int32)
    return counts, np.concatenate([[0], np.cumsum([len(m) for m in masks])]).astype(np.int64)


def _numpy_strings(masks):
    return _rle_cpu.to_str_list(*_rle_cpu.rle_strings(*_flat(masks)))


# ------------------------------------------------------------------------------------------------ the coding
def test_the_eight_vectors_through_the_literal_coder_and_numpy():
    for counts, text in R.VECTORS:
        assert R.rle_to_string(counts) == text, counts
        assert R.rle_from_string(text) == counts, counts
    assert _numpy_strings([c for c, _ in R.VECTORS]) == [t for _, t in R.VECTORS]
    assert [_numpy_strings([c])[0] for c, _ in R.VECTORS] == [t for _, t in R.VECTORS]


def test_seeded_masks_numpy_equals_the_literal_coder_byte_for_byte():
    masks = R.seeded_masks()
    assert len(masks) == 2000 and {len(m) for m in masks} == set(range(1, 41))
    counts, run_offset = _flat(masks)
    data, byte_offset = _rle_cpu.rle_strings(counts, run_offset)
    strings = _rle_cpu.to_str_list(data, byte_offset)
    want = [R.rle_to_string(m) for m in masks]
    assert strings == want
    assert data.dtype == np.uint8 and bytes(data) == "".join(want).encode("ascii")
    assert byte_offset.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    for m, s in zip(masks, strings):
        assert R.rle_from_string(s) == m
    # the closed form, per value; the draws reach every length and both signs on both sides of every group boundary
    x = _rle_cpu.deltas(counts, run_offset)
    lengths = _rle_cpu.code_lengths(x)
    assert lengths.tolist() == [R.code_length(int(v)) for v in x]
    assert int(lengths.sum()) == data.size
    assert set(lengths.tolist()) == set(range(1, 8))
    for k in range(1, 8):                                     # every length with both signs
        assert ((lengths == k) & (x >= 0)).any() and ((lengths == k) & (x < 0)).any(), k
    for v in R.EDGE_VALUES:                                   # the values at the group boundaries, as they are and negated
        assert (x == v).any() and (x == -v).any(), v
    for k in range(1, 6):                                     # ... which lie on both sides of every boundary they touch
        half = 1 << (5 * k - 1)
        assert R.code_length(half - 1) == k and R.code_length(half) == k + 1 and half - 1 in R.EDGE_VALUES and half in R.EDGE_VALUES
        assert R.code_length(-half) == k and R.code_length(-half - 1) == k + 1
    k = _rle_cpu.deltas(np.arange(8, dtype=np.int32), np.array([0, 8]))          # runs 0 to 3 around the `i > 2` rule
    assert k.tolist() == [0, 1, 2, 2, 2, 2, 2, 2]
    # the product's wrapper on CPU tensors is the numpy path
    d2, o2 = _C.rle_strings(torch.from_numpy(counts), torch.from_numpy(run_offset))
    assert np.array_equal(d2.numpy(), data) and np.array_equal(o2.numpy(), byte_offset)
    assert _C.rle_string_list(d2, o2) == want


def test_the_rule_is_greater_than_two_per_mask():
    """runs 0, 1, 2 are coded as they are; run 3 is the first difference; the rule starts over with every mask"""
    a = [9, 9, 9, 9, 9]
    assert R.rle_to_string(a) == "99900"
    assert _numpy_strings([a, a, [], a[:3], a[:4]]) == ["99900", "99900", "", "999", "9990"]
    with pytest.raises(ValueError):
        _rle_cpu.rle_strings(np.zeros(3, np.int32), np.array([0, 2]))
    assert _numpy_strings([]) == []


# ------------------------------------------------------------------------------------------------ the entries
class _Dataset(object):
    def __init__(self, images, categories):
        self.images = images
        self.id_to_img_map = {i: im["id"] for i, im in enumerate(images)}
        self.contiguous_category_id_to_json_id = categories

    def get_img_info(self, index):
        return self.images[index]


def _golden():
    g = json.load(open(GOLDEN))
    dataset = _Dataset(g["images"], {int(k): v for k, v in g["categories"].items()})
    predictions = []
    for p in g["predictions"]:
        b = BoxList(torch.tensor(p["boxes"], dtype=torch.float32).reshape(-1, 4), tuple(p["size"]), mode="xyxy")
        b.add_field("scores", torch.tensor(p["scores"], dtype=torch.float32))
        b.add_field("labels", torch.tensor(p["labels"], dtype=torch.int64))
        b.add_field("keypoints", PersonKeypoints(torch.tensor(p["keypoints"], dtype=torch.float32).reshape(-1, 17, 3), tuple(p["size"])))
        predictions.append(b)
    return g, dataset, predictions


def test_bbox_and_keypoint_entries_reproduce_the_reference_exactly():
    g, dataset, predictions = _golden()
    assert [len(p) for p in predictions] == [7, 0, 4]
    bbox = CR.prepare_for_coco_detection(predictions, dataset)
    kps = CR.prepare_for_coco_keypoint(predictions, dataset)
    assert bbox == g["bbox"] and kps == g["keypoints"]                       # ids, every float, order
    assert [list(e) for e in bbox] == [list(e) for e in g["bbox"]]           # and the keys' order
    assert [list(e) for e in kps] == [list(e) for e in g["keypoints"]]
    assert {e["image_id"] for e in bbox} == {139, 632} and {e["category_id"] for e in bbox} <= {1, 3, 18, 44, 90}
    assert json.loads(json.dumps(bbox)) == g["bbox"]
    # the streaming writer, two batches, is the same lists
    writer = CR.COCOResultsWriter(dataset, ("bbox", "keypoints"))
    writer.update(predictions[:2], [0, 1])
    writer.update(predictions[2:], [2])
    assert writer.results["bbox"] == g["bbox"] and writer.results["keypoints"] == g["keypoints"]
    with pytest.raises(ValueError):
        CR.COCOResultsWriter(dataset, ("bbox", "boxes"))


def _segm_case(dense):
    """two images of 97 x 131 and 40 x 33 (h x w), predictions made in a frame of another size with unequal ratios"""
    g = torch.Generator().manual_seed(7)
    images = [{"id": 11, "width": 131, "height": 97}, {"id": 5, "width": 33, "height": 40}, {"id": 8, "width": 20, "height": 20}]
    dataset = _Dataset(images, {1: 2, 2: 7, 3: 50})
    predictions = []
    for im, n, size in zip(images, (5, 3, 0), ((262, 200), (50, 57), (31, 31))):
        w, h = size
        lo = torch.rand(n, 2, generator=g) * torch.tensor([w * 0.7, h * 0.7]) - 4.0
        boxes = torch.cat([lo, lo + torch.rand(n, 2, generator=g) * torch.tensor([w * 0.5, h * 0.5]) + 3.0], 1)
        p = BoxList(boxes, size, mode="xyxy")
        p.add_field("scores", torch.rand(n, generator=g))
        p.add_field("labels", torch.randint(1, 4, (n,), generator=g))
        if dense:
            p.add_field("mask", torch.rand(n, 1, im["height"], im["width"], generator=g) > 0.6)
        else:
            p.add_field("mask", torch.rand(n, 1, 28, 28, generator=g))
        predictions.append(p)
    return dataset, predictions


@pytest.mark.parametrize("dense", [True, False], ids=["dense_planes", "probabilities_28"])
def test_segmentation_entries_decode_to_the_pasted_planes(dense):
    dataset, predictions = _segm_case(dense)
    entries = CR.prepare_for_coco_segmentation(predictions, dataset)
    assert len(entries) == 8
    at = 0
    for index, p in enumerate(predictions):
        info = dataset.get_img_info(index)
        h, w = info["height"], info["width"]
        q = p.resize((w, h))
        planes = p.get_field("mask") if dense else paste_masks_torch(q.get_field("mask"), q.bbox, h, w, 0.5, 1)
        for k in range(len(p)):
            e = entries[at]
            assert list(e) == ["image_id", "category_id", "segmentation", "score"]        # the reference's dict
            assert list(e["segmentation"]) == ["size", "counts"] and isinstance(e["segmentation"]["counts"], str)
            assert e["image_id"] == info["id"] and e["segmentation"]["size"] == [h, w]
            assert e["category_id"] == dataset.contiguous_category_id_to_json_id[int(p.get_field("labels")[k])]
            assert e["score"] == p.get_field("scores").tolist()[k]
            want = rle_encode(planes[k, 0])
            assert R.rle_from_string(e["segmentation"]["counts"]) == want["counts"]
            assert sum(want["counts"]) == h * w
            at += 1
    assert at == len(entries)
    json.dumps(entries)


def test_masks_that_are_neither_image_planes_nor_probability_maps_raise():
    """bool planes pasted at the network's input size (POSTPROCESS_MASKS on a resized image) must not be pasted again as if
    they were probabilities; nor floating maps that are not square"""
    dataset, predictions = _segm_case(dense=True)
    p = predictions[0]
    w, h = p.size
    for bad in (torch.zeros(len(p), 1, h, w, dtype=torch.bool), torch.zeros(len(p), 1, 28, 28, dtype=torch.uint8),
                torch.zeros(len(p), 1, 28, 14)):
        q = p.copy_with_fields(["scores", "labels"])
        q.add_field("mask", bad)
        with pytest.raises(ValueError, match="neither planes"):
            CR.prepare_for_coco_segmentation([q], dataset)
    q = p.copy_with_fields(["scores", "labels"])
    q.add_field("mask", torch.rand(len(p), 1, 14, 14).half())                  # any floating dtype, any M
    assert len(CR.prepare_for_coco_segmentation([q], dataset)) == len(p)


def test_plane_runs_is_rle_encode_of_every_plane():
    g = torch.Generator().manual_seed(3)
    planes = torch.rand(6, 9, 7, generator=g) > 0.5
    planes[1] = False
    planes[2] = True
    planes[3, 0, 0] = True
    planes[4, 0, 0] = False
    counts, run_offset = CR.plane_runs(planes)
    off = run_offset.tolist()
    assert counts.dtype == torch.int32 and run_offset.dtype == torch.int64
    for i in range(6):
        assert counts[off[i]:off[i + 1]].tolist() == rle_encode(planes[i])["counts"]
    assert counts[off[1]:off[2]].tolist() == [63] and counts[off[2]:off[3]].tolist() == [0, 63]
    c0, r0 = CR.plane_runs(planes[:0])
    assert c0.numel() == 0 and r0.tolist() == [0]


def test_a_dataset_without_maps_uses_index_and_label():
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset

    ds = SyntheticCOCODataset(length=2, height=40, width=48, num_classes=5)
    p = BoxList(torch.tensor([[1.0, 2.0, 11.0, 22.0]]), (96, 80))
    p.add_field("scores", torch.tensor([0.5]))
    p.add_field("labels", torch.tensor([4]))
    (e,) = CR.prepare_for_coco_detection([BoxList(torch.zeros(0, 4), (96, 80)), p], ds)
    assert e == {"image_id": 1, "category_id": 4, "bbox": [0.5, 1.0, 6.0, 11.0], "score": 0.5}   # xywh with the reference's + 1


# ------------------------------------------------------------------------------------------------ the post-processor
def test_mask_post_processor_compressed_against_uncompressed():
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(7, 4, 28, 28, generator=g) * 3
    boxes = []
    for n, size in ((4, (131, 97)), (0, (50, 40)), (3, (33, 40))):
        lo = torch.rand(n, 2, generator=g) * torch.tensor([size[0] * 0.6, size[1] * 0.6])
        b = BoxList(torch.cat([lo, lo + 5 + torch.rand(n, 2, generator=g) * 30], 1), size)
        b.add_field("labels", torch.randint(1, 4, (n,), generator=g))
        b.add_field("scores", torch.rand(n, generator=g))
        boxes.append(b)
    default = MaskPostProcessorCOCOFormat(Masker(0.5, 1))
    assert default.compressed is False
    plain = default(logits, boxes)
    explicit = MaskPostProcessorCOCOFormat(Masker(0.5, 1), compressed=False)(logits, boxes)
    packed = MaskPostProcessorCOCOFormat(Masker(0.5, 1), compressed=True)(logits, boxes)
    assert [p.get_field("mask") for p in plain] == [p.get_field("mask") for p in explicit]
    for a, b, box in zip(plain, packed, boxes):
        ma, mb = a.get_field("mask"), b.get_field("mask")
        assert len(ma) == len(mb) == len(box)
        for u, c in zip(ma, mb):
            assert isinstance(u["counts"], list) and isinstance(c["counts"], str)          # the default is today's output
            assert list(c) == ["size", "counts"] and c["size"] == u["size"] == [box.size[1], box.size[0]]
            assert R.rle_from_string(c["counts"]) == u["counts"]
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))


# ------------------------------------------------------------------------------------------------ the loop and the tool
NAME = "tiny_coco_results"
MASK_OPTS = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4",
             "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16", "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", "32",
             "MODEL.ROI_MASK_HEAD.CONV_LAYERS", "(16, 16)", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "100",
             "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "50", "MODEL.ROI_HEADS.SCORE_THRESH", "0.0", "TEST.DETECTIONS_PER_IMG", "20",
             "INPUT.MIN_SIZE_TEST", "96", "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0",
             "DATALOADER.SIZE_DIVISIBILITY", "32", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", "4"]


@pytest.fixture()
def registered(tmp_path):
    pytest.importorskip("PIL.Image")
    data = tmp_path / "data"
    data.mkdir()
    DatasetCatalog.register(NAME, *B.write_coco(str(data)))
    yield NAME
    DatasetCatalog.REGISTERED.pop(NAME, None)


def _check_files(folder, types, sizes):
    out = {}
    for t in types:
        entries = json.load(open(os.path.join(folder, t + ".json")))
        assert isinstance(entries, list)
        for e in entries:
            assert e["image_id"] in sizes and e["category_id"] in (3, 7, 9) and isinstance(e["score"], float)
            if t == "segm":
                w, h = sizes[e["image_id"]]
                assert e["segmentation"]["size"] == [h, w]
                assert sum(R.rle_from_string(e["segmentation"]["counts"])) == h * w
            if t == "bbox":
                assert len(e["bbox"]) == 4
        out[t] = entries
    return out


def test_inference_writes_bbox_and_segm_files_next_to_the_table(registered, tmp_path, caplog):
    from maskrcnn_benchmark.data import make_data_loader
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.engine.inference import inference

    cfg = load_cfg("e2e_mask_rcnn_R_50_FPN_1x.yaml", MASK_OPTS + ["DATASETS.TEST", "('%s',)" % registered])
    model = B.build_model(cfg, "cpu")
    folder = str(tmp_path / "out")
    with cpu_shim.install(), caplog.at_level(logging.INFO, logger="maskrcnn_benchmark"):
        res = inference(model, make_data_loader(cfg, is_train=False), registered, iou_types=("bbox", "segm"), device="cpu",
                        output_folder=folder)
    assert set(res.results) == {"bbox", "segm"}
    files = _check_files(folder, ("bbox", "segm"), B.SIZES)
    text = "\n".join(r.getMessage() for r in caplog.records)
    matched = int(re.search(r"Matched (\d+) detections", text).group(1))
    assert matched > 0 and len(files["bbox"]) == len(files["segm"]) == matched
    assert os.path.exists(os.path.join(folder, "coco_results.txt")) and os.path.exists(os.path.join(folder, "coco_results.pth"))
    assert sorted({e["image_id"] for e in files["bbox"]}) == [1, 2]


class _KeypointStub(torch.nn.Module):
    """a detector's output, without the detector: 3 detections with keypoints per image"""

    def forward(self, images):
        out = []
        for i, (h, w) in enumerate(images.image_sizes):
            b = BoxList(torch.tensor([[1.0, 2.0, 20.0, 30.0]] * 3) + i, (w, h))
            b.add_field("scores", torch.tensor([0.9, 0.8, 0.7]))
            b.add_field("labels", torch.tensor([1, 1, 1]))
            b.add_field("keypoints", PersonKeypoints(torch.arange(3 * 17 * 3, dtype=torch.float32).reshape(3, 17, 3), (w, h)))
            out.append(b)
        return out


def _synthetic_loader(length=3):
    from maskrcnn_benchmark.data.synthetic import BatchCollator, SyntheticCOCODataset

    ds = SyntheticCOCODataset(length=length, height=40, width=48, num_classes=3, min_objects=1, max_objects=2, with_masks=False,
                              with_keypoints=True)
    return torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, collate_fn=BatchCollator(0))


def test_results_only_writes_keypoints_and_builds_no_evaluator(tmp_path, monkeypatch):
    from maskrcnn_benchmark.engine import inference as I

    def refuse(*a, **k):
        raise AssertionError("evaluate=False must not get here")

    monkeypatch.setattr(I, "COCOStyleEvaluator", refuse)
    monkeypatch.setattr(I, "check_scope", refuse)
    monkeypatch.setattr(I, "finish_coco", refuse)
    folder = str(tmp_path / "res")
    paths = I.inference(_KeypointStub(), _synthetic_loader(), "synthetic", iou_types=("bbox", "keypoints"), device="cpu",
                        output_folder=folder, evaluate=False)
    assert sorted(paths) == ["bbox", "keypoints"] and sorted(os.listdir(folder)) == ["bbox.json", "keypoints.json"]
    bbox, kps = (json.load(open(paths[t])) for t in ("bbox", "keypoints"))
    assert len(bbox) == len(kps) == 9 and [e["image_id"] for e in kps] == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert all(len(e["keypoints"]) == 51 and list(e) == ["image_id", "category_id", "keypoints", "score"] for e in kps)
    assert bbox[3]["bbox"] == [2.0, 3.0, 20.0, 29.0]


def test_results_only_needs_a_folder_and_evaluation_still_refuses_keypoints(tmp_path):
    from maskrcnn_benchmark.engine.inference import inference

    with pytest.raises(ValueError, match="output_folder"):
        inference(_KeypointStub(), _synthetic_loader(), "synthetic", iou_types=("bbox",), device="cpu", evaluate=False)
    with pytest.raises(NotImplementedError, match="keypoints"):
        inference(_KeypointStub(), _synthetic_loader(), "synthetic", iou_types=("bbox", "keypoints"), device="cpu",
                  output_folder=str(tmp_path))


def _strip_annotations(registered):
    ann_file = DatasetCatalog.REGISTERED[registered]["ann_file"]
    data = json.load(open(ann_file))
    del data["annotations"]
    with open(ann_file, "w") as f:
        json.dump(data, f)


def test_write_results_tool_on_a_set_without_annotations(registered, tmp_path, capsys):
    """results only from the command line: tools/test_net.py's own main(), every option of it, with evaluate=False"""
    import write_results

    _strip_annotations(registered)
    out = tmp_path / "run"
    torch.manual_seed(0)
    with cpu_shim.install():
        results = write_results.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml"] + MASK_OPTS
                                     + ["DATASETS.TEST", "('%s',)" % registered, "OUTPUT_DIR", str(out)])
    folder = str(out / "inference" / registered)
    assert sorted(os.listdir(folder)) == ["bbox.json", "segm.json"]
    files = _check_files(folder, ("bbox", "segm"), B.SIZES)
    assert len(files["bbox"]) == len(files["segm"]) > 0
    assert sorted(results[0]) == ["bbox", "segm"] and "Task:" not in capsys.readouterr().out
    with pytest.raises(SystemExit, match="OUTPUT_DIR"):
        write_results.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml"] + MASK_OPTS)
    import test_net

    assert test_net.inference is write_results.test_net.inference and not hasattr(test_net.inference, "keywords")   # put back


def test_test_net_with_an_output_dir_writes_the_files_next_to_its_tables(registered, tmp_path, capsys):
    import test_net

    out = tmp_path / "run"
    torch.manual_seed(0)
    with cpu_shim.install():
        test_net.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml"] + MASK_OPTS
                      + ["DATASETS.TEST", "('%s',)" % registered, "OUTPUT_DIR", str(out)])
    folder = str(out / "inference" / registered)
    assert {"bbox.json", "segm.json", "coco_results.txt"} <= set(os.listdir(folder))
    files = _check_files(folder, ("bbox", "segm"), B.SIZES)
    assert len(files["bbox"]) == len(files["segm"]) > 0 and "Task: segm" in capsys.readouterr().out
