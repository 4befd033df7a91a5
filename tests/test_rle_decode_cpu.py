"""Reading COCO result files back, without a GPU: the numpy decoder of compressed RLE strings against the literal decoder of
tests/rle_string_refs.py, its status bits, bit rows straight from runs against bit rows from planes, result files through
COCOResultsWriter.save -> load_results -> the evaluator against the direct evaluation of the same predictions,
tools/evaluate_results.py against the tables of the tools/test_net.py run that wrote the files, and a COCO-json crowd
annotation whose `counts` is a compressed string.  Everything is exact equality."""
import json
import os
import re

import numpy as np
import pytest
import torch

import eval_cases as C
import rle_decode_cases as K
import rle_string_refs as R
from maskrcnn_benchmark import _C, _eval_cpu, _rle_cpu
from maskrcnn_benchmark.data.datasets.evaluation import COCOStyleEvaluator
from maskrcnn_benchmark.data.datasets.evaluation import coco_results as CR
from maskrcnn_benchmark.structures.rle_masks import RLEMasks


def decode(strings, hw=None):
    return _rle_cpu.rle_decode(*_rle_cpu.from_str_list(strings), hw)


# ------------------------------------------------------------------------------------------------ the decoder
def test_numpy_decoder_equals_the_literal_one_on_the_seeded_strings():
    masks, strings = K.seeded_strings()
    assert len(strings) == 2000
    counts, run_offset, status = decode(strings)
    assert counts.dtype == np.int32 and run_offset.dtype == np.int64 and status.dtype == np.int32 and not status.any()
    lengths = set()
    for n, s in enumerate(strings):
        want = R.rle_from_string(s)
        assert counts[run_offset[n]:run_offset[n + 1]].tolist() == want == masks[n]       # encode, then decode: the runs
        x = [want[i] - (want[i - 2] if i > 2 else 0) for i in range(len(want))]
        lengths |= {(R.code_length(v), v < 0) for v in x}
    assert lengths == {(k, neg) for k in range(1, 8) for neg in (False, True)}            # 1 to 7 bytes, both signs
    # the wrappers on CPU tensors are the numpy path
    c2, o2 = _C.rle_string_decode(*K.tensors(strings))
    assert np.array_equal(c2.numpy(), counts) and np.array_equal(o2.numpy(), run_offset)
    c3, o3 = _C.rle_string_decode_list(strings)
    assert torch.equal(c3, c2) and torch.equal(o3, o2)
    # and the inverse of the coder, as tensors
    data, byte_offset = _C.rle_strings(c2, o2)
    assert _C.rle_string_list(data, byte_offset) == strings


def test_the_eight_vectors_decode():
    for runs, text in R.VECTORS:
        counts, run_offset, status = decode([text])
        assert counts.tolist() == runs == R.rle_from_string(text) and run_offset.tolist() == [0, len(runs)] and status.tolist() == [0]
    counts, run_offset, status = decode([t for _, t in R.VECTORS])
    assert counts.tolist() == [v for r, _ in R.VECTORS for v in r] and not status.any()


def test_one_long_mask_next_to_short_ones():
    masks, strings = K.long_and_short()
    counts, run_offset, status = decode(strings)
    assert run_offset.tolist() == [0, 0, 1, 50001, 50004, 50004] and not status.any()
    assert counts.tolist() == [v for m in masks for v in m]


def test_every_status_bit_by_a_string_of_its_own():
    strings = [s for s, _, _, _ in K.MALFORMED]
    hw = [h for _, h, _, _ in K.MALFORMED]
    for bit in (K.BAD_BYTE, K.TRUNCATED, K.LONG_VALUE, K.BAD_RUN, K.BAD_SUM):
        assert any(b == bit for _, _, b, _ in K.MALFORMED), bit
    counts, run_offset, status = decode(strings, hw)
    assert status.tolist() == [whole for _, _, _, whole in K.MALFORMED]
    assert all(whole & bit == bit for _, _, bit, whole in K.MALFORMED)
    for n, (s, h, bit, whole) in enumerate(K.MALFORMED):          # alone, the same status; without hw, no BAD_SUM
        assert decode([s], [h])[2].tolist() == [whole]
        assert decode([s])[2].tolist() == [whole & ~K.BAD_SUM]
    assert (_rle_cpu.BAD_BYTE, _rle_cpu.TRUNCATED, _rle_cpu.LONG_VALUE, _rle_cpu.BAD_RUN, _rle_cpu.BAD_SUM) == (1, 2, 4, 8, 16)
    # a malformed string leaves its well-formed neighbours alone, and the error names it
    mixed = ["053", "/", "?`0a0A", "P", "P]aP1"]
    counts, run_offset, status = decode(mixed)
    assert status.tolist() == [0, K.BAD_BYTE | K.TRUNCATED | K.BAD_RUN, 0, K.TRUNCATED, 0]
    assert counts[:3].tolist() == [0, 5, 3] and counts[run_offset[2]:run_offset[3]].tolist() == [15, 16, 17, 1]
    with pytest.raises(ValueError, match=r"mask 1 .*status 11.*DETOPS_RLE_BAD_BYTE.*DETOPS_RLE_TRUNCATED.*2 of 5"):
        _C.rle_string_decode(*K.tensors(mixed))
    with pytest.raises(ValueError, match=r"mask 2 .*status 16.*DETOPS_RLE_BAD_SUM"):
        _C.rle_string_decode_list(["053", "44", "053"], [(2, 4), (4, 2), (3, 3)])
    with pytest.raises(ValueError, match="byte_offset"):
        _C.rle_string_decode(torch.zeros(3, dtype=torch.uint8), torch.tensor([0, 2]))
    # no strings, and only empty strings
    assert [a.tolist() for a in decode([])] == [[], [0], []]
    assert [a.tolist() for a in decode(["", ""], [(0, 7), (1, 1)])] == [[], [0, 0, 0], [0, K.BAD_SUM]]


# ------------------------------------------------------------------------------------------------ bit rows from runs
def test_pack_from_runs_equals_pack_from_planes():
    planes, runs = K.pack_cases()
    shapes = [p.shape for p in planes]
    assert {(7, 1), (33, 17), (64, 80), (20, 130), (5, 64), (130, 20)} <= set(shapes)
    for p, r in zip(planes, runs):
        assert sum(r) == p.size and np.array_equal(K.plane_of(r, *p.shape), p)
    assert any(0 in r[1:-1] for r in runs)                                       # zero-length runs in the middle
    assert any(len(r) == 3 and r[1] > 5 * p.shape[0] and (r[0] // p.shape[0]) < 64 < ((r[0] + r[1]) // p.shape[0])
               for p, r in zip(planes, runs))                                    # one run over whole columns across column 64
    want = _eval_cpu.mask_pack([p[None] for p in planes])
    got = _eval_cpu.mask_pack_rle(*[t.numpy() for t in K.run_tensors(runs)], shapes)
    wrapped = _C.mask_pack_rle(*K.run_tensors(runs), shapes)
    for w, g, t, name in zip(want, got, wrapped, ("words", "word_offset", "hw", "area", "extent")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
        assert np.array_equal(t.numpy().view(w.dtype), w), name
    # plane_runs (the writer's run-length coder) makes the same runs as the literal coder, canonical ones
    counts, run_offset = CR.plane_runs(torch.from_numpy(np.stack([planes[2]] * 2)))
    assert counts.tolist() == K.runs_of(planes[2]) * 2 and run_offset.tolist() == [0, len(counts) // 2, len(counts)]
    with pytest.raises(ValueError):
        _C.mask_pack_rle(*K.run_tensors(runs), shapes[:-1])


def test_rle_masks_field():
    planes, runs = K.pack_cases()
    three = [runs[3], runs[3][:1] + [0, 0] + runs[3][1:], [20 * 130]]
    m = RLEMasks.from_lists(three, (130, 20))
    assert len(m) == 3 and m.size == (130, 20) and m.resize((130, 20)) is m and m.to("cpu").counts.tolist() == m.counts.tolist()
    with pytest.raises(ValueError):
        m.resize((65, 10))
    with pytest.raises(ValueError):
        RLEMasks.from_lists([[5, 5]], (130, 20))
    s = RLEMasks.from_strings([R.rle_to_string(r) for r in three], (130, 20))
    assert s.counts.tolist() == m.counts.tolist() and s.run_offset.tolist() == m.run_offset.tolist()
    with pytest.raises(ValueError, match="DETOPS_RLE_BAD_SUM"):
        RLEMasks.from_strings([R.rle_to_string(three[0])], (20, 130 + 1))
    picked = m[torch.tensor([2, 0])]
    assert picked.counts.tolist() == three[2] + three[0] and picked.run_offset.tolist() == [0, 1, 1 + len(three[0])]
    assert len(m[1]) == 1 and m[1].counts.tolist() == three[1] and len(m[torch.tensor([True, False, True])]) == 2
    words = _C.mask_pack_rle(m.counts, m.run_offset, m.hw())[0]
    assert torch.equal(words[:len(words) // 3], words[len(words) // 3:2 * len(words) // 3])      # zero-length runs only toggle


# ------------------------------------------------------------------------------------------------ through files
class _Dataset(object):
    """make_images() as a COCO-shaped dataset: image ids and category ids that are not the indices and labels"""
    evaluation_style = "coco"
    num_classes = C.NUM_CLASSES

    def __init__(self, images):
        self.targets = C.to_boxlists(images)[1]
        self.id_to_img_map = {i: 1000 + 7 * (len(images) - i) for i in range(len(images))}       # descending ids
        self.json_category_id_to_contiguous_id = {11 * k: k for k in range(1, C.NUM_CLASSES)}
        self.contiguous_category_id_to_json_id = {v: k for k, v in self.json_category_id_to_contiguous_id.items()}
        self.infos = [{"id": self.id_to_img_map[i], "width": im["size"][0], "height": im["size"][1]} for i, im in enumerate(images)]

    def __len__(self):
        return len(self.targets)

    def get_img_info(self, index):
        return self.infos[index]

    def get_groundtruth(self, index):
        return self.targets[index]


@pytest.fixture(scope="module")
def round_trip(tmp_path_factory):
    """seeded predictions (boxes on quarter pixels: xywh <-> xyxy is exact in fp32; dense planes, and M = 28 probabilities
    for images 1 and 4), their direct evaluation, and the files COCOResultsWriter saved"""
    images = C.make_images()
    dataset = _Dataset(images)
    preds, _ = C.to_boxlists(images)
    g = torch.Generator().manual_seed(3)
    for i, p in enumerate(preds):
        p.bbox = torch.round(p.bbox * 4) / 4
        if i in (1, 4):
            p.add_field("mask", torch.sigmoid(3 * torch.randn(len(p), 1, 28, 28, generator=g)))
    direct = COCOStyleEvaluator(("bbox", "segm"), C.NUM_CLASSES)
    direct.update(preds[:5], dataset.targets[:5])
    direct.update(preds[5:], dataset.targets[5:])
    direct.summarize()
    writer = CR.COCOResultsWriter(dataset, ("bbox", "segm"))
    writer.update(preds[:3], [0, 1, 2])
    writer.update(preds[3:], list(range(3, len(preds))))
    paths = writer.save(str(tmp_path_factory.mktemp("results")))
    return dataset, preds, direct, paths


def _same_evaluation(got, want, iou_type):
    ra, rb = C.records_by_key(got, iou_type), C.records_by_key(want, iou_type)
    assert sorted(ra) == sorted(rb) and len(rb) > 0
    for key in rb:
        for field in ("scores", "dt_match", "dt_ignore", "gt_ignore"):
            np.testing.assert_array_equal(ra[key][field], rb[key][field], err_msg="%s %s %s" % (iou_type, key, field))
    np.testing.assert_array_equal(got.stats[iou_type], want.stats[iou_type])
    assert got.stats[iou_type].shape == (12,) and 0 < got.stats[iou_type][0] < 1


@pytest.mark.parametrize("iou_type", ["bbox", "segm"])
def test_files_round_trip_to_the_same_evaluation(round_trip, iou_type):
    dataset, preds, direct, paths = round_trip
    loaded = CR.load_results(paths[iou_type], dataset, iou_type)
    assert [len(p) for p in loaded] == [len(p) for p in preds] and len(loaded) == len(dataset)
    for p, q in zip(preds, loaded):                                # dataset order; file order inside an image
        assert q.mode == "xyxy" and q.size == p.size
        assert torch.equal(q.get_field("scores"), p.get_field("scores")) and torch.equal(q.get_field("labels"), p.get_field("labels"))
        if iou_type == "bbox":
            assert torch.equal(q.bbox, p.bbox)
        else:
            assert isinstance(q.get_field("mask"), RLEMasks) and len(q.get_field("mask")) == len(p)
    ev = COCOStyleEvaluator((iou_type,), C.NUM_CLASSES)
    ev.update(loaded[:3], dataset.targets[:3])
    ev.update(loaded[3:], dataset.targets[3:])
    ev.summarize()
    _same_evaluation(ev, direct, iou_type)


def test_evaluate_result_files_and_what_load_results_refuses(round_trip, tmp_path):
    dataset, preds, direct, paths = round_trip
    res = CR.evaluate_result_files(dataset, paths, output_folder=str(tmp_path / "scored"), batch=3)
    for t in ("bbox", "segm"):
        assert list(res.results[t].values()) == [float(v) for v in direct.stats[t][:6]]
    assert sorted(os.listdir(tmp_path / "scored")) == ["coco_results.pth", "coco_results.txt"]
    only = CR.evaluate_result_files(dataset, {"segm": json.load(open(paths["segm"]))})      # entries serve as a path
    assert list(only.results) == ["segm"] and only.results["segm"] == res.results["segm"]
    with pytest.raises(NotImplementedError, match="keypoints"):
        CR.evaluate_result_files(dataset, {"bbox": paths["bbox"], "keypoints": "keypoints.json"})
    with pytest.raises(NotImplementedError, match="keypoints"):
        CR.load_results([], dataset, "keypoints")
    segm = json.load(open(paths["segm"]))
    first = dict(segm[0])
    # uncompressed lists are read too, and a segm entry without bbox gets the full-image box
    as_list = dict(first, segmentation={"size": first["segmentation"]["size"], "counts": R.rle_from_string(first["segmentation"]["counts"])})
    a, b = CR.load_results([first], dataset, "segm"), CR.load_results([as_list], dataset, "segm")
    index = [i for i, p in enumerate(a) if len(p)][0]
    assert a[index].get_field("mask").counts.tolist() == b[index].get_field("mask").counts.tolist()
    W, H = a[index].size
    assert a[index].bbox.tolist() == [[0.0, 0.0, W - 1.0, H - 1.0]] and [len(p) for p in a].count(0) == len(dataset) - 1
    for bad, what in ((dict(first, image_id=5), "image_id"), (dict(first, category_id=2), "category_id"),
                      (dict(first, segmentation=[[1, 1, 5, 1, 5, 5]]), "polygons"),
                      (dict(first, segmentation={"size": [H + 1, W], "counts": first["segmentation"]["counts"]}), "size"),
                      (dict(first, segmentation={"size": [H, W], "counts": first["segmentation"]["counts"] + "1"}), "DETOPS_RLE_BAD_SUM")):
        with pytest.raises(ValueError, match=what):
            CR.load_results([bad], dataset, "segm")
    with pytest.raises(ValueError, match="bbox"):
        CR.load_results([first], dataset, "bbox")


# ------------------------------------------------------------------------------------------------ the tool
def _tables(text):
    return re.findall(r"Task: \w+\n[^\n]*\n[^\n]*\n", text)


def test_the_tool_prints_the_tables_of_the_run_that_wrote_the_files(tmp_path, capsys):
    pytest.importorskip("PIL.Image")
    import bbox_aug_cases as B
    import cpu_shim
    import evaluate_results
    import test_net
    from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog

    name = "rle_decode_tool_val"
    data = tmp_path / "data"
    data.mkdir()
    DatasetCatalog.register(name, *B.write_coco(str(data)))
    opts = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4",
            "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16", "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", "32",
            "MODEL.ROI_MASK_HEAD.CONV_LAYERS", "(16, 16)", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "100",
            "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "50", "MODEL.ROI_HEADS.SCORE_THRESH", "0.0", "TEST.DETECTIONS_PER_IMG", "20",
            "INPUT.MIN_SIZE_TEST", "96", "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0",
            "DATALOADER.SIZE_DIVISIBILITY", "32", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", "4", "DATASETS.TEST", "('%s',)" % name]
    out = tmp_path / "run"
    try:
        torch.manual_seed(0)
        with cpu_shim.install():
            test_net.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml"] + opts + ["OUTPUT_DIR", str(out)])
        written = _tables(capsys.readouterr().out)
        folder = out / "inference" / name
        assert {"bbox.json", "segm.json"} <= set(os.listdir(folder)) and len(json.load(open(folder / "segm.json"))) > 0
        evaluate_results.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml", "--results", str(folder)] + opts)
        scored = _tables(capsys.readouterr().out)
        with pytest.raises(SystemExit, match="no bbox.json"):
            evaluate_results.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml", "--results", str(tmp_path)] + opts)
    finally:
        DatasetCatalog.REGISTERED.pop(name, None)
    assert [t.split("\n")[0] for t in written] == ["Task: bbox", "Task: segm"]
    assert scored == written


# ------------------------------------------------------------------------------------------------ a compressed crowd
def test_a_compressed_crowd_annotation_loads(tmp_path):
    from maskrcnn_benchmark.data.datasets.coco import COCODataset, decode_rle, rle_to_mask

    w, h = 72, 40
    runs = [50 * h + 3, 17, 20 + 9 * h, 2 * h, (w - 62) * h]            # part of column 50 and columns 60, 61 as one crowd
    assert sum(runs) == w * h

    def dataset(counts):
        ann = [{"id": 1, "image_id": 4, "category_id": 7, "bbox": [5.0, 4.0, 30.0, 20.0], "area": 500.0, "iscrowd": 0,
                "segmentation": [[5, 4, 17, 4, 17, 24, 5, 24]]},
               {"id": 2, "image_id": 4, "category_id": 3, "bbox": [50.0, 0.0, 12.0, 40.0], "area": 463.0, "iscrowd": 1,
                "segmentation": {"size": [h, w], "counts": counts}}]
        path = tmp_path / ("crowd_%s.json" % type(counts).__name__)
        path.write_text(json.dumps({"images": [{"id": 4, "file_name": "img4.png", "width": w, "height": h}], "annotations": ann,
                                    "categories": [{"id": 3, "name": "a"}, {"id": 7, "name": "b"}]}))
        return COCODataset(str(path), str(tmp_path), False)

    as_string, as_list = dataset(R.rle_to_string(runs)).get_groundtruth(0), dataset(runs).get_groundtruth(0)
    a, b = as_string.get_field("masks").get_mask_tensor(), as_list.get_field("masks").get_mask_tensor()
    assert tuple(a.shape) == (2, h, w) and torch.equal(a, b) and int(a[1].sum()) == 17 + 2 * h
    assert np.array_equal(a[1].numpy(), K.plane_of(runs, h, w))
    assert as_string.get_field("iscrowd").tolist() == [0, 1]
    assert torch.equal(decode_rle({"size": [h, w], "counts": R.rle_to_string(runs)}), rle_to_mask({"size": [h, w], "counts": runs}))
    with pytest.raises(NotImplementedError, match="compressed RLE"):      # the plain decoder keeps refusing strings
        rle_to_mask({"size": [h, w], "counts": R.rle_to_string(runs)})
    with pytest.raises(ValueError, match="DETOPS_RLE_BAD_SUM"):
        decode_rle({"size": [h, w + 1], "counts": R.rle_to_string(runs)})
