"""The real-data input path without a GPU: COCODataset over a COCO json and PNGs the test writes itself, the dataset
catalog, make_data_loader with its samplers and collators, and the two input paths (DETOPS_INPUT_PREP=host: Pillow on the
host; device: raw uint8 + records, here through the numpy implementation because the tensors are on the CPU) under one
`random` seed."""
import json
import math
import random

import numpy as np
import pytest
import torch

import cpu_shim
import image_prep_cases as C

Image = pytest.importorskip("PIL.Image")

from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog  # noqa: E402
from maskrcnn_benchmark.data import build as data_build  # noqa: E402
from maskrcnn_benchmark.data import collate_batch, make_data_loader  # noqa: E402
from maskrcnn_benchmark.data.datasets import COCODataset  # noqa: E402
from maskrcnn_benchmark.data.datasets.coco import rle_to_mask  # noqa: E402
from maskrcnn_benchmark.data.samplers import GroupedBatchSampler, IterationBasedBatchSampler  # noqa: E402
from maskrcnn_benchmark.data.transforms import build_transforms  # noqa: E402

SIZES = {1: (64, 48), 2: (40, 56), 3: (48, 48), 4: (72, 40)}     # id -> (w, h)


def _rect(x, y, w, h):
    return [x, y, x + w, y, x + w, y + h, x, y + h]


def _crowd_rle(w, h, x0, x1):
    """columns [x0, x1) of an h x w plane, column-major runs"""
    return {"size": [h, w], "counts": [x0 * h, (x1 - x0) * h, (w - x1) * h]}


@pytest.fixture(scope="module")
def coco_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("coco")
    rng = np.random.RandomState(11)
    images = []
    for i, (w, h) in SIZES.items():
        name = "img%d.png" % i
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), "RGB").save(str(root / name))
        images.append({"id": i, "file_name": name, "width": w, "height": h})
    ann = [
        # image 4 (listed first: ids are sorted by the dataset): a two-polygon instance, a plain one and a crowd with an RLE
        {"id": 1, "image_id": 4, "category_id": 7, "bbox": [5.0, 4.0, 30.0, 20.0], "area": 500.0, "iscrowd": 0,
         "segmentation": [_rect(5, 4, 12, 20), _rect(20, 6, 15, 16)]},
        {"id": 2, "image_id": 4, "category_id": 90, "bbox": [40.5, 10.0, 20.0, 25.5], "area": 510.0, "iscrowd": 0,
         "segmentation": [_rect(40.5, 10, 20, 25.5)]},
        {"id": 3, "image_id": 4, "category_id": 3, "bbox": [50.0, 0.0, 22.0, 40.0], "area": 880.0, "iscrowd": 1,
         "segmentation": _crowd_rle(72, 40, 50, 72)},
        # image 2: only degenerate boxes
        {"id": 4, "image_id": 2, "category_id": 3, "bbox": [3.0, 3.0, 1.0, 20.0], "area": 20.0, "iscrowd": 0,
         "segmentation": [_rect(3, 3, 1, 20)]},
        {"id": 5, "image_id": 2, "category_id": 7, "bbox": [8.0, 3.0, 20.0, 0.5], "area": 10.0, "iscrowd": 0,
         "segmentation": [_rect(8, 3, 20, 0.5)]},
        # image 1: one instance, partly outside the image (clipped), and a degenerate one next to it
        {"id": 6, "image_id": 1, "category_id": 3, "bbox": [30.0, 20.0, 50.0, 20.0], "area": 600.0, "iscrowd": 0,
         "segmentation": [_rect(30, 20, 50, 20)]},
        {"id": 7, "image_id": 1, "category_id": 90, "bbox": [2.0, 2.0, 30.0, 1.0], "area": 30.0, "iscrowd": 0,
         "segmentation": [_rect(2, 2, 30, 1)]},
    ]                                                             # image 3 has no annotations
    cats = [{"id": 90, "name": "c"}, {"id": 3, "name": "a"}, {"id": 7, "name": "b"}]
    path = root / "instances.json"
    path.write_text(json.dumps({"images": images, "annotations": ann, "categories": cats}))
    return str(path), str(root)


def test_filtering_and_label_mapping(coco_dir):
    ann_file, root = coco_dir
    ds = COCODataset(ann_file, root, True)
    assert ds.ids == [1, 4]                                       # no annotations (3) and only degenerate boxes (2) are dropped
    assert COCODataset(ann_file, root, False).ids == [1, 2, 3, 4]
    assert ds.json_category_id_to_contiguous_id == {3: 1, 7: 2, 90: 3} and ds.num_classes == 4
    assert ds.contiguous_category_id_to_json_id == {1: 3, 2: 7, 3: 90}
    assert ds.evaluation_style == "coco"
    assert ds.get_img_info(1) == {"id": 4, "file_name": "img4.png", "width": 72, "height": 40}


def test_items_follow_the_reference(coco_dir):
    ann_file, root = coco_dir
    ds = COCODataset(ann_file, root, True)
    img, target, idx = ds[1]                                      # image 4
    assert idx == 1 and img.size == (72, 40) and target.size == (72, 40) and target.mode == "xyxy"
    assert sorted(target.fields()) == ["labels", "masks"]
    assert target.get_field("labels").tolist() == [2, 3]          # the crowd is dropped
    # xywh -> xyxy with the reference's TO_REMOVE = 1
    assert target.bbox.tolist() == [[5.0, 4.0, 34.0, 23.0], [40.5, 10.0, 59.5, 34.5]]
    masks = target.get_field("masks")
    assert masks.mode == "poly" and len(masks) == 2 and len(masks.instances.polygons[0].polygons) == 2
    img, target, _ = ds[0]          # image 1: clipped to the image; the box of height 1 is empty as xyxy and is removed
    assert target.bbox.tolist() == [[30.0, 20.0, 63.0, 39.0]] and target.get_field("labels").tolist() == [1]
    assert len(target.get_field("masks")) == 1


def test_groundtruth_keeps_crowds_and_decodes_rle(coco_dir):
    ann_file, root = coco_dir
    ds = COCODataset(ann_file, root, False)
    gt = ds.get_groundtruth(3)                                    # image 4
    assert gt.size == (72, 40) and gt.get_field("labels").tolist() == [2, 3, 1]
    assert gt.get_field("iscrowd").tolist() == [0, 0, 1]
    assert gt.get_field("area").tolist() == [500.0, 510.0, 880.0]
    masks = gt.get_field("masks")
    assert masks.mode == "mask"
    planes = masks.get_mask_tensor()
    assert tuple(planes.shape) == (3, 40, 72)
    crowd = np.zeros((40, 72), dtype=np.uint8)
    crowd[:, 50:] = 1
    assert np.array_equal(planes[2].numpy(), crowd)
    assert int(planes[0].sum()) > 0 and int(planes[0][:, 40:].sum()) == 0
    plain = ds.get_groundtruth(0).get_field("masks")              # no RLE in the image: the polygons stay polygons
    assert plain.mode == "poly" and len(plain) == 2
    empty = ds.get_groundtruth(2)                                 # image 3
    assert len(empty) == 0 and not empty.has_field("masks")
    with pytest.raises(NotImplementedError, match="compressed RLE"):
        rle_to_mask({"size": [4, 4], "counts": "04"})
    assert rle_to_mask({"size": [2, 3], "counts": [1, 2, 3]}).tolist() == [[0, 1, 0], [1, 0, 0]]


def _cfg(name, opts=()):
    from maskrcnn_benchmark.engine.bench_step import load_cfg

    base = ["MODEL.DEVICE", "cpu", "MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 60, "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", 80,
            "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 8, "MODEL.RESNETS.WIDTH_PER_GROUP", 2,
            "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 8, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 16, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 4,
            "SOLVER.BASE_LR", 0.001, "SOLVER.MAX_ITER", 2, "SOLVER.IMS_PER_BATCH", 2, "INPUT.MIN_SIZE_TRAIN", (64, 72, 80),
            "INPUT.MAX_SIZE_TRAIN", 112, "INPUT.VERTICAL_FLIP_PROB_TRAIN", 0.5, "DATALOADER.NUM_WORKERS", 0,
            "DATALOADER.SIZE_DIVISIBILITY", 32, "DATASETS.TRAIN", (name,), "DATASETS.TEST", (name,)]
    return load_cfg("e2e_faster_rcnn_R_50_FPN_1x.yaml", base + list(opts))


@pytest.fixture()
def registered(coco_dir):
    DatasetCatalog.register("tiny_coco_train", *coco_dir)
    yield "tiny_coco_train"
    DatasetCatalog.REGISTERED.pop("tiny_coco_train", None)


def test_catalog(registered, coco_dir, monkeypatch):
    got = DatasetCatalog.get(registered)
    assert got == {"factory": "COCODataset", "args": {"ann_file": coco_dir[0], "root": coco_dir[1]}}
    std = DatasetCatalog.get("coco_2017_train")
    assert std["factory"] == "COCODataset" and std["args"]["ann_file"].endswith("coco/annotations/instances_train2017.json")
    assert std["args"]["root"].endswith("coco/train2017")
    assert "keypoints_coco_2014_minival" in DatasetCatalog.DATASETS and "coco_2014_valminusminival" in DatasetCatalog.DATASETS
    with pytest.raises(RuntimeError, match="not available"):
        DatasetCatalog.get("no_such_dataset")
    with pytest.raises(ValueError):
        DatasetCatalog.register("synthetic_mine", *coco_dir)


def _same_target(a, b):
    assert a.size == b.size and a.mode == b.mode and torch.equal(a.bbox, b.bbox)
    assert sorted(a.fields()) == sorted(b.fields())
    assert torch.equal(a.get_field("labels"), b.get_field("labels"))
    pa, pb = a.get_field("masks").instances.polygons, b.get_field("masks").instances.polygons
    assert len(pa) == len(pb)
    for x, y in zip(pa, pb):
        assert len(x.polygons) == len(y.polygons) and all(torch.equal(p, q) for p, q in zip(x.polygons, y.polygons))


def test_host_and_device_prep_agree_bit_for_bit(registered, monkeypatch):
    """the same seed: the same size choice and flips, in the same order, whichever path makes the pixels"""
    cfg = _cfg(registered)
    got = {}
    for mode in ("host", "device"):
        monkeypatch.setattr(collate_batch, "INPUT_PREP", mode)
        random.seed(1234)
        torch.manual_seed(99)                                     # the RandomSampler's order
        loader = make_data_loader(cfg, is_train=True)
        assert len(loader) == 2 and isinstance(loader.batch_sampler, IterationBasedBatchSampler)
        assert isinstance(loader.batch_sampler.batch_sampler, GroupedBatchSampler)
        got[mode] = [(images.to("cpu"), targets, ids) for images, targets, ids in loader]
        assert isinstance(loader.collate_fn, collate_batch.RawBatchCollator if mode == "device" else collate_batch.BatchCollator)
    assert len(got["host"]) == len(got["device"]) == 2
    sizes = set()
    for (hi, ht, hids), (di, dt, dids) in zip(got["host"], got["device"]):
        assert hids == dids and hi.image_sizes == [tuple(s) for s in di.image_sizes]
        assert hi.tensors.shape[-1] % 32 == 0 and hi.tensors.shape[-2] % 32 == 0
        assert np.array_equal(C.bits(hi.tensors), C.bits(di.tensors))
        for a, b in zip(ht, dt):
            _same_target(a, b)
        sizes.update(tuple(s) for s in hi.image_sizes)
    assert len(sizes) > 1                                         # the multi-scale choice was exercised


def test_deferred_transform_makes_the_same_draws(coco_dir):
    """item by item, 12 draws: destination size and flip bits of the deferred pipeline = what the host pipeline did"""
    ann_file, root = coco_dir
    cfg = _cfg("unused")
    host = COCODataset(ann_file, root, True, build_transforms(cfg, True))
    dev = COCODataset(ann_file, root, True, build_transforms(cfg, True, device_prep=True))
    seen = set()
    for seed in range(12):
        random.seed(seed)
        h_img, h_t, _ = host[seed % 2]
        after_host = random.random()
        random.seed(seed)
        d_img, d_t, _ = dev[seed % 2]
        assert random.random() == after_host                      # the generator is in the same state afterwards
        assert (d_img.size[1], d_img.size[0]) == tuple(h_img.shape[1:]) and d_img.data.dtype == np.uint8
        _same_target(h_t, d_t)
        seen.add(d_img.flip)
    assert seen == {0, 1, 2, 3}


def test_registered_dataset_trains_the_narrow_cpu_model(registered, monkeypatch):
    from maskrcnn_benchmark.engine.bench_step import build_training

    monkeypatch.setattr(collate_batch, "INPUT_PREP", "device")
    cfg = _cfg(registered)
    random.seed(7)
    torch.manual_seed(0)
    model, optimizer, scheduler, _ = build_training(cfg, torch.device("cpu"))
    loader = make_data_loader(cfg, is_train=True)
    steps = 0
    with cpu_shim.install():
        for images, targets, _ in loader:
            assert isinstance(images, collate_batch.RawImageBatch)
            losses = model(images.to("cpu"), [t.to("cpu") for t in targets])
            total = sum(losses.values())
            assert all(math.isfinite(float(v.detach())) for v in losses.values()) and float(total.detach()) > 0
            optimizer.zero_grad()
            total.backward()
            optimizer.step()
            scheduler.step()
            steps += 1
    assert steps == 2


def test_test_loader_hands_out_groundtruth_targets(registered, monkeypatch):
    monkeypatch.setattr(collate_batch, "INPUT_PREP", "host")
    cfg = _cfg(registered, ["TEST.IMS_PER_BATCH", 1])
    loader = make_data_loader(cfg, is_train=False, length=16)     # one loader, as tools/test_net.py asks for it
    assert isinstance(loader, torch.utils.data.DataLoader) and len(loader.dataset) == 4
    images, targets, ids = list(loader)[3]                        # image 4: 72 x 40 -> MIN_SIZE_TEST 800 capped by MAX_SIZE_TEST
    assert ids == (3,) and targets[0].size == (72, 40) and targets[0].get_field("iscrowd").tolist() == [0, 0, 1]
    assert images.image_sizes[0][0] < images.image_sizes[0][1]
    assert make_data_loader(cfg, is_train=False, dataset_name=registered).dataset.ids == [1, 2, 3, 4]
    two = _cfg(registered, ["DATASETS.TEST", (registered, "coco_2017_val")])
    with pytest.raises(ValueError, match="dataset_name"):
        make_data_loader(two, is_train=False)
    with pytest.raises(ValueError, match="not in DATASETS.TEST"):
        make_data_loader(cfg, is_train=False, dataset_name="coco_2017_val")
    assert len(make_data_loader(two, is_train=False, dataset_name=registered).dataset) == 4


def test_synthetic_names_still_get_the_synthetic_loader():
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset
    from maskrcnn_benchmark.engine.bench_step import load_cfg

    cfg = load_cfg("e2e_faster_rcnn_R_50_FPN_1x.yaml", ["MODEL.DEVICE", "cpu", "INPUT.MIN_SIZE_TRAIN", (64,), "INPUT.MAX_SIZE_TRAIN", 96])
    assert cfg.DATASETS.TRAIN == ("synthetic_coco_train",)
    loader = make_data_loader(cfg, is_train=True, length=3)
    assert isinstance(loader.dataset, SyntheticCOCODataset) and len(loader.dataset) == 3
    assert isinstance(make_data_loader(cfg, is_train=False, length=2).dataset, SyntheticCOCODataset)
    assert data_build._is_synthetic(()) and not data_build._is_synthetic(("coco_2017_train",))


def test_samplers():
    sampler = torch.utils.data.sampler.SequentialSampler(range(7))
    grouped = GroupedBatchSampler(sampler, [0, 1, 0, 1, 0, 1, 0], 2)
    batches = list(grouped)
    assert batches == [[0, 2], [1, 3], [4, 6], [5]] and len(grouped) == 4
    assert list(GroupedBatchSampler(sampler, [0, 1, 0, 1, 0, 1, 0], 2, drop_uneven=True)) == [[0, 2], [1, 3], [4, 6]]
    it = IterationBasedBatchSampler(grouped, num_iterations=6, start_iter=1)
    assert len(it) == 5 and list(it) == [[0, 2], [1, 3], [4, 6], [5], [0, 2]]


def test_test_net_evaluates_a_registered_dataset(registered, tmp_path, capsys, monkeypatch):
    """tools/test_net.py as it stands, DATASETS.TEST naming a real dataset: images through the host transforms, detections
    scored against get_groundtruth (the crowd and its RLE plane included) at the original image sizes"""
    import test_net

    monkeypatch.setattr(collate_batch, "INPUT_PREP", "device")
    opts = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4",
            "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16", "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", "32",
            "MODEL.ROI_MASK_HEAD.CONV_LAYERS", "(16, 16)", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "100",
            "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "50", "MODEL.ROI_HEADS.SCORE_THRESH", "0.0", "TEST.DETECTIONS_PER_IMG", "20",
            "INPUT.MIN_SIZE_TEST", "96", "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0",
            "DATALOADER.SIZE_DIVISIBILITY", "32", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", "4", "DATASETS.TEST", "('%s',)" % registered,
            "OUTPUT_DIR", str(tmp_path)]
    torch.manual_seed(0)
    with cpu_shim.install():
        results = test_net.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml"] + opts)
    out = capsys.readouterr().out
    assert "Task: bbox" in out and "Task: segm" in out
    assert "AR100" in open(tmp_path / "inference" / registered / "coco_results.txt").read()
    assert all(-1 <= v <= 1 for task in results[0].results.values() for v in task.values())
