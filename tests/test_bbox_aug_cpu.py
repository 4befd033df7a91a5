"""Test-time box augmentation without a GPU: the config node and yaml, the loader and the re-prepared RawImageBatch, the
torch formulation of the merge against the reference's own BoxList arithmetic and filter_results
(tests/golden/bbox_aug_reference.npz), and the two model-level identities on a 2-image COCO-json set with the narrow
random-init Faster R-CNN (the segmented NMS served by the oracle: tests/cpu_shim.py)."""
import numpy as np
import pytest
import torch

import bbox_aug_cases as B
import cpu_shim

from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog
from maskrcnn_benchmark.data import collate_batch, make_data_loader
from maskrcnn_benchmark.data.collate_batch import RawImageBatch
from maskrcnn_benchmark.data.transforms import RawImage, Resize, normalisation_table

NAME = "tiny_coco_bbox_aug"


@pytest.fixture()
def registered(tmp_path):
    pytest.importorskip("PIL.Image")                              # only the tests that write PNGs need Pillow
    DatasetCatalog.register(NAME, *B.write_coco(str(tmp_path)))
    yield NAME
    DatasetCatalog.REGISTERED.pop(NAME, None)


def test_config_node_and_yaml_load():
    from maskrcnn_benchmark.config import cfg
    from maskrcnn_benchmark.engine.bbox_aug import augmentation_passes
    from maskrcnn_benchmark.engine.bench_step import load_cfg

    aug = cfg.TEST.BBOX_AUG
    assert (aug.ENABLED, aug.H_FLIP, aug.SCALES, aug.MAX_SIZE, aug.SCALE_H_FLIP) == (False, False, (), 4000, False)
    tta = load_cfg("test_time_aug/e2e_faster_rcnn_R_50_FPN_1x.yaml")
    aug = tta.TEST.BBOX_AUG
    assert aug.ENABLED and aug.H_FLIP and aug.SCALE_H_FLIP and aug.MAX_SIZE == 2000
    assert aug.SCALES == (400, 500, 600, 700, 900, 1000, 1100, 1200)
    passes = augmentation_passes(tta)
    assert passes[:4] == [(800, 1333, False), (800, 1333, True), (400, 2000, False), (400, 2000, True)] and len(passes) == 18
    plain = load_cfg("e2e_faster_rcnn_R_50_FPN_1x.yaml")
    assert augmentation_passes(plain) == [(800, 1333, False)]
    from maskrcnn_benchmark.modeling.roi_heads.box_head.inference import make_roi_box_post_processor

    assert make_roi_box_post_processor(tta).bbox_aug_enabled and not make_roi_box_post_processor(plain).bbox_aug_enabled


def test_torch_formulation_maps_every_box_like_the_reference():
    """threshold below every score: every (row, class >= 1) pair is a candidate, and the candidates are the reference's
    clipped, transposed and resized boxes bit for bit, segment by segment in row order"""
    fx = B.load_fixture()
    R, C = fx["scores"].shape
    boxes, scores, seg, longest = B.reference(fx, thresh=-1.0)
    merged = fx["merged"].view(R, C, 4)
    per_image = fx["row_offset"][::fx["T"]].tolist()
    want_b = torch.cat([merged[lo:hi, j] for lo, hi in zip(per_image[:-1], per_image[1:]) for j in range(1, C)])
    want_s = torch.cat([fx["scores"][lo:hi, j] for lo, hi in zip(per_image[:-1], per_image[1:]) for j in range(1, C)])
    assert torch.equal(B.bits(boxes), B.bits(want_b)) and torch.equal(scores, want_s)
    lengths = [hi - lo for lo, hi in zip(per_image[:-1], per_image[1:]) for _ in range(1, C)]
    assert seg.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist() and longest == max(lengths)


def test_torch_formulation_reproduces_the_reference_detections():
    fx = B.load_fixture()
    with cpu_shim.install():
        B.check_fixture_detections(fx, "cpu")


def test_merge_cases_are_well_formed_on_the_cpu():
    """the cases the device test runs: `_C.bbox_aug_merge` on CPU tensors is the torch formulation, segments are in row order
    and the empty shapes are served"""
    from maskrcnn_benchmark import _C

    for name, args in B.MERGE_CASES.items():
        case = B.make_case(**args)
        boxes, scores, seg, longest = _C.bbox_aug_merge(case["boxes"], case["scores"], case["row_offset"], case["geom"],
                                                        case["ratio"], case["N"], case["T"], B.THRESH)
        C = case["scores"].shape[1]
        assert seg.dtype == torch.int32 and seg.numel() == case["N"] * (C - 1) + 1 and seg[0] == 0, name
        assert boxes.shape == (int(seg[-1]), 4) and scores.shape == (int(seg[-1]),), name
        want = int((case["scores"][:, 1:] > B.THRESH).sum())
        assert int(seg[-1]) == want and longest == int((seg[1:] - seg[:-1]).max()), name
        if name in ("nothing_passes", "no_rows"):
            assert want == 0
    with pytest.raises(ValueError):
        _C.bbox_aug_merge(case["boxes"], case["scores"], case["row_offset"][:-1], case["geom"], case["ratio"], case["N"],
                          case["T"], B.THRESH)


def test_loader_under_bbox_aug_is_deferred_whatever_the_switch(registered, monkeypatch):
    monkeypatch.setattr(collate_batch, "INPUT_PREP", "host")
    cfg = B.narrow_cfg(registered, "cpu", ["TEST.BBOX_AUG.ENABLED", True])
    loader = make_data_loader(cfg, is_train=False)
    assert isinstance(loader.collate_fn, collate_batch.RawBatchCollator)
    (images, targets, ids), = list(loader)
    assert isinstance(images, RawImageBatch) and len(images) == 2 and images.buffer.dtype == torch.uint8
    assert [t.size for t in targets] == [B.SIZES[1], B.SIZES[2]]           # ground truth at the original size
    plain = make_data_loader(B.narrow_cfg(registered, "cpu"), is_train=False)
    assert isinstance(plain.collate_fn, collate_batch.BatchCollator)      # the switch still rules without BBOX_AUG
    from maskrcnn_benchmark.engine.bench_step import load_cfg

    synthetic = load_cfg("e2e_faster_rcnn_R_50_FPN_1x.yaml", ["MODEL.DEVICE", "cpu", "TEST.BBOX_AUG.ENABLED", True])
    with pytest.raises(ValueError, match="synthetic"):
        make_data_loader(synthetic, is_train=False, length=2)
    from maskrcnn_benchmark.engine.bbox_aug import im_detect_bbox_aug

    with pytest.raises(ValueError, match="RawImageBatch"):
        im_detect_bbox_aug(None, torch.zeros(1, 3, 32, 32), "cpu", cfg)


def test_preparing_again_equals_a_fresh_pack_at_that_target():
    """one packed batch prepared at (size, flip) = the batch packed for that target from the start, byte for byte"""
    rng = np.random.RandomState(3)
    data = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for w, h in ((64, 48), (40, 56), (33, 33))]
    table = normalisation_table([102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0], True)
    base_resize = Resize(96, 128)
    base = RawImageBatch.pack([RawImage(d, base_resize.get_size((d.shape[1], d.shape[0]))[::-1]) for d in data], table, True, 32)
    once = base.on("cpu")
    assert once is base
    for min_size, max_size, flip in ((96, 128, False), (96, 128, True), (50, 4000, False), (131, 150, True), (20, 4000, True)):
        resize = Resize(min_size, max_size)
        fresh = RawImageBatch.pack([RawImage(d, resize.get_size((d.shape[1], d.shape[0]))[::-1], int(flip)) for d in data],
                                   table, True, 32).to("cpu")
        again = once.prepare(min_size, max_size, flip)
        assert again.image_sizes == fresh.image_sizes and again.tensors.shape == fresh.tensors.shape
        assert torch.equal(B.bits(again.tensors), B.bits(fresh.tensors)), (min_size, max_size, flip)
    assert torch.equal(B.bits(once.prepare(96, 128).tensors), B.bits(base.to("cpu").tensors))
    assert base.image_sizes == [(int(g[2]), int(g[3])) for g in base.geom.tolist()]      # preparing again changed nothing


def _same(a, b):
    assert a.size == b.size and torch.equal(B.bits(a.bbox), B.bits(b.bbox))
    assert torch.equal(a.get_field("scores"), b.get_field("scores")) and torch.equal(a.get_field("labels"), b.get_field("labels"))


def test_enabled_without_passes_is_plain_inference(registered, monkeypatch):
    monkeypatch.setattr(collate_batch, "INPUT_PREP", "device")
    with cpu_shim.install():
        plain, aug = B.plain_and_augmented(registered, "cpu", "nchw", [])
    for a, b in zip(plain, aug):
        _same(a, b)


def test_the_test_scale_twice_is_plain_inference_in_value(registered, monkeypatch):
    """SCALES = (MIN_SIZE_TEST,) with MAX_SIZE = MAX_SIZE_TEST: every candidate meets its exact duplicate and NMS removes one"""
    monkeypatch.setattr(collate_batch, "INPUT_PREP", "device")
    with cpu_shim.install():
        plain, aug = B.plain_and_augmented(registered, "cpu", "nchw", ["TEST.BBOX_AUG.SCALES", (96,), "TEST.BBOX_AUG.MAX_SIZE", 128])
    for a, b in zip(plain, aug):
        assert a.size == b.size and np.array_equal(B.canonical(a), B.canonical(b))


def test_inference_with_bbox_aug_returns_a_bbox_table(registered, monkeypatch):
    from maskrcnn_benchmark.engine.inference import inference

    monkeypatch.setattr(collate_batch, "INPUT_PREP", "host")
    cfg = B.narrow_cfg(registered, "cpu", ["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (64,),
                                           "TEST.BBOX_AUG.MAX_SIZE", 100, "TEST.BBOX_AUG.SCALE_H_FLIP", True])
    model = B.build_model(cfg, "cpu")
    with cpu_shim.install():
        res = inference(model, make_data_loader(cfg, is_train=False), registered, bbox_aug=True, device="cpu", cfg=cfg)
    assert set(res.results) == {"bbox"} and all(-1 <= v <= 1 for v in res.results["bbox"].values())


def test_inference_follows_the_model_and_refuses_a_contradiction(registered, monkeypatch):
    """bbox_aug left out: as the model was built, through a wrapper's `.module` too; an explicit value against the model's
    config raises; a BBOX_AUG model whose config cannot be found is recognised by its output"""
    from maskrcnn_benchmark.engine.inference import inference

    monkeypatch.setattr(collate_batch, "INPUT_PREP", "host")
    aug_cfg = B.narrow_cfg(registered, "cpu", ["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True])
    plain_cfg = B.narrow_cfg(registered, "cpu")
    aug, plain = B.build_model(aug_cfg, "cpu"), B.build_model(plain_cfg, "cpu")

    class Wrapped(torch.nn.Module):
        def __init__(self, module):
            super().__init__()
            self.module = module

        def forward(self, images):
            return self.module(images)

    class Opaque(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = [inner]                                  # not a sub-module: nothing to look through

        def forward(self, images):
            return self.inner[0].eval()(images)

    with cpu_shim.install():
        for model in (aug, Wrapped(aug)):
            res = inference(model, make_data_loader(aug_cfg, is_train=False), registered, device="cpu")
            assert set(res.results) == {"bbox"}
        with pytest.raises(ValueError, match="built with TEST.BBOX_AUG.ENABLED True"):
            inference(aug, make_data_loader(aug_cfg, is_train=False), registered, bbox_aug=False, device="cpu")
        with pytest.raises(ValueError, match="built with TEST.BBOX_AUG.ENABLED False"):
            inference(plain, make_data_loader(plain_cfg, is_train=False), registered, bbox_aug=True, device="cpu")
        with pytest.raises(ValueError, match="without `labels`"):
            inference(Opaque(aug), make_data_loader(aug_cfg, is_train=False), registered, device="cpu")
        res = inference(Opaque(aug), make_data_loader(aug_cfg, is_train=False), registered, bbox_aug=True, device="cpu", cfg=aug_cfg)
        assert set(res.results) == {"bbox"}


def test_test_net_evaluates_a_bbox_aug_config_bbox_only(registered, capsys, caplog, monkeypatch):
    """tools/test_net.py as it stands does not pass the flag: inference() takes it from the config the model was built
    with, drops the segm task and logs that"""
    import logging

    import test_net

    opts = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", "16", "MODEL.RESNETS.WIDTH_PER_GROUP", "4",
            "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", "16", "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", "32",
            "MODEL.ROI_MASK_HEAD.CONV_LAYERS", "(16, 16)", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "100",
            "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", "50", "TEST.DETECTIONS_PER_IMG", "20", "INPUT.MIN_SIZE_TEST", "96",
            "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "DATALOADER.NUM_WORKERS", "0", "DATALOADER.SIZE_DIVISIBILITY", "32",
            "MODEL.ROI_BOX_HEAD.NUM_CLASSES", "4", "DATASETS.TEST", "('%s',)" % registered, "TEST.BBOX_AUG.ENABLED", "True",
            "TEST.BBOX_AUG.H_FLIP", "True"]
    torch.manual_seed(0)
    with cpu_shim.install(), caplog.at_level(logging.INFO, logger="maskrcnn_benchmark"):
        results = test_net.main(["--config-file", "e2e_mask_rcnn_R_50_FPN_1x.yaml"] + opts)
    out = capsys.readouterr().out
    assert "Task: bbox" in out and "Task: segm" not in out
    assert set(results[0].results) == {"bbox"}
    assert any("bbox only" in r.getMessage() for r in caplog.records)
