"""GroupNorm models without a GPU: the layer class and its CPU paths (bit-equal to F.group_norm compositions), the cfg a
model is built from reaching its GroupNorm layers, the two gn_baselines configs, and the GN Mask R-CNN against the
reference's own detector (tests/golden/whole_model_mask_rcnn_gn.npz, made by tests/golden/make_golden_whole_model_gn.py)."""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import cpu_shim
from test_whole_model_parity import TOL, _build

CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "maskrcnn-benchmark_amd", "configs")
GN_YAMLS = ["gn_baselines/e2e_mask_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml", "gn_baselines/e2e_faster_rcnn_R_50_FPN_1x_gn.yaml"]
NARROW = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", 16, "MODEL.RESNETS.WIDTH_PER_GROUP", 4,
          "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 32, "MODEL.ROI_BOX_HEAD.CONV_HEAD_DIM", 16,
          "MODEL.ROI_MASK_HEAD.CONV_LAYERS", (16, 16)]
GROUPS_OF_2 = ["MODEL.GROUP_NORM.NUM_GROUPS", -1, "MODEL.GROUP_NORM.DIM_PER_GP", 2]


def _gn_modules(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, nn.GroupNorm)]


def test_layer_is_an_nn_groupnorm_with_the_reference_keys():
    from maskrcnn_benchmark.layers import GroupNorm
    from maskrcnn_benchmark.modeling.make_layers import group_norm
    gn = GroupNorm(4, 8, 1e-5, True)
    assert isinstance(gn, nn.GroupNorm) and list(gn.state_dict()) == ["weight", "bias"]
    made = group_norm(64)
    assert type(made) is GroupNorm and made.num_groups == 32 and made.num_channels == 64      # outside a build: the global cfg
    assert type(group_norm(64, affine=False, divisor=2)) is GroupNorm and group_norm(64, divisor=2).num_groups == 16


@pytest.mark.parametrize("channels_last", [False, True])
def test_cpu_paths_equal_f_group_norm_bit_for_bit(channels_last):
    from maskrcnn_benchmark.layers import GroupNorm
    torch.manual_seed(3)
    gn = GroupNorm(4, 8)
    with torch.no_grad():
        gn.weight.normal_()
        gn.bias.normal_()
    x = torch.randn(3, 8, 5, 7)
    res = torch.randn(3, 8, 5, 7)
    if channels_last:
        x, res = x.contiguous(memory_format=torch.channels_last), res.contiguous(memory_format=torch.channels_last)
    ref = F.group_norm(x, 4, gn.weight, gn.bias, gn.eps)
    assert torch.equal(gn(x), ref)
    assert torch.equal(gn.fused(x), ref)
    assert torch.equal(gn.fused(x, True, res), torch.relu(ref + res))
    assert torch.equal(gn.fused(x, relu=True), torch.relu(ref))
    x2 = torch.randn(6, 8)                                      # the FC layers' 2-d input
    assert torch.equal(gn(x2), F.group_norm(x2, 4, gn.weight, gn.bias, gn.eps))
    # gradients flow through the composed path
    xg = x.clone().requires_grad_(True)
    gn.fused(xg, True, res).sum().backward()
    assert xg.grad is not None and gn.weight.grad is not None


def test_group_norm_settings_come_from_the_cfg_the_model_is_built_from():
    """MODEL.GROUP_NORM.* given to load_cfg (a yaml or a command line) reaches every GN layer; the global cfg stays as it was."""
    from maskrcnn_benchmark.config import cfg as global_cfg
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.modeling.backbone import build_backbone
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    before = (global_cfg.MODEL.GROUP_NORM.NUM_GROUPS, global_cfg.MODEL.GROUP_NORM.DIM_PER_GP, global_cfg.MODEL.GROUP_NORM.EPSILON)
    cfg = load_cfg(os.path.join(CONFIGS, GN_YAMLS[0]), GROUPS_OF_2 + ["MODEL.GROUP_NORM.EPSILON", 1e-3] + NARROW)
    for built in (build_detection_model(cfg), build_backbone(cfg)):
        gns = _gn_modules(built)
        assert len(gns) > 50
        for name, m in gns:
            assert m.num_groups == m.num_channels // 2, (name, m.num_groups, m.num_channels)
            assert m.eps == 1e-3, name
    assert before == (32, -1, 1e-5)
    assert (global_cfg.MODEL.GROUP_NORM.NUM_GROUPS, global_cfg.MODEL.GROUP_NORM.DIM_PER_GP, global_cfg.MODEL.GROUP_NORM.EPSILON) == before


@pytest.mark.parametrize("yaml", GN_YAMLS)
def test_shipped_gn_configs_load_and_build_narrow(yaml):
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.layers import GroupNorm
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    cfg = load_cfg(os.path.join(CONFIGS, yaml), GROUPS_OF_2 + NARROW)
    assert cfg.MODEL.WEIGHT == "" and cfg.DATASETS.TRAIN == ("synthetic_coco_train",)
    assert cfg.MODEL.RESNETS.TRANS_FUNC == "BottleneckWithGN" and cfg.MODEL.RESNETS.STEM_FUNC == "StemWithGN"
    assert cfg.MODEL.FPN.USE_GN and cfg.MODEL.ROI_BOX_HEAD.USE_GN and not cfg.MODEL.RESNETS.STRIDE_IN_1X1
    model = build_detection_model(cfg)
    assert all(type(m) is GroupNorm for _, m in _gn_modules(model))
    keys = set(model.state_dict())
    # a conv + GN block keeps the reference's child indices
    assert {"backbone.fpn.fpn_inner1.0.weight", "backbone.fpn.fpn_inner1.1.weight", "backbone.fpn.fpn_inner1.1.bias"} <= keys
    assert "backbone.fpn.fpn_inner1.0.bias" not in keys
    assert {"backbone.body.stem.bn1.weight", "backbone.body.layer1.0.downsample.1.bias"} <= keys
    if cfg.MODEL.MASK_ON:
        assert {"roi_heads.mask.feature_extractor.mask_fcn1.0.weight", "roi_heads.mask.feature_extractor.mask_fcn1.1.bias",
                "roi_heads.box.feature_extractor.xconvs.0.weight", "roi_heads.box.feature_extractor.xconvs.1.weight"} <= keys
    else:
        assert {"roi_heads.box.feature_extractor.fc6.0.weight", "roi_heads.box.feature_extractor.fc6.1.weight"} <= keys


def test_gn_state_dict_keys_equal_the_reference_and_load_strict():
    _, model, ref_sd, _, _, _ = _build("mask_rcnn_gn", "cpu")
    mine = model.state_dict()
    assert len(ref_sd) == 222
    assert list(mine) == list(ref_sd), sorted(set(mine) ^ set(ref_sd))[:10]
    for k, v in ref_sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape) and mine[k].dtype == v.dtype, k
    model.load_state_dict(ref_sd, strict=True)


@pytest.mark.parametrize("dev", ["cpu", "cpu-product-wrappers"])
def test_gn_losses_equal_the_reference_with_its_weights(dev):
    backend = "emu-lib" if dev == "cpu-product-wrappers" else "oracle"
    _, model, ref_sd, il, targets, ref_losses = _build("mask_rcnn_gn", "cpu")
    model.load_state_dict(ref_sd, strict=True)
    model.train()
    with cpu_shim.install(backend), torch.no_grad():
        losses = model(il, targets)
    got = {k: float(v) for k, v in losses.items()}
    assert set(got) == set(ref_losses) and len(got) == 5
    for k, ref in ref_losses.items():
        assert abs(got[k] - ref) <= TOL * max(1.0, abs(ref)), (k, got[k], ref)
