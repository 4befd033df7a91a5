"""Whole-model parity against the REFERENCE's detector (tests/golden/make_golden_whole_model.py ran the reference's own
`GeneralizedRCNN`, modeling/detector/generalized_rcnn.py:46-65, on the CPU with its own compiled `_C`):

  * checkpoint compatibility — this repository's detector, built from the same configuration, has EXACTLY the reference's
    `state_dict()` key set and shapes (what utils/model_serialization.py:10-71 matches on) and loads it with strict=True;
  * loss parity — with those weights, the same two-image batch and sampler quotas >= candidates (take-all: no random
    stream enters), every entry of the training loss dict agrees with the reference's within 1e-4 relative — on the CPU
    (HIP-only operators served by the oracle through tests/cpu_shim.py, and again by the product's own wrappers over the
    host-emulation library) and, in the `-m gpu` suite, on the device through the real HIP kernels (ROIAlign, NMS, target
    kernels, focal loss, fused FrozenBN).
"""
import ast
import contextlib
import os

import numpy as np
import pytest
import torch

import cpu_shim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


def _build(name, device):
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.image_list import to_image_list
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    g = np.load(os.path.join(GOLDEN, "whole_model_%s.npz" % name), allow_pickle=False)
    opts = list(ast.literal_eval(str(g["opts"])))
    opts[opts.index("MODEL.DEVICE") + 1] = device
    cfg = load_cfg(str(g["yaml"]), opts)
    model = build_detection_model(cfg)
    ref_sd = {k[len("sd__"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd__")}
    images, targets = [], []
    for i in range(2):
        im = torch.from_numpy(g["image_%d" % i])
        H, W = im.shape[-2:]
        t = BoxList(torch.from_numpy(g["boxes_%d" % i]), (W, H), mode="xyxy")
        t.add_field("labels", torch.from_numpy(g["labels_%d" % i]))
        if "masks_%d" % i in g.files:
            t.add_field("masks", SegmentationMask(torch.from_numpy(g["masks_%d" % i]), (W, H), mode="mask"))
        images.append(im)
        targets.append(t)
    il = to_image_list(images, int(g["size_divisibility"]))
    ref_losses = {k[len("loss__"):]: float(g[k]) for k in g.files if k.startswith("loss__")}
    return cfg, model, ref_sd, il, targets, ref_losses


@pytest.mark.parametrize("name", ["mask_rcnn", "retinanet"])
def test_state_dict_keys_equal_the_reference_and_load_strict(name):
    _, model, ref_sd, _, _, _ = _build(name, "cpu")
    mine = model.state_dict()
    assert set(mine) == set(ref_sd), {"missing here": sorted(set(ref_sd) - set(mine))[:10],
                                      "unknown to the reference": sorted(set(mine) - set(ref_sd))[:10]}
    assert list(mine) == list(ref_sd), "same registration order as the reference (checkpoint files list keys in it)"
    for k, v in ref_sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
        assert mine[k].dtype == v.dtype, k
    model.load_state_dict(ref_sd, strict=True)


@pytest.mark.parametrize("name", ["mask_rcnn", "retinanet"])
@pytest.mark.parametrize("dev", ["cpu", "cpu-product-wrappers", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_losses_equal_the_reference_with_its_weights(name, dev, monkeypatch):
    backend = "oracle"
    if dev == "cpu-product-wrappers":
        # CPU tensors, but the model takes the branches it takes on the GPU (fused labels / sampler / sampled-slot targets /
        # proposal decode / batched proposal hand-over) through the product's own `_C` wrappers and autograd functions,
        # every operator of the model included, over the host-emulation build of the HIP sources (cpu_shim backend
        # "emu-lib"): nothing of `_C` is replaced
        dev, backend = "cpu", "emu-lib"
    cfg, model, ref_sd, il, targets, ref_losses = _build(name, dev)
    model.load_state_dict(ref_sd, strict=True)
    model.to(dev).train()
    if dev == "cpu" and backend != "emu-lib":
        import maskrcnn_benchmark.layers.sigmoid_focal_loss as sfl
        monkeypatch.setattr(sfl.SigmoidFocalLoss, "forward",
                            lambda self, l, t: sfl.sigmoid_focal_loss_sum(l.float(), t, self.gamma, self.alpha))
    with (cpu_shim.install(backend) if dev == "cpu" else contextlib.nullcontext()):
        with torch.no_grad():
            losses = model(il.to(dev), [t.to(dev) for t in targets])
    got = {k: float(v) for k, v in losses.items()}
    assert set(got) == set(ref_losses)
    for k, ref in ref_losses.items():
        assert abs(got[k] - ref) <= TOL * max(1.0, abs(ref)), (k, got[k], ref, got, ref_losses)


def _loss_and_grads(model, il, targets, dev):
    for p in model.parameters():
        p.grad = None
    losses = model(il.to(dev), [t.to(dev) for t in targets])
    sum(losses.values()).backward()
    return ({k: float(v.detach()) for k, v in losses.items()},
            {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None})


GRAD_TOL = 4e-5       # relative Frobenius distance per parameter (observed at most 4.6e-6 on an MI355X, see below)
GRAD_FLOOR = 1e-3     # ... measured against max(|g_ref|, GRAD_FLOOR * the largest |g_ref| of the model)


def _grad_spread(got, ref):
    """per-parameter ||got - ref||_F / max(||ref||_F, GRAD_FLOOR * max_p ||ref_p||_F)"""
    gmax = max(float(g.norm()) for g in ref.values())
    return {n: float((got[n] - ref[n]).norm()) / max(float(ref[n].norm()), GRAD_FLOOR * gmax) for n in ref}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mask_rcnn", "retinanet"])
def test_layouts_losses_and_gradients_equal_the_cpu_run(name, monkeypatch):
    """One training forward + `sum(losses).backward()` of the device model with the reference's weights and batch, in the
    layouts `nchw`, `backbone` (set_channels_last(True)) and `all` (set_channels_last(True, heads=True), the headline's):
    every loss within TOL of the reference's fixture, the same set of parameters with a gradient in every run, and every
    parameter gradient within GRAD_TOL (relative Frobenius, floored) of the same model's CPU run (the `[cpu]` path: oracle
    stand-ins, focal-loss composition) and of the device NCHW run.  TF32 off.  The channels-last runs are checked to take
    the NHWC kernels (FrozenBN, FPN top-down, bias_act, and for `all` the NHWC pooler).
    Observed on an MI355X: largest spread 4.6e-6 (RetinaNet `rpn.head.cls_logits.bias`, device vs CPU, every layout); Mask
    R-CNN 1.1e-6 (`roi_heads.mask.predictor.conv5_mask.bias`); channels-last vs device NCHW at most 2.3e-6."""
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)

    _, model, ref_sd, il, targets, ref_losses = _build(name, "cpu")
    model.load_state_dict(ref_sd, strict=True)
    model.train()
    import maskrcnn_benchmark.layers.sigmoid_focal_loss as sfl
    with monkeypatch.context() as m:
        m.setattr(sfl.SigmoidFocalLoss, "forward", lambda self, l, t: sfl.sigmoid_focal_loss_sum(l.float(), t, self.gamma, self.alpha))
        with cpu_shim.install("oracle"):
            cpu_losses, cpu_grads = _loss_and_grads(model, il, targets, "cpu")
    for k, ref in ref_losses.items():
        assert abs(cpu_losses[k] - ref) <= TOL * max(1.0, abs(ref)), ("cpu", k, cpu_losses[k], ref)

    _, model, _, _, _, _ = _build(name, "cuda")
    model.load_state_dict(ref_sd, strict=True)
    model.to("cuda").train()
    seen = []

    def spy(fname, args_of):
        f = getattr(_C, fname)

        def wrapped(*a, **k):
            seen.append((fname, tuple(_C.is_channels_last(t) for t in args_of(*a, **k))))
            return f(*a, **k)
        monkeypatch.setattr(_C, fname, wrapped)

    spy("fpn_topdown", lambda lat, top: (lat, top))
    spy("frozen_bn_act_forward", lambda x, *a: (x,))
    spy("bias_act", lambda x, *a, **k: (x,))
    spy("_roi_align_fpn_forward_nhwc", lambda inputs, *a: tuple(inputs))

    runs = {}
    for layout in ("nchw", "backbone", "all"):
        if layout != "nchw":
            model.set_channels_last(True, heads=(layout == "all"))
        del seen[:]
        losses, grads = _loss_and_grads(model, il, targets, "cuda")
        torch.cuda.synchronize()
        calls = {}
        for fname, cl in seen:
            calls.setdefault(fname, set()).update(cl)
        assert calls.get("fpn_topdown") == {layout != "nchw"}, (layout, calls)
        assert calls.get("frozen_bn_act_forward") == {layout != "nchw"}, (layout, calls)
        if layout == "all":
            assert calls.get("bias_act") == {True}, calls
            assert name != "mask_rcnn" or calls.get("_roi_align_fpn_forward_nhwc") == {True}, calls
        else:
            assert "_roi_align_fpn_forward_nhwc" not in calls, (layout, calls)
        for k, ref in ref_losses.items():
            assert abs(losses[k] - ref) <= TOL * max(1.0, abs(ref)), (layout, k, losses[k], ref)
        assert set(grads) == set(cpu_grads), (layout, sorted(set(grads) ^ set(cpu_grads))[:10])
        runs[layout] = grads

    worst = {}
    for layout, grads in runs.items():
        for against, ref in (("cpu", cpu_grads), ("nchw", runs["nchw"])):
            if layout == against:
                continue
            spread = _grad_spread(grads, ref)
            n = max(spread, key=spread.get)
            worst[(layout, against)] = (spread[n], n)
    print("\ngradient spread %s: %s" % (name, {"%s-vs-%s" % k: "%.3g (%s)" % v for k, v in worst.items()}))
    for key, (s, n) in worst.items():
        assert s <= GRAD_TOL, (key, n, s, worst)
