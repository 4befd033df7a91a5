"""Keypoint R-CNN on the MI355X (`-m gpu`): the three keypoint kernels of csrc/keypoint.hip against their torch formulations
(the CPU path of the head, itself pinned to the reference by tests/test_keypoint_cpu.py), and the keypoint model on the
device: reference losses under both layouts, training steps in fp32 / bf16, slot modes, eval decoding."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_keypoint_cpu as kcpu

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _targets_case(gen, P, G, K=17):
    gt = torch.rand(G, 2, generator=gen) * 400
    gt = torch.cat([gt, gt + 20 + torch.rand(G, 2, generator=gen) * 300], 1)
    kp = gt[:, None, :2] + torch.rand(G, K, 2, generator=gen) * 1.2 * (gt[:, None, 2:] - gt[:, None, :2]) - \
        0.1 * (gt[:, None, 2:] - gt[:, None, :2])
    v = torch.randint(0, 3, (G, K), generator=gen).float()
    kp = torch.cat([torch.where((v == 0)[..., None], torch.zeros_like(kp), kp), v[..., None]], 2)
    kp[0, :, 2] = 0                                                 # no labelled keypoint
    matched = torch.randint(-2, G, (P,), generator=gen)
    boxes = gt[matched.clamp(min=0)] + torch.randn(P, 4, generator=gen) * 10
    boxes[:, 2:] = torch.maximum(boxes[:, 2:], boxes[:, :2] + 0.5)
    labels = torch.where(matched >= 0, torch.ones_like(matched), torch.zeros_like(matched))
    labels[::7] = -1
    # boundary points: the matched keypoint on the slot box's right / bottom edge and just outside its left edge
    for p in range(0, P, 5):
        g = int(matched[p])
        if g >= 0:
            kp[g, 1, 0], kp[g, 2, 1] = boxes[p, 2], boxes[p, 3]
            kp[g, 3, 0] = torch.nextafter(boxes[p, 0], torch.tensor(-1e9))
            kp[g, 1:4, 2] = 2
    return boxes, matched, labels, gt, kp


@pytest.mark.parametrize("P,G", [(512, 20), (64, 3), (1, 1)])
def test_targets_kernel_bit_equal_to_torch(P, G):
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.loss import keypoint_targets_torch
    args = _targets_case(torch.Generator().manual_seed(P + G), P, G)
    heat, valid = keypoint_targets_torch(*args, 56)
    dh, dv = _C.keypoint_targets(*[a.to(DEV) for a in args], 56)
    assert torch.equal(dh.cpu(), heat) and torch.equal(dv.cpu(), valid)
    assert (~valid).any() and (valid.any() or G == 1)   # G == 1: the only ground truth has no labelled keypoint


def test_targets_kernel_on_the_reference_boundary_cases():
    from maskrcnn_benchmark import _C
    G = kcpu.G
    rois, kp = torch.from_numpy(G["hm_rois"]), torch.from_numpy(G["hm_kp"])
    n = rois.shape[0]
    # each roi matched to "its" ground truth, a huge box so that every labelled keypoint counts as inside it
    heat, valid = _C.keypoint_targets(rois.to(DEV), torch.arange(n, device=DEV), torch.ones(n, dtype=torch.int64, device=DEV),
                                      torch.tensor([[-1e9, -1e9, 1e9, 1e9]], device=DEV).expand(n, 4).contiguous(),
                                      kp.to(DEV), 56)
    assert np.array_equal(heat.cpu().numpy(), G["hm_heat"]) and np.array_equal(valid.cpu().long().numpy(), G["hm_valid"])


def test_targets_kernel_on_integer_aligned_boxes():
    """integer widths and half-integer points (the reference's fixture): the kernel must round M / w as torch does"""
    from maskrcnn_benchmark import _C
    G = kcpu.G
    rois, kp = torch.from_numpy(G["hi_rois"]), torch.from_numpy(G["hi_kp"])
    n = rois.shape[0]
    heat, valid = _C.keypoint_targets(rois.to(DEV), torch.arange(n, device=DEV), torch.ones(n, dtype=torch.int64, device=DEV),
                                      torch.tensor([[-1e9, -1e9, 1e9, 1e9]], device=DEV).expand(n, 4).contiguous(),
                                      kp.to(DEV), 56)
    assert np.array_equal(heat.cpu().numpy(), G["hi_heat"]) and np.array_equal(valid.cpu().long().numpy(), G["hi_valid"])


@pytest.mark.parametrize("width,offset", [(49, 7.0), (3, 1.5), (7, 3.5), (98, 21.0)])
def test_targets_kernel_bit_equal_to_torch_on_integer_cells(width, offset):
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.loss import keypoint_targets_torch
    x0 = 10.0
    gt = torch.tensor([[x0, x0, x0 + width, x0 + width]])
    kp = torch.zeros(1, 17, 3)
    kp[0, :, 0] = x0 + torch.arange(17).float() * (offset / 2)      # multiples of offset / 2, the first ones inside the box
    kp[0, :, 1] = x0 + offset
    kp[0, :, 2] = 2
    args = (gt.clone(), torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int64), gt, kp)
    heat, valid = keypoint_targets_torch(*args, 56)
    dh, dv = _C.keypoint_targets(*[a.to(DEV) for a in args], 56)
    assert torch.equal(dh.cpu(), heat) and torch.equal(dv.cpu(), valid) and bool(valid[0, 0])


def _loss_inputs(P=256, K=17, M=56, seed=0, frac=0.7):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(P, K, M, M, generator=g) * 3
    heat = torch.randint(0, M * M, (P, K), generator=g)
    valid = torch.rand(P, K, generator=g) < frac
    return logits, heat, valid


def _fp64_reference(logits, heat, valid):
    x = logits.double().reshape(-1, logits.shape[2] * logits.shape[3]).clone().requires_grad_(True)
    v = valid.reshape(-1)
    loss = F.cross_entropy(x[v], heat.reshape(-1)[v]) if v.any() else x.sum() * 0
    loss.backward()
    return float(loss), x.grad.view(logits.shape)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_loss_kernel_value_and_gradient(layout):
    from maskrcnn_benchmark import _C
    logits, heat, valid = _loss_inputs()
    ref, ref_g = _fp64_reference(logits, heat, valid)
    d = logits.to(DEV)
    if layout == "channels_last":
        d = d.contiguous(memory_format=torch.channels_last)
    d.requires_grad_(True)
    loss = _C.keypoint_loss(d, heat.to(DEV), valid.to(DEV))
    (loss * 2.5).backward()
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)
    g = d.grad.cpu().double()
    assert (g - 2.5 * ref_g).abs().max() <= 1e-5 * (2.5 * ref_g).abs().max()
    assert torch.all(g[~valid] == 0)


def test_loss_kernel_without_valid_rows_is_zero():
    from maskrcnn_benchmark import _C
    logits, heat, valid = _loss_inputs(P=8, frac=0.0)
    d = logits.to(DEV).requires_grad_(True)
    loss = _C.keypoint_loss(d, heat.to(DEV), valid.to(DEV))
    loss.backward()
    assert float(loss) == 0.0 and torch.all(d.grad == 0)


def test_loss_forward_backward_without_host_sync():
    from maskrcnn_benchmark import _C
    logits, heat, valid = _loss_inputs(P=32)
    d = logits.to(DEV).requires_grad_(True)
    h, v = heat.to(DEV), valid.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = _C.keypoint_loss(d, h, v)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref, _ = _fp64_reference(logits, heat, valid)
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)


def _decode_case(seed=0, K=17):
    g = torch.Generator().manual_seed(seed)
    sides = [0.3, 0.9, 1.0, 1.5, 2.2, 7.7, 13.0, 31.4, 55.5, 56.0, 57.3, 100.0, 240.6, 512.0, 800.25, 1333.0]
    n = len(sides)
    w = torch.tensor(sides)
    h = torch.tensor(sides[::-1])
    x1 = torch.rand(n, generator=g) * 600
    y1 = torch.rand(n, generator=g) * 400
    boxes = torch.stack([x1, y1, x1 + w, y1 + h], 1)
    maps = torch.randn(n, K, 56, 56, generator=g) * 2
    return maps, boxes


def _fp64_decode(maps, boxes):
    """the reference's arithmetic with the fp64 bicubic resize -> (xy [n,K,2], scores [n,K], top-two margin [n,K])"""
    n, K = maps.shape[:2]
    xy = np.zeros((n, K, 2), np.float32)
    sc = np.zeros((n, K), np.float32)
    margin = np.zeros((n, K))
    b = boxes.numpy()
    wd, ht = np.maximum(b[:, 2] - b[:, 0], 1), np.maximum(b[:, 3] - b[:, 1], 1)
    for i in range(n):
        ow, oh = int(np.ceil(wd[i])), int(np.ceil(ht[i]))
        r = F.interpolate(maps[i:i + 1].double(), size=(oh, ow), mode="bicubic", align_corners=False)[0].reshape(K, -1)
        pos = r.argmax(dim=1).numpy()
        s = np.sort(r.numpy(), axis=1)
        margin[i] = s[:, -1] - s[:, -2] if s.shape[1] > 1 else np.inf
        sc[i] = r.numpy()[np.arange(K), pos]
        xy[i, :, 0] = (pos % ow + 0.5) * (wd[i] / np.float32(np.ceil(wd[i]))) + b[i, 0]
        xy[i, :, 1] = (pos // ow + 0.5) * (ht[i] / np.float32(np.ceil(ht[i]))) + b[i, 1]
    return xy, sc, margin


def test_decoder_against_fp64_bicubic():
    from maskrcnn_benchmark import _C
    maps, boxes = _decode_case()
    kps, scores = _C.heatmaps_to_keypoints(maps.to(DEV), boxes.to(DEV))
    kps, scores = kps.cpu().numpy(), scores.cpu().numpy()
    xy, sc, margin = _fp64_decode(maps, boxes)
    sharp = margin > 1e-4 * np.abs(sc)
    assert sharp.mean() > 0.9
    assert np.array_equal(kps[..., :2][sharp], xy[sharp])
    assert np.all(kps[..., 2] == 1)
    np.testing.assert_allclose(scores, sc, rtol=1e-5, atol=1e-6)


def test_decoder_equals_the_cpu_decoder_and_reads_channels_last():
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.inference import heatmaps_to_keypoints_torch
    maps, boxes = _decode_case(seed=1)
    ref_k, ref_s = heatmaps_to_keypoints_torch(maps, boxes)
    for m in (maps.to(DEV), maps.to(DEV).contiguous(memory_format=torch.channels_last)):
        k, s = _C.heatmaps_to_keypoints(m, boxes.to(DEV))
        assert torch.equal(k.cpu(), ref_k) and torch.equal(s.cpu(), ref_s)


def test_decoder_plateau_returns_the_first_maximum():
    from maskrcnn_benchmark import _C
    maps = torch.zeros(2, 3, 56, 56)
    maps[:, 1] = 5.0                         # constant map: every resized pixel is the maximum -> flat index 0
    maps[:, 2, 20:30, 10:40] = 7.0           # a plateau: the first row-major pixel of the resized plateau wins
    boxes = torch.tensor([[10.0, 20.0, 66.0, 76.0], [0.0, 0.0, 112.0, 112.0]])
    k, s = _C.heatmaps_to_keypoints(maps.to(DEV), boxes.to(DEV))
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.inference import heatmaps_to_keypoints_torch
    rk, rs = heatmaps_to_keypoints_torch(maps, boxes)
    assert torch.equal(k.cpu(), rk) and torch.equal(s.cpu(), rs)
    assert k[0, 1, 0].item() == 10.5 and k[0, 1, 1].item() == 20.5


def test_decoder_batched_equals_one_image_at_a_time():
    from maskrcnn_benchmark import _C
    maps, boxes = _decode_case(seed=2)
    md, bd = maps.to(DEV), boxes.to(DEV)
    k, s = _C.heatmaps_to_keypoints(md, bd)
    k0, s0 = _C.heatmaps_to_keypoints(md[:7], bd[:7])
    k1, s1 = _C.heatmaps_to_keypoints(md[7:], bd[7:])
    assert torch.equal(k, torch.cat([k0, k1])) and torch.equal(s, torch.cat([s0, s1]))


@pytest.mark.parametrize("layout", ["nchw", "all"])
def test_whole_keypoint_model_losses_on_device(layout):
    model, ref_sd, il, targets, ref_losses = kcpu._whole_model_case()
    model.load_state_dict(ref_sd, strict=True)
    model.to(DEV).train()
    if layout == "all":
        model.set_channels_last(True, heads=True)
    with torch.no_grad():
        losses = model(il.to(DEV), [t.to(DEV) for t in targets])
    got = {k: float(v) for k, v in losses.items()}
    assert set(got) == set(ref_losses)
    for k, ref in ref_losses.items():
        assert abs(got[k] - ref) <= 1e-4 * max(1.0, abs(ref)), (k, got, ref_losses)


SMALL = ["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 500, "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", 500,
         "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 256]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_training_steps_give_finite_losses(dtype):
    from maskrcnn_benchmark.engine.bench_step import build_training, load_cfg, make_device_batches
    cfg = load_cfg("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", SMALL + ["DTYPE", dtype])
    torch.manual_seed(0)
    model, _, _, step = build_training(cfg, DEV)
    batches = make_device_batches(cfg, DEV, images_per_gpu=2, num_batches=2, height=320, width=448)
    for i in range(5):
        losses = step(*batches[i % 2])
        vals = {k: float(v.detach()) for k, v in losses.items()}
        assert "loss_kp" in vals and all(np.isfinite(v) for v in vals.values()), (i, vals)


def test_slot_modes_give_the_same_keypoint_loss(monkeypatch):
    from maskrcnn_benchmark.engine.bench_step import load_cfg, make_device_batches
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.roi_heads.mask_head import mask_head as mh
    cfg = load_cfg("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", SMALL)
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(DEV).train()
    (images, targets), = make_device_batches(cfg, DEV, images_per_gpu=2, num_batches=1, height=320, width=448)
    out = {}
    for mode in ("fixed", "dynamic"):
        monkeypatch.setattr(mh, "SLOT_MODE", mode)
        torch.manual_seed(1)
        torch.cuda.manual_seed(1)
        with torch.no_grad():
            out[mode] = float(model(images, targets)["loss_kp"])
        out[mode + "_slots"] = model.roi_heads["keypoint"].last_slots
    assert abs(out["fixed"] - out["dynamic"]) <= 1e-5 * abs(out["fixed"]), out


def test_eval_forward_decodes_every_image_like_the_cpu_decoder():
    from maskrcnn_benchmark.engine.bench_step import load_cfg, make_device_batches
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.inference import heatmaps_to_keypoints_torch
    cfg = load_cfg("e2e_keypoint_rcnn_R_50_FPN_1x.yaml", [])
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(DEV).eval()
    (images, _), = make_device_batches(cfg, DEV, images_per_gpu=2, num_batches=1, height=320, width=448)
    seen = {}
    head = model.roi_heads["keypoint"]
    hook = head.predictor.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o.detach()))
    with torch.no_grad():
        dets = model(images)
    hook.remove()
    assert len(dets) == 2
    boxes = torch.cat([d.bbox for d in dets])
    ref_k, ref_s = heatmaps_to_keypoints_torch(seen["logits"].cpu(), boxes.cpu())
    k = torch.cat([d.get_field("keypoints").keypoints for d in dets]).cpu()
    s = torch.cat([d.get_field("keypoints").get_field("logits") for d in dets]).cpu()
    for d in dets:
        assert tuple(d.get_field("keypoints").keypoints.shape) == (len(d), 17, 3)
        assert tuple(d.get_field("keypoints").get_field("logits").shape) == (len(d), 17)
    assert torch.equal(k, ref_k) and torch.equal(s, ref_s)
