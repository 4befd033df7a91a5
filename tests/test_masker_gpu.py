"""Masks at inference on the MI355X (`-m gpu`): the kernels of csrc/masker.hip (`_C.paste_masks`, `_C.paste_masks_rle`)
against the reference's `Masker` (tests/golden/masker_reference.npz) and against `paste_masks_torch` (the CPU path, itself
pinned to the reference by tests/test_masker_cpu.py), the row head / tail stores behind guard bands, and the mask model in
eval with MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS.

The kernels restate ATen's CPU bilinear resize in fp32; where the interpolated value lies within 1e-5 of the threshold the
two may land on different sides.  Those "near" pixels (at most 2e-4 of a case's pixels; the reference's own share is below
1e-4, a restatement differs by ~1.6e-6 in value) are excluded; everything else is exact."""
import ctypes

import numpy as np
import pytest
import torch

import test_masker_cpu as mcpu
from maskrcnn_benchmark.modeling.roi_heads.mask_head import inference as mi

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_NEAR_SHARE = 2e-4


def _C():
    from maskrcnn_benchmark import _C as c
    return c


def _windows(boxes, M, padding, det_sizes):
    """the clipped integer windows (x_lo, x_hi, y_lo, y_hi) of the definition, in torch on the CPU"""
    scale = float(M + 2 * padding) / M
    out = []
    for (x1, y1, x2, y2), (h, w) in zip(mi.expand_boxes(boxes.float().cpu(), scale).to(torch.int32).tolist(), det_sizes):
        out.append((max(x1, 0), min(x2 + 1, w), max(y1, 0), min(y2 + 1, h)))
    return out


def _check_case(views, planes, near, windows):
    """views: per-image [n, 1, H, W] device masks; planes / near: per-detection CPU [H, W]"""
    got = [p for v in views for p in v[:, 0].cpu()]
    assert len(got) == len(planes)
    pixels = sum(p.numel() for p in planes)
    excluded = sum(int(n.sum()) for n in near)
    assert excluded <= MAX_NEAR_SHARE * pixels, (excluded, pixels)
    for k, (g, p, n, (x_lo, x_hi, y_lo, y_hi)) in enumerate(zip(got, planes, near, windows)):
        assert g.dtype == torch.bool and g.shape == p.shape
        assert torch.equal(g | n, p | n), "detection %d: %d pixels differ outside the near set" % (k, int(((g != p) & ~n).sum()))
        outside = torch.ones_like(g)
        if x_hi > x_lo and y_hi > y_lo:
            outside[y_lo:y_hi, x_lo:x_hi] = False
        assert not (g & outside).any(), "detection %d: ones outside the clipped window" % k


@pytest.mark.parametrize("b", range(4))
def test_paste_masks_on_the_reference_fixture_in_one_launch(b):
    case = mcpu.batches()[b]
    flat, views = _C().paste_masks(case["maps"].to(DEV), case["boxes"].to(DEV), case["sizes"], case["threshold"],
                                   case["padding"], counts=case["counts"])
    assert flat.dtype == torch.uint8 and int(flat.max()) <= 1
    assert [tuple(v.shape) for v in views] == [(n, 1, h, w) for (h, w), n in zip(case["sizes"], case["counts"])]
    _check_case(views, case["planes"], case["near"], _windows(case["boxes"], case["M"], case["padding"], case["det_sizes"]))


def _random_case(seed, M, images, dtype=torch.float32, threshold=0.5, padding=1):
    """images: [(H, W, n)] -> maps [N, 1, M, M] of `dtype`, boxes [N, 4] (one in eight off the image, one in eight larger
    than it, the rest anywhere), per-image sizes and counts, and the CPU planes / near planes of paste_masks_torch"""
    g = torch.Generator().manual_seed(seed)
    N = sum(n for _, _, n in images)
    maps = torch.sigmoid(3 * torch.randn(N, 1, M, M, generator=g)).to(dtype)
    boxes, planes, near, det_sizes = [], [], [], []
    k = 0
    for H, W, n in images:
        u = torch.rand(n, 4, generator=g)
        x = torch.sort(u[:, :2] * W, dim=1).values
        y = torch.sort(u[:, 2:] * H, dim=1).values
        bx = torch.stack([x[:, 0], y[:, 0], x[:, 1] + 0.5, y[:, 1] + 0.5], dim=1)
        idx = torch.arange(n)
        bx[idx % 8 == 3] += torch.tensor([W + 40.0, 0.0, W + 40.0, 0.0])
        big = idx % 8 == 5
        bx[big] = torch.tensor([-0.3 * W - 2, -0.2 * H - 2, 1.3 * W + 2, 1.4 * H + 2]).expand(int(big.sum()), 4)
        m = maps[k:k + n]
        planes += list(mi.paste_masks_torch(m, bx, H, W, threshold, padding)[:, 0])
        near += list(mcpu.near_planes(m, bx, H, W, threshold, padding))
        det_sizes += [(H, W)] * n
        boxes.append(bx)
        k += n
    # a case is admitted the way tests/golden/make_golden_masker.py admits one: by the CPU path's own near share
    assert sum(int(n.sum()) for n in near) <= 1e-4 * sum(p.numel() for p in planes), "pick another seed"
    return dict(M=M, maps=maps, boxes=torch.cat(boxes), sizes=[(H, W) for H, W, _ in images],
                counts=[n for _, _, n in images], planes=planes, near=near, det_sizes=det_sizes, threshold=threshold,
                padding=padding)


_RANDOM = {}
RANDOM_CASES = {
    "f32_m28_mixed_sizes": (1, 28, [(61, 83, 9), (40, 129, 0), (97, 31, 8), (3, 200, 8), (150, 1, 3)], torch.float32, 0.5, 1),
    "f16_m28": (2, 28, [(70, 95, 12), (33, 47, 8)], torch.float16, 0.5, 1),
    "bf16_m14_pad2": (3, 14, [(52, 77, 12), (18, 16, 8)], torch.bfloat16, 0.4, 2),
    "f32_m56": (4, 56, [(120, 160, 8), (64, 49, 8)], torch.float32, 0.5, 1),
    "f32_m7_debug_mode": (8, 7, [(45, 66, 10)], torch.float32, -1.0, 1),
    "f32_m28_wide_row": (6, 28, [(6, 4500, 3)], torch.float32, 0.5, 1),      # more 16-byte segments than threads in a workgroup
}


def random_case(name):
    if name not in _RANDOM:
        _RANDOM[name] = _random_case(*RANDOM_CASES[name])
    return _RANDOM[name]


@pytest.mark.parametrize("name", sorted(RANDOM_CASES))
def test_paste_masks_equals_the_torch_path_on_random_cases(name):
    case = random_case(name)
    flat, views = _C().paste_masks(case["maps"].to(DEV), case["boxes"].to(DEV), case["sizes"], case["threshold"],
                                   case["padding"], counts=case["counts"])
    _check_case(views, case["planes"], case["near"], _windows(case["boxes"], case["M"], case["padding"], case["det_sizes"]))
    # per-detection sizes give the same planes
    _, single = _C().paste_masks(case["maps"].to(DEV), case["boxes"].to(DEV), case["det_sizes"], case["threshold"],
                                 case["padding"])
    assert all(torch.equal(a[0, 0], b) for a, b in zip(single, [p for v in views for p in v[:, 0]]))


@pytest.mark.parametrize("shift", [1, 7, 16])
def test_guard_bands_around_planes_at_odd_offsets(shift):
    """through the C ABI: planes back to back from an odd byte address inside a buffer of 0xAB, 64 guard bytes before and
    after — the narrow stores at the head and tail of every row must stay inside the planes and cover them.  Shift 16 is
    the aligned control: the first plane starts on a 16-byte boundary (the later ones still do not: odd plane sizes)"""
    from maskrcnn_benchmark import _lib
    case = random_case("f32_m28_mixed_sizes")
    maps, boxes = case["maps"][:, 0].contiguous().to(DEV), case["boxes"].to(DEV)
    N = maps.shape[0]
    offsets, end = [], 64 + shift
    for h, w in case["det_sizes"]:
        offsets.append(end)
        end += h * w
    buf = torch.full((end + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    det_hw = torch.tensor(case["det_sizes"], dtype=torch.int32, device=DEV)
    out_offset = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib.detops_paste_masks(maps.data_ptr(), 0, boxes.data_ptr(), det_hw.data_ptr(), out_offset.data_ptr(), N,
                                           case["M"], 1, 0.5, buf.data_ptr(), _lib.stream_of(maps)), "paste_masks")
    host = buf.cpu()
    assert bool((host[:64 + shift] == 0xAB).all()) and bool((host[end:] == 0xAB).all())
    body = host[64 + shift:end]
    assert int(body.max()) <= 1, "a plane byte was left unwritten"
    _, views = _C().paste_masks(maps, boxes, case["det_sizes"], 0.5, 1)
    for (h, w), o, v in zip(case["det_sizes"], offsets, views):
        assert torch.equal(host[o:o + h * w].view(h, w).bool(), v[0, 0].cpu())


def _rle_dicts(counts, run_offset, det_sizes):
    counts, run_offset = counts.cpu().tolist(), run_offset.cpu().tolist()
    return [{"size": [h, w], "counts": counts[run_offset[i]:run_offset[i + 1]]} for i, (h, w) in enumerate(det_sizes)]


@pytest.mark.parametrize("name", sorted(RANDOM_CASES) + ["fixture0", "fixture3"])
def test_rle_decodes_to_the_dense_planes_exactly(name):
    case = mcpu.batches()[int(name[-1])] if name.startswith("fixture") else random_case(name)
    args = (case["maps"].to(DEV), case["boxes"].to(DEV), case["sizes"], case["threshold"], case["padding"])
    _, views = _C().paste_masks(*args, counts=case["counts"])
    counts, run_offset = _C().paste_masks_rle(*args, counts=case["counts"])
    N = len(case["det_sizes"])
    assert counts.is_cuda and run_offset.is_cuda and counts.dtype == torch.int32 and run_offset.dtype == torch.int64
    assert tuple(run_offset.shape) == (N + 1,) and int(run_offset[0]) == 0 and int(run_offset[-1]) == counts.numel()
    dense = [p for v in views for p in v[:, 0].cpu()]
    windows = _windows(case["boxes"], case["M"], case["padding"], case["det_sizes"])
    misses = 0
    for rle, plane, (x_lo, x_hi, y_lo, y_hi) in zip(_rle_dicts(counts, run_offset, case["det_sizes"]), dense, windows):
        mcpu.assert_canonical(rle)
        assert torch.equal(mcpu.rle_decode(rle), plane)          # the same device function: no exclusions
        if x_hi <= x_lo or y_hi <= y_lo:
            misses += 1
            assert rle["counts"] == [plane.numel()]
    if not name.startswith("fixture") and "wide" not in name:
        assert misses > 0, "no box off the image in this case"


@pytest.mark.parametrize("W", [63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 64, 65])
def test_rle_across_the_scan_tiles_of_64_columns_and_64_detections(N, W):
    """the scan over a detection's columns runs in tiles of 64 columns of the widest image, the scan over the detections'
    run counts in tiles of 64 detections: widths and batch sizes on both sides of a tile, on tiny maps (M = 4, padding 1).
    From 8 detections on the batch holds boxes off the image (no foreground: one run) and boxes larger than it (a window of
    the full height, whose columns chain).  The runs decode to the dense kernel's planes exactly, and those are the torch
    path's outside its near pixels."""
    H = 21
    case = _random_case(1000 + 10 * N + W, 4, [(H, W, N)])
    args = (case["maps"].to(DEV), case["boxes"].to(DEV), case["sizes"], case["threshold"], case["padding"])
    _, views = _C().paste_masks(*args, counts=case["counts"])
    counts, run_offset = _C().paste_masks_rle(*args, counts=case["counts"])
    windows = _windows(case["boxes"], case["M"], case["padding"], case["det_sizes"])
    _check_case(views, case["planes"], case["near"], windows)
    assert tuple(run_offset.shape) == (N + 1,) and int(run_offset[0]) == 0 and int(run_offset[-1]) == counts.numel()
    rles = _rle_dicts(counts, run_offset, case["det_sizes"])
    for rle, plane in zip(rles, views[0][:, 0].cpu()):
        mcpu.assert_canonical(rle)
        assert torch.equal(mcpu.rle_decode(rle), plane)
    assert any(len(r["counts"]) > 1 for r in rles)
    if N >= 8:
        assert any(r["counts"] == [H * W] for r in rles), "no detection without foreground"
        assert any(y_lo == 0 and y_hi == H and len(r["counts"]) > 1 for r, (_, _, y_lo, y_hi) in zip(rles, windows)), \
            "no window of the full height"


def test_rle_special_planes():
    """pixel (0, 0) set (first count 0), a full-height window whose columns chain, an all-ones plane"""
    maps = torch.ones(3, 1, 14, 14, device=DEV)
    boxes = torch.tensor([[-20.0, -20.0, 60.0, 60.0], [-5.0, -50.0, 6.0, 90.0], [3.0, -50.0, 9.0, 90.0]], device=DEV)
    sizes = [(12, 10)] * 3
    _, views = _C().paste_masks(maps, boxes, sizes)
    counts, run_offset = _C().paste_masks_rle(maps, boxes, sizes)
    rles = _rle_dicts(counts, run_offset, sizes)
    assert rles[0]["counts"] == [0, 120] and bool(views[0].all())
    assert rles[1]["counts"][0] == 0 and rles[2]["counts"][0] > 0
    for rle, v in zip(rles, views):
        mcpu.assert_canonical(rle)
        assert torch.equal(mcpu.rle_decode(rle), v[0, 0].cpu())
        assert torch.equal(mcpu.rle_decode(mi.rle_encode(v[0, 0].cpu())), v[0, 0].cpu())
        assert mi.rle_encode(v[0, 0].cpu())["counts"] == rle["counts"]


def test_argument_errors_and_empty_batch():
    from maskrcnn_benchmark import _lib
    lib = _lib.lib
    f = ctypes.c_float
    maps, boxes = torch.rand(2, 28, 28, device=DEV), torch.tensor([[1.0, 1.0, 9.0, 9.0]] * 2, device=DEV)
    hw = torch.tensor([[16, 16]] * 2, dtype=torch.int32, device=DEV)
    off = torch.tensor([0, 256], dtype=torch.int64, device=DEV)
    out = torch.full((512,), 0xAB, dtype=torch.uint8, device=DEV)
    call = lambda N, M, pad: lib.detops_paste_masks(maps.data_ptr(), 0, boxes.data_ptr(), hw.data_ptr(), off.data_ptr(),  # noqa: E731
                                                    N, M, pad, f(0.5), out.data_ptr(), None)
    assert call(2, 28, 0) == -1            # DETOPS_EINVAL: padding < 1
    assert call(2, 28, -1) == -1
    assert call(2, 63, 1) == -1            # M + 2 * padding beyond the kernel's LDS map
    assert call(2, 28, 19) == -1
    assert call(0, 28, 1) == 0             # no-op
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()), "an error or the empty batch wrote something"
    assert call(2, 28, 1) == 0
    torch.cuda.synchronize()
    assert int(out.max()) <= 1
    with pytest.raises(RuntimeError, match="DETOPS_EINVAL"):
        _C().paste_masks(maps, boxes, [(16, 16)] * 2, padding=0)
    with pytest.raises(RuntimeError, match="DETOPS_EINVAL"):
        _C().paste_masks_rle(maps, boxes, [(16, 16)] * 2, padding=0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _C().paste_masks(maps.cpu(), boxes.cpu(), [(16, 16)] * 2)
    flat, views = _C().paste_masks(maps[:0], boxes[:0], [(16, 16)], counts=[0])
    assert flat.numel() == 0 and tuple(views[0].shape) == (0, 1, 16, 16)
    counts, run_offset = _C().paste_masks_rle(maps[:0], boxes[:0], [(16, 16)], counts=[0])
    assert counts.numel() == 0 and run_offset.tolist() == [0]
    # 58 = a 56 x 56 map with padding 1 is served
    big = torch.rand(1, 56, 56, device=DEV)
    _, v = _C().paste_masks(big, boxes[:1], [(16, 16)])
    assert tuple(v[0].shape) == (1, 1, 16, 16)


def test_tiny_model_in_eval_pastes_on_the_device():
    from maskrcnn_benchmark.engine.bench_step import load_cfg, make_device_batches
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    opts = [o for o in mcpu.TINY if o not in ("MODEL.DEVICE", "cpu")]
    cfg = load_cfg("e2e_mask_rcnn_R_50_FPN_1x.yaml", opts + ["MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS", True])
    torch.manual_seed(0)
    model = build_detection_model(cfg).to(DEV).eval()
    (images, _), = make_device_batches(cfg, DEV, images_per_gpu=2, num_batches=1, height=96, width=128)
    seen = {}
    head = model.roi_heads["mask"]
    hook = head.predictor.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o.detach()))
    with torch.no_grad():
        dets = model(images)
    hook.remove()
    assert len(dets) == 2 and sum(len(d) for d in dets) > 0
    logits = seen["logits"]
    labels = torch.cat([d.get_field("labels") for d in dets])
    prob = logits.sigmoid()[torch.arange(logits.shape[0], device=DEV), labels][:, None].cpu()
    k = 0
    for d in dets:
        n, (w, h) = len(d), d.size
        mask = d.get_field("mask")
        assert mask.dtype == torch.bool and tuple(mask.shape) == (n, 1, h, w) and mask.is_cuda
        ref = mi.paste_masks_torch(prob[k:k + n], d.bbox.cpu(), h, w, 0.5, 1)[:, 0]
        near = mcpu.near_planes(prob[k:k + n], d.bbox.cpu(), h, w, 0.5, 1)
        assert int(near.sum()) <= MAX_NEAR_SHARE * max(near.numel(), 1)
        assert torch.equal(mask[:, 0].cpu() | near, ref | near)
        k += n
    coco = mi.MaskPostProcessorCOCOFormat(head.post_processor.masker)
    with torch.no_grad():
        out = coco(logits, dets)
    for d, o in zip(dets, out):
        rles = o.get_field("mask")
        assert isinstance(rles, list) and len(rles) == len(d)
        w, h = d.size
        for rle, m in zip(rles, d.get_field("mask")):
            assert rle["size"] == [h, w] and sum(rle["counts"]) == h * w
            mcpu.assert_canonical(rle)
            assert torch.equal(mcpu.rle_decode(rle), m[0].cpu())
