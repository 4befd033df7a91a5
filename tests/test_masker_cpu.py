"""Masks at inference on the CPU (`-m "not gpu"`): `Masker` / `paste_masks_torch` / `expand_boxes` / `expand_masks` of
modeling/roi_heads/mask_head/inference.py against tests/golden/masker_reference.npz (the reference's own `Masker`, see
tests/golden/make_golden_masker.py), the uncompressed-RLE encoder, and MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS on the tiny
model.  tests/test_masker_gpu.py reuses the fixture loader and the decoder."""
import os

import numpy as np
import pytest
import torch

import cpu_shim
from maskrcnn_benchmark.modeling.roi_heads.mask_head import inference as mi
from maskrcnn_benchmark.structures.bounding_box import BoxList

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masker_reference.npz")
_CACHE = {}


def batches():
    """[{M, threshold, padding, maps [N,M,M], boxes [N,4], sizes [(H, W)], counts [n_i], planes / near: one bool [H, W] per
    detection, expanded [N,4]}], loaded once and shared (read-only)"""
    if "b" not in _CACHE:
        z = np.load(GOLDEN)
        out = []
        for b in range(int(z["n_batches"])):
            g = lambda k: z["b%d_%s" % (b, k)]  # noqa: E731
            sizes = [(int(h), int(w)) for h, w in g("sizes")]
            counts = [int(c) for c in g("counts")]
            det_sizes = [s for s, c in zip(sizes, counts) for _ in range(c)]
            total = sum(h * w for h, w in det_sizes)
            planes = np.unpackbits(g("planes"))[:total].astype(bool)
            near = np.unpackbits(g("near"))[:total].astype(bool)
            cuts = np.cumsum([0] + [h * w for h, w in det_sizes])
            split = lambda a: [torch.from_numpy(a[cuts[i]:cuts[i + 1]].reshape(det_sizes[i]))  # noqa: E731
                               for i in range(len(det_sizes))]
            out.append(dict(M=g("maps").shape[-1], threshold=float(g("threshold")), padding=int(g("padding")),
                            maps=torch.from_numpy(g("maps")), boxes=torch.from_numpy(g("boxes")), sizes=sizes, counts=counts,
                            det_sizes=det_sizes, planes=split(planes), near=split(near),
                            expanded=torch.from_numpy(g("expanded"))))
        _CACHE["b"] = out
        _CACHE["z"] = z
    return _CACHE["b"]


def rle_decode(rle):
    """uncompressed COCO RLE -> bool [H, W] (column-major runs, starting with a 0-run)"""
    H, W = rle["size"]
    counts = np.asarray(rle["counts"], np.int64)
    assert counts.sum() == H * W
    flat = np.zeros(H * W, bool)
    ends = np.cumsum(counts)
    for k in range(1, len(counts), 2):
        flat[ends[k - 1]:ends[k]] = True
    return torch.from_numpy(flat.reshape(W, H).T.copy())


NEAR = 1e-5


def near_planes(masks, boxes, im_h, im_w, threshold=0.5, padding=1):
    """bool [n, im_h, im_w] on the CPU: the pixels whose interpolated value (ATen's CPU resize) lies within NEAR of the
    threshold, where an fp32 restatement of the resize may land on the other side (`threshold < 0`: within NEAR of 0, not
    0); the fixture's "near" planes are the same thing from the reference's functions"""
    import torch.nn.functional as F
    masks, boxes = masks.detach().float().cpu(), boxes.detach().float().cpu()
    n = masks.shape[0]
    out = torch.zeros((n, im_h, im_w), dtype=torch.bool)
    if n == 0:
        return out
    padded, scale = mi.expand_masks(masks, padding)
    for i, (x1, y1, x2, y2) in enumerate(mi.expand_boxes(boxes, scale).to(torch.int32).tolist()):
        w, h = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
        x_lo, x_hi, y_lo, y_hi = max(x1, 0), min(x2 + 1, im_w), max(y1, 0), min(y2 + 1, im_h)
        if x_hi <= x_lo or y_hi <= y_lo:
            continue
        v = F.interpolate(padded[i:i + 1], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
        near = (v - max(threshold, 0.0)).abs() <= NEAR
        if threshold < 0:
            near &= v != 0
        out[i, y_lo:y_hi, x_lo:x_hi] = near[y_lo - y1:y_hi - y1, x_lo - x1:x_hi - x1]
    return out


def test_near_planes_helper_equals_the_fixture():
    for case in batches():
        k = 0
        for (m, bl), (h, w) in zip(boxlists(case), case["sizes"]):
            got = near_planes(m, bl.bbox, h, w, case["threshold"], case["padding"])
            for i in range(len(bl)):
                assert torch.equal(got[i], case["near"][k])
                k += 1


def assert_canonical(rle):
    H, W = rle["size"]
    c = rle["counts"]
    assert all(isinstance(v, int) for v in c) and len(c) >= 1
    assert sum(c) == H * W
    assert all(v > 0 for v in c[1:]), "only the first count may be 0"
    assert c[0] >= 0


def boxlists(case):
    out, k = [], 0
    for (h, w), n in zip(case["sizes"], case["counts"]):
        out.append((case["maps"][k:k + n, None], BoxList(case["boxes"][k:k + n], (w, h), mode="xyxy")))
        k += n
    return out


def test_fixture_covers_what_it_should():
    bs = batches()
    assert sorted({b["M"] for b in bs}) == [7, 14, 28]
    assert any(b["threshold"] < 0 for b in bs)
    assert {0, 1, 67} <= set(bs[0]["counts"])
    widths = {w for b in bs for _, w in b["sizes"]}
    assert {1, 15, 16, 17, 53, 64} <= widths and max(max(s) for b in bs for s in b["sizes"]) <= 80
    for b in bs:
        pixels = sum(h * w for h, w in b["det_sizes"])
        assert sum(int(n.sum()) for n in b["near"]) <= 1e-4 * pixels
        lo = b["expanded"][:, :2]
        assert ((lo > -1) & (lo < 0)).any(), "no box where truncation and floor differ"


@pytest.mark.parametrize("b", range(4))
def test_masker_reproduces_the_reference_exactly(b):
    case = batches()[b]
    pairs = boxlists(case)
    res = mi.Masker(threshold=case["threshold"], padding=case["padding"])([m for m, _ in pairs], [bl for _, bl in pairs])
    assert len(res) == len(pairs)
    k = 0
    for r, (m, bl), (h, w) in zip(res, pairs, case["sizes"]):
        if len(bl) == 0:
            assert tuple(r.shape) == (0, 1, case["M"], case["M"]) and r.dtype == m.dtype
            continue
        assert r.dtype == torch.bool and tuple(r.shape) == (len(bl), 1, h, w)
        for i in range(len(bl)):
            assert torch.equal(r[i, 0], case["planes"][k]), (b, k)     # every pixel, the near ones included
            k += 1
    assert k == len(case["planes"])


def test_forward_single_image_and_single_boxlist_call():
    case = batches()[1]
    m, bl = boxlists(case)[0]
    masker = mi.Masker(threshold=case["threshold"], padding=case["padding"])
    one = masker.forward_single_image(m, bl)
    assert torch.equal(one, masker(m, bl)[0]) and torch.equal(one, masker([m], [bl])[0])
    assert torch.equal(one[:, 0], torch.stack(case["planes"][:len(bl)]))
    # xywh boxes are converted
    assert torch.equal(masker.forward_single_image(m, bl.convert("xywh")), one)


def test_expand_boxes_and_expand_masks_equal_the_reference():
    for case in batches():
        scale = float(case["M"] + 2 * case["padding"]) / case["M"]
        assert torch.equal(mi.expand_boxes(case["boxes"], scale), case["expanded"])
    z = _CACHE["z"]
    padded, scale = mi.expand_masks(torch.from_numpy(z["pad_in"]), 2)
    assert scale == float(z["pad_scale"]) and torch.equal(padded, torch.from_numpy(z["pad_out"]))
    with pytest.raises(ValueError):
        mi.expand_masks(torch.zeros(1, 1, 4, 4), 0)


def test_empty_image_and_assertions_behave_like_the_reference():
    z_shape = tuple(int(v) for v in (batches(), _CACHE["z"])[1]["empty_shape"])
    masker = mi.Masker()
    empty = masker([torch.zeros(0, 1, 28, 28)], [BoxList(torch.zeros(0, 4), (53, 40), mode="xyxy")])[0]
    assert tuple(empty.shape) == z_shape == (0, 1, 28, 28) and empty.dtype == torch.float32
    bl = BoxList(torch.tensor([[1.0, 1.0, 5.0, 5.0]]), (16, 16), mode="xyxy")
    with pytest.raises(AssertionError, match="Masks and boxes should have the same length."):
        masker([torch.zeros(1, 1, 28, 28)], [bl, bl])
    with pytest.raises(AssertionError, match="Number of objects should be the same."):
        masker([torch.zeros(2, 1, 28, 28)], [bl])


def test_box_off_the_image_gives_an_all_zero_plane():
    boxes = torch.tensor([[40.0, 3.0, 60.0, 9.0], [-30.0, -30.0, -8.0, -8.0], [2.0, 2.0, 9.0, 9.0]])
    out = mi.paste_masks_torch(torch.full((3, 1, 14, 14), 0.9), boxes, 20, 16)
    assert not out[0].any() and not out[1].any() and out[2].any()


def test_truncation_toward_zero_not_floor():
    # expanded left / top edge -0.4 -> integer 0: the map is resized to x2 + 1 pixels and starts at pixel 0; floor would
    # resize it to x2 + 2 pixels and start at -1
    import torch.nn.functional as F
    M, scale = 14, 16.0 / 14
    hi = 9.3
    lo = (2 * -0.4 - hi * (1 - scale)) / (1 + scale)
    box = torch.tensor([[lo, lo, hi, hi]])
    exp = mi.expand_boxes(box, scale)[0]
    assert -1 < float(exp[0]) < 0 and int(exp[0]) == 0
    x2 = int(exp[2])
    m = torch.sigmoid(3 * torch.randn(1, 1, M, M, generator=torch.Generator().manual_seed(3)))
    got = mi.paste_masks_torch(m, box, 16, 16)[0, 0]
    padded = F.pad(m, (1, 1, 1, 1))
    trunc = F.interpolate(padded, size=(x2 + 1, x2 + 1), mode="bilinear", align_corners=False)[0, 0] > 0.5
    floor = F.interpolate(padded, size=(x2 + 2, x2 + 2), mode="bilinear", align_corners=False)[0, 0] > 0.5
    assert torch.equal(got[:x2 + 1, :x2 + 1], trunc) and not got[x2 + 1:].any() and not got[:, x2 + 1:].any()
    assert not torch.equal(got[:x2 + 1, :x2 + 1], floor[1:, 1:])


def test_rle_encoder_roundtrip_and_canonical_form():
    for case in batches():
        for plane in case["planes"][::3]:
            rle = mi.rle_encode(plane)
            assert rle["size"] == list(plane.shape)
            assert_canonical(rle)
            assert torch.equal(rle_decode(rle), plane)
    zero = mi.rle_encode(torch.zeros(5, 7, dtype=torch.bool))
    assert zero == {"size": [5, 7], "counts": [35]}
    first = torch.zeros(4, 3, dtype=torch.bool)
    first[0, 0] = True
    first[3, 2] = True
    rle = mi.rle_encode(first)
    assert rle["counts"] == [0, 1, 10, 1]
    assert_canonical(rle)
    assert torch.equal(rle_decode(rle), first)
    assert mi.rle_encode(torch.ones(2, 2, dtype=torch.bool))["counts"] == [0, 4]


def test_coco_format_post_processor_on_cpu_tensors():
    case = batches()[1]
    m, bl = boxlists(case)[0]
    n, M = len(bl), case["M"]
    bl.add_field("labels", torch.ones(n, dtype=torch.int64))
    logits = torch.zeros(n, 2, M, M)
    logits[:, 1] = torch.logit(m[:, 0].double().clamp(1e-6, 1 - 1e-6)).float()
    pp = mi.MaskPostProcessorCOCOFormat(mi.Masker(threshold=0.5, padding=1))
    out = pp(logits, [bl])[0]
    rles = out.get_field("mask")
    dense = mi.MaskPostProcessor(mi.Masker(threshold=0.5, padding=1))(logits, [bl])[0].get_field("mask")
    assert len(rles) == n and tuple(dense.shape) == (n, 1, bl.size[1], bl.size[0])
    for r, d in zip(rles, dense):
        assert_canonical(r)
        assert torch.equal(rle_decode(r), d[0])
    with pytest.raises(ValueError):
        mi.MaskPostProcessorCOCOFormat(None)(logits, [bl])


TINY = ["MODEL.DEVICE", "cpu", "MODEL.RPN.PRE_NMS_TOP_N_TEST", 100, "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", 50,
        "MODEL.RESNETS.RES2_OUT_CHANNELS", 16, "MODEL.RESNETS.WIDTH_PER_GROUP", 4, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16,
        "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 32, "MODEL.ROI_MASK_HEAD.CONV_LAYERS", (16, 16), "MODEL.ROI_HEADS.SCORE_THRESH", 0.0,
        "MODEL.ROI_HEADS.DETECTIONS_PER_IMG", 8]


def test_postprocess_masks_switch_on_the_tiny_model():
    from maskrcnn_benchmark.data.synthetic import BatchCollator, SyntheticCOCODataset
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    ds = SyntheticCOCODataset(length=2, height=96, width=128, with_masks=True, min_objects=2, max_objects=4)
    images, _, _ = BatchCollator(32)([ds[0], ds[1]])
    dets = {}
    for on in (False, True):
        cfg = load_cfg("e2e_mask_rcnn_R_50_FPN_1x.yaml", TINY + ["MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS", on])
        torch.manual_seed(0)
        model = build_detection_model(cfg).eval()
        assert (model.roi_heads["mask"].post_processor.masker is not None) == on
        with cpu_shim.install(), torch.no_grad():
            dets[on] = model(images)
    assert sum(len(d) for d in dets[True]) > 0
    for plain, pasted in zip(dets[False], dets[True]):
        n = len(plain)
        assert len(pasted) == n and torch.equal(plain.bbox, pasted.bbox)
        prob = plain.get_field("mask")
        assert tuple(prob.shape) == (n, 1, 28, 28) and prob.dtype == torch.float32
        mask = pasted.get_field("mask")
        if n == 0:
            continue
        w, h = pasted.size
        assert mask.dtype == torch.bool and tuple(mask.shape) == (n, 1, h, w)
        assert torch.equal(mask, mi.paste_masks_torch(prob, plain.bbox, h, w, 0.5, 1))
