"""Test-time box augmentation on the device: the HIP merge (csrc/bbox_aug.hip) against the torch formulation bit for bit at
every shape where it takes another route, the reference's fixture end to end through merge + segmented NMS + top-k, and the
model-level identities in the layouts `nchw` and `all`.  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

import bbox_aug_cases as B

pytestmark = pytest.mark.gpu

NAME = "tiny_coco_bbox_aug_gpu"


def _device_merge(case, thresh=B.THRESH):
    from maskrcnn_benchmark import _C

    return _C.bbox_aug_merge(case["boxes"].cuda(), case["scores"].cuda(), case["row_offset"], case["geom"], case["ratio"],
                             case["N"], case["T"], thresh)


@pytest.mark.parametrize("name", sorted(B.MERGE_CASES))
def test_merge_equals_the_torch_formulation_bit_for_bit(name):
    case = B.make_case(**B.MERGE_CASES[name])
    want_b, want_s, want_seg, want_longest = B.reference(case)
    boxes, scores, seg, longest = _device_merge(case)
    assert boxes.is_cuda and scores.is_cuda and seg.is_cuda and seg.dtype == torch.int32
    assert seg.cpu().tolist() == want_seg.tolist() and longest == want_longest
    assert boxes.shape == want_b.shape and scores.shape == want_s.shape
    assert torch.equal(B.bits(scores), B.bits(want_s))
    assert torch.equal(B.bits(boxes), B.bits(want_b))
    if name == "nothing_passes" or name == "no_rows":
        assert boxes.shape[0] == 0 and longest == 0 and not seg.any()
    else:
        assert boxes.shape[0] > 0
    again = _device_merge(case)                                   # two runs: identical bytes
    assert torch.equal(B.bits(again[0]), B.bits(boxes)) and torch.equal(B.bits(again[1]), B.bits(scores))
    assert torch.equal(again[2], seg) and again[3] == longest


def test_boxes_at_an_unaligned_address_are_served():
    """a contiguous view that starts 4 bytes into its storage: the kernel's 16-byte box loads need an aligned copy"""
    from maskrcnn_benchmark import _C

    case = B.make_case(**B.MERGE_CASES["c21_n3_t4"])
    want_b, want_s, want_seg, _ = B.reference(case)
    flat = torch.zeros(case["boxes"].numel() + 1, device="cuda")
    flat[1:] = case["boxes"].reshape(-1).cuda()
    view = flat[1:].view(case["boxes"].shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    boxes, scores, seg, _ = _C.bbox_aug_merge(view, case["scores"].cuda(), case["row_offset"], case["geom"], case["ratio"],
                                              case["N"], case["T"], B.THRESH)
    assert torch.equal(B.bits(boxes), B.bits(want_b)) and torch.equal(B.bits(scores), B.bits(want_s))
    assert seg.cpu().tolist() == want_seg.tolist()


def test_every_pair_is_a_candidate_below_every_score():
    """threshold -1: M = R * (C - 1), every box of the fixture mapped like the reference's BoxList arithmetic"""
    fx = B.load_fixture()
    R, C = fx["scores"].shape
    boxes, scores, seg, _ = _device_merge(fx, thresh=-1.0)
    want_b, want_s, want_seg, _ = B.reference(fx, thresh=-1.0)
    assert boxes.shape[0] == R * (C - 1)
    assert torch.equal(B.bits(boxes), B.bits(want_b)) and torch.equal(B.bits(scores), B.bits(want_s))
    assert seg.cpu().tolist() == want_seg.tolist()
    merged = fx["merged"].view(R, C, 4)
    lo, hi = fx["row_offset"][0].item(), fx["row_offset"][fx["T"]].item()
    assert torch.equal(B.bits(boxes[:hi - lo]), B.bits(merged[lo:hi, 1]))      # image 0, class 1: the reference's own boxes


def test_fixture_end_to_end_on_the_device():
    B.check_fixture_detections(B.load_fixture(), "cuda")


@pytest.fixture()
def registered(tmp_path):
    pytest.importorskip("PIL.Image")
    from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog

    DatasetCatalog.register(NAME, *B.write_coco(str(tmp_path)))
    yield NAME
    DatasetCatalog.REGISTERED.pop(NAME, None)


def test_preparing_again_on_the_device_equals_a_fresh_pack_at_that_target():
    """one packed batch, its bytes uploaded once (`on`), prepared at (size, flip) with separately uploaded geometry records =
    the batch packed for that target from the start and sent through `.to("cuda")`, bit for bit, in both memory formats;
    and = the numpy path of the same definition"""
    from maskrcnn_benchmark.data.collate_batch import RawImageBatch
    from maskrcnn_benchmark.data.transforms import RawImage, Resize, normalisation_table

    rng = np.random.RandomState(3)
    data = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for w, h in ((64, 48), (40, 56), (33, 33))]
    table = normalisation_table([102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0], True)

    def pack(min_size, max_size, flip, channels_last):
        resize = Resize(min_size, max_size)
        return RawImageBatch.pack([RawImage(d, resize.get_size((d.shape[1], d.shape[0]))[::-1], int(flip)) for d in data],
                                  table, True, 32, channels_last)

    for channels_last in (False, True):
        base = pack(96, 128, False, channels_last)
        once = base.on("cuda")
        assert once.buffer.is_cuda and once.on("cuda") is once and not once.geom.is_cuda
        for min_size, max_size, flip in ((96, 128, False), (96, 128, True), (50, 4000, False), (131, 150, True), (20, 4000, True)):
            fresh = pack(min_size, max_size, flip, channels_last)
            want = fresh.to("cuda")
            again = once.prepare(min_size, max_size, flip)
            assert again.tensors.is_cuda and again.image_sizes == want.image_sizes and again.tensors.shape == want.tensors.shape
            assert again.tensors.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
            assert torch.equal(B.bits(again.tensors), B.bits(want.tensors)), (min_size, max_size, flip)
            assert torch.equal(B.bits(again.tensors), B.bits(fresh.to("cpu").tensors)), (min_size, max_size, flip)


def _exactly_equal(a, b):
    assert a.size == b.size and torch.equal(B.bits(a.bbox), B.bits(b.bbox))
    assert torch.equal(a.get_field("scores"), b.get_field("scores")) and torch.equal(a.get_field("labels"), b.get_field("labels"))


@pytest.mark.parametrize("layout", ["nchw", "all"])
def test_model_level_identities(registered, layout, monkeypatch):
    """The plain model through model(images.to(device)) against the BBOX_AUG model (same weights) through
    im_detect_bbox_aug (on + prepare per pass, unfiltered head outputs, merge, one segmented NMS, limit), two forwards.
    ENABLED without flip and scales: exactly the plain detections.  The test scale once more: the same detections in value
    (every candidate meets its exact duplicate, NMS removes one).

    MIOpen's default convolution solvers are not reproducible from call to call (the backbone features of two forwards of
    one batch differ, boxes by 3e-5 of a pixel); with torch.backends.cudnn.deterministic it picks reproducible ones and the
    forward is bit-stable, which the test asserts first, as tests/test_model_gpu.py does for its comparison."""
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    plain, aug = B.plain_and_augmented(registered, "cuda", layout, [])
    twice, _ = B.plain_and_augmented(registered, "cuda", layout, [])
    for a, b in zip(plain, twice):
        _exactly_equal(a, b)                                      # the yardstick: plain inference reproduces itself
    for a, b in zip(plain, aug):
        _exactly_equal(a, b)
    plain, aug = B.plain_and_augmented(registered, "cuda", layout, ["TEST.BBOX_AUG.SCALES", (96,), "TEST.BBOX_AUG.MAX_SIZE", 128])
    for a, b in zip(plain, aug):
        assert a.size == b.size and np.array_equal(B.canonical(a), B.canonical(b))


def test_inference_with_bbox_aug_returns_a_bbox_table(registered):
    from maskrcnn_benchmark.data import make_data_loader
    from maskrcnn_benchmark.engine.inference import inference

    cfg = B.narrow_cfg(registered, "cuda", ["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (64,),
                                            "TEST.BBOX_AUG.MAX_SIZE", 100, "TEST.BBOX_AUG.SCALE_H_FLIP", True])
    model = B.build_model(cfg, "cuda", "all")
    res = inference(model, make_data_loader(cfg, is_train=False), registered, bbox_aug=True, device="cuda")
    assert set(res.results) == {"bbox"} and all(-1 <= v <= 1 for v in res.results["bbox"].values())
