"""The input path without a GPU: the numpy implementation of detops_image_batch_u8's definition (_image_prep_cpu.py)
and the host transforms (data/transforms) against tests/golden/image_prep_reference.npz, which holds Pillow's own
resizes and the batches made by the torch expressions of ToTensor / Normalize / to_image_list.  No tolerance: the
definition is integer arithmetic plus a fixed sequence of fp32 operations, every comparison is of bits."""
import ctypes
import random

import numpy as np
import pytest
import torch

import image_prep_cases as C
from maskrcnn_benchmark import _image_prep_cpu
from maskrcnn_benchmark.data import transforms as T


def _table(b):
    return T.normalisation_table(b["mean"].tolist(), b["std"].tolist(), bool(b["bgr"]))


def test_numpy_resize_equals_pillow_fixture():
    for src, resized in C.cases():
        out = _image_prep_cpu.resize_u8(src, resized.shape[0], resized.shape[1])
        assert out.dtype == np.uint8 and np.array_equal(out, resized), (src.shape, resized.shape)


def test_skipped_pass_leaves_the_axis_untouched():
    src, resized = C.cases()[6]                                    # 40 x 30 -> 40 x 30
    assert np.array_equal(resized, src)                            # Pillow returns the image itself
    assert np.array_equal(_image_prep_cpu.resize_u8(src, 40, 30), src)
    wide = _image_prep_cpu.resize_u8(src, 40, 45)                  # only the horizontal pass runs: rows stay independent
    assert np.array_equal(wide[7:8], _image_prep_cpu.resize_u8(src[7:8], 1, 45))


def test_numpy_batches_equal_fixture_bits():
    """three batches: divisibility 32 and 0, every flip combination, std != 1, TO_BGR255 on and off"""
    cs = C.cases()
    seen_flips = set()
    for b in C.batches():
        items = [(cs[c][0], cs[c][1].shape[:2], int(f)) for c, f in zip(b["cases"], b["flips"])]
        seen_flips.update(int(f) for f in b["flips"])
        out = C.raw_batch(items, _table(b), bool(b["bgr"]), int(b["divisible"])).to("cpu")
        assert tuple(out.tensors.shape) == b["batch"].shape
        assert np.array_equal(C.bits(out.tensors), C.bits(b["batch"]))
        assert out.image_sizes == [tuple(cs[c][1].shape[:2]) for c in b["cases"]]
    assert seen_flips == {0, 1, 2, 3}
    assert any((b["std"] != 1).any() for b in C.batches()) and any(not b["bgr"] for b in C.batches())


@pytest.mark.parametrize("flip", [1, 2, 3])
def test_flips_mirror_the_resized_image(flip):
    src, resized = C.cases()[0]
    out = C.raw_batch([(src, resized.shape[:2], flip)], C.identity_table(), False).to("cpu").tensors[0]
    want = np.ascontiguousarray(C.flipped(resized, flip)).transpose(2, 0, 1).astype(np.float32)
    assert np.array_equal(out.numpy(), want)


def test_padding_is_positive_zero():
    src, resized = C.cases()[1]                                    # 50 x 37 inside 64 x 64
    table = T.normalisation_table([102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0], True)
    out = C.raw_batch([(src, resized.shape[:2], 0)], table, True, 32).to("cpu").tensors
    assert tuple(out.shape) == (1, 3, 64, 64)
    pad = np.ones((64, 64), dtype=bool)
    pad[:50, :37] = False
    assert pad.sum() and (C.bits(out)[0][:, pad] == 0).all()       # all bits clear: +0.0, not -0.0
    assert (C.bits(out)[0][:, ~pad] != 0).any()


def test_normalisation_table_is_the_torch_expressions():
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    u8 = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16).expand(3, 16, 16).contiguous()
    for bgr in (False, True):
        want = T.Normalize(mean, std, bgr)(u8.to(torch.float32) / 255)
        assert np.array_equal(C.bits(T.normalisation_table(mean, std, bgr)), C.bits(want.reshape(3, 256)))


def test_get_size_hand_values():
    r = T.Resize((800,), 1333)
    assert r.get_size((640, 480)) == (800, 1066)
    assert r.get_size((640, 427)) == (800, 1199)
    assert r.get_size((640, 360)) == (750, 1333)
    assert r.get_size((480, 640)) == (1066, 800)
    assert T.Resize(480, 1333).get_size((640, 480)) == (480, 640)  # the shorter side is there already: unchanged
    random.seed(3)
    draws = {T.Resize((640, 672, 704), 1333).get_size((640, 480))[0] for _ in range(40)}
    assert draws == {640, 672, 704}


def _cfg(opts=()):
    from maskrcnn_benchmark.engine.bench_step import load_cfg

    return load_cfg("e2e_mask_rcnn_R_50_FPN_1x.yaml", ["MODEL.DEVICE", "cpu"] + list(opts))


def test_host_pipeline_equals_fixture(monkeypatch):
    """build_transforms on PIL images (Pillow's own resize) + BatchCollator.  The fixture's shape pairs are not ones
    Resize.get_size produces, so get_size is pinned per image; the flips come from probabilities 0 and 1."""
    Image = pytest.importorskip("PIL.Image")
    from maskrcnn_benchmark.data.collate_batch import BatchCollator
    from maskrcnn_benchmark.structures.bounding_box import BoxList

    cs = C.cases()
    for b in C.batches():
        samples = []
        for c, f in zip(b["cases"], b["flips"]):
            src, resized = cs[c]
            cfg = _cfg(["INPUT.PIXEL_MEAN", b["mean"].tolist(), "INPUT.PIXEL_STD", b["std"].tolist(), "INPUT.TO_BGR255", bool(b["bgr"]),
                        "INPUT.HORIZONTAL_FLIP_PROB_TRAIN", float(f & 1), "INPUT.VERTICAL_FLIP_PROB_TRAIN", float((f >> 1) & 1)])
            pipeline = T.build_transforms(cfg, is_train=True)
            monkeypatch.setattr(T.Resize, "get_size", lambda self, size, hw=resized.shape[:2]: tuple(hw))
            target = BoxList(torch.tensor([[1.0, 1.0, 3.0, 3.0]]), (src.shape[1], src.shape[0]))
            image, target = pipeline(Image.fromarray(src, "RGB"), target)
            assert target.size == (resized.shape[1], resized.shape[0])
            samples.append((image, target, 0))
        out = BatchCollator(int(b["divisible"]))(samples)[0]
        assert np.array_equal(C.bits(out.tensors), C.bits(b["batch"]))


def test_host_pipeline_with_its_own_get_size():
    """no pinning: 37 x 53 at MIN_SIZE 75, through the host pipeline and through the deferred one + the numpy path"""
    Image = pytest.importorskip("PIL.Image")
    src = C.cases()[0][0]                                          # h 37, w 53
    cfg = _cfg(["INPUT.MIN_SIZE_TRAIN", (75,), "INPUT.MAX_SIZE_TRAIN", 200, "INPUT.HORIZONTAL_FLIP_PROB_TRAIN", 1.0])
    image, _ = T.build_transforms(cfg, True)(Image.fromarray(src, "RGB"), _box(src))
    assert tuple(image.shape) == (3, 75, 107)                      # int(75 * 53 / 37) = int(107.43): truncation
    raw, _ = T.build_transforms(cfg, True, device_prep=True)(Image.fromarray(src, "RGB"), _box(src))
    assert (raw.size, raw.flip) == ((107, 75), 1)
    table = T.normalisation_table(cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255)
    out = C.raw_batch([(raw.data, (75, 107), raw.flip)], table, cfg.INPUT.TO_BGR255).to("cpu").tensors[0]
    assert np.array_equal(C.bits(out), C.bits(image))


def _box(src):
    from maskrcnn_benchmark.structures.bounding_box import BoxList

    return BoxList(torch.tensor([[1.0, 1.0, 3.0, 3.0]]), (src.shape[1], src.shape[0]))


def test_nonzero_jitter_is_not_built():
    for key in ("BRIGHTNESS", "CONTRAST", "SATURATION", "HUE"):
        with pytest.raises(NotImplementedError, match="BRIGHTNESS / CONTRAST / SATURATION / HUE"):
            T.build_transforms(_cfg(["INPUT." + key, 0.1]), is_train=True)
    T.build_transforms(_cfg(), is_train=True)                      # the default zeros are the identity
    T.build_transforms(_cfg(["INPUT.HUE", 0.1]), is_train=False)   # jitter is a training transform


def test_wrapper_rejects_malformed_arguments():
    from maskrcnn_benchmark import _C

    raw, off = torch.zeros(12, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    geom, table = torch.tensor([[2, 2, 2, 2, 0]], dtype=torch.int32), C.identity_table()
    assert tuple(_C.image_batch(raw, off, geom, table, False, 2, 2).shape) == (1, 3, 2, 2)
    with pytest.raises(ValueError):
        _C.image_batch(raw, off, geom, table[:, :255], False, 2, 2)
    with pytest.raises(ValueError):
        _C.image_batch(raw, off, geom, table, False, 1, 2)         # oh > Hp
    with pytest.raises(ValueError):
        _C.image_batch(raw.to(torch.int8), off, geom, table, False, 2, 2)


def test_entry_point_validates_on_the_host():
    """the library checks the host copy of the records before it touches the device: no GPU needed"""
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark._lib import lib

    one = ctypes.c_char()
    p = ctypes.addressof(one)

    def call(h, w, oh, ow, N=1, Hp=64, Wp=64):
        geom = (ctypes.c_int32 * 5)(h, w, oh, ow, 0)
        return lib.detops_image_batch_u8(p, 0, p, p, ctypes.addressof(geom), N, p, 0, Hp, Wp, 0, p, None)

    assert call(8, 8, 8, 8, N=0) == 0 and call(8, 8, 8, 8, Hp=0) == 0           # nothing to do
    assert call(8, 8, 8, 8, N=-1) == -1
    assert call(8, 8, 65, 8) == -1 and call(8, 8, 8, 65) == -1 and call(0, 8, 8, 8) == -1
    assert _C.IMAGE_PREP_MAX_KSIZE == 17 == _image_prep_cpu.axis_ksize(80, 10)
    assert _image_prep_cpu.axis_ksize(81, 10) == 19
    assert call(81, 8, 10, 8) == -1 and call(8, 81, 8, 10) == -1               # a downscale beyond 8: DETOPS_EINVAL
    assert lib.detops_image_batch_u8(None, 0, p, p, p, 1, p, 0, 8, 8, 0, p, None) == -1
