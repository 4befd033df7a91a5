"""detops_image_batch_u8 on the device (csrc/image_prep.hip) against tests/golden/image_prep_reference.npz (Pillow's own
resizes, the torch expressions of ToTensor / Normalize / to_image_list) and against the numpy implementation of the same
definition.  Never imports PIL.  No tolerance anywhere: every comparison is of bits."""
import numpy as np
import pytest
import torch

import image_prep_cases as C
from maskrcnn_benchmark import _C, _image_prep_cpu
from maskrcnn_benchmark.data import transforms as T

pytestmark = pytest.mark.gpu

LAYOUTS = [False, True]        # channels_last


def _assert_layout(t, channels_last):
    if channels_last:
        assert t.is_contiguous(memory_format=torch.channels_last)
    else:
        assert t.is_contiguous()


@pytest.mark.parametrize("channels_last", LAYOUTS)
def test_every_fixture_case_on_the_device(channels_last):
    """the uint8 stage through the identity table, one image per launch: odd sizes, a single pass, no pass, one pixel, a
    one-pixel-wide source, output widths 65 and 129"""
    for src, resized in C.cases():
        oh, ow = resized.shape[:2]
        out = C.raw_batch([(src, (oh, ow), 0)], C.identity_table(), False, 0, channels_last).to("cuda").tensors
        assert tuple(out.shape) == (1, 3, oh, ow)
        _assert_layout(out, channels_last)
        assert np.array_equal(out[0].cpu().numpy(), resized.transpose(2, 0, 1).astype(np.float32)), (src.shape, resized.shape)


@pytest.mark.parametrize("channels_last", LAYOUTS)
def test_raw_image_batch_equals_the_host_pipelines_batches(channels_last):
    """RawImageBatch.to("cuda") against the fixture's batches (= the host pipeline's, tests/test_image_prep_cpu.py)"""
    cs = C.cases()
    for b in C.batches():
        items = [(cs[c][0], cs[c][1].shape[:2], int(f)) for c, f in zip(b["cases"], b["flips"])]
        table = T.normalisation_table(b["mean"].tolist(), b["std"].tolist(), bool(b["bgr"]))
        out = C.raw_batch(items, table, bool(b["bgr"]), int(b["divisible"]), channels_last).to("cuda")
        assert tuple(out.tensors.shape) == b["batch"].shape and out.tensors.is_cuda
        _assert_layout(out.tensors, channels_last)
        assert np.array_equal(C.bits(out.tensors), C.bits(b["batch"]))
        assert out.image_sizes == [tuple(cs[c][1].shape[:2]) for c in b["cases"]]


@pytest.mark.parametrize("divisible", [32, 0])
@pytest.mark.parametrize("flip", [0, 1, 2, 3])
def test_three_image_batch_against_the_cpu_path(flip, divisible):
    """different source and destination sizes in one launch; an odd Wp (divisibility 0) takes the 4-byte stores"""
    cs = C.cases()
    items = [(cs[0][0], (70, 131), flip), (cs[1][0], (33, 20), flip ^ 1), (cs[7][0], (45, 77), flip)]
    table = T.normalisation_table([102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0], True)
    for channels_last in LAYOUTS:
        batch = C.raw_batch(items, table, True, divisible, channels_last)
        want, got = batch.to("cpu").tensors, batch.to("cuda").tensors
        assert tuple(got.shape) == ((3, 3, 96, 160) if divisible else (3, 3, 70, 131))
        assert np.array_equal(C.bits(got), C.bits(want))
        for i, (_, (oh, ow), _) in enumerate(items):
            pad = torch.ones(got.shape[2:], dtype=torch.bool)
            pad[:oh, :ow] = False
            assert (torch.from_numpy(C.bits(got))[i][:, pad] == 0).all()        # exactly +0.0


def test_largest_served_downscale_and_one_beyond():
    from maskrcnn_benchmark._lib import lib, ptr, stream_of

    rng = np.random.RandomState(5)
    src = rng.randint(0, 256, (320, 560, 3)).astype(np.uint8)
    table = C.identity_table()
    served = C.raw_batch([(src, (40, 70), 0)], table, False)                   # 8 x on both axes: ksize 17
    assert _image_prep_cpu.axis_ksize(320, 40) == _C.IMAGE_PREP_MAX_KSIZE
    assert np.array_equal(C.bits(served.to("cuda").tensors), C.bits(served.to("cpu").tensors))
    beyond = C.raw_batch([(src, (39, 70), 0), (src[:40, :70].copy(), (40, 70), 3)], table, False)   # 320 / 39 > 8
    assert _image_prep_cpu.axis_ksize(320, 39) > _C.IMAGE_PREP_MAX_KSIZE
    buf = beyond.buffer.cuda()
    out = torch.full((2, 3, 40, 70), 7.0, device="cuda")
    rc = lib.detops_image_batch_u8(ptr(buf), buf.numel(), ptr(buf), ptr(buf[16:]), ptr(beyond.geom), 2, ptr(buf[56:]), 0, 40, 70,
                                   0, ptr(out), stream_of(buf))
    assert rc == -1                                                            # DETOPS_EINVAL ...
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                  # ... with nothing launched
    got = beyond.to("cuda").tensors                                            # the wrapper takes the host path
    assert got.is_cuda and np.array_equal(C.bits(got), C.bits(beyond.to("cpu").tensors))


def test_empty_batch_is_a_no_op():
    z = lambda dt: torch.zeros(0, dtype=dt, device="cuda")  # noqa: E731
    out = _C.image_batch(z(torch.uint8), z(torch.int64), z(torch.int32).reshape(0, 5), C.identity_table().cuda(), False, 32, 32)
    assert tuple(out.shape) == (0, 3, 32, 32)
    from maskrcnn_benchmark.data.collate_batch import RawImageBatch

    assert tuple(RawImageBatch.pack([], C.identity_table(), False, 32).to("cuda").tensors.shape) == (0, 3, 0, 0)
