"""detops_color_jitter_u8 on the device against tests/golden/color_jitter_reference.npz (Pillow's own outputs) and the
numpy implementation of the same definition.  Never imports PIL.  No tolerance anywhere: every comparison is of bytes."""
import numpy as np
import pytest
import torch

import color_jitter_cases as K
import image_prep_cases as P
from maskrcnn_benchmark import _C
from maskrcnn_benchmark import _color_jitter_cpu as J

pytestmark = pytest.mark.gpu

B, C, S, H = K.B, K.C, K.S, K.H
GUARD = 256                                    # bytes after the buffer that must stay as they were


def _on_device(b):
    """the batch's buffer on the device with GUARD bytes of 0xA5 behind it -> (whole, buf = whole[:n])"""
    n = b.buffer.numel()
    whole = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    whole[:n].copy_(b.buffer)
    return whole, whole[:n]


def _jitter(b):
    """-> the buffer and the guard bytes after one color_jitter on the device, on the host"""
    whole, buf = _on_device(b)
    offsets, geom, jitter = K.views(buf, len(b))
    assert _C.color_jitter(buf, offsets, geom, jitter, geom_host=b.geom, jitter_host=b.jitter) is buf
    out = whole.cpu().numpy()
    assert (out[buf.numel():] == 0xA5).all()
    return out[:buf.numel()]


def test_every_fixture_case_on_the_device():
    cases = K.fixture_cases()
    b = K.batch([src for src, _, _ in cases], [rec for _, rec, _ in cases])
    got = _jitter(b)
    for off, (src, rec, want) in zip(K.views(b.buffer, len(b))[0].tolist(), cases):
        assert np.array_equal(got[off:off + want.size].reshape(want.shape), want), rec.tolist()     # Pillow's bytes
    assert np.array_equal(got, K.expected_buffer(b))               # the numpy path, and every byte outside the images


def test_unaligned_bases_heads_tails_and_untouched_bytes():
    rng = np.random.RandomState(7)
    shapes = [(1, w) for w in range(1, 17)] + [(1, 1), (5, 3), (37, 53), (8, 16), (2, 2), (3, 11)]    # 8 x 16: 384 bytes
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    menu = [K.FOUR_STEPS, [], [(H, 200)], [(C, 1.4)], [(B, 0.5), (C, 0.6)], [(S, 0.0)], []]
    records = [K.record(menu[i % len(menu)]) for i in range(len(images))]
    records[18], records[19] = K.record(K.FOUR_STEPS), K.record([(H, 1), (C, 1.9), (S, 1.7)])
    b = K.batch(images, records)
    offsets = K.views(b.buffer, len(b))[0].numpy()
    assert {int(o) % 16 for o in offsets[:16]} == set(range(16))   # image bases on every residue of 16
    assert sum(1 for r in records if r[0] == 0) >= 5
    got, want = _jitter(b), K.expected_buffer(b)
    assert np.array_equal(got, want)
    before = b.buffer.numpy()
    for off, im, rec in zip(offsets.tolist(), images, records):
        if rec[0] == 0:
            assert np.array_equal(got[off:off + im.size], before[off:off + im.size])               # no steps: untouched
    end = int(offsets[-1]) + images[-1].size
    assert np.array_equal(got[:offsets[0]], before[:offsets[0]]) and np.array_equal(got[end:], before[end:])
    assert not np.array_equal(got, before)


def test_colour_sample_through_hue_saturation_and_four_steps():
    sample = K.colour_sample()
    b = K.batch([sample] * 3, [K.record([(H, 37)]), K.record([(S, 1.6)]), K.record(K.FOUR_STEPS)])
    assert np.array_equal(_jitter(b), K.expected_buffer(b))


@pytest.mark.parametrize("side", [4104, 4105])
def test_sum_of_a_large_image_is_kept_in_64_bits(side):
    """An all-255 square under contrast 0: every byte is m = 255, no reference needed.  4105 is the smallest square whose
    sum 255 * side^2 passes 2^32 (2^32 / 255 = 16 843 009 pixels = 4104.02^2; a sum kept in 32 bits gives m = 0 there);
    4104, 49 216 short of it, is the largest that does not."""
    assert 255 * 4104 ** 2 < 2 ** 32 < 255 * 4105 ** 2
    b = K.batch([np.full((side, side, 3), 255, dtype=np.uint8)], [K.record([(C, 0.0)])])
    buf = b.buffer.cuda()
    offsets, geom, jitter = K.views(buf, 1)
    _C.color_jitter(buf, offsets, geom, jitter, geom_host=b.geom, jitter_host=b.jitter)
    off = int(b.buffer[:8].view(torch.int64)[0])
    assert bool((buf[off:off + 3 * side * side] == 255).all())


def test_contrast_first_in_the_middle_and_last():
    src = K.fixture()["image_1"]
    first = [(C, 0.7), (S, 1.6), (H, 37), (B, 1.3)]
    middle = [(B, 0.6), (C, 0.7), (H, 37), (S, 1.6)]
    last = [(S, 1.6), (H, 37), (B, 1.3), (C, 0.7)]
    b = K.batch([src] * 3, [K.record(first), K.record(middle), K.record(last)])
    means = [J.contrast_mean(J.jitter_image(src, K.record(steps[:[c for c, _ in steps].index(C)])))
             for steps in (first, middle, last)]
    assert len(set(means)) == 3                                    # the sum depends on the steps in front of contrast
    assert np.array_equal(_jitter(b), K.expected_buffer(b))


def test_two_runs_give_identical_bytes():
    rng = np.random.RandomState(9)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((61, 67), (40, 30), (7, 129))]
    b = K.batch(images, [K.record(K.FOUR_STEPS), K.record([(C, 1.5)]), K.record([(H, 77), (C, 0.2)])])
    assert np.array_equal(_jitter(b), _jitter(b))


@pytest.mark.parametrize("channels_last", [False, True])
def test_jittered_batch_end_to_end(channels_last):
    from maskrcnn_benchmark.data.collate_batch import RawImageBatch
    from maskrcnn_benchmark.data.transforms import RawImage, normalisation_table

    cases = P.cases()
    table = normalisation_table([102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0], True)
    picks = [(0, 1, K.FOUR_STEPS), (1, 2, []), (2, 0, [(C, 1.3), (H, 250)])]
    images = [RawImage(cases[c][0], cases[c][1].shape[1::-1], flip, steps) for c, flip, steps in picks]
    b = RawImageBatch.pack(images, table, True, 32, channels_last)
    before = b.buffer.clone()
    want = b.to("cpu")
    plain = RawImageBatch.pack([RawImage(im.data, im.size, im.flip) for im in images], table, True, 32, channels_last).to("cpu")
    assert not np.array_equal(P.bits(want.tensors), P.bits(plain.tensors))
    one, two = b.to("cuda"), b.to("cuda")
    assert one.tensors.is_cuda and one.tensors.is_contiguous(memory_format=torch.channels_last) == channels_last
    assert np.array_equal(P.bits(one.tensors), P.bits(want.tensors)) and np.array_equal(P.bits(two.tensors), P.bits(want.tensors))
    assert one.image_sizes == want.image_sizes and torch.equal(b.buffer, before)
    on = b.on("cuda")
    assert on.buffer.is_cuda and on.jitter is None
    first, second = on.prepare(48, 90), on.prepare(48, 90)         # `prepare` after `on` does not jitter again
    host = b.on("cpu").prepare(48, 90)
    assert np.array_equal(P.bits(first.tensors), P.bits(second.tensors))
    assert np.array_equal(P.bits(first.tensors), P.bits(host.tensors))


def test_entry_point_refusals_launch_nothing():
    from maskrcnn_benchmark._lib import lib, ptr, stream_of

    rng = np.random.RandomState(4)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((9, 13), (4, 4))]
    b = K.batch(images, [K.record([(B, 1.2), (C, 0.8)]), K.record([(H, 9)])])
    whole, buf = _on_device(b)
    offsets, geom, jitter = K.views(buf, 2)
    ws = torch.zeros(2, dtype=torch.int64, device="cuda")
    one = J.factor_bits(1.0)

    def call(jitter_host=b.jitter, geom_host=b.geom, raw=buf, off=offsets, g=geom, j=jitter, n=2, w=ws, wbytes=16, size=None):
        rc = lib.detops_color_jitter_u8(ptr(raw), buf.numel() if size is None else size, ptr(off), ptr(g), ptr(geom_host), ptr(j),
                                        ptr(jitter_host), n, ptr(w), wbytes, stream_of(buf))
        torch.cuda.synchronize()
        assert torch.equal(whole[:buf.numel()].cpu(), b.buffer) and bool((whole[buf.numel():] == 0xA5).all())
        return rc

    def with_record(rec):
        j = b.jitter.clone()
        j[0] = torch.tensor(rec, dtype=torch.int32)
        return j

    EINVAL, EWORKSPACE = -1, -2
    assert call(with_record([B, B, 0, 0, one, one, 0, 0])) == EINVAL          # an operation twice
    assert call(with_record([5, 0, 0, 0, one, 0, 0, 0])) == EINVAL            # unknown codes
    assert call(with_record([-1, 0, 0, 0, one, 0, 0, 0])) == EINVAL
    assert call(with_record([0, B, 0, 0, 0, one, 0, 0])) == EINVAL            # a code after the end of the list
    assert call(with_record([H, 0, 0, 0, 256, 0, 0, 0])) == EINVAL            # k outside 0 .. 255
    assert call(with_record([H, 0, 0, 0, -1, 0, 0, 0])) == EINVAL
    assert call(with_record([S, 0, 0, 0, J.factor_bits(float("inf")), 0, 0, 0])) == EINVAL
    assert call(with_record([C, 0, 0, 0, J.factor_bits(float("nan")), 0, 0, 0])) == EINVAL
    small = b.geom.clone()
    small[1, 0] = 0
    assert call(geom_host=small) == EINVAL                                    # a size below 1
    assert call(n=-1) == EINVAL and call(size=-1) == EINVAL
    for null in ("raw", "off", "g", "j", "geom_host", "jitter_host", "w"):
        assert call(**{null: None}) == EINVAL, null
    assert call(wbytes=15) == EWORKSPACE
    assert call(n=0) == 0                                                     # the empty batch
    assert call(jitter_host=torch.zeros(2, 8, dtype=torch.int32)) == 0        # no image with a step
    z = lambda dt: torch.zeros(0, dtype=dt, device="cuda")  # noqa: E731
    empty = z(torch.uint8)
    assert _C.color_jitter(empty, z(torch.int64), z(torch.int32).reshape(0, 5), z(torch.int32).reshape(0, 8)) is empty
    with pytest.raises(ValueError, match="twice"):
        _C.color_jitter(buf, offsets, geom, jitter, jitter_host=with_record([B, B, 0, 0, one, one, 0, 0]))
    assert torch.equal(buf.cpu(), b.buffer)
    assert np.array_equal(_jitter(b), K.expected_buffer(b))                   # and the well-formed call does its work
