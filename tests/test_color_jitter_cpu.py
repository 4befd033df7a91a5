"""Colour jitter without a GPU: the numpy implementation of detops_color_jitter_u8's definition (_color_jitter_cpu.py)
against tests/golden/color_jitter_reference.npz (Pillow's own outputs) and against live Pillow where it is installed, the
draws of RawColorJitter, the deferred pipeline and loader, the buffer layout and the wrapper's refusals.  No tolerance:
every pixel comparison is of bytes."""
import json
import random

import numpy as np
import pytest
import torch

import color_jitter_cases as K
import image_prep_cases as P
from maskrcnn_benchmark import _C
from maskrcnn_benchmark import _color_jitter_cpu as J
from maskrcnn_benchmark.data import transforms as T

B, C, S, H = K.B, K.C, K.S, K.H


# ---------------------------------------------------------------------------------------------- pixels
def test_numpy_equals_pillow_fixture():
    cases = K.fixture_cases()
    assert len(cases) == 56
    for src, rec, want in cases:
        got = J.jitter_image(src, rec)
        assert got.dtype == np.uint8 and np.array_equal(got, want), rec.tolist()
    orders = {tuple(rec[:4].tolist()) for _, rec, _ in cases if rec[3] != 0}
    assert len(orders) == 24                                       # every order of the four operations


def test_wrapper_on_cpu_tensors_equals_fixture_and_keeps_other_bytes():
    cases = K.fixture_cases()
    b = K.batch([src for src, _, _ in cases], [rec for _, rec, _ in cases])
    N = len(cases)
    buf = b.buffer.clone()
    offsets, geom, jitter = K.views(buf, N)
    assert _C.color_jitter(buf, offsets, geom, jitter) is buf
    for off, (src, _, want) in zip(offsets.tolist(), cases):
        assert np.array_equal(buf[off:off + want.size].numpy().reshape(want.shape), want)
    head, end = int(offsets[0]), int(offsets[-1]) + cases[-1][0].size
    assert torch.equal(buf[:head], b.buffer[:head]) and torch.equal(buf[end:], b.buffer[end:])


def _pil_steps(Image, rgb, steps):
    from PIL import ImageEnhance

    enhancer = {B: ImageEnhance.Brightness, C: ImageEnhance.Contrast, S: ImageEnhance.Color}
    img = Image.fromarray(np.ascontiguousarray(rgb), "RGB")
    for code, par in steps:
        if code == H:
            h, s, v = img.convert("HSV").split()
            h = Image.fromarray((np.asarray(h).astype(np.int64) + par).astype(np.uint8), "L")
            img = Image.merge("HSV", (h, s, v)).convert("RGB")
        else:
            img = enhancer[code](img).enhance(par)
    return img


@pytest.mark.parametrize("steps", [[(B, 0.3)], [(B, 1.7)], [(C, 0.3)], [(C, 1.7)], [(S, 0.3)], [(S, 1.7)], [(H, 37)], [(H, 200)],
                                   K.FOUR_STEPS, [(H, 129), (B, 0.8), (S, 0.4), (C, 1.5)]],
                         ids=lambda s: "-".join("%d:%g" % cp for cp in s))
def test_numpy_equals_live_pillow_on_the_colour_sample(steps):
    Image = pytest.importorskip("PIL.Image")
    sample = K.colour_sample()
    assert sample.shape == (1024, 1024, 3)
    flat = sample.reshape(-1, 3)
    assert (flat[:, 0] == flat[:, 1]).any() and ((flat[:, 0] == flat[:, 1]) & (flat[:, 1] == flat[:, 2])).sum() == 16
    want = np.asarray(_pil_steps(Image, sample, steps))
    assert np.array_equal(J.jitter_image(sample, K.record(steps)), want)


def _grey(levels):
    """a one-row image whose pixels have L = levels (greys: L(v, v, v) = v)"""
    return np.repeat(np.asarray(levels, dtype=np.uint8)[None, :, None], 3, axis=2)


def test_contrast_mean_rounds_half_up_and_sees_the_steps_before_it():
    assert J.luma(_grey([0, 1, 255])).tolist() == [[0, 1, 255]]
    assert J.contrast_mean(_grey([0, 1])) == 1                     # mean 0.5: int(0.5 + 0.5)
    assert J.contrast_mean(_grey([0, 0, 1])) == 0                  # mean 1/3
    zero = K.record([(C, 0.0)])                                    # factor 0: every byte becomes m
    assert J.jitter_image(_grey([0, 1]), zero).tolist() == [[[1] * 3, [1] * 3]]
    assert J.jitter_image(_grey([0, 0, 1]), zero).tolist() == [[[0] * 3] * 3]
    bright = _grey([200, 250])
    assert (J.jitter_image(bright, zero) == 225).all()
    assert (J.jitter_image(bright, K.record([(B, 0.0), (C, 0.0)])) == 0).all()      # contrast after brightness 0: m = 0
    assert (J.jitter_image(bright, K.record([(C, 0.0), (B, 0.0)])) == 0).all()


# ---------------------------------------------------------------------------------------------- draws
def _raw(h=6, w=8):
    return T.RawImage(np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3))


def test_draws_one_uniform_per_operation_then_one_shuffle():
    spans = {B: (0.6, 1.4), C: (0.7, 1.3), S: (0.8, 1.2), H: (-0.1, 0.1)}
    for enabled in ([B, C, S, H], [C, H], [S], [B, S, H]):
        t = T.RawColorJitter(*(0.4 if B in enabled else 0, 0.3 if C in enabled else 0, 0.2 if S in enabled else 0,
                               0.1 if H in enabled else 0))
        for seed in range(6):
            random.seed(seed)
            image = t(_raw())
            after = random.random()
            random.seed(seed)
            want = []
            for code in enabled:
                f = random.uniform(*spans[code])
                assert spans[code][0] <= f <= spans[code][1]
                want.append((code, int(f * 255) % 256 if code == H else f))
            random.shuffle(want)
            assert random.random() == after                       # the generator is in the same state: no other draw
            assert list(image.jitter) == want
            for code, par in image.jitter:
                assert (isinstance(par, int) and 0 <= par <= 255) if code == H else spans[code][0] <= par <= spans[code][1]


def test_parameter_rules():
    t = T.RawColorJitter(brightness=1.5, contrast=(0.2, 0.9), saturation=0, hue=(-0.5, 0.25))
    assert t.brightness == (0.0, 2.5) and t.contrast == (0.2, 0.9) and t.saturation is None and t.hue == (-0.5, 0.25)
    assert T.RawColorJitter(0, 0.0, None, 0).hue is None and T.RawColorJitter((1, 1), 0, 0, (0, 0)).brightness is None
    for bad in (dict(brightness=-0.1), dict(hue=0.6), dict(hue=(-0.6, 0.1)), dict(contrast=(0.9, 0.2)), dict(saturation=(-1, 1))):
        with pytest.raises(ValueError):
            T.RawColorJitter(**bad)
    # k = int(f * 255) mod 256, truncated toward zero: a negative factor wraps like the uint8 add
    shift = T.RawColorJitter.hue_shift
    assert [shift(f) for f in (0.0, 0.1, 0.5, -0.1, -0.5, -0.001, 0.004)] == [0, 25, 127, 231, 129, 0, 1]


def test_zero_values_draw_nothing_and_leave_every_seeded_sequence_alone():
    random.seed(5)
    state = random.getstate()
    image = T.RawColorJitter(0, 0, 0, 0)(_raw())
    assert random.getstate() == state and image.jitter == ()
    assert T.RawImage(np.zeros((2, 2, 3), np.uint8)).jitter == ()  # the attribute's default


def _cfg(opts=()):
    from maskrcnn_benchmark.engine.bench_step import load_cfg

    return load_cfg("e2e_mask_rcnn_R_50_FPN_1x.yaml", ["MODEL.DEVICE", "cpu", "INPUT.MIN_SIZE_TRAIN", (64, 72, 80),
                                                        "INPUT.MAX_SIZE_TRAIN", 112, "INPUT.VERTICAL_FLIP_PROB_TRAIN", 0.5]
                    + list(opts))


def _box(w, h):
    from maskrcnn_benchmark.structures.bounding_box import BoxList

    return BoxList(torch.tensor([[1.0, 1.0, 3.0, 3.0]]), (w, h))


JITTER = ["INPUT.BRIGHTNESS", 0.4, "INPUT.CONTRAST", 0.3, "INPUT.SATURATION", 0.2, "INPUT.HUE", 0.1]


def test_resize_and_flip_draws_follow_the_jitter_draws_unchanged():
    """after the jitter's own draws the pipeline draws what the pipeline without jitter draws from that state"""
    Image = pytest.importorskip("PIL.Image")
    src = Image.fromarray(np.random.RandomState(3).randint(0, 256, (40, 56, 3)).astype(np.uint8), "RGB")
    plain = T.build_transforms(_cfg(), True, device_prep=True)
    jittered = T.build_transforms(_cfg(JITTER), True, device_prep=True)
    seen = set()
    for seed in range(10):
        random.seed(seed)
        a, ta = jittered(src, _box(56, 40))
        after = random.random()
        random.seed(seed)
        for lo, hi in ((0.6, 1.4), (0.7, 1.3), (0.8, 1.2), (-0.1, 0.1)):
            random.uniform(lo, hi)
        random.shuffle([0, 1, 2, 3])
        b, tb = plain(src, _box(56, 40))
        assert random.random() == after
        assert (a.size, a.flip) == (b.size, b.flip) and torch.equal(ta.bbox, tb.bbox) and b.jitter == ()
        assert len(a.jitter) == 4 and np.array_equal(a.data, b.data)   # the source bytes wait, untouched
        seen.add((a.size, a.flip))
    assert len(seen) > 3


# ---------------------------------------------------------------------------------------------- pipeline and loader
def test_build_transforms_serves_jitter_on_the_deferred_path_only():
    Image = pytest.importorskip("PIL.Image")
    cfg = _cfg(["INPUT.BRIGHTNESS", 0.1])
    pipeline = T.build_transforms(cfg, True, device_prep=True)
    assert [type(t).__name__ for t in pipeline.transforms] == ["ToRaw", "RawColorJitter", "Resize", "RandomHorizontalFlip",
                                                              "RandomVerticalFlip"]
    image, _ = pipeline(Image.fromarray(np.full((40, 56, 3), 90, np.uint8), "RGB"), _box(56, 40))
    assert len(image.jitter) == 1 and image.jitter[0][0] == B and 0.9 <= image.jitter[0][1] <= 1.1
    with pytest.raises(NotImplementedError, match="BRIGHTNESS / CONTRAST / SATURATION / HUE"):
        T.build_transforms(cfg, True, device_prep=False)
    test_time = T.build_transforms(cfg, False, device_prep=True)   # test pipelines never jitter
    assert "RawColorJitter" not in [type(t).__name__ for t in test_time.transforms]
    assert [type(t).__name__ for t in T.build_transforms(_cfg(), True, device_prep=True).transforms][:2] == ["ColorJitter", "ToRaw"]


def test_jitter_forces_the_deferred_path(monkeypatch):
    from maskrcnn_benchmark.data import build as data_build
    from maskrcnn_benchmark.data import collate_batch

    for mode in ("auto", "host", "device"):
        monkeypatch.setattr(collate_batch, "INPUT_PREP", mode)
        assert data_build.deferred_prep(_cfg(["INPUT.HUE", 0.05]), True)
        assert data_build.deferred_prep(_cfg(["INPUT.HUE", 0.05]), False) == (mode == "device")
        assert data_build.deferred_prep(_cfg(), True) == (mode == "device")
    monkeypatch.setattr(collate_batch, "INPUT_PREP", "auto")
    assert isinstance(data_build.make_collator(_cfg(JITTER), True), collate_batch.RawBatchCollator)


SIZES = {1: (64, 48), 2: (40, 56), 3: (48, 48), 4: (72, 40)}     # id -> (w, h)


@pytest.fixture()
def tiny_coco(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog

    rng = np.random.RandomState(17)
    images, ann = [], []
    for i, (w, h) in SIZES.items():
        name = "img%d.png" % i
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), "RGB").save(str(tmp_path / name))
        images.append({"id": i, "file_name": name, "width": w, "height": h})
        x, y, bw, bh = 4.0, 5.0, 20.0, 18.0
        ann.append({"id": i, "image_id": i, "category_id": 1, "bbox": [x, y, bw, bh], "area": bw * bh, "iscrowd": 0,
                    "segmentation": [[x, y, x + bw, y, x + bw, y + bh, x, y + bh]]})
    path = tmp_path / "instances.json"
    path.write_text(json.dumps({"images": images, "annotations": ann, "categories": [{"id": 1, "name": "a"}]}))
    DatasetCatalog.register("tiny_jitter_train", str(path), str(tmp_path))
    yield "tiny_jitter_train", str(tmp_path)
    DatasetCatalog.REGISTERED.pop("tiny_jitter_train", None)


class _PillowPipeline(object):
    """the reference's training Compose written out by hand on PIL images: ColorJitter (draws as documented, Pillow's
    enhancers), Resize, flips, ToTensor, Normalize"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.rest = T.Compose([T.Resize(cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN),
                               T.RandomHorizontalFlip(cfg.INPUT.HORIZONTAL_FLIP_PROB_TRAIN),
                               T.RandomVerticalFlip(cfg.INPUT.VERTICAL_FLIP_PROB_TRAIN), T.ToTensor(),
                               T.Normalize(cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255)])

    def __call__(self, image, target):
        from PIL import Image

        c = self.cfg.INPUT
        steps = [(B, random.uniform(max(0.0, 1 - c.BRIGHTNESS), 1 + c.BRIGHTNESS)),
                 (C, random.uniform(max(0.0, 1 - c.CONTRAST), 1 + c.CONTRAST)),
                 (S, random.uniform(max(0.0, 1 - c.SATURATION), 1 + c.SATURATION)),
                 (H, int(random.uniform(-c.HUE, c.HUE) * 255) % 256)]
        random.shuffle(steps)
        return self.rest(_pil_steps(Image, np.asarray(image.convert("RGB")), steps), target)


def test_loader_on_cpu_equals_a_hand_composed_pillow_pipeline(tiny_coco, monkeypatch):
    from maskrcnn_benchmark.data import collate_batch, make_data_loader
    from maskrcnn_benchmark.data.collate_batch import BatchCollator

    name, _ = tiny_coco
    monkeypatch.setattr(collate_batch, "INPUT_PREP", "auto")        # MODEL.DEVICE cpu: only the jitter defers the pixels
    cfg = _cfg(JITTER + ["DATASETS.TRAIN", (name,), "SOLVER.IMS_PER_BATCH", 2, "SOLVER.MAX_ITER", 3,
                         "DATALOADER.NUM_WORKERS", 0, "DATALOADER.SIZE_DIVISIBILITY", 32])
    random.seed(77)
    torch.manual_seed(5)
    loader = make_data_loader(cfg, is_train=True)
    assert isinstance(loader.collate_fn, collate_batch.RawBatchCollator)
    got = [(images, images.to("cpu"), ids) for images, _, ids in loader]
    assert len(got) == 3 and all(raw.jitter is not None and int((raw.jitter[:, :4] != 0).sum()) == 8 for raw, _, _ in got)

    random.seed(77)
    torch.manual_seed(5)
    hand = make_data_loader(cfg, is_train=True)
    hand.dataset._transforms = _PillowPipeline(cfg)
    hand.collate_fn = BatchCollator(32)
    want = [(images, ids) for images, _, ids in hand]              # the same sampler draws, the same item order
    assert len(want) == 3
    for (_, g, gids), (w, wids) in zip(got, want):
        assert list(gids) == list(wids) and g.image_sizes == [tuple(s) for s in w.image_sizes]
        assert np.array_equal(P.bits(g.tensors), P.bits(w.tensors))
    plain = _cfg(["DATASETS.TRAIN", (name,), "SOLVER.IMS_PER_BATCH", 2, "SOLVER.MAX_ITER", 1, "DATALOADER.NUM_WORKERS", 0])
    assert isinstance(make_data_loader(plain, is_train=True).collate_fn, BatchCollator)   # the host path, as before


# ---------------------------------------------------------------------------------------------- buffer layout
def _images(rng, shapes):
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]


def test_buffer_without_jitter_is_the_present_layout_byte_for_byte():
    from maskrcnn_benchmark.data.collate_batch import RawImageBatch

    images = _images(np.random.RandomState(0), [(5, 7), (3, 3), (8, 2)])
    table = T.normalisation_table([102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0], True)
    b = RawImageBatch.pack([T.RawImage(im, (9, 11), 1) for im in images], table, True)
    N, head = 3, (3 * 28 + 3072 + 15) // 16 * 16
    want = np.zeros(head + sum(im.size for im in images), dtype=np.uint8)
    offsets = np.cumsum([head] + [im.size for im in images[:-1]]).astype(np.int64)
    want[:N * 8] = offsets.view(np.uint8)
    want[N * 8:N * 28] = np.array([[im.shape[0], im.shape[1], 11, 9, 1] for im in images], np.int32).reshape(-1).view(np.uint8)
    want[N * 28:N * 28 + 3072] = table.numpy().reshape(-1).view(np.uint8)
    want[head:] = np.concatenate([im.reshape(-1) for im in images])
    assert b.jitter is None and np.array_equal(b.buffer.numpy(), want)
    assert b.on("cpu") is b                                         # nothing to apply: the batch itself

    steps = [(H, 37), (B, 1.3)]
    j = RawImageBatch.pack([T.RawImage(images[0], (9, 11), 1), T.RawImage(images[1], (9, 11), 1, steps),
                            T.RawImage(images[2], (9, 11), 1)], table, True)
    block = (want.size + 15) // 16 * 16
    assert j.buffer.numel() == block + N * 32 and np.array_equal(j.buffer.numpy()[:want.size], want)   # only bytes beyond
    assert not j.buffer.numpy()[want.size:block].any()
    assert np.array_equal(j.buffer.numpy()[block:].view(np.int32).reshape(N, 8), j.jitter.numpy())
    assert j.jitter.tolist() == [[0] * 8, [H, B, 0, 0, 37, J.factor_bits(1.3), 0, 0], [0] * 8]
    with pytest.raises(ValueError, match="at most 4"):             # a fifth step does not spill into the parameters
        RawImageBatch.pack([T.RawImage(images[0], jitter=[(B, 1.1), (C, 1.1), (S, 1.1), (H, 3), (B, 0.9)])], table, True)
    with pytest.raises(ValueError, match="twice"):
        RawImageBatch.pack([T.RawImage(images[0], jitter=[(B, 1.1), (B, 0.9)])], table, True)


def test_to_cpu_applies_the_jitter_once_on_a_copy():
    images = _images(np.random.RandomState(1), [(5, 7), (1, 1), (8, 9)])
    records = [K.record(K.FOUR_STEPS), K.record([]), K.record([(C, 1.5)])]
    b = K.batch(images, records)
    before = b.buffer.clone()
    first, second = b.to("cpu"), b.to("cpu")
    assert torch.equal(b.buffer, before)                            # the loader's buffer is never changed
    assert torch.equal(first.tensors, second.tensors)
    for i, (im, rec) in enumerate(zip(images, records)):
        want = J.jitter_image(im, rec).transpose(2, 0, 1).astype(np.float32)
        assert np.array_equal(first.tensors[i, :, :im.shape[0], :im.shape[1]].numpy(), want)
    assert not np.array_equal(J.jitter_image(images[0], records[0]), images[0])
    on = b.on("cpu")
    assert on is not b and on.jitter is None and torch.equal(b.buffer, before)
    h, w = images[2].shape[:2]
    one, two = on.prepare(h, 100), on.prepare(h, 100)               # `prepare` after `on` does not jitter again
    assert torch.equal(one.tensors, two.tensors)
    assert np.array_equal(one.tensors[2, :, :h, :w].numpy(), J.jitter_image(images[2], records[2]).transpose(2, 0, 1))


# ---------------------------------------------------------------------------------------------- refusals
def test_wrapper_rejects_malformed_arguments():
    images = _images(np.random.RandomState(2), [(4, 5), (3, 3)])
    b = K.batch(images, [K.record([(B, 1.2)]), K.record([(H, 9)])])
    buf = b.buffer.clone()
    offsets, geom, jitter = K.views(buf, 2)

    def refused(jit=jitter, raw=buf, off=offsets, g=geom, match="color_jitter"):
        with pytest.raises(ValueError, match=match):
            _C.color_jitter(raw, off, g, jit)
        assert torch.equal(buf, b.buffer)

    def with_record(rec):
        j = jitter.clone()
        j[0] = torch.tensor(rec, dtype=torch.int32)
        return j

    one = J.factor_bits(1.0)
    refused(with_record([B, B, 0, 0, one, one, 0, 0]), match="twice")
    refused(with_record([5, 0, 0, 0, one, 0, 0, 0]), match="unknown step code")
    refused(with_record([-1, 0, 0, 0, one, 0, 0, 0]), match="unknown step code")
    refused(with_record([0, B, 0, 0, 0, one, 0, 0]), match="after the end")
    refused(with_record([H, 0, 0, 0, 256, 0, 0, 0]), match="outside 0 .. 255")
    refused(with_record([H, 0, 0, 0, -1, 0, 0, 0]), match="outside 0 .. 255")
    refused(with_record([S, 0, 0, 0, J.factor_bits(float("inf")), 0, 0, 0]), match="non-finite")
    refused(with_record([C, 0, 0, 0, J.factor_bits(float("nan")), 0, 0, 0]), match="non-finite")
    refused(jitter.to(torch.int64), match="expected raw")          # dtypes
    refused(raw=buf.to(torch.int16), match="expected raw")
    refused(off=offsets.to(torch.int32), match="expected raw")
    refused(g=geom.to(torch.int64), match="expected raw")
    refused(jitter[:, :7], match="expected raw")                   # shapes
    refused(jitter[:1], match="expected raw")
    refused(jitter.reshape(-1), match="expected raw")
    refused(g=geom[:, :4], match="expected raw")
    refused(raw=buf.unsqueeze(0), match="expected raw")
    far = offsets.clone()
    far[1] = buf.numel() - 3
    refused(off=far, match="outside the buffer")
    assert _C.color_jitter(buf, offsets, geom, jitter) is buf and not torch.equal(buf, b.buffer)
