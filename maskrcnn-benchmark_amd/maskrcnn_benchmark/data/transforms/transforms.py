"""Image / target transforms (reference data/transforms/transforms.py: the class names, argument names and order are the
reference's).  The reference goes through torchvision; its `F.resize` of a PIL image is `img.resize((ow, oh),
Image.BILINEAR)`, `F.hflip` / `F.vflip` are `img.transpose`, `F.to_tensor` is float32(u8) / 255 and `F.normalize` is
(t - mean) / std in fp32.  Those are written out here, so Pillow is the only dependency.

Every geometric transform also accepts a RawImage: the raw uint8 pixels plus the destination size and the flip bits the
transform would have applied.  It makes the same random draws in the same order and transforms the target alike, but the
pixels wait for the device (csrc/image_prep.hip through data/collate_batch.py: RawImageBatch)."""
import random

import numpy as np
import torch

FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM = 0, 1      # BoxList.transpose / PIL.Image.transpose


class RawImage(object):
    """An image whose resize and flips are deferred: data [h, w, 3] uint8 (RGB), size (ow, oh) = what the PIL image's
    `.size` would be by now, flip bits (1 horizontal, 2 vertical), jitter = the colour steps that run on the source bytes
    first, in order: (code, parameter) pairs (RawColorJitter), empty for none."""

    def __init__(self, data, size=None, flip=0, jitter=()):
        self.data = data
        self.size = (data.shape[1], data.shape[0]) if size is None else size
        self.flip = flip
        self.jitter = tuple(jitter)


class Compose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, image, target):
        for t in self.transforms:
            image, target = t(image, target)
        return image, target

    def __repr__(self):
        return self.__class__.__name__ + "(" + "".join("\n    {0}".format(t) for t in self.transforms) + "\n)"


class ToRaw(object):
    """PIL image -> RawImage (first in a deferred pipeline)"""

    def __call__(self, image, target=None):
        image = RawImage(np.array(image.convert("RGB"), dtype=np.uint8))
        return image if target is None else (image, target)


class Resize(object):
    def __init__(self, min_size, max_size):
        if not isinstance(min_size, (list, tuple)):
            min_size = (min_size,)
        self.min_size = min_size
        self.max_size = max_size

    def get_size(self, image_size):
        """(w, h) -> (oh, ow): the shorter side to a size drawn from min_size, the longer one by truncation, the size
        lowered first where the longer side would pass max_size"""
        w, h = image_size
        size = random.choice(self.min_size)
        if self.max_size is not None:
            lo, hi = float(min(w, h)), float(max(w, h))
            if hi / lo * size > self.max_size:
                size = int(round(self.max_size * lo / hi))
        if (w <= h and w == size) or (h <= w and h == size):
            return (h, w)
        if w < h:
            return (int(size * h / w), size)
        return (size, int(size * w / h))

    def __call__(self, image, target=None):
        oh, ow = self.get_size(image.size)
        if isinstance(image, RawImage):
            image = RawImage(image.data, (ow, oh), image.flip, image.jitter)
        else:
            from PIL import Image

            image = image.resize((ow, oh), Image.BILINEAR)
        if target is None:
            return image
        return image, target.resize(image.size)


class _RandomFlip(object):
    bit, method = None, None

    def __init__(self, prob=0.5):
        self.prob = prob

    def __call__(self, image, target):
        if random.random() < self.prob:
            if isinstance(image, RawImage):
                image = RawImage(image.data, image.size, image.flip ^ self.bit, image.jitter)
            else:
                image = image.transpose(self.method)       # PIL's FLIP_LEFT_RIGHT = 0, FLIP_TOP_BOTTOM = 1
            target = target.transpose(self.method)
        return image, target


class RandomHorizontalFlip(_RandomFlip):
    bit, method = 1, FLIP_LEFT_RIGHT


class RandomVerticalFlip(_RandomFlip):
    bit, method = 2, FLIP_TOP_BOTTOM


class ColorJitter(object):
    """The reference hands these to torchvision.transforms.ColorJitter, which defines them; torchvision is not a
    dependency here, so only the identity (all zero / None) is accepted."""

    def __init__(self, brightness=None, contrast=None, saturation=None, hue=None):
        if any(v not in (None, 0, 0.0) for v in (brightness, contrast, saturation, hue)):
            raise NotImplementedError("ColorJitter with non-zero BRIGHTNESS / CONTRAST / SATURATION / HUE needs torchvision's "
                                      "definition, which is not built for the host pipeline (the deferred input path serves it: "
                                      "RawColorJitter, build_transforms(cfg, is_train, device_prep=True))")

    def __call__(self, image, target):
        return image, target


class RawColorJitter(object):
    """ColorJitter of the deferred pipeline: draws the parameters and leaves the steps on the RawImage; the pixels are
    jittered where the batch lands (include/detops.h: detops_color_jitter_u8, Pillow's arithmetic byte for byte).
    torchvision's rules: a number v >= 0 for brightness / contrast / saturation is a factor uniform in [max(0, 1 - v),
    1 + v], hue 0 <= v <= 0.5 is uniform in [-v, v], a (lo, hi) pair is taken as given; a range that is the identity
    disables the operation, which then makes no draw.  Draws from `random`: one uniform per enabled operation in the order
    brightness, contrast, saturation, hue, then one shuffle of the enabled operations.  That order is this library's
    definition (torchvision's get_params as recalled; not checked against torchvision)."""
    BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 3, 4           # the step codes of the jitter record

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = self._range(brightness, "brightness")
        self.contrast = self._range(contrast, "contrast")
        self.saturation = self._range(saturation, "saturation")
        self.hue = self._range(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    @staticmethod
    def _range(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
        if value is None:
            return None
        if isinstance(value, (int, float)):
            if value < 0:
                raise ValueError("%s must be non-negative, got %r" % (name, value))
            lo, hi = center - float(value), center + float(value)
            if clip_first_on_zero:
                lo = max(lo, 0.0)
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            lo, hi = float(value[0]), float(value[1])
        else:
            raise TypeError("%s is a number or a (lo, hi) pair, got %r" % (name, value))
        if not bound[0] <= lo <= hi <= bound[1]:
            raise ValueError("%s values must lie in %r, got %r" % (name, bound, value))
        return None if lo == hi == center else (lo, hi)

    @staticmethod
    def hue_shift(factor):
        """the byte added to the H plane: int(f * 255) mod 256 (the uint8 add wraps), fp64, truncated toward zero"""
        return int(factor * 255) % 256

    def __call__(self, image, target=None):
        steps = []
        for code, span in ((self.BRIGHTNESS, self.brightness), (self.CONTRAST, self.contrast),
                           (self.SATURATION, self.saturation), (self.HUE, self.hue)):
            if span is not None:
                f = random.uniform(span[0], span[1])
                steps.append((code, self.hue_shift(f) if code == self.HUE else f))
        if steps:
            random.shuffle(steps)
        image = RawImage(image.data, image.size, image.flip, steps)
        return image if target is None else (image, target)


class ToTensor(object):
    def __call__(self, image, target):
        t = torch.from_numpy(np.array(image.convert("RGB"), dtype=np.uint8)).permute(2, 0, 1).contiguous()
        return t.to(torch.float32) / 255, target


class Normalize(object):
    def __init__(self, mean, std, to_bgr255=True):
        self.mean = mean
        self.std = std
        self.to_bgr255 = to_bgr255

    def __call__(self, image, target=None):
        if self.to_bgr255:
            image = image[[2, 1, 0]] * 255
        mean = torch.as_tensor(self.mean, dtype=torch.float32)
        std = torch.as_tensor(self.std, dtype=torch.float32)
        image = (image - mean[:, None, None]) / std[:, None, None]
        return image if target is None else (image, target)


def normalisation_table(mean, std, to_bgr255=True):
    """[3, 256] float32: row c = ToTensor and Normalize applied to the 256 bytes as the pixels of OUTPUT channel c (which
    reads source channel 2 - c under to_bgr255).  The same expressions on the same values: the same bits."""
    t = torch.arange(256, dtype=torch.uint8)[None, :, None].expand(3, 256, 1).contiguous()
    t = t.to(torch.float32) / 255
    if to_bgr255:
        t = t * 255                                        # the channel swap moves values, it does not change them
    mean = torch.as_tensor(mean, dtype=torch.float32)
    std = torch.as_tensor(std, dtype=torch.float32)
    return ((t - mean[:, None, None]) / std[:, None, None]).reshape(3, 256).contiguous()
