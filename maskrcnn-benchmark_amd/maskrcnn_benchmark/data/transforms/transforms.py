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
    `.size` would be by now, flip bits (1 horizontal, 2 vertical)."""

    def __init__(self, data, size=None, flip=0):
        self.data = data
        self.size = (data.shape[1], data.shape[0]) if size is None else size
        self.flip = flip


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
            image = RawImage(image.data, (ow, oh), image.flip)
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
                image = RawImage(image.data, image.size, image.flip ^ self.bit)
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
                                      "definition, which is not built")

    def __call__(self, image, target):
        return image, target


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
