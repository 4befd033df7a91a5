"""Collators (reference data/collate_batch.py) and the deferred batch of the device input path.

BatchCollator pads host-prepared fp32 images into an ImageList.  RawBatchCollator packs the raw uint8 images of a batch,
their records and the normalisation table into ONE uint8 buffer (RawImageBatch); the loader's workers never touch the
GPU.  RawImageBatch.to(device) makes the single host-to-device copy and the single launch of detops_image_batch_u8 and
returns an ordinary ImageList, so the training and inference loops do not know which path fed them."""
import os

import numpy as np
import torch

from maskrcnn_benchmark.structures.image_list import ImageList

from .synthetic import BatchCollator  # noqa: F401  (the host path's collator)

# A/B switch, read once at import: device | host | auto (= device when MODEL.DEVICE is a GPU)
INPUT_PREP = os.environ.get("DETOPS_INPUT_PREP", "auto")
if INPUT_PREP not in ("auto", "device", "host"):
    raise ValueError("DETOPS_INPUT_PREP must be device | host, got %r" % (INPUT_PREP,))


def device_prep(cfg):
    """does this config prepare its batches on the device?"""
    return INPUT_PREP == "device" or (INPUT_PREP == "auto" and cfg.MODEL.DEVICE != "cpu")


class RawImageBatch(object):
    """buffer [bytes] uint8 = offsets int64 [N] | geom int32 [N, 5] | table float32 [3, 256] | padding to 16 | the images'
    RGB HWC bytes back to back.  The offsets count from the start of the buffer."""

    def __init__(self, buffer, geom, bgr, size, channels_last=False):
        self.buffer, self.geom, self.bgr = buffer, geom, bool(bgr)        # geom: the records once more, for the host
        self.size, self.channels_last = size, channels_last              # size: (Hp, Wp)
        self.image_sizes = [(int(g[2]), int(g[3])) for g in geom.tolist()]

    @staticmethod
    def pack(images, table, bgr, size_divisible=0, channels_last=False):
        """images: RawImage records"""
        N = len(images)
        head = (N * 8 + N * 20 + 3 * 256 * 4 + 15) // 16 * 16
        sizes = [im.data.shape[0] * im.data.shape[1] * 3 for im in images]
        offsets = np.cumsum([head] + sizes[:-1]).astype(np.int64) if N else np.zeros(0, np.int64)
        geom = np.array([[im.data.shape[0], im.data.shape[1], im.size[1], im.size[0], im.flip] for im in images],
                        dtype=np.int32).reshape(N, 5)
        buf = np.empty(head + sum(sizes), dtype=np.uint8)
        buf[:N * 8] = offsets.view(np.uint8)
        buf[N * 8:N * 28] = geom.reshape(-1).view(np.uint8)
        buf[N * 28:N * 28 + 3072] = table.numpy().reshape(-1).view(np.uint8)
        buf[N * 28 + 3072:head] = 0
        for o, n, im in zip(offsets, sizes, images):
            buf[o:o + n] = np.ascontiguousarray(im.data, dtype=np.uint8).reshape(-1)
        Hp, Wp = (int(geom[:, 2].max()), int(geom[:, 3].max())) if N else (0, 0)
        if size_divisible > 0:
            d = int(size_divisible)
            Hp, Wp = (Hp + d - 1) // d * d, (Wp + d - 1) // d * d
        return RawImageBatch(torch.from_numpy(buf), torch.from_numpy(geom), bgr, (Hp, Wp), channels_last)

    def pin_memory(self):
        """torch's DataLoader(pin_memory=True) calls this in the main process"""
        self.buffer = self.buffer.pin_memory()
        return self

    def to(self, device, *args, **kwargs):
        from maskrcnn_benchmark import _C

        device = torch.device(device)
        N = self.geom.shape[0]
        buf = self.buffer if device.type == "cpu" else self.buffer.to(device, non_blocking=True)
        offsets = buf[:N * 8].view(torch.int64)
        geom = buf[N * 8:N * 28].view(torch.int32).view(N, 5)
        table = buf[N * 28:N * 28 + 3072].view(torch.float32).view(3, 256)
        out = _C.image_batch(buf, offsets, geom, table, self.bgr, self.size[0], self.size[1],
                             channels_last=self.channels_last and device.type != "cpu", geom_host=self.geom)
        return ImageList(out, self.image_sizes)


class RawBatchCollator(object):
    """[(RawImage, target, id)] -> (RawImageBatch, tuple(targets), tuple(ids))"""

    def __init__(self, size_divisible=0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), to_bgr255=True, channels_last=False):
        from .transforms import normalisation_table

        self.size_divisible, self.bgr, self.channels_last = size_divisible, to_bgr255, channels_last
        self.table = normalisation_table(mean, std, to_bgr255)

    def __call__(self, batch):
        images, targets, ids = zip(*batch)
        return RawImageBatch.pack(images, self.table, self.bgr, self.size_divisible, self.channels_last), targets, ids
