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
    RGB HWC bytes back to back.  The offsets count from the start of the buffer.  A batch with colour jitter (some image
    carries steps) adds: padding to 16 | jitter int32 [N, 8] (include/detops.h: detops_color_jitter_u8); `jitter` holds
    those records once more for the host while the jitter is still to be applied to the bytes, None otherwise.  The jitter
    runs once, on the bytes where they land (`to`, `on`), never on the loader's buffer."""

    def __init__(self, buffer, geom, bgr, size, channels_last=False, size_divisible=0, jitter=None):
        self.buffer, self.geom, self.bgr = buffer, geom, bool(bgr)        # geom: the records once more, for the host
        self.jitter = jitter
        self.size, self.channels_last = size, channels_last              # size: (Hp, Wp)
        self.size_divisible = int(size_divisible)
        self.image_sizes = [(int(g[2]), int(g[3])) for g in geom.tolist()]

    def __len__(self):
        return self.geom.shape[0]

    @staticmethod
    def pack(images, table, bgr, size_divisible=0, channels_last=False):
        """images: RawImage records"""
        N = len(images)
        head = (N * 8 + N * 20 + 3 * 256 * 4 + 15) // 16 * 16
        sizes = [im.data.shape[0] * im.data.shape[1] * 3 for im in images]
        offsets = np.cumsum([head] + sizes[:-1]).astype(np.int64) if N else np.zeros(0, np.int64)
        geom = np.array([[im.data.shape[0], im.data.shape[1], im.size[1], im.size[0], im.flip] for im in images],
                        dtype=np.int32).reshape(N, 5)
        from maskrcnn_benchmark import _color_jitter_cpu as J

        jitter, end = None, head + sum(sizes)
        if any(getattr(im, "jitter", ()) for im in images):
            jitter = np.zeros((N, J.FIELDS), dtype=np.int32)
            for rec, im in zip(jitter, images):
                if len(im.jitter) > J.MAX_STEPS:
                    raise ValueError("RawImageBatch.pack: an image carries %d colour steps, at most %d (each operation "
                                     "once) fit a record" % (len(im.jitter), J.MAX_STEPS))
                for k, (code, par) in enumerate(im.jitter):
                    rec[k], rec[J.MAX_STEPS + k] = code, (int(par) if code == J.HUE else J.factor_bits(par))
            J.check_records(jitter)
            block = (end + 15) // 16 * 16
            end = block + N * J.FIELDS * 4
        buf = np.empty(end, dtype=np.uint8)
        buf[:N * 8] = offsets.view(np.uint8)
        buf[N * 8:N * 28] = geom.reshape(-1).view(np.uint8)
        buf[N * 28:N * 28 + 3072] = table.numpy().reshape(-1).view(np.uint8)
        buf[N * 28 + 3072:head] = 0
        for o, n, im in zip(offsets, sizes, images):
            buf[o:o + n] = np.ascontiguousarray(im.data, dtype=np.uint8).reshape(-1)
        if jitter is not None:
            buf[head + sum(sizes):block] = 0
            buf[block:] = jitter.reshape(-1).view(np.uint8)
            jitter = torch.from_numpy(jitter)
        geom = torch.from_numpy(geom)
        return RawImageBatch(torch.from_numpy(buf), geom, bgr, RawImageBatch._padded(geom, size_divisible), channels_last,
                             size_divisible, jitter)

    @staticmethod
    def _padded(geom, size_divisible):
        """(Hp, Wp) of the batch tensor: the largest destination, rounded up to size_divisible"""
        Hp, Wp = (int(geom[:, 2].max()), int(geom[:, 3].max())) if geom.shape[0] else (0, 0)
        if size_divisible > 0:
            d = int(size_divisible)
            Hp, Wp = (Hp + d - 1) // d * d, (Wp + d - 1) // d * d
        return Hp, Wp

    def pin_memory(self):
        """torch's DataLoader(pin_memory=True) calls this in the main process"""
        self.buffer = self.buffer.pin_memory()
        return self

    def _batch(self, buf, geom, geom_host, size):
        from maskrcnn_benchmark import _C

        N = geom_host.shape[0]
        offsets = buf[:N * 8].view(torch.int64)
        table = buf[N * 28:N * 28 + 3072].view(torch.float32).view(3, 256)
        out = _C.image_batch(buf, offsets, geom, table, self.bgr, size[0], size[1],
                             channels_last=self.channels_last and buf.device.type != "cpu", geom_host=geom_host)
        return ImageList(out, [(int(g[2]), int(g[3])) for g in geom_host.tolist()])

    def _jittered(self, buf):
        """`buf`: this batch's bytes where they landed, a copy the caller owns -> the same tensor with the colour jitter
        applied to the images (one color_jitter call; nothing when no image carries steps)"""
        if self.jitter is not None:
            from maskrcnn_benchmark import _C

            N = self.geom.shape[0]
            block = buf.numel() - N * 32
            _C.color_jitter(buf, buf[:N * 8].view(torch.int64), buf[N * 8:N * 28].view(torch.int32).view(N, 5),
                            buf[block:].view(torch.int32).view(N, 8), geom_host=self.geom, jitter_host=self.jitter)
        return buf

    def _landed(self, device):
        """the bytes on `device` with the jitter applied; the loader's buffer itself is never changed"""
        here = self.buffer.device                      # ("cuda" names the device the bytes are on)
        there = device.type == "cpu" or (here.type == device.type and device.index in (None, here.index))
        if self.jitter is None:
            return self.buffer if there else self.buffer.to(device, non_blocking=True)
        return self._jittered(self.buffer.clone() if there else self.buffer.to(device, non_blocking=True))

    def to(self, device, *args, **kwargs):
        device = torch.device(device)
        N = self.geom.shape[0]
        buf = self._landed(device)
        return self._batch(buf, buf[N * 8:N * 28].view(torch.int32).view(N, 5), self.geom, self.size)

    def on(self, device):
        """The same batch with its bytes on `device`: the ONE host-to-device copy of a batch that is prepared several times
        (`prepare`).  The host records stay on the host."""
        buf = self._landed(torch.device(device))
        if buf is self.buffer:
            return self                                # already there, and no jitter to run
        return RawImageBatch(buf, self.geom, self.bgr, self.size, self.channels_last,
                             self.size_divisible)      # jitter None: it has been applied to these bytes

    def target(self, min_size, max_size, flip=False):
        """The records of this batch prepared at another target: every SOURCE image through Resize(min_size, max_size) and,
        with `flip`, mirrored horizontally -> geom int32 [N, 5] on the host (the batch's own flips are not carried over)."""
        from .transforms import Resize

        resize = Resize(min_size, max_size)
        geom = self.geom.clone()
        for i, (h, w) in enumerate(self.geom[:, :2].tolist()):
            oh, ow = resize.get_size((w, h))
            geom[i, 2], geom[i, 3], geom[i, 4] = oh, ow, int(bool(flip))
        return geom

    def prepare(self, min_size, max_size, flip=False):
        """-> ImageList of the batch at that target, on the device the bytes are on (`on`): one small record upload and one
        image_batch launch; the raw bytes are not copied again."""
        geom = self.target(min_size, max_size, flip)
        dev = self.buffer.device
        return self._batch(self.buffer, geom if dev.type == "cpu" else geom.to(dev, non_blocking=True), geom,
                           self._padded(geom, self.size_divisible))


class RawBatchCollator(object):
    """[(RawImage, target, id)] -> (RawImageBatch, tuple(targets), tuple(ids))"""

    def __init__(self, size_divisible=0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), to_bgr255=True, channels_last=False):
        from .transforms import normalisation_table

        self.size_divisible, self.bgr, self.channels_last = size_divisible, to_bgr255, channels_last
        self.table = normalisation_table(mean, std, to_bgr255)

    def __call__(self, batch):
        images, targets, ids = zip(*batch)
        return RawImageBatch.pack(images, self.table, self.bgr, self.size_divisible, self.channels_last), targets, ids
